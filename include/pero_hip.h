/* pero_hip.h - C ABI of libpero_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * per-step hot path of DCGM/pero-pretraining (masked / joint-embedding pre-training over text-line
 * images).
 *
 * The reference is pure Python and has no FFI of its own for this path: every function below
 * replaces a PyTorch library call made by the reference (cited per function, paths relative to
 * /root/reference/pero_pretraining/).  A Python caller binds this header with ctypes (see
 * INTEGRATION.md); nothing in the signatures is a torch type.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (workspaces included); the library never
 *     allocates, frees, copies from the host or synchronises (its only host-side state: pero_set_option's
 *     knobs, and two immutable values initialised once, thread-safely: the device's CU count and each
 *     kernel's dynamic-LDS limit);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it;
 *   - `dtype`: PERO_F32 (parity mode, exact f32 MFMA / VALU arithmetic) or PERO_BF16 (bf16 storage
 *     and MFMA operands, f32 accumulation, f32 statistics);
 *   - return value 0 = ok, negative = PERO_E_*; text via pero_last_error() (thread local);
 *   - re-entrant, callable from any thread (autograd worker threads call the backward entry points).
 */
#ifndef PERO_HIP_H
#define PERO_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PERO_F32 0
#define PERO_BF16 1

#define PERO_OK 0
#define PERO_E_INVALID (-1)   /* bad argument (shape, alignment, null pointer) */
#define PERO_E_UNSUPPORTED (-2)
#define PERO_E_LAUNCH (-3)    /* hipLaunch / runtime error; message holds hipGetErrorString */

/* epilogue / mode flags of pero_gemm */
#define PERO_GEMM_RELU 1        /* C = max(C, 0) after bias/residual */
#define PERO_GEMM_ATOMIC 2      /* f32 C only: the product is ADDED into C (split-K safe).  Without a `workspace` the additions are f32
                                 * atomics: several streams may add into one C at the same time.  WITH a `workspace` of
                                 * pero_gemm_workspace_bytes() the slices of a tile are summed in slice order and added to C by a plain
                                 * read-modify-write: bit-reproducible from run to run, but C must then have ONE writer at a time
                                 * (calls that add into the same C must be ordered on one stream or by events) */
#define PERO_GEMM_ACCUM 4       /* f32 C only: C += result (non-atomic) */
#define PERO_GEMM_TRANS_A 8     /* A is stored [K][M] (lda = row pitch of that storage) */
#define PERO_GEMM_TRANS_B 16    /* B is stored [K][N]; default B is stored [N][K] (Linear weight layout) */
#define PERO_GEMM_TILE128 64     /* force the persistent 128x128x64 bf16 kernel */
#define PERO_GEMM_TILE256 128    /* take the eight-phase 256x256x64 kernel whatever the tile count (when the shape allows: M, N % 256, K % 64, K >= 128) */
#define PERO_GEMM_TILE_V 512     /* accepted, no effect (a round-1 tile hint) */
#define PERO_GEMM_ROWDOT 4096   /* bf16 C, N % 128 == 0: `gate` is a bf16 matrix of C's shape that is NOT applied as a gate, and `bias`
                                 * is an OUTPUT (f32 [M][N/128]): bias[m][b] = sum over columns 128b..128b+127 of C[m][c] * gate[m][c],
                                 * with C as stored (bf16).  The attention backward's D = rowsum(dO * O) per head, out of the
                                 * epilogue of the product that writes dO.  No input bias / gate in this mode. */
#define PERO_GEMM_RELU_BITS 8192 /* the ReLU gate as a BIT MASK, bit (n & 7) of byte gate[m * ldg + n / 8] (ldg in bytes).  With
                                   PERO_GEMM_RELU `gate` is an OUTPUT: bit = (stored C[m][n] > 0); without it `gate` is that mask
                                   as INPUT and replaces the bf16 gate matrix (1/16 of its bytes).  bf16 C, batch 1, the 256-row
                                   tile kernels only (M % 256 == 0, N % 128 == 0, K % 32 == 0): anything else is PERO_E_INVALID */
#define PERO_GEMM_MASK_TILED 16384 /* with PERO_GEMM_RELU_BITS, N % 256 == 0: the bit mask is stored per 256-column block - bit (n & 7) of byte
                                   gate[(n / 256) * M * 32 + m * 32 + (n % 256) / 8] (ldg ignored; the same M * N / 8 bytes) - so that a 256 x 256
                                   tile's mask is 8 KiB of contiguous bytes (whole lines) instead of a quarter of a line per row.  Producer and consumer
                                   of a mask must agree. */
#define PERO_GEMM_COLSUM 1024   /* `bias` is an OUTPUT (f32 [N], accumulated atomically): column sums over the M rows of the
                                 * stored result - the bias gradient of the Linear whose output gradient this product
                                 * writes (replaces a separate pero_colsum pass over C).  No input bias in this mode. */
#define PERO_GEMM_FORCE_GENERIC 32 /* testing: take the exact-f32 generic kernel even when the fast bf16 kernel applies */

const char* pero_last_error(void);
int pero_abi_version(void);
/* tuning knobs for benchmarking and tests (defaults are the measured best; the one table: csrc/options.hpp): "gemm_policy" (0 = auto, 1 / 4 / 7 / 20 = force
 * one tile-kernel family, table in csrc/gemm.hip), "attn_bwd_pair" (1: the attention backward with D handed in runs as one launch, csrc/attention_bwd.hip),
 * "attn_order" (32: dispatch order of that launch's blocks; 0 = a unit's blocks side by side - same bits), "splitk_workspace" (1: the split-K
 * products of the eight-phase kernel leave partial tiles in the caller's `workspace`, summed in slice order by a second kernel - deterministic;
 * 0: f32 atomics even when a workspace is passed), "splitk_table" (1: unaligned slice counts hand their work items out XCD by XCD), "gemm_nw" (0; 1: stored
 * N = 512 products with a bias / residual epilogue run on the row-complete 128 x 512 tile that pero_gemm_resid_layernorm uses - same bits),
 * "gemm_e256_min" (192: stored products with at least that many 256x256 tiles take the eight-phase kernel; 0 = never), "gemm_e_splitk_min" (4),
 * "splitk_xcd" (1), "splitk_nearest" (0), "splitk_items" (512).  Process-wide; not meant to be changed while products are in flight.
 * "attn_bwd_pair" and "attn_order" have no effect at head_dim 64: those kernels (csrc/attention_hd64.hip) have one form -
 * compiler-scheduled loops, the dQ kernel then the dK / dV kernel whether D is computed or handed in. */
int pero_set_option(const char* name, int value);

/* ---- front end ------------------------------------------------------------------------------
 * images u8 (N,H,W,C) -> patch rows (N*S, C*H*P) ordered (c,h,p), value/255, masked patches replaced
 * by the (C,H,P) noise tile.  Replaces BatchOperator._prepare_batch_images
 * (masked_pretraining/batch_operator.py:17-20) + TransformerEncoder.mask (models/transformers.py:53-68)
 * + the im2col of Conv2d(kernel=stride=(H,P)) (models/transformers.py:99-107).  mask may be null.
 * ld_out >= C*H*P is the row pitch of `patches` in elements; the padding columns are zero-filled (a pitch
 * that is a multiple of 128 lets the weight-gradient GEMM of the patch embedding run on the fast kernel). */
int pero_patches_from_u8(const uint8_t* images, const int64_t* mask, const float* tile, void* patches,
                         int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t ld_out, int dtype, void* stream);
/* same from float NCHW images (the reference's own model input layout) */
int pero_patches_from_f32(const float* images_nchw, const int64_t* mask, const float* tile, void* patches,
                          int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t ld_out, int dtype, void* stream);
/* in-place TransformerEncoder.mask on float NCHW images (models/transformers.py:53-68) */
int pero_apply_mask_f32(float* images_nchw, const int64_t* mask, const float* tile,
                        int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, void* stream);

/* ---- GEMM -------------------------------------------------------------------------------------
 * C[b] = alpha * op(A[b]) * op(B[b])^T (+ bias[n]) (+ residual) (relu) (* (gate > 0)),  M x N x K.
 * Replaces torch.nn.Linear / F.linear / torch.matmul / Conv2d-as-GEMM call sites:
 * models/transformers.py:37-43,99 ; masked_pretraining/model.py:102 ; models/autoencoders.py:214 ;
 * joint_embedding_pretraining/losses.py:42,77 and their autograd backward products.
 * Batch b = bo * batch_inner + bi; operand base offset = bo * s?o + bi * s?i (elements).
 * in_dtype: A, B (and residual, gate); out_dtype: C.  bias is f32.  k_split > 1 needs PERO_GEMM_ATOMIC;
 * k_split == 0 with PERO_GEMM_ATOMIC lets the library choose tile size and split.
 * workspace (device, 16-byte aligned, may be null) / workspace_bytes: scratch for this ONE call, owned by the caller and free again
 * when the work enqueued by the call has run (calls on one stream may share it; concurrent streams need one each).  Only the split-K
 * weight-gradient products use it (partial tiles, see PERO_GEMM_ATOMIC); with less than pero_gemm_workspace_bytes() they add with
 * f32 atomics instead - same value up to the order of the additions. */
int pero_gemm(const void* A, const void* B, void* C, const float* bias, const void* residual, const void* gate,
              int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldg,
              int64_t batch, int64_t batch_inner,
              int64_t sAo, int64_t sAi, int64_t sBo, int64_t sBi, int64_t sCo, int64_t sCi,
              float alpha, int flags, int k_split, int in_dtype, int out_dtype, void* workspace, int64_t workspace_bytes,
              void* stream);
/* bytes of `workspace` with which pero_gemm runs the product of this shape / flags / k_split deterministically (0: it needs none).
 * Depends on the arguments and the pero_set_option knobs only (no device query). */
int64_t pero_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t batch, int flags, int k_split, int in_dtype, int out_dtype);
/* What pero_gemm would do with these arguments, without doing it: returns the kernel family that takes the product (PERO_GEMM_KERNEL_*), or the
 * negative status (and pero_last_error() text) with which pero_gemm refuses the call.  *k_split_out (may be null): the k-slices the kernel runs
 * with (1: a stored product); *extra_pass_out (may be null): 0, or the PERO_GEMM_PASS_* that pero_gemm runs over C afterwards because the chosen
 * kernel has no fused PERO_GEMM_COLSUM / PERO_GEMM_ROWDOT epilogue.  Launches nothing, needs no GPU and reads no operand (only the pointers'
 * alignment counts); depends on the arguments and the pero_set_option knobs only. */
#define PERO_GEMM_KERNEL_GENERIC 1      /* gemm_generic: exact f32, any shape */
#define PERO_GEMM_KERNEL_T128 2         /* gemm_bf16_t128: persistent 128x128x64 */
#define PERO_GEMM_KERNEL_O128 3         /* gemm_bf16_o128: 128x128x64, one tile per workgroup */
#define PERO_GEMM_KERNEL_R256 4         /* gemm_bf16_r256: 256x128x32 */
#define PERO_GEMM_KERNEL_E256 5         /* gemm_bf16_e256, stored product */
#define PERO_GEMM_KERNEL_E256_SPLITK 6  /* gemm_bf16_e256, split-K */
#define PERO_GEMM_KERNEL_N512 7         /* gemm_bf16_n512: row-complete 128x512 ("gemm_nw") */
#define PERO_GEMM_PASS_COLSUM 1
#define PERO_GEMM_PASS_ROWDOT 2
int pero_gemm_plan(const void* A, const void* B, void* C, const float* bias, const void* residual, const void* gate,
                   int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldg,
                   int64_t batch, int64_t batch_inner,
                   int64_t sAo, int64_t sAi, int64_t sBo, int64_t sBi, int64_t sCo, int64_t sCi,
                   float alpha, int flags, int k_split, int in_dtype, int out_dtype, void* workspace, int64_t workspace_bytes,
                   void* stream, int* k_split_out, int* extra_pass_out);

/* Linear + residual + LayerNorm in ONE launch (bf16; N = 512, M % 128 == 0, K % 64 == 0, K >= 192): Y = A W^T + bias + R stored (the backward
 * reads it), T = LayerNorm(Y) * gamma + beta computed from the rounded rows of Y exactly as pero_layernorm_fwd does, mean / rstd f32 per row.
 * Replaces the pair (Linear with the residual add, torch.nn.LayerNorm) of TransformerEncoderLayer's post-norm blocks
 * (x = norm1(x + out_proj(attn)), x = norm2(x + linear2(...)): models/transformers.py:36-43) - the LayerNorm's read of Y goes away.
 * bias may be null.  PERO_E_INVALID for other shapes: the caller falls back to pero_gemm + pero_layernorm_fwd.
 * Y may be null (round 4): the pre-norm rows are then not stored at all - a backward pass through pero_layernorm_bwd_out needs T and rstd
 * only (16 fewer 16-byte stores per lane and tile, a quarter of the launch's HBM traffic at K = 512). */
int pero_gemm_resid_layernorm(const void* A, const void* W, const float* bias, const void* R, const float* gamma, const float* beta,
                              void* Y, void* T, float* mean, float* rstd, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                              int64_t ldy, int64_t ldr, int64_t ldt, float eps, void* stream);

/* Input gradient of a Linear + residual gradient + LayerNorm BACKWARD of the norm in front of that Linear, in ONE launch (round 4; bf16, N = 512,
 * M % 128 == 0, K % 64 == 0, K >= 192): dt = A Wt^T + R with the rows complete in a workgroup (Wt = the transposed bf16 weight copy, N x K), then
 * pero_layernorm_bwd_out's arithmetic on the rounded dt: DX = rstd (dt gamma - mean(dt gamma) - xhat mean(dt gamma xhat)), xhat = (T - beta) / gamma;
 * dgamma / dbeta / dxsum (dxsum may be null) are ACCUMULATED (+=) from per-workgroup partial column sums.  dt itself never reaches memory: replaces
 * pero_gemm (residual epilogue) + pero_layernorm_bwd_out for the two input-gradient products of TransformerEncoderLayer that feed a norm's backward
 * (linear1 -> norm1, in_proj -> the previous layer's norm2; models/transformers.py:36-43).  work: f32, 3 * PERO_LN_BWD_BLOCKS * 512 elements. */
int pero_gemm_resid_layernorm_bwd(const void* A, const void* Wt, const void* R, const void* T, const float* rstd, const float* gamma,
                                  const float* beta, void* DX, float* dgamma, float* dbeta, float* dxsum, float* work, int64_t M, int64_t N,
                                  int64_t K, int64_t lda, int64_t ldw, int64_t ldr, int64_t ldt, int64_t lddx, void* stream);

/* ---- LayerNorm (+ positional encoding) --------------------------------------------------------------
 * y = (x - mean) * rstd * gamma + beta (+ pe[offsets[row / S] + row % S]) ; rows x d.
 * Replaces torch.nn.LayerNorm (models/transformers.py:28,83-84 and the norm1/norm2 of
 * TransformerEncoderLayer) and PositionalEncoding.forward (models/transformers.py:174-188).
 * pe (f32 [max_len][d]) and offsets (int64 [rows/S]) may be null (offsets null => offset 0). */
int pero_layernorm_fwd(const void* x, const float* gamma, const float* beta, const float* pe, const int64_t* offsets,
                       void* y, float* mean, float* rstd, int64_t rows, int64_t d, int64_t S, float eps,
                       int dtype, void* stream);
/* dx, and dgamma/dbeta/dxsum ACCUMULATED (+=) into f32 [d] buffers (dxsum = column sums of dx, i.e. the bias
 * gradient of the Linear that produced x; may be null).  work: f32 workspace of 3 * PERO_LN_BWD_BLOCKS * d. */
#define PERO_LN_BWD_BLOCKS 512
int pero_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                       void* dx, float* dgamma, float* dbeta, float* dxsum, float* work, int64_t rows, int64_t d,
                       int dtype, void* stream);
/* The same backward from the layer's OUTPUT t = xhat * gamma + beta instead of its input rows: xhat = (t - beta) / gamma, so the
 * forward pass keeps t (which the next Linear reads anyway) and rstd, not x and mean ("memory-efficient" LayerNorm; torch.nn.LayerNorm
 * saves its input - models/transformers.py:28,36-43 - the gradient is the same function of the same quantities).  In f32 the two forms
 * agree to rounding; in bf16 t carries the 2^-9 relative rounding x carried before.  A column with gamma == 0 exactly has no xhat left in
 * t: it is taken as 0 (that column's gamma gradient and its -xhat * c2 share of dx are lost, nothing is NaN, other columns are exact) -
 * keep pero_layernorm_bwd where a scale can be exactly zero.  Same accumulation semantics and workspace as above. */
int pero_layernorm_bwd_out(const void* dy, const void* t, const float* rstd, const float* gamma, const float* beta,
                           void* dx, float* dgamma, float* dbeta, float* dxsum, float* work, int64_t rows, int64_t d,
                           int dtype, void* stream);

/* ---- BatchNorm1d (+ ReLU) over the rows of an (rows, d) matrix: the optional `use_bn=True` layers of the joint-embedding MLPHead
 * (Linear -> torch.nn.BatchNorm1d(hidden) -> ReLU on the (N*S, hidden) rows: joint_embedding_pretraining/model.py:99-103).
 * training != 0: batch statistics (mean, BIASED variance; two passes), save_mean / save_rstd (f32 [d]) for the backward, and - when given -
 * running_mean / running_var updated in place as torch does (momentum; the running variance takes the unbiased batch variance).
 * training == 0: the running statistics.  y = (x - mean) * rstd * weight + bias, then ReLU if relu != 0.  work: f32 [2 * d].  Deterministic
 * (no atomics).  Statistics are per CALL, i.e. per data-parallel rank (torch.nn.BatchNorm1d under DDP without SyncBatchNorm). */
int pero_bn_fwd(const void* x, const float* weight, const float* bias, float* running_mean, float* running_var, void* y,
                float* save_mean, float* save_rstd, float* work, int64_t rows, int64_t d, float eps, float momentum, int training,
                int relu, int dtype, void* stream);
/* dx; dweight / dbias (may be null) ACCUMULATED (+=).  relu != 0: dy is first zeroed where the layer's output y is <= 0.  work: f32 [2 * d]. */
int pero_bn_bwd(const void* dy, const void* x, const void* y, const float* weight, const float* save_mean, const float* save_rstd,
                void* dx, float* dweight, float* dbias, float* work, int64_t rows, int64_t d, int relu, int dtype, void* stream);

/* ---- softmax over the last dim (attention probabilities; torch SDPA inside
 * TransformerEncoderLayer._sa_block, models/transformers.py:86) ---------------------------------------
 * p = softmax(scale * s) row-wise; s is f32 (rows, cols), p has `dtype` */
int pero_softmax_fwd(const float* s, void* p, int64_t rows, int64_t cols, float scale, int dtype, void* stream);
/* ds = scale * p * (dp - sum_j p*dp); dp is f32, p and ds have `dtype` */
int pero_softmax_bwd(const void* p, const float* dp, void* ds, int64_t rows, int64_t cols, float scale, int dtype,
                     void* stream);

/* pero_softmax_fwd over the keys [k0, k1) of each row's line: key_ranges is int32 (lines, 2) on the device, line = row / rows_per_line
 * (rows_per_line = num_heads * S for scores laid out (N * num_heads, S, S)); the ranges are clamped as for pero_attention_fwd_keys.  p is exactly 0
 * outside the range, so pero_softmax_bwd serves unchanged. */
int pero_softmax_fwd_keys(const float* s, const int* key_ranges, void* p, int64_t rows, int64_t cols, int64_t rows_per_line, float scale,
                          int dtype, void* stream);

/* ---- fused attention (bf16, head_dim hd = 128 or 64, any S >= 1) on the packed qkv (N*S, 3*nh*hd) tensor ---------
 * out (N*S, nh*hd) = softmax(q k^T / sqrt(hd)) v per (line, head); lse (N*nh, S) f32 = base-2 log-sum-exp of the
 * scaled scores (kept for the backward kernels).  Scores never touch memory.  A line is cut into ceil(S/128) blocks of 128
 * rows; when S % 128 != 0 the last block is ragged: no address outside the line's S rows is read or written, and out,
 * lse, dvec and dqkv keep their unpadded shapes.  head_dim 128: csrc/attention_fwd.hip, attention_bwd.hip; head_dim 64:
 * csrc/attention_hd64.hip, same layouts.  Every other head_dim, and f32, is refused on the host before any launch (PERO_E_INVALID; the
 * message names the accepted widths): use the batched pero_gemm + pero_softmax_* path. */
int pero_attention_fwd(const void* qkv, void* out, float* lse, int64_t N, int64_t S, int64_t num_heads,
                       int64_t head_dim, int dtype, void* stream);
/* dqkv (N*S, 3d) from dout (N*S, d).  dvec (N*S, nh) f32: D[row][head] = sum over the head's hd columns of dout*out -
 * computed and stored by the call when `out` is given, or supplied by the caller (out == null; e.g. written by the
 * PERO_GEMM_ROWDOT epilogue of the product that produced dout - 128-column blocks, so head_dim 128 only).  At head_dim 64 the same two
 * kernels run in both forms and dqkv is bit-identical between them.  dbias (f32 [3d], may be null):
 * the column sums of dqkv - in_proj's bias gradient - are ACCUMULATED into it: per-workgroup partial rows from the kernels'
 * staged output tiles into work (f32, 3 * N * nh * ceil(S/128) * 128 elements - head_dim 64 uses the first half; required with dbias), then
 * one small reduction. */
/* head_dim 64: how many heads of a line one forward workgroup walks for this shape on this process's device (>= 1; a divisor of num_heads;
 * results do not depend on it).  For tests and tools. */
int pero_attention_hd64_heads_per_block(int64_t N, int64_t S, int64_t num_heads);
int pero_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* dvec, void* dqkv,
                       float* dbias, float* work, int64_t N, int64_t S, int64_t num_heads, int64_t head_dim, int dtype,
                       void* stream);

/* ---- fused attention with per-line key ranges (the src_key_padding_mask of a padded, collated batch, as an interval per line).
 * key_ranges: contiguous int32 (N, 2) on the device; line b attends to the keys [k0_b, k1_b) only:
 *   out[q] = sum over k in [k0, k1) of softmax_k(q . k / sqrt(hd)) v_k   for EVERY query q in [0, S), padded ones included
 * (torch scaled_dot_product_attention with a boolean attn_mask of shape (N, 1, 1, S)); lse is the base-2 log-sum-exp over the same keys.
 * Backward: the dK and dV rows outside the range are exact zeros, dQ is computed for every query.  The library never reads device data on
 * the host, so the KERNELS clamp a bad range: k0 into [0, S - 1], then k1 into [k0 + 1, S] - an empty or inverted range means "the single
 * key k0".  Only intervals: no per-key masks, causal masks, biases or dropout.  The other arguments, the `out` / `dvec` conventions, the
 * dbias accumulation and the size of `work` are those of pero_attention_fwd / pero_attention_bwd.  A full range [0, S) on every line gives
 * the bits of the calls without ranges.  head_dim 128 runs the ragged bodies (KEYS instantiations: csrc/attention_fwd.hip,
 * attention_bwd.hip) at every S; key tiles without a live key are not visited. */
int pero_attention_fwd_keys(const void* qkv, const int* key_ranges, void* out, float* lse, int64_t N, int64_t S, int64_t num_heads,
                            int64_t head_dim, int dtype, void* stream);
int pero_attention_bwd_keys(const void* qkv, const int* key_ranges, const void* out, const void* dout, const float* lse, float* dvec,
                            void* dqkv, float* dbias, float* work, int64_t N, int64_t S, int64_t num_heads, int64_t head_dim,
                            int dtype, void* stream);

/* ---- masked cross entropy (masked_pretraining/model.py:72-95) -------------------------------------------
 * logits (rows, V); labels, mask int64 (rows).  loss_out[0] = mean CE over mask==1 rows
 * (+ unmasked_weight * mean CE over mask==0 & label>=0 rows when unmasked_weight >= 0; pass a negative
 * value for "None").  work: f32 workspace of PERO_CE_WORK(rows) elements, kept by the caller for the backward
 * call (row losses, the two row counts, row logsumexps, partial sums of the final reduction).  Empty selections give NaN
 * like the reference.
 * bwd: dlogits (dtype, rows x V) = dloss[0] * d loss / d logits (dloss: device f32 scalar, null = 1). */
#define PERO_CE_WORK(rows) (2 * (rows) + 8 + 256)
int pero_masked_ce_fwd(const void* logits, const int64_t* labels, const int64_t* mask, float unmasked_weight,
                       float* loss_out, float* work, int64_t rows, int64_t V, int dtype, void* stream);
int pero_masked_ce_bwd(const void* logits, const int64_t* labels, const int64_t* mask, float unmasked_weight,
                       const float* dloss, const float* work, void* dlogits, int64_t rows, int64_t V, int dtype,
                       void* stream);
/* pero_masked_ce_fwd for a caller that knows the rows with mask == 1 (index: int64 device list of n_idx rows) and passes
 * unmasked_weight "None": only those rows are visited (one workgroup each instead of one per position); same loss bits. */
int pero_masked_ce_fwd_rows(const void* logits, const int64_t* labels, const int64_t* mask, const int64_t* index, int64_t n_idx,
                            float* loss_out, float* work, int64_t rows, int64_t V, int dtype, void* stream);
/* The same gradient in COMPACT form: dlogits_rows (dtype, n_rows_out x V) row i = the gradient row of logits row index[i] for
 * i < n_idx (bit-identical to row index[i] of pero_masked_ce_bwd's result), zero rows for n_idx <= i < n_rows_out (padding up to whole
 * GEMM tiles).  With unmasked_weight "None" every row outside mask == 1 of the dense gradient is an exact zero, so the head's
 * backward products (masked_pretraining/model.py:60-61 through autograd) run on the listed rows alone.  index: int64 device list. */
int pero_masked_ce_bwd_rows(const void* logits, const int64_t* labels, const int64_t* mask, float unmasked_weight,
                            const float* dloss, const float* work, const int64_t* index, int64_t n_idx, int64_t n_rows_out,
                            void* dlogits_rows, int64_t rows, int64_t V, int dtype, void* stream);

/* ---- reductions / elementwise ---------------------------------------------------------------------- */
/* out[n] += sum_m x[m][n]  (bias gradients); out f32 */
int pero_colsum(const void* x, float* out, int64_t rows, int64_t cols, int64_t ld, int dtype, void* stream);
/* out[m][b] = sum over columns 128b..128b+127 of x[m][c] * y[m][c]  (bf16 x, y; the pass PERO_GEMM_ROWDOT fuses) */
int pero_rowdot_blocks(const void* x, const void* y, float* out, int64_t rows, int64_t cols, int64_t ldx, int64_t ldy,
                       void* stream);
/* Transposed bf16 copies of every matrix of a flat buffer in one launch (2-byte elements): table (device, int64[n][5]) =
 * {src offset, dst offset, rows, cols, first tile} in elements / 64x64 tiles; dst matrix t is [cols][rows].  The input
 * gradient dX = dY W (torch.nn.Linear backward, models/transformers.py:36-43 layers) reads these K-contiguous copies. */
int pero_transpose_multi(const void* src, void* dst, const int64_t* table, int64_t n_matrices, int64_t total_tiles, void* stream);
/* f32 -> bf16 copy (low-precision weight copies) */
int pero_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
int pero_cast_bf16_f32(const void* src, float* dst, int64_t n, void* stream);
/* dst[r][0:cols] = bf16(src[r][0:cols]), dst[r][cols:ld_dst] = 0   (K-padded low-precision weight copy) */
int pero_cast_pad_f32_bf16(const float* src, void* dst, int64_t rows, int64_t cols, int64_t ld_dst, void* stream);
/* dst[r][c] += src[r][c] for c < cols (f32, row pitches ld_dst / ld_src) */
int pero_add_rows2d(float* dst, const float* src, int64_t rows, int64_t cols, int64_t ld_dst, int64_t ld_src, void* stream);
/* nbytes of zeros at p */
int pero_zero_fill(void* p, int64_t nbytes, void* stream);
/* y = x * scale (in place allowed), dtype elements */
int pero_scale(void* x, int64_t n, float scale, int dtype, void* stream);

/* ---- Adam (torch.optim.Adam defaults: masked_pretraining/train.py:146) ----------------------------------
 * one launch over a flat f32 parameter / gradient / moment buffer; `step` is 1-based; optionally also
 * writes the bf16 copy of the updated parameters (p_bf16 may be null). */
int pero_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, double lr,
                   double beta1, double beta2, double eps, int64_t step, double grad_scale, void* stream);
/* The same launch with torch.optim.Adam's remaining arguments and a fused global-norm clip.  Per element, in torch's order
 * (bc1 = 1 - beta1^step, bc2 = 1 - beta2^step; lr / bc1, 1 / sqrt(bc2) and 1 - lr * weight_decay are formed in f64 on the host):
 *   g = grad * grad_scale
 *   grad_norm != null:  g *= min(1, max_norm / (*grad_norm + 1e-6))           (torch.nn.utils.clip_grad_norm_)
 *   maximize:           g = -g
 *   weight_decay != 0:  decoupled ? p *= 1 - lr * weight_decay : g += weight_decay * p        (AdamW : Adam)
 *   m = beta1 * m + (1 - beta1) * g ;  v = beta2 * v + (1 - beta2) * g * g
 *   vmax != null (amsgrad):  vmax = max(vmax, v) ; denom = sqrt(vmax) / sqrt(bc2) + eps ;  else denom = sqrt(v) / sqrt(bc2) + eps
 *   p -= (lr / bc1) * m / denom ;  p_bf16 = round-to-nearest-even(p)
 * vmax: f32, the length and alignment of v.  grad_norm: DEVICE pointer to one f32, the global gradient norm already multiplied by
 * grad_scale (pero_grad_norm_finish writes it); every thread reads it, no host copy of it exists.  decoupled, maximize: 0 or 1.
 * With weight_decay = 0, maximize = 0, vmax = null and grad_norm = null the results are bit-identical to pero_adam_step. */
int pero_adam_step_ex(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, double lr,
                      double beta1, double beta2, double eps, int64_t step, double grad_scale, double weight_decay,
                      int decoupled, float* vmax, int maximize, const float* grad_norm, double max_norm, void* stream);
/* Global L2 norm of one or several flat f32 buffers in two kinds of launch, without float atomics: every addition has a fixed place,
 * so the same input gives the same bits from run to run and from device to device.
 * pero_sumsq_partials: partials[b] = sum of x[i]^2 over the elements of workgroup b, b < pero_sumsq_num_partials(n) (a function of n
 * alone: min(ceil(ceil(n / 4) / 1024), 2048); returns that count, not a status).  x 16-byte aligned; the caller lays the partials of
 * several buffers one behind the other in one workspace.
 * pero_grad_norm_finish: norm[0] = (f32)(scale * sqrt(sum_i partials[i])), the sum in f64 in index order (256 contiguous runs, then the
 * run sums), one workgroup. */
int pero_sumsq_num_partials(int64_t n);
int pero_sumsq_partials(const float* x, int64_t n, float* partials, void* stream);
int pero_grad_norm_finish(const float* partials, int64_t count, double scale, float* norm, void* stream);

/* ---- layer-wise optimizers: LAMB (You et al. 2020) and LARS (You et al. 2017) over flat buffers (csrc/optim_layerwise.hip) ------------
 * The reference has no counterpart (it trains with torch.optim.Adam); tests/layerwise_ref.py restates these formulas in f64.
 *
 * Layout.  A flat f32 buffer holds n_tensors parameter tensors.  table (DEVICE, int64[n_tensors][3]) = {offset, numel, first tile}:
 * every tensor is cut into ceil(numel / PERO_LAYER_TILE) tiles of PERO_LAYER_TILE elements, tile 0 starting AT the tensor's offset and
 * the last one possibly short, so no tile crosses a tensor; first tile = the number of tiles of the tensors in front; total_tiles = the
 * sum.  In this table, in pero_ema_update's and in pero_transpose_multi's, first tile is the LAST column and never decreases from row to
 * row: a workgroup finds its row by binary search, the last one whose first tile is <= its index (csrc/flat_tiles.hpp).  Offsets are multiples of 8 elements (16-byte aligned f32 AND bf16 tiles) and numel >= 1; the library cannot read the table on
 * the host, so the caller vouches for it.  The layout is a function of the tensor sizes alone.  One workgroup of 256 lanes takes one
 * tile: lane t holds the four 16-byte pieces at elements (k * 256 + t) * 4, k = 0..3, of the tile.
 *
 * Three launches per step, no float atomics, no waiting between workgroups, no buffer for the update u:
 *   stage 1   computes u per element and writes partials[2 * tile] = sum p^2, partials[2 * tile + 1] = sum u^2 over the tile (p: the
 *             parameter BEFORE the step).  Each lane keeps four running f32 sums (one per element of a piece, over its four pieces: 4
 *             additions), folds them ((a0+a1)+(a2+a3): 2), the 64 lanes of a wave by a butterfly (6), the four waves in order (3).
 *             partials: f32 [2 * total_tiles].
 *   finish    one workgroup per tensor adds its tiles' partials in index order in f64 (256 contiguous runs, then the run sums) and
 *             writes stats[t] = (|p|, |u|, r) as f32: pn = (f32)sqrt(sum p^2), un = (f32)sqrt(sum u^2),
 *             r = (c * pn) / un in f32 (c = (f32)coefficient) if adapt != 0 and pn > 0 and un > 0, else exactly 1.0 - so a NaN norm
 *             gives 1 and the NaN reaches p through u.  stats: f32 [n_tensors][3].
 *   stage 2   computes u again from the same operands by the same f32 operations (the library is compiled with -ffp-contract=off:
 *             the same bits) and applies it with the tensor's r, writing p and, when p_bf16 is given, its round-to-nearest-even copy.
 *
 * Per element, every operation in f32 in exactly this order (coef, 1 / bc1, 1 / sqrt(bc2) with bc1 = 1 - beta1^step,
 * bc2 = 1 - beta2^step are formed in f64 on the host and rounded once):
 *   g = grad * grad_scale
 *   grad_norm != null:  g = g * coef,  coef = min(1, max_norm / (*grad_norm + 1e-6))     (as pero_adam_step_ex; one device float)
 *   maximize:           g = -g
 *  LAMB  stage 1:  m = m * beta1 + (1 - beta1) * g ;  v = v * beta2 + ((1 - beta2) * g) * g        (stored)
 *                  u = (m * (1 / bc1)) / (sqrt(v) * (1 / sqrt(bc2)) + eps) + weight_decay * p
 *        stage 2:  u from the stored m, v and p as above ;  p = p - (lr * r) * u
 *  LARS  stage 1:  u = g + weight_decay * p                                                        (nothing stored but the partials)
 *        stage 2:  u as above ;  buf = momentum * buf + r * u ;  p = p - lr * buf
 * With r = 1 (adapt == 0) LAMB is AdamW with the decay inside the step, p(1 - lr wd) - lr mhat / denom, and LARS is
 * torch.optim.SGD(momentum, weight_decay).  Both stages of a step take the same grad_scale, weight_decay, maximize, grad_norm,
 * max_norm (and betas, eps, step).  step is 1-based; maximize, adapt: 0 or 1. */
#define PERO_LAYER_TILE 4096
int pero_lamb_stage1(const float* p, const float* g, float* m, float* v, const int64_t* table, int64_t n_tensors,
                     int64_t total_tiles, float* partials, double beta1, double beta2, int64_t step, double eps,
                     double grad_scale, double weight_decay, int maximize, const float* grad_norm, double max_norm, void* stream);
int pero_lamb_stage2(float* p, const float* m, const float* v, void* p_bf16, const int64_t* table, int64_t n_tensors,
                     int64_t total_tiles, const float* stats, double lr, double beta1, double beta2, int64_t step, double eps,
                     double weight_decay, void* stream);
int pero_lars_stage1(const float* p, const float* g, const int64_t* table, int64_t n_tensors, int64_t total_tiles,
                     float* partials, double grad_scale, double weight_decay, int maximize, const float* grad_norm,
                     double max_norm, void* stream);
int pero_lars_stage2(float* p, const float* g, float* buf, void* p_bf16, const int64_t* table, int64_t n_tensors,
                     int64_t total_tiles, const float* stats, double lr, double momentum, double grad_scale,
                     double weight_decay, int maximize, const float* grad_norm, double max_norm, void* stream);
int pero_layer_ratio_finish(const float* partials, const int64_t* table, int64_t n_tensors, double coefficient, int adapt,
                            float* stats, void* stream);

/* ---- quantizers (models/autoencoders.py:212-217 ; scripts/produce_kmeans_labels.py:72-76) ---------------
 * indices[m] = argmin_k ( sum(x_m^2) + sum(e_k^2) - 2 x_m . e_k )  in exact f32, first minimum wins.
 * x (M,D) f32, codebook (K,D) f32, indices int64 (M).  best_dist (f32, M) may be null.
 * work: f32 workspace of at least M + K elements (row / code squared norms). */
int pero_vq_argmin(const float* x, const float* codebook, int64_t* indices, float* best_dist, float* work,
                   int64_t M, int64_t K, int64_t D, void* stream);
/* quantized[m] = x[m] + (codebook[indices[m]] - x[m])  (straight-through arithmetic, autoencoders.py:239) */
int pero_vq_gather(const float* x, const float* codebook, const int64_t* indices, float* quantized,
                   int64_t M, int64_t D, void* stream);
/* EMA codebook update of the tokenizer in training mode (models/autoencoders.py:225-237), in place:
 * ema_cluster_size (K) <- Laplace-smoothed decayed counts, ema_w (K,D) <- decayed sums of the rows assigned to each
 * code, codebook (K,D) <- ema_w / ema_cluster_size.  indices are those of pero_vq_argmin on the OLD codebook.
 * work: f32 workspace of K + K*D elements (zeroed by the call). */
int pero_vq_ema_update(const float* x, const int64_t* indices, float* ema_cluster_size, float* ema_w, float* codebook,
                       float* work, int64_t M, int64_t K, int64_t D, double decay, double epsilon, void* stream);

/* ---- mini-batch k-means fit (scripts/fit_kmeans.py: sklearn MiniBatchKMeans) -----------------------------
 * Every sum has a fixed order (no float atomics): the same inputs give the same bits from run to run.
 *
 * One centre update with the semantics of sklearn's _minibatch_update_dense, in place: for every centre k with
 * n_k > 0 rows in the batch  centers[k] = (centers[k]*weight_sums[k] + sum of its rows) / (weight_sums[k] + n_k),
 * weight_sums[k] += n_k; centres without rows keep their bits.  shift_out[0] = sum_k |c_new - c_old|^2.
 * x (B,D) f32; sorted_labels / order (B) int64: the batch labels sorted ascending (stable) and the permutation that
 * sorts them (order[j] = batch row at sorted position j); centers (K,D) f32; weight_sums (K) f64.
 * work: at least (2K + 1) * 4 bytes. */
int pero_kmeans_update(const float* x, const int64_t* order, const int64_t* sorted_labels, float* centers,
                       double* weight_sums, float* shift_out, void* work, int64_t B, int64_t K, int64_t D, void* stream);
/* out[r] = |x_r|^2, x (rows,D) f32 */
int pero_kmeans_sqnorm(const float* x, float* out, int64_t rows, int64_t D, void* stream);
/* The work for one new centre of greedy k-means++ (sklearn _kmeans_plusplus): for each of the t candidate rows
 * (1 <= t <= 32) the distances of all n rows, their minimum with closest_dist_sq and the potential (the sum of
 * those minima); the candidate with the lowest potential (the first on a tie) is committed: chosen[0] = its row
 * index, potential[0] = its potential (f64), closest_dist_sq (n, in/out) <- its minima.  sqnorm (n) = |x_i|^2.
 * work: f32 workspace of at least 4 + t*n + t*ceil(n/64) elements. */
int pero_kmeans_pp_step(const float* x, const float* sqnorm, float* closest_dist_sq, const int64_t* candidates,
                        int64_t* chosen, double* potential, float* work, int64_t n, int64_t D, int64_t t, void* stream);
/* Early stopping of the fit loop on the device (sklearn _mini_batch_convergence), one call per step.
 * batch_inertia[0]: sum of the batch's squared distances to the centres before the update; shift[0]: shift_out of
 * the update.  state (f64[6], zeroed by the caller before the first step): EWA inertia, its minimum, steps without
 * improvement, stop flag, steps seen, step at which the flag was raised.  tol <= 0 and max_no_improvement < 0
 * switch the respective rule off. */
int pero_kmeans_converge(const float* batch_inertia, const float* shift, double* state, int64_t n_samples,
                         int64_t batch_size, double tol, int64_t max_no_improvement, void* stream);

/* ---- row gather / scatter by index (boolean-mask selections of the losses) ----------------------------- */
/* dst[i] = src[index[i]] for i < n_idx, zero rows for n_idx <= i < n_rows_out (padding) */
int pero_gather_rows(const void* src, const int64_t* index, void* dst, int64_t n_idx, int64_t n_rows_out,
                     int64_t d, int dtype, void* stream);
/* dst[index[i]] += src[i] (indices unique) */
int pero_scatter_add_rows(const void* src, const int64_t* index, void* dst, int64_t n_idx, int64_t d,
                          int dtype, void* stream);

/* ---- joint-embedding losses (joint_embedding_pretraining/losses.py) ---------------------------------------
 * The dense products (covariance SYRK z^T z, its backward zc @ G, per-line similarity x y^T and its backward)
 * are pero_gemm calls; these entry points are the surrounding reductions.  `g` arguments are DEVICE f32
 * scalars holding the upstream gradient (null = 1), so backward needs no host synchronisation. */
/* out[0] = scale * sum_rows |x[ix[r]] - y[iy[r]]|^2   (VICReg invariance, losses.py:14-16); partial: f32 [n] */
int pero_sqdiff_rows(const void* x, const int64_t* ix, const void* y, const int64_t* iy, float* partial, float* out,
                     int64_t n, int64_t d, float scale, int dtype, void* stream);
/* dx[ix[r]] += g*coef*(x-y) ; dy[iy[r]] -= g*coef*(x-y) */
int pero_sqdiff_rows_bwd(const void* x, const int64_t* ix, const void* y, const int64_t* iy, void* dx, void* dy,
                         const float* g, float coef, int64_t n, int64_t d, int dtype, void* stream);
/* out[0] = scale * sum(partial[0..n)) in a fixed order */
int pero_sum_scale(const float* partial, float* out, int64_t n, float scale, void* stream);
/* zc = z - colsum/m for rows < m, 0 for padding rows m..m_pad; sumsq[c] += sum_r zc[r][c]^2 (losses.py:38,41) */
int pero_center_cols(const void* z, const float* colsum, void* zc, float* sumsq, int64_t m, int64_t m_pad, int64_t d,
                     int dtype, void* stream);
/* variance hinge loss_var = mean_j relu(threshold - sqrt(sumsq_j/(m-1) + eps)) and its per-column gradient
 * coefficient cvar_j (losses.py:37-38) */
int pero_vicreg_var(const float* sumsq, float* cvar, float* loss_var, int64_t m, int64_t d, float threshold, float eps,
                    void* stream);
/* loss_cov = sum_{i!=j} cov_ij^2 / d (losses.py:40-47) and the backward operand G (dtype, d x d):
 * G_ij = wc*4*cov_ij/(d*(m-1)) (i != j), G_jj = wv*cvar_j, so that d(wv*var + wc*cov)/d zc = zc @ G.
 * rowpart: f32 [d] scratch */
int pero_vicreg_cov(const float* cov, const float* cvar, void* G, float* rowpart, float* loss_cov, int64_t d, int64_t m,
                    float wv, float wc, int dtype, void* stream);
/* dst[index[i]] += g * src[i] */
int pero_scatter_add_rows_scaled(const void* src, const int64_t* index, void* dst, const float* g, int64_t n, int64_t d,
                                 int dtype, void* stream);
/* xn = x / max(|x|_2, 1e-12) per row, inv[r] = 1 / max(|x_r|, 1e-12)   (F.normalize, losses.py:58-59) */
int pero_rownorm_fwd(const void* x, void* xn, float* inv, int64_t rows, int64_t d, int dtype, void* stream);
int pero_rownorm_bwd(const void* xn, const void* dxn, const float* inv, const float* g, void* dx, int64_t rows, int64_t d,
                     int dtype, void* stream);
/* sim (lines, S, S) f32: line_loss[l] = mean_j (logsumexp_r sim[l][r][j] - sim[l][j][j]) (losses.py:80, softmax over
 * dim 0), loss_out[0] = mean_l line_loss[l]; dsim (dtype, may be null) = d loss_out / d sim */
int pero_ntxent_cols(const float* sim, float* line_loss, float* loss_out, void* dsim, int64_t lines, int64_t S, int dtype,
                     void* stream);
/* Cross-rank negatives (NTXentLoss(cross_rank_negatives=True): the data-parallel extension named by BASELINE.json's north_star; the
 * reference's loss is per line and has no such term).  cross (lines*S, L) f32: similarities of every view-2 row with the L pooled
 * embeddings of all ranks' lines (pooled embedding own0 + l belongs to line l itself and is left out).  Column j of line l is
 * normalised over its S own rows AND those L - 1 negatives in one log-sum-exp:
 *   line_loss[l] = mean_j ( log( sum_i exp(sim[l][i][j]) + sum_{l' != own0 + l} exp(cross[l*S + j][l']) ) - sim[l][j][j] ),
 * loss_out[0] = mean_l line_loss[l]; dsim (dtype, lines x S x S) and dcross (dtype, lines*S x L), may be null = d loss_out / d input. */
int pero_ntxent_cols_cross(const float* sim, const float* cross, float* line_loss, float* loss_out, void* dsim, void* dcross,
                           int64_t lines, int64_t S, int64_t L, int64_t own0, int dtype, void* stream);
/* out[l][c] (f32) = mean over the S rows of line l of x[l*S + s][c] (the pooled embedding of a line); d % 8 == 0 */
int pero_line_mean(const void* x, float* out, int64_t lines, int64_t S, int64_t d, int dtype, void* stream);
/* dst[l*S + s][c] += scale * src[l][c] for every row s of line l (the backward of pero_line_mean: scale = 1 / S); dst dtype, src f32 */
int pero_add_line_rows(void* dst, const float* src, int64_t lines, int64_t S, int64_t d, float scale, int dtype, void* stream);

/* ---- NT-Xent on collated batches (NTXentLoss(apply_masks=True), csrc/ntxent_ragged.hip) ---------------------------
 * A position of line l is SELECTED in view v when shift_mask_v[l][p] == 1 and image_mask_v[l][p] == 1 (2 in a shift mask, "shared
 * but padding", is not).  The k-th selected position of view 1 pairs with the k-th of view 2; m_l is their common number.  The
 * selected rows are compacted to the front of a block of Sp >= S rows per line (Sp % 128 == 0 keeps the per-line products on
 * pero_gemm's bf16 tile kernel); every row, column and gradient entry behind m_l is an explicit zero.
 *
 * masks u8 (lines, S): slot_v[l][p] (int32) = the rank of position p among the selected positions of view v, -1 when not selected;
 * count[l] (int32) = m_l, -1 when the two views select different numbers.  One wave per line; S <= 4096. */
int pero_ntxent_slots(const void* image_mask1, const void* image_mask2, const void* shift_mask1, const void* shift_mask2, int* slot1,
                      int* slot2, int* count, int64_t lines, int64_t S, void* stream);
/* x (lines, S, d), slot (lines, S), count (count_lines; line l uses count[l % count_lines]: the two views stacked are lines =
 * 2 count_lines).  With m = max(count, 0):  xn[l][k] = x[l][p] / max(|x[l][p]|_2, 1e-12), inv[l][k] = 1 / max(|x[l][p]|_2, 1e-12) for
 * slot[l][p] = k < m;  xn[l][k] = 0, inv[l][k] = 0 for m <= k < Sp.  xn (lines, Sp, d) dtype, inv (lines, Sp) f32: every element is
 * written. */
int pero_ntxent_rows_fwd(const void* x, const int* slot, const int* count, void* xn, float* inv, int64_t lines, int64_t count_lines,
                         int64_t S, int64_t Sp, int64_t d, int dtype, void* stream);
/* dx[l][p] = (dxn[l][k] - xn[l][k] <xn[l][k], dxn[l][k]>) inv[l][k] g  for slot[l][p] = k in [0, count);  dx[l][p] = 0 elsewhere.
 * xn, dxn (lines, Sp, d), dx (lines, S, d): every element is written; g (f32 scalar on the device) may be null = 1. */
int pero_ntxent_rows_bwd(const void* xn, const void* dxn, const float* inv, const int* slot, const int* count, const float* g, void* dx,
                         int64_t lines, int64_t count_lines, int64_t S, int64_t Sp, int64_t d, int dtype, void* stream);
/* sim (lines, Sp, Sp) f32, m = count[l]; cross (lines*Sp, L) f32 or null (then dcross null, L and own0 unused).
 *   lse_j = log( sum_{i<m} exp(sim[l][i][j]) + sum_{l' != own0 + l} exp(cross[l*Sp + j][l']) )                      (j < m)
 *   line_loss[l] = mean_{j<m} (lse_j - sim[l][j][j]),  loss_out[0] = mean_l line_loss[l],  w = 1 / (m lines)
 *   dsim[l][i][j] = (exp(sim[l][i][j] - lse_j) - [i == j]) w   (i, j < m),  0 for every other entry of the Sp x Sp block
 *   dcross[l*Sp + j][l'] = exp(cross[l*Sp + j][l'] - lse_j) w  (j < m, l' != own0 + l),  0 for every other entry
 * m <= 0: line_loss[l] = NaN (so loss_out is NaN) and all of the line's gradient entries are 0.  dsim, dcross (dtype) may be null. */
int pero_ntxent_cols_ragged(const float* sim, const int* count, const float* cross, float* line_loss, float* loss_out, void* dsim,
                            void* dcross, int64_t lines, int64_t Sp, int64_t L, int64_t own0, int dtype, void* stream);
/* out[l][c] (f32) = (1 / count[l]) sum_{s < count[l]} x[l*Sp + s][c]  (0 for count[l] <= 0); d % 8 == 0 */
int pero_line_mean_ragged(const void* x, const int* count, float* out, int64_t lines, int64_t Sp, int64_t d, int dtype, void* stream);
/* dst[l*Sp + s][c] += src[l][c] / count[l] for s < count[l] (the backward of pero_line_mean_ragged); dst dtype, src f32 */
int pero_add_line_rows_ragged(void* dst, const float* src, const int* count, int64_t lines, int64_t Sp, int64_t d, int dtype, void* stream);

/* ---- evaluation -------------------------------------------------------------
 * replaces masked_pretraining/tester.py:72-113 (_update_errors / _topk / _calculate_errors: host numpy argmax and
 * argsort over the full logit tensor).  For every row with mask == 1: gt = #{j : logit[j] > logit[label]},
 * eq_lo / eq_hi = #{j : logit[j] == logit[label], j < label / j > label}.  counters (u64 [1 + nk], ACCUMULATED, caller
 * zeroes them once per test()): [0] += rows with mask == 1 ("length"), [1 + i] += rows whose label is not in the top
 * ks[i] (k == 1: argmax = first maximum; k > 1: stable-argsort order, see csrc/eval.hip).  ranks (int32 [rows][3],
 * may be null): gt, eq_lo, eq_hi, or -1 where mask != 1.  ks is a DEVICE pointer (nk <= PERO_MAX_TOPK). */
#define PERO_MAX_TOPK 8
int pero_label_rank(const void* logits, int64_t ld, const int64_t* labels, const int64_t* mask, int64_t rows, int64_t V,
                    const int32_t* ks, int32_t nk, uint64_t* counters, int32_t* ranks, int dtype, void* stream);

/* ---- batch collation -------------------------------------------------------------
 * replaces common/dataloader.py:68-155 (BatchCreator.stack_images: host numpy zero-fill + slice copies + mask loops).
 * packed: the ragged uint8 lines back to back, line b = (H, widths[b], C) row-major at byte offsets[b]; the buffer must
 * be readable 8 bytes past its end.  out (B, H, Wt, C) u8, every byte written: line b's pixels at columns
 * [left_px[b], left_px[b] + widths[b]), zero elsewhere.  Wt*C must be a multiple of 16 (Wt % 32 == 0 in the reference). */
int pero_stack_lines(const void* packed, const int64_t* offsets, const int32_t* widths, const int32_t* left_px, void* out,
                     int64_t B, int64_t H, int64_t Wt, int64_t C, void* stream);
/* image masks (B, S) u8 (dataloader.py:92-96), shifts (B) i32 = crop_shifts + left1 - left2 (:126; left* in label
 * positions), three-valued shift masks (:124-138).  Second-view outputs may all be null (unpaired batch);
 * crop_shifts may be null (= 0). */
int pero_line_masks(const int32_t* widths1, const int32_t* widths2, const int32_t* left1, const int32_t* left2,
                    const int32_t* crop_shifts, uint8_t* image_masks1, uint8_t* image_masks2, uint8_t* shift_masks1,
                    uint8_t* shift_masks2, int32_t* shifts, int64_t B, int64_t S, int64_t subsampling, void* stream);

/* ---- line augmentation fused into collation (csrc/augment.hip) ---------------------------------
 * pero_stack_lines with a per-line warp, tone curve and noise on the way: the same packed / offsets / widths / left_px (packed
 * readable 8 bytes past its end) and the same out (B, H, Wt, C) u8, every byte written exactly once.  The transform keeps the
 * width: line b occupies columns [left_px[b], left_px[b] + w), w = widths[b], and every byte outside is zero.  C <= 4: the two
 * horizontal taps of a source row are fetched as one 8-byte read, which may run into the 8 bytes behind the buffer.
 *   params (B, P) i32, P = PERO_AUGMENT_PARAMS, columns: sy (vertical scale, 8.8 fixed point: 256 = 1), ty (vertical translation,
 *     1/256 px), slope (vertical shift per pixel of x, 1/256 px), slant (horizontal shift per pixel of y, 1/256 px), noise_amp,
 *     seed_lo, seed_hi (the last two as 32 raw bits).
 *   knots (B, 2, NK) i32, NK = (Wt >> knot_shift) + 2: vertical ([b][0]) and horizontal ([b][1]) displacement in 1/256 px at the
 *     line's own columns 0, K, 2 K, ..., K = 1 << knot_shift, knot_shift in [3, 8].
 *   lut (B, C, 256) u8, a tone curve per line and channel; null = identity.
 * All arithmetic is integer, in 64 bits (every product is i32 x i32; B, H < 65536, C <= 4, Wt < 2^24 keep every sum below 2^58),
 * >> is the arithmetic shift (floor), clamp(v, a, b) = min(max(v, a), b).  No value of params or knots reads out of bounds.
 * Output byte (b, y, x_out, c) with x = x_out - left_px[b] in [0, w), cy = (H - 1) * 128, xc = w / 2, yr = (y << 8) - cy:
 *   j = clamp(x >> knot_shift, 0, NK - 2), t = x & (K - 1)
 *   dy = (knots[b][0][j] * (K - t) + knots[b][0][j + 1] * t) >> knot_shift;   dx likewise from knots[b][1]
 *   ys = cy + ((yr * sy) >> 8) + ty + slope * (x - xc) + dy
 *   xs = (x << 8) + ((yr * slant) >> 8) + dx
 *   y0 = clamp(ys >> 8, 0, H - 1), y1 = clamp((ys >> 8) + 1, 0, H - 1), x0 = clamp(xs >> 8, 0, w - 1), x1 = clamp((xs >> 8) + 1, 0, w - 1)
 *     (edge replication: no tap leaves the line's own pixels);  fx = xs & 255, fy = ys & 255;  pYX = line b's byte (yY, xX, c)
 *   v = ((p00 * (256 - fx) + p01 * fx) * (256 - fy) + (p10 * (256 - fx) + p11 * fx) * fy + 32768) >> 16
 *   v = lut[b][c][v]
 *   if noise_amp != 0:  i = ((b * H + y) * Wt + x_out) * C + c  (u64: the byte's index in out);
 *     h = fmix32(fmix32((i & 0xffffffff) ^ seed_lo) ^ (i >> 32) ^ seed_hi), where fmix32 is murmur3's 32-bit finaliser on u32:
 *       h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16;
 *     s = (h & 255) + ((h >> 8) & 255) + ((h >> 16) & 255) + (h >> 24) - 510   (Irwin-Hall: mean 0, standard deviation 147.8);
 *     v = clamp(v + ((s * noise_amp + 32768) >> 16), 0, 255)   (noise_amp = 65536 sigma / 147.8 for a standard deviation of sigma)
 * Neutral values - sy = 256, every other column 0, zero knots, identity or null lut - give pero_stack_lines' bytes. */
#define PERO_AUGMENT_PARAMS 7
int pero_augment_stack_lines(const void* packed, const int64_t* offsets, const int32_t* widths, const int32_t* left_px,
                             const int32_t* params, const int32_t* knots, const uint8_t* lut, void* out, int64_t B, int64_t H,
                             int64_t Wt, int64_t C, int64_t P, int64_t knot_shift, void* stream);

/* ---- CTC (fine-tuning a recogniser on a pre-trained backbone; csrc/ctc.hip, DESIGN.md "CTC") -------------------------
 * logits (N*S, C) row-major in `dtype` - the head's own output rows, line n at rows [n S, (n + 1) S); all arithmetic f32.
 * The log-softmax is fused: logp_t(c) = x[n][t][c] - row_lse[n S + t], row_lse = log sum_c exp(x) per row; no (N*S, C) f32
 * log-probability tensor exists.  targets (N, Lmax) int64, padded (entries behind target_lengths[n] are never read);
 * input_lengths, target_lengths (N) int64; every index / length is a DEVICE pointer, nothing synchronises.  Lengths are
 * clamped to [0, S] and [0, Lmax].  blank: any class in [0, C).  Line n with T = input_lengths[n] frames and L =
 * target_lengths[n] labels l_0 .. l_{L-1} has the L' = 2 L + 1 extended states l' = (blank, l_0, blank, l_1, .., blank).
 * A label outside [0, C) emits with probability 0 (the line is infeasible); a label equal to blank counts as blank.
 *
 * pero_ctc_fwd: row_lse (N*S) f32 for every row; alpha (N, S, 2 Lmax + 1) f32, entries [n][t][s] with t < T, s < L' written:
 *   alpha_0(s) = logp_0(l'_s) for s < 2, -inf else;
 *   alpha_t(s) = logp_t(l'_s) + log(exp alpha_{t-1}(s) + exp alpha_{t-1}(s-1) + [l'_s != l'_{s-2}] exp alpha_{t-1}(s-2));
 *   nll[n] = -log(exp alpha_{T-1}(L'-1) + exp alpha_{T-1}(L'-2)), +inf for an infeasible line (T < L + repeats; -inf states
 *   propagate, no NaN).  T = 0: nll = 0 for L = 0, +inf otherwise.
 * pero_ctc_bwd: beta (N, S, 2 Lmax + 1) f32, a caller buffer written here, INCLUDES the emission at t:
 *   beta_{T-1}(s) = logp_{T-1}(l'_s) for s >= L' - 2, -inf else;
 *   beta_t(s) = logp_t(l'_s) + log(exp beta_{t+1}(s) + exp beta_{t+1}(s+1) + [l'_{s+2} != l'_s] exp beta_{t+1}(s+2));
 *   dlogits[n][t][c] = g[n] (exp(logp_t(c)) - sum_{s: l'_s = c} exp(alpha_t(s) + beta_t(s) + nll[n] - logp_t(c)))   in `dtype`,
 *   exact zeros for t >= T, and with zero_infinity != 0 for every row of a line whose nll is not finite (without the flag such
 *   a line's rows are unspecified).  g (N) f32: the upstream scale per line, on the device.  The states of one class are summed in a
 *   fixed order without atomics: two calls give the same bits.  chain: (N, Lmax) int32 scratch written here.
 * pero_ctc_greedy: per row the first maximal class (numpy.argmax; NaN-free input), per line over t < T repeats collapsed, then blanks
 *   dropped: out (N, S) int64 padded with -1, out_lengths (N) int64.
 * Workspaces (caller-owned): row_lse 4 N S bytes; alpha, beta 4 N S (2 Lmax + 1) bytes each; chain 4 N Lmax bytes; nll 4 N.
 * Supported: 2 <= C <= 8192, 1 <= S <= 512, 0 <= Lmax <= 512 (PERO_E_UNSUPPORTED above; Lmax may exceed S, a line with L > T is
 * infeasible), N S < 2^31. */
int pero_ctc_fwd(const void* logits, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths, float* row_lse,
                 float* alpha, float* nll, int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int dtype, void* stream);
int pero_ctc_bwd(const void* logits, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths,
                 const float* row_lse, const float* alpha, const float* nll, const float* g, float* beta, int32_t* chain, void* dlogits,
                 int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int zero_infinity, int dtype, void* stream);
int pero_ctc_greedy(const void* logits, const int64_t* input_lengths, int64_t* out, int64_t* out_lengths, int64_t N, int64_t S, int64_t C,
                    int64_t blank, int dtype, void* stream);

/* ---- CTC decoding and scoring (evaluation of a recogniser; csrc/ctc_decode.hip, pero_edit_distance: csrc/edit.hip; DESIGN.md "CTC decoding")
 * pero_ctc_beam: CTC prefix beam search of width W, one line per workgroup, no class pruning, no language model.  logits,
 * input_lengths, blank, dtype and the clamp of the lengths as for pero_ctc_greedy; all arithmetic f32 in the log domain,
 * logp_t(c) = x[n][t][c] - row_lse[n S + t] (a -inf logit has logp -inf), (+) = log-sum-exp (all -inf -> -inf, never NaN).
 *   A beam entry is a label string p with pb, pnb: the log-probabilities of its alignments ending in blank / in a non-blank.
 *   Before frame 0 the beam is {(): pb = 0, pnb = -inf}.  At frame t < T every entry, with tot = pb (+) pnb and last label e, gives
 *     stay:           p    gets pb' (+)= tot + logp_t(blank), and for p != (): pnb' (+)= pnb + logp_t(e);
 *     extend, c != blank: p+c gets pnb' (+)= logp_t(c) + (c == e ? pb : tot).
 *   Contributions to the same STRING are merged before ranking (a string has one node in the line's trie of prefixes, found or
 *   created through a hash of (parent node, label) that keeps every node ever created: a prefix that left the beam and comes
 *   back gets its old node, so an extension that stayed in the beam still merges with it).  The W candidates with the largest
 *   finite total pb' (+) pnb' are kept, in rank order.
 *   Tie rule (equal f32 totals): the candidates of a frame are numbered - first the strings of the current beam in slot order,
 *   then, for beam slot j = 0, 1, .. in turn, the new strings p_j + c for the row's classes c in the order (logit descending, class
 *   ascending) - and the smaller number ranks first.  Only the first min(W + 1, C - 1) non-blank classes of that order are
 *   candidates; the others cannot reach the best W under this rule.  Nothing depends on timing: two calls give the same bits.
 * Outputs: out (N, W, S) int64 padded with -1; out_lengths (N, W) int64; out_scores (N, W) f32 totals, best first; out_count (N)
 *   int64 <= W.  Slots >= out_count: score -inf, length 0.  T = 0: one hypothesis, the empty string, score 0.
 * Trace (always written; the lattice of the search): node_parent, node_label (N, S W + 1) int32 - node 0 is the empty prefix
 *   (parent, label -1), node k > 0 spells node_parent[k]'s string + node_label[k], parents have smaller numbers, entries
 *   [0, node_count[n]) are written; node_count (N) int32; beam_node (N, S, W) int32: the node in each rank slot after frame
 *   t < T, -1 for an unused slot; beam_score (N, S, W, 2) f32: (pb, pnb) of that slot, (-inf, -inf) if unused.  Rows t >= T are
 *   not written.
 * Workspaces (caller-owned, contents unspecified before and after): row_lse 4 N S bytes; top_logp 4 N S K and top_class 4 N S K
 *   bytes, K = min(W + 1, C - 1); hash 8 N H bytes, H = the smallest power of two >= 2 S W (cleared by the call itself).
 * Supported: 2 <= C <= 8192, 1 <= S <= 512, 1 <= W <= 32 (PERO_E_UNSUPPORTED above), N S < 2^31.
 *
 * pero_ctc_beam_lm: pero_ctc_beam with shallow fusion of a back-off n-gram model over the class ids (the blank is no symbol); DESIGN.md
 * section 15.  Arguments, outputs, trace, workspaces and tie rule of pero_ctc_beam, the same kernel body, and in addition:
 *   The model, a deterministic automaton of M states in flat arrays on the device (read-only for the call).  State 0 is the empty context,
 *   `start` the state before the first label.  Per state s: lm_backoff_state (M) int32 (-1 for state 0), lm_backoff_weight (M) f32,
 *   lm_final (M) f32 = ln p(end | s) with the back-off already resolved (zeros for a model without an end symbol); all logs natural.
 *   Arcs in CSR form: lm_arc_begin (M + 1) int32, and per arc lm_arc_label (A) int32 ascending inside a state, lm_arc_logp (A) f32,
 *   lm_arc_next (A) int32, the state behind the arc.
 *     lookup(s, c):  acc = 0;  while c is no arc of s: acc = acc + lm_backoff_weight[s], s = lm_backoff_state[s];
 *                    lm = acc + lm_arc_logp[arc], next = lm_arc_next[arc]                      f32 additions in exactly this order.
 *   c without an arc in state 0: p + c is NO candidate, whatever the weights are (how a caller forbids a class).  The kernel checks every
 *   index it reads from these arrays against M and A and follows at most PERO_CTC_LM_MAX_ORDER back-off steps; a look-up that fails a check
 *   counts as "no candidate", so malformed tables cannot make it read out of range.
 *   Scores.  pb, pnb of a string carry alpha LM(string) + beta |string| inside them (alpha = lm_weight, beta = length_bonus, both finite).
 *   With w(p, c) = fadd(fmul(alpha, lm(state(p), c)), beta), one f32 multiplication and one f32 addition, never fused:
 *     stay:           p    gets pb' (+)= tot + logp_t(blank), and for p != (): pnb' (+)= pnb + logp_t(e);                       (unchanged)
 *     extend, c != blank: p+c gets pnb' (+)= (logp_t(c) + w(p, c)) + (c == e ? pb : tot),                  the additions in this order,
 *       if p + c is an entry of the current beam (the contribution is part of that entry's stay; every class, as in pero_ctc_beam), or
 *       if c is among the first K non-blank classes of the frame's order (logit descending, class ascending) - a NEW string.
 *   w is a function of the string, so the contributions merged into one string carry the same w.  K is clamped to [1, C - 1].  With a
 *   language model the W + 1 argument of pero_ctc_beam fails (the score of p + c depends on p), so K < C - 1 is a pruning of the new
 *   strings ("cutoff top n"), K = C - 1 the unpruned search.  Candidate numbers for the tie rule: as in pero_ctc_beam with this K.
 *   Nodes.  node_lm_state, node_lm_weight (N, S W + 1) int32 / f32, entries [0, node_count[n]) written: node 0 has (start, 0); the node
 *   of p + c gets (next, w(p, c)) when it is created, and a prefix that comes back into the beam takes both from its node.
 *   node_lm_total[k] = fadd(node_lm_total[parent], node_lm_weight[k]) from the root down (node 0: 0) is the LM part of a string's score.
 *   End of line.  use_final != 0: every hypothesis' total becomes fadd(total, fmul(alpha, lm_final[state])); the <= W hypotheses are
 *   ranked again by these values (equal values: the order of the last frame); the trace's last frame keeps the order before.
 *   out_scores (N, W): these totals, best first.  out_lm (N, W) f32: node_lm_total of the hypothesis, with use_final
 *   fadd(that, fmul(alpha, lm_final[state])); 0 in unused slots.  T = 0: the empty string, score and out_lm 0 (+ alpha lm_final[start]).
 *   With alpha = 0, beta = 0, use_final = 0 and K = min(W + 1, C - 1), w = +0 for finite tables and every output and trace entry that
 *   pero_ctc_beam specifies has pero_ctc_beam's bits (state 0 must hold an arc for every non-blank class).
 * Workspaces as pero_ctc_beam with this K.  Supported: as pero_ctc_beam, and W (K + 1) <= 1088 after the clamp (PERO_E_UNSUPPORTED
 * above: K <= 67 at W = 16, K <= 33 at W = 32), 1 <= M, 0 <= A < 2^31, 0 <= start < M.
 *
 * pero_edit_distance: dist[n] (int64) = the Levenshtein distance (insertion, deletion, substitution: 1 each) of a[n][0, a_len[n])
 * and b[n][0, b_len[n]).  a (N, La), b (N, Lb) int64, padded (entries behind the lengths are never read; a null pointer is
 * allowed for a zero-width matrix); a_len, b_len (N) int64, clamped to [0, La], [0, Lb].  totals (2 int64 on the device, may be
 * null; ACCUMULATED, the caller zeroes them once): totals[0] += sum_n dist[n], totals[1] += sum_n b_len[n] (clamped), by integer
 * atomics: exact in any order.  Integer arithmetic only.  Supported: La, Lb <= 512 (PERO_E_UNSUPPORTED above). */
int pero_ctc_beam(const void* logits, const int64_t* input_lengths, int64_t* out, int64_t* out_lengths, float* out_scores,
                  int64_t* out_count, int32_t* node_parent, int32_t* node_label, int32_t* node_count, int32_t* beam_node,
                  float* beam_score, float* row_lse, float* top_logp, int32_t* top_class, uint64_t* hash, int64_t N, int64_t S, int64_t C,
                  int64_t blank, int64_t W, int dtype, void* stream);
#define PERO_CTC_LM_MAX_ORDER 16   /* back-off steps of one look-up the kernel follows: the longest context + 1 of a model it can walk */
int pero_ctc_beam_lm(const void* logits, const int64_t* input_lengths, const int32_t* lm_backoff_state, const float* lm_backoff_weight,
                     const float* lm_final, const int32_t* lm_arc_begin, const int32_t* lm_arc_label, const float* lm_arc_logp,
                     const int32_t* lm_arc_next, int64_t* out, int64_t* out_lengths, float* out_scores, float* out_lm, int64_t* out_count,
                     int32_t* node_parent, int32_t* node_label, int32_t* node_lm_state, float* node_lm_weight, int32_t* node_count,
                     int32_t* beam_node, float* beam_score, float* row_lse, float* top_logp, int32_t* top_class, uint64_t* hash, int64_t N,
                     int64_t S, int64_t C, int64_t blank, int64_t W, int64_t K, int64_t M, int64_t A, int64_t start, float lm_weight,
                     float length_bonus, int use_final, int dtype, void* stream);
int pero_edit_distance(const int64_t* a, const int64_t* a_len, const int64_t* b, const int64_t* b_len, int64_t* dist, int64_t* totals,
                       int64_t N, int64_t La, int64_t Lb, void* stream);

/* ---- Edit operations (which symbols, or words, were wrong: the backtrace of pero_edit_distance's table; csrc/edit.hip, DESIGN.md
 * "Edit operations") ------------------------------------------------------------------------------------------------------
 * pero_edit_ops: a is the hypothesis, b the reference.  a, a_len, b, b_len, their layout, padding, the clamp of the lengths and the null
 * pointer for a zero-width matrix: as for pero_edit_distance.  With la, lb the clamped lengths of pair n and a_i, b_j its elements
 * (1-based; the labels, or with is_sep the words):
 *   Table.  D(i, j) = pero_edit_distance's table: D(i, 0) = i, D(0, j) = j,
 *     D(i, j) = min(D(i-1, j) + 1, D(i, j-1) + 1, D(i-1, j-1) + [a_i != b_j]).
 *   Script.  Walk from (la, lb) to (0, 0).  At (i, j):
 *     1. if i > 0, j > 0 and D(i-1, j-1) + [a_i != b_j] == D(i, j): go to (i-1, j-1); a HIT (code 0) if a_i == b_j, else a SUBSTITUTION
 *        (code 1);
 *     2. otherwise, if j > 0 and D(i, j-1) + 1 == D(i, j): go to (i, j-1); a DELETION of b_j (code 3);
 *     3. otherwise go to (i-1, j); an INSERTION of a_i (code 2).
 *     This tie rule makes the script unique; it is a minimal script: substitutions + insertions + deletions = D(la, lb),
 *     hits + substitutions + insertions = la, hits + substitutions + deletions = lb.
 *   Outputs (caller-owned, every entry written):
 *     counts (N, 4) int64: substitutions, insertions, deletions, hits of the pair.
 *     script (N, La + Lb) int8 and script_len (N) int32, both null or both given (script may be null for La + Lb = 0: a zero-width
 *       matrix): the codes in FORWARD order (the first element's operation first), script_len <= la + lb of them, -1 behind.
 *   totals (6 int64 on the device, may be null; ACCUMULATED, the caller zeroes them once; integer atomics, exact in any order):
 *     totals[0..3] += the pair's four counts; totals[4] += 1 per pair; totals[5] += 1 per pair with D(la, lb) > 0.
 *   confusion ((C + 1, C + 1) int64 on the device, may be null; ACCUMULATED likewise; symbol level only): a hit or substitution of
 *     reference label r by hypothesis label h: confusion[r][h] += 1; a deletion of r: confusion[r][C] += 1; an insertion of h:
 *     confusion[C][h] += 1.  An operation that involves a label outside [0, C) is counted in counts and totals and skipped here: no
 *     index is formed from it.
 *   Word level (is_sep given: C bytes on the device, non-zero = class c separates words).  A word is a maximal run of labels c with
 *     !(0 <= c < C && is_sep[c]): labels outside [0, C) belong to words; leading, trailing and repeated separators make no empty
 *     words.  Two words are equal iff they have the same length and the same labels, decided by comparing the labels (a hash only
 *     skips unequal words).  Table, script, counts and totals are over the two word sequences (script keeps its width La + Lb).
 *     a_spans (N, (La + 1) / 2, 2), b_spans (N, (Lb + 1) / 2, 2) int32, each may be null: [begin, end) of every word in its row, -1
 *     behind the last word.  confusion must be null (PERO_E_INVALID); without is_sep the spans must be null.
 *   C is read only with confusion or is_sep and must then be >= 1.  Integer arithmetic only; nothing depends on timing: two calls give
 *   the same bits.  Supported: La, Lb <= 512 (PERO_E_UNSUPPORTED above). */
int pero_edit_ops(const int64_t* a, const int64_t* a_len, const int64_t* b, const int64_t* b_len, const uint8_t* is_sep, int64_t* counts,
                  int8_t* script, int32_t* script_len, int32_t* a_spans, int32_t* b_spans, int64_t* totals, int64_t* confusion, int64_t N,
                  int64_t La, int64_t Lb, int64_t C, void* stream);

/* ---- CTC forced alignment (where each character of a known string sits, and how sure the model is of it; csrc/ctc_align.hip,
 * DESIGN.md "CTC forced alignment") ---------------------------------------------------------------------------------------
 * pero_ctc_align: the best state path (Viterbi) of every line's label string.  logits, targets, input_lengths, target_lengths,
 * blank, dtype, the clamp of the lengths, the extended states l' and the treatment of labels outside [0, C) or equal to blank: as
 * for pero_ctc_fwd.  x_t(c) = the logit converted to f32.  The best path does not depend on a frame's log-sum-exp, so the recursion
 * runs on RAW logits and holds f32 additions and comparisons only:
 *   v_0(s) = x_0(l'_s) for s < 2, -inf else;
 *   v_t(s) = x_t(l'_s) + max(v_{t-1}(s), v_{t-1}(s-1), [l'_s != l'_{s-2}] v_{t-1}(s-2))          one f32 addition per state and frame;
 *   back_t(s) in {0, 1, 2}: the step of the winning predecessor; equal values -> the SMALLEST step; all -inf -> 0;
 *   end state: L'-1 if v_{T-1}(L'-1) >= v_{T-1}(L'-2), else L'-2 (L = 0: state 0); the path follows back_t from there to frame 0;
 *   the line is feasible iff that v is finite.  T = 0: feasible iff L = 0, path_logit = score = 0.
 *   Tie rule in words: among the paths with the best f32 value, the one whose state sequence is lexicographically LARGEST when read
 *   from the last frame back to the first (it advances as early as it can).  The library is built without fused multiply-adds, so
 *   a float32 restatement of these formulas gives the same bits for every input.
 * Outputs (caller-owned, every entry written):
 *   states (N, S) int32: the extended-state index at frame t < T; -1 for t >= T and for every frame of an infeasible line.
 *   spans (N, Lmax, 2) int32: [first frame, last frame + 1) of label k's state 2 k + 1 (a feasible line gives every label at least
 *     one frame); -1 for k >= L and for infeasible lines.
 *   path_logit (N) f32: v_{T-1}(end) = the path's logits added in frame order; -inf for an infeasible line.
 *   score (N) f32: the path's log-probability, path_logit - sum_{t < T} lse_t, with lse_t = max + log sum_c exp(x_t(c) - max) (the
 *     kernel of pero_ctc_fwd's row_lse, run here for the rows t < T: the same bits) added in frame order; -inf for an infeasible line.
 *   label_logp (N, Lmax) f32: sum_{t in span k} (x_t(l_k) - lse_t), added in frame order; 0 for k >= L and for infeasible lines.
 * No float atomics, nothing depends on timing: two calls give the same bits.  Rows t >= T and targets behind L are never read.
 * Workspaces (caller-owned, contents unspecified before and after): row_lse 4 N S bytes; back N S (2 Lmax + 1) bytes, one
 *   backpointer byte per (t, s).  When S (2 Lmax + 1) <= PERO_CTC_ALIGN_LDS_BACK_BYTES (host-known sizes only) the backpointers stay
 *   in LDS and `back` is not touched; flags = PERO_CTC_ALIGN_GLOBAL_BACK forces the workspace (for measurements; the results are the
 *   same bits).  `back` is required either way.
 * Supported: 2 <= C <= 8192, 1 <= S <= 512, 0 <= Lmax <= 512 (PERO_E_UNSUPPORTED above; Lmax may exceed S), N S < 2^31. */
#define PERO_CTC_ALIGN_LDS_BACK_BYTES (96 * 1024)
#define PERO_CTC_ALIGN_GLOBAL_BACK 1
int pero_ctc_align(const void* logits, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths,
                   int32_t* states, int32_t* spans, float* path_logit, float* score, float* label_logp, float* row_lse, void* back,
                   int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int flags, int dtype, void* stream);

/* ---- Retrieval (evaluation of the joint-embedding model: does a position of one view find its twin in the other?  csrc/retrieval.hip,
 * DESIGN.md "Retrieval").  The reference looks at this by eye (joint_embedding_pretraining/visualizer.py:63-97: normalise, the full
 * similarity matrix, torch.topk).
 *
 * pero_sim_topk: q (M, D) and keys (N, D) of `dtype`, row pitches ldq, ldk in elements;
 *   score[m][n] = ((q_m . key_n) * q_scale[m]) * key_scale[n]
 * the dot accumulated in f32 on the MFMA units, the two multiplications in f32 in this order.  q_scale (M) and key_scale (N) are f32 and
 * may be null = 1 (the multiplication by 1 is exact: null and a vector of ones give the same bits).  With pero_inv_rownorm's values (or the `inv` of
 * pero_rownorm_fwd) as scales the score is the cosine; no normalised copy of the rows is written, and the (M, N) score matrix is never stored.
 * Outputs idx (M, k) int32 and val (M, k) f32, every element written: the k best keys of query m under this STRICT order -
 *   higher score first;  equal f32 scores: lower key index first
 * - among the keys that qualify.  A key never enters a list when key_valid[n] == 0 (u8 (N), may be null = all valid), when
 * n == skip[m] (int32 (M), may be null; self-retrieval, where queries and keys are the same rows), or when its score is NaN
 * (+-inf scores qualify).  If fewer than k keys qualify the remaining slots are idx = -1, val = -inf.
 * Because the order is strict the result depends neither on the number of key splits nor on anything else about how the keys are
 * visited; no float atomics: two calls give the same bits.
 * Key splits: the grid is (ceil(M / 64) query tiles, key_splits); split s takes the 128-key tiles [T s / S, T (s + 1) / S) of the
 * T = ceil(N / 128) (a split may be empty), writes its lists to `work`, and a second kernel merges them.  0 <= key_splits <= 128;
 * key_splits = 0 chooses pero_sim_topk_key_splits(M, N) = max(1, min(ceil(512 / ceil(M / 64)), ceil(N / 128), 128)): two workgroups for
 * each CU of a 256-CU device where the query tiles alone do not give them, never less than one key tile per split (returns the count,
 * not a status; a function of M and N alone).
 * work: at least 8 * S * M * k bytes for S splits in effect (S * M * k f32 scores, then as many int32 indices); may be null for S = 1.
 * 1 <= k <= PERO_SIM_TOPK_MAX; M, N >= 1; D % 8 == 0; q, keys and both pitches in bytes multiples of 16, pitches >= D: anything else
 * is PERO_E_INVALID, checked on the host before any launch.
 *
 * pero_retrieval_hist: idx (M, k) int32 as written by pero_sim_topk, target (M) int32: the key index of query m's twin, -1 for none.
 * hist (u64 [k + 2], ACCUMULATED: the caller zeroes it once per test()):  hist[0] += #{m : target[m] >= 0};  hist[1 + r] += #{m :
 * target[m] >= 0 and idx[m][r] == target[m]} (the first such r);  hist[k + 1] += #{m : target[m] >= 0 and not in idx[m][0..k)}.
 * recall@j = sum(hist[1..j]) / hist[0];  MRR@k = sum_r hist[1 + r] / (r + 1) / hist[0].  Integer atomics only.  M = 0 is a no-op.
 *
 * pero_inv_rownorm: inv[r] (f32) = 1 / max(sqrt(sum_c x[r][c]^2), 1e-12), the sum in f32 (pero_rownorm_fwd's `inv` without its normalised
 * copy, and with a row pitch): the scales that make pero_sim_topk's score the cosine.  x (rows, D) of `dtype`, pitch ld in elements;
 * D % 8 == 0 and 16-byte aligned rows as for pero_sim_topk. */
#define PERO_SIM_TOPK_MAX 16
int pero_inv_rownorm(const void* x, int64_t ld, float* inv, int64_t rows, int64_t D, int dtype, void* stream);
int pero_sim_topk_key_splits(int64_t M, int64_t N);
int pero_sim_topk(const void* q, int64_t ldq, const void* keys, int64_t ldk, const float* q_scale, const float* key_scale,
                  const unsigned char* key_valid, const int32_t* skip, int32_t* idx, float* val, void* work, int64_t M, int64_t N, int64_t D,
                  int32_t k, int32_t key_splits, int dtype, void* stream);
int pero_retrieval_hist(const int32_t* idx, const int32_t* target, uint64_t* hist, int64_t M, int32_t k, void* stream);

/* ---- latent-target self-distillation: EMA teacher, normalised layer-averaged targets, regression loss (csrc/latent.hip) --------------
 * The reference has no counterpart (it predicts discrete labels); tests/latent_ref.py restates these formulas in f64.  No float atomics:
 * every addition has a fixed place, so the same inputs give the same bits from run to run.  All HBM-bound.
 *
 * pero_ema_update: the weight average of a whole model in one launch.  table (DEVICE, int64[n_segments][4]) = {source address, destination
 * offset, count, first tile}: segment s averages `count` f32 values at the device ADDRESS table[s][0] (any 4-byte alignment, any
 * allocation) into avg[offset .. offset + count).  Every segment is cut into ceil(count / PERO_LAYER_TILE) tiles that start AT the segment,
 * the last one possibly short; first tile = the tiles of the segments in front, total_tiles = the sum.  Offsets are multiples of 8 elements
 * (16-byte aligned f32 and bf16 pieces: optim.FusedAdam's layout), count >= 1; the library cannot read the table on the host, so the
 * caller vouches for it.  One workgroup of 256 lanes per tile, lane t holding the four 16-byte pieces at elements (k * 256 + t) * 4; a
 * tile whose source is not 16-byte aligned reads it by scalar loads (a branch per workgroup).  Per element, in f32, in this order:
 *   a = a + w * (p - a),  w = (float)(1 - tau) formed by the caller in f64 and rounded once
 * avg_bf16 (may be null; the layout of avg) <- round-to-nearest-even(a) in the same launch.  Elements of avg between the segments (the
 * padding to 8) are neither read nor written.
 *
 * pero_latent_targets: mats = HOST array of K DEVICE pointers (the one host pointer of this header: read during the call, the addresses
 * travel in the kernel's arguments), 1 <= K <= PERO_LATENT_MAX_K matrices (rows, d) of `dtype`, contiguous; index (n) int64, unique rows;
 * y f32 (n_pad, d), n_pad >= n.  For i < n, r = index[i], for every matrix t_k (all statistics in f32):
 *   mu = (sum_j t_k[r][j]) / d ;  var = (sum_j (t_k[r][j] - mu)^2) / d ;  rs = 1 / sqrt(var + eps) ;  xhat_k[j] = (t_k[r][j] - mu) * rs
 *   y[i][j] = (xhat_0[j] + xhat_1[j] + ... + xhat_{K-1}[j]) * (float)(1 / K)          (added in the order k = 0 .. K - 1)
 * Rows n <= i < n_pad are exact zeros; a row with an index outside [0, rows) is NaN (nothing is read for it).  One 64-lane wave per row
 * holds the row in registers, so each row of each matrix is read exactly once.  Order of the two row sums: lane l adds its elements in
 * ascending column order - columns (c * 64 + l) * 4 .. + 3 for c = 0, 1, .. - then the 64 lanes by a butterfly (xor 32, 16, .. 1).
 * Supported widths: d % 4 == 0, 4 <= d <= PERO_LATENT_MAX_D, every matrix 16-byte aligned; anything else is PERO_E_INVALID, checked on
 * the host before any launch (no scalar path for other widths).
 *
 * pero_latent_loss_fwd / _bwd: pred (n_pad, d) of `dtype`, y f32 (n_pad, d), rows i < n count.  e = pred - y in f32;
 *   beta > 0:  l(e) = ((0.5 * e) * e) / beta  if |e| < beta,  else |e| - 0.5 * beta         (torch smooth_l1_loss)
 *   beta == 0: l(e) = e * e                                                                   (MSE)
 *   loss[0] = (float)((sum_{i < n} rowsum[i]) / ((double)n * d)),  rowsum[i] = sum_j l(e[i][j]) in f32
 * rowsum (work, f32 [n]): one wave per row, lane l adding columns (c * 64 + l) * 4 .. + 3 for c = 0, 1, .. in ascending order, then the
 * butterfly; the finishing pass is one workgroup adding rowsum in f64 in index order (256 contiguous runs, then the run sums).  n = 0
 * gives NaN (0 / 0), as a mean over nothing does.
 *   dpred[i][j] = g * l'(e),  g = dloss[0] * (float)(1 / ((double)n * d)) in f32;  l'(e) = e / beta if |e| < beta else sign(e);  MSE: 2 * e
 * written in pred's dtype; rows n <= i < n_pad are exact zeros.  dloss: DEVICE pointer to one f32 (null = 1).  d % 4 == 0, d >= 4,
 * pred / y / dpred 16-byte aligned, beta >= 0: anything else is PERO_E_INVALID. */
#define PERO_LATENT_MAX_K 16
#define PERO_LATENT_MAX_D 4096
int pero_ema_update(float* avg, void* avg_bf16, const int64_t* table, int64_t n_segments, int64_t total_tiles, float w, void* stream);
int pero_latent_targets(const void** mats, int64_t K, const int64_t* index, float* y, int64_t rows, int64_t n, int64_t n_pad, int64_t d,
                        float eps, int dtype, void* stream);
int pero_latent_loss_fwd(const void* pred, const float* y, float* work, float* loss, int64_t n, int64_t d, float beta, int dtype,
                         void* stream);
int pero_latent_loss_bwd(const void* pred, const float* y, const float* dloss, void* dpred, int64_t n, int64_t n_pad, int64_t d, float beta,
                         int dtype, void* stream);

/* ---- Barlow Twins loss (csrc/barlow.hip; BarlowTwinsLoss) -----------------------------------------------
 * z1[r] = x[ix[r]], z2[r] = y[iy[r]], r < n: the n paired rows of the two views (x, y: rows of d values of `dtype`; ix, iy: DEVICE int64
 * lists, unique within a list).  Per view and column j: mu_j = mean_r z[r][j], var_j = mean_r (z[r][j] - mu_j)^2 (biased),
 * rstd_j = 1 / sqrt(var_j + eps), zh[r][j] = (z[r][j] - mu_j) * rstd_j.  With c = zh1^T zh2 / n (the caller's pero_gemm):
 *   on = sum_i (c_ii - 1)^2,  off = sum_{i != j} c_ij^2,  loss = on + lambda * off,  G_ii = 2 (c_ii - 1) / n,  G_ij = 2 lambda c_ij / n,
 * d zh1 = zh2 G^T, d zh2 = zh1 G (pero_gemm again), and per view with a_j = sum_r dzh[r][j], b_j = sum_r dzh[r][j] zh[r][j]:
 *   dz[r][j] = g * rstd_j * (dzh[r][j] - a_j / n - zh[r][j] * b_j / n).
 * Every per-view array holds view 1 then view 2: mean, rstd, a, b are f32 [2][d]; zh, dzh are `dtype` [2][n_pad][d], n_pad >= n.
 * No atomics: the column reductions leave one partial per column and tile of PERO_BARLOW_TILE_ROWS rows, merged in tile order in
 * f64 ((count, mean, M2) partials and the parallel-variance formula for the statistics), so a second call gives the same bits.
 * part: f32 workspace of PERO_BARLOW_PART(n, d) values.  16-byte accesses when d % 8 == 0 and every row is 16-byte aligned, element
 * by element otherwise; 1 <= d <= 65535 * 256.
 *
 * pero_barlow_stats           mean, rstd of both views in one pass over the gathered rows
 * pero_barlow_standardize     zh, rows n <= r < n_pad explicit zeros (every element of zh is written)
 * pero_barlow_corr            one read of c (f32 d x d): out = {loss, on, off} and G (`dtype`, d x d); rowpart: f32 [2][d] scratch
 * pero_barlow_bwd_stats       a, b of both views in one pass over dzh and zh
 * pero_barlow_standardize_bwd dz STORED to dx[ix[r]] / dy[iy[r]] (other rows untouched); g: DEVICE pointer to one f32 (null = 1) */
#define PERO_BARLOW_TILE_ROWS 1024
#define PERO_BARLOW_PART(n, d) (4 * (((n) + PERO_BARLOW_TILE_ROWS - 1) / PERO_BARLOW_TILE_ROWS) * (d))
int pero_barlow_stats(const void* x, const int64_t* ix, const void* y, const int64_t* iy, float* part, float* mean, float* rstd,
                      int64_t n, int64_t d, float eps, int dtype, void* stream);
int pero_barlow_standardize(const void* x, const int64_t* ix, const void* y, const int64_t* iy, const float* mean, const float* rstd,
                            void* zh, int64_t n, int64_t n_pad, int64_t d, int dtype, void* stream);
int pero_barlow_corr(const float* c, void* G, float* rowpart, float* out, int64_t d, int64_t n, float lambda, int dtype, void* stream);
int pero_barlow_bwd_stats(const void* dzh, const void* zh, float* part, float* a, float* b, int64_t n, int64_t n_pad, int64_t d,
                          int dtype, void* stream);
int pero_barlow_standardize_bwd(const void* dzh, const void* zh, const float* rstd, const float* a, const float* b, const int64_t* ix,
                                const int64_t* iy, void* dx, void* dy, const float* g, int64_t n, int64_t n_pad, int64_t d, int dtype,
                                void* stream);

/* ---- VGG tokenizer front end (csrc/conv.hip; models/autoencoders.py VGGEncoder) ---------------------------
 * Halo layout: an activation of N images, H x W pixels, C channels is stored NHWC with a one-pixel border, (N, H + 2, W + 2, C) values
 * of `dtype`, and read as R = N (H + 2)(W + 2) rows of C.  Border ("halo") pixels hold zeros: they are the convolution's padding.
 * Every entry point below WRITES the zeros of its output's halo; none reads or writes outside the N (H + 2)(W + 2) C values of a
 * buffer: loads are guarded, so PERO_CONV_SLACK_ROWS, the spare rows a caller has to leave in front of and behind a buffer, is 0.
 *
 * pero_conv3x3       Conv2d(Cin -> Cout, kernel 3, stride 1, padding 1) + bias + activation.  x: halo layout with Cin channels;
 *                    w: the weight REPACKED to [Cout][ky][kx][Cin] (`dtype`); bias: f32 [Cout] or null; y: halo layout with Cout channels:
 *                      y[r][co] = act(sum_{ky, kx, ci} x[r + (ky - 1)(W + 2) + (kx - 1)][ci] * w[co][ky][kx][ci] + bias[co])   interior rows r
 *                      y[r][co] = 0                                                                                        halo rows r
 *                    act: PERO_CONV_ACT_NONE, _RELU (max(v, 0)), _LEAKY_RELU (v > 0 ? v : v * slope).  f32 accumulation in a fixed order,
 *                    one rounding of the output.  128-row tiles on the matrix pipe when Cin is a multiple of 8 (PERO_BF16:
 *                    v_mfma_f32_32x32x16_bf16) or of 4 (PERO_F32: v_mfma_f32_32x32x2_f32, exact f32 products and sums, no sum of more than
 *                    a tap's terms in one chain); other channel counts take a plain FMA kernel (exact f32 as well, no speed target) - so
 *                    the caller pads the first layer's 3 channels with zeros (pero_image_to_halo's C_pad; zero weights behind them).
 *                    Any N, H, W, Cin, Cout >= 1.  x, w, y 16-byte aligned, y != x.  The im2col matrix is never formed.
 * pero_image_to_halo src -> dst (halo layout, C_pad >= C channels, the channels C .. C_pad - 1 zeros).  PERO_IMAGE_U8_NHWC: uint8
 *                    (N, H, W, C), dst = value / 255 (the f64 quotient rounded once to f32, then to `dtype`).  PERO_IMAGE_F32_NCHW:
 *                    f32 (N, C, H, W), dst = value.  One 16-byte store per pixel when C_pad values are 16 bytes.
 * pero_maxpool_nhwc  MaxPool2d(kernel = stride = (ph, pw)), ph, pw in {1, 2}, H % ph == 0, W % pw == 0, over the interior of x (halo
 *                    layout, C channels), then, where a and b (f32 [C]) are given, y = max * a[c] + b[c] (an eval-mode BatchNorm2d; a may be
 *                    negative, so it is applied after the maximum).  token_rows 0: y in halo layout (N, H / ph + 2, W / pw + 2, C).
 *                    token_rows 1: y (N * W / pw, (H / ph) * C): row n * (W / pw) + xo holds that column's H / ph pixels top to bottom - the A
 *                    operand of the (h, 1) aggregation convolution as one pero_gemm with K = h * C.  16-byte accesses when C % 8 == 0. */
#define PERO_CONV_SLACK_ROWS 0
#define PERO_CONV_ACT_NONE 0
#define PERO_CONV_ACT_RELU 1
#define PERO_CONV_ACT_LEAKY_RELU 2
#define PERO_IMAGE_U8_NHWC 0
#define PERO_IMAGE_F32_NCHW 1
int pero_conv3x3(const void* x, const void* w, const float* bias, void* y, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                 int act, float slope, int dtype, void* stream);
int pero_image_to_halo(const void* src, void* dst, int64_t N, int64_t H, int64_t W, int64_t C, int64_t C_pad, int src_kind, int dtype,
                       void* stream);
int pero_maxpool_nhwc(const void* x, void* y, const float* a, const float* b, int64_t N, int64_t H, int64_t W, int64_t C, int ph, int pw,
                      int token_rows, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
