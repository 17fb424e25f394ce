// What the attention kernel families share: the forward (attention_fwd.hip) and the tiled backward (attention_bwd.hip) at head_dim 128; the
// head_dim-64 kernels (attention_hd64.hip) take the key ranges, the block map and the bias reduction from here.  Fused multi-head attention for the encoder layers (torch SDPA inside
// TransformerEncoderLayer._sa_block, reference models/transformers.py:36-43,86): softmax(q k^T / sqrt(hd)) v over all S keys of a line - or,
// opt-in, over one interval of keys per line (KEYS: "Per-line key ranges" below); bf16, head_dim 128, any S >= 1, operating directly on the packed qkv (N*S, 3d) tensor.
// Each kernel has ONE body (attn_fwd_p_body, attn_bwd_dq_body_p, attn_bwd_dkv2_body_p: software-pipelined operand reads, below) in up to three
// instantiations: full tiles, RAGGED, and RAGGED with KEYS.
// Ragged S (S % 128 != 0): a line has nb = ceil(S / 128) query blocks and key tiles, the last one with S - 128 (nb - 1) rows.  The launchers then
// start the RAGGED = true instantiations under three rules: (1) every row index that feeds a global address is clamped to
// the line's last row (the LDS-DMA source rows here, the Q / dO / O / lse / D reads in the bodies), so a tail row holds a copy of a real row and
// every MFMA operand is finite; (2) P is SELECTED to 0 wherever the key >= S or the query >= S; (3) every row store is guarded by row < S.
// S % 128 == 0 starts RAGGED = false: no clamp, no select, no guard.
// In this header: the AT_* sizes; the LDS-DMA tile loaders and the fragment reads of the forward's K and V images and of the backward's
// dual-use image (img_f); the workgroup -> ((line, head), block) map; the software-pipelining helpers (at_*: operand reads by inline asm, each
// MFMA tied to a counted lgkmcnt; the forward's asm vector-memory and LDS wrappers); the reduction of the bias gradient's partial rows; the
// declarations of attention_hd64.hip's launchers.
#pragma once
#include "common.hpp"
#include "options.hpp"
#include <type_traits>

#define AT_TILE_BYTES (128 * 128 * 2)  // 32 KiB: 128 keys x 128 head-dim bf16
#define AT_HALF_BYTES 16384   // 64 rows x 256 B
#define AT_SUB_BYTES 8192     // 32 rows x 256 B
#define AT_DKV2_LDS (4 * AT_SUB_BYTES + 128 * 128 * 2 + 512)  // Q / dO stages x 2, V tile, row statistics x 2
#define AT_PRIO(n_) __builtin_amdgcn_s_setprio(n_)
typedef short s8v __attribute__((ext_vector_type(8)));

// ---- LDS-DMA tile loaders.  An image is rows of 256 B (128 head-dim bf16) in pieces of 1 KiB: piece p = rows 4p..4p+3, filled by ONE
// global_load_lds of 16 bytes per lane, lane -> (row 4p + (lane >> 4), 16-byte slot lane & 15); wave w of the four takes pieces w, w + 4, ...
// LDS is filled lane-linearly, so the swizzle sits on the SOURCE address: slot `slot` of a row receives the row's chunk
//   K image (forward):         slot ^ (row & 15)                              conflict-free ds_read_b128 row reads
//   V image (forward):         64-byte block index ^ (row & 3)                conflict-free transposed reads (ds_read_b64_tr_b16)
//   dual-use image (backward): slot ^ img_f(row), img_f = ((row&3)<<2)|((row>>2)&3)   conflict-free for both kinds of read, so K (dQ bodies)
//                              and Q, dO (dK / dV bodies) are staged once
// RAGGED: LDS row `row` receives source row min(row, lim.last), lim.last = the last row of the line counted from g (>= 0): the source address is per
// lane, the swizzle stays that of the LDS row.
// a whole 128 x 128 tile (pieces 0..31) of the forward's K (VIMG = false) or V (true) image
// The limit's type has a default only in the full-tile form, which ignores it: a ragged call without a limit does not compile.
struct at_no_limit { __device__ constexpr at_no_limit(int = 0) {} };
struct at_row_limit { int last; __device__ constexpr at_row_limit(int l) : last(l) {} };
template <bool RAGGED> using at_limit = std::conditional_t<RAGGED, at_row_limit, at_no_limit>;
template <bool VIMG, bool RAGGED = false>
__device__ __forceinline__ void attn_glds_tile(const bf16raw* g, long long ld, unsigned char* lds, int wave, int lane, at_limit<RAGGED> lim = {}) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int p = wave + 4 * i;
    const int row = 4 * p + (lane >> 4), slot = lane & 15;
    const int chunk = VIMG ? ((((slot >> 2) ^ (row & 3)) << 2) | (slot & 3)) : (slot ^ (row & 15));
    int srow = row;
    if constexpr (RAGGED) srow = row < lim.last ? row : lim.last;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + (long long)srow * ld + chunk * 8),
                                     (__attribute__((address_space(3))) void*)(lds + p * 1024), 16, 0, 0);
  }
}
__device__ __forceinline__ int img_f(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
// NP pieces per wave of the dual-use image: 8 = a 128-row tile (32 KiB), 4 = a 64-row half (16 KiB), 2 = a 32-row stage (8 KiB)
template <int NP, bool RAGGED = false>
__device__ __forceinline__ void attn_glds_img(const bf16raw* g, long long ld, unsigned char* lds, int wave, int lane, at_limit<RAGGED> lim = {}) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    const int p = wave + 4 * i;
    const int row = 4 * p + (lane >> 4), slot = lane & 15;
    const int chunk = slot ^ img_f(row);
    int srow = row;
    if constexpr (RAGGED) srow = row < lim.last ? row : lim.last;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + (long long)srow * ld + chunk * 8),
                                     (__attribute__((address_space(3))) void*)(lds + p * 1024), 16, 0, 0);
  }
}

// ---- fragment reads of the forward's images
__device__ __forceinline__ bf8v attn_k_frag(const unsigned char* kimg, int key, int ks, int h5) {
  const int chunk = 2 * ks + h5;
  return *(const bf8v*)(kimg + key * 256 + ((chunk ^ (key & 15)) << 4));
}
// A operand of O^T += V^T P^T for k-step (kb .. kb+15) and d-tile dt: element j <- V[kb + 8(j>>2) + 4h + (j&3)][dt*32 + (lane&31)]
__device__ __forceinline__ bf8v attn_vT_frag(const unsigned char* vimg, int kb, int dt, int lane) {
  const int i = lane & 15, g1 = (lane >> 4) & 1, h5 = lane >> 5;
  const int key = kb + 4 * h5 + (i >> 2);  // (key & 3) == (i >> 2) for both reads (kb, 4*h5, +8 are multiples of 4)
  const unsigned char* a = vimg + key * 256 + ((dt ^ (key & 3)) << 6) + g1 * 32 + (i & 3) * 8;
  s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s4v, a));
  s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s4v, a + 8 * 256));
  s8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf8v, v);
}
__device__ __forceinline__ bf8v pack8(const f16v& a, int s) {
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  u4v u = {pack2bf(a[8 * s + 0], a[8 * s + 1]), pack2bf(a[8 * s + 2], a[8 * s + 3]), pack2bf(a[8 * s + 4], a[8 * s + 5]),
           pack2bf(a[8 * s + 6], a[8 * s + 7])};
  return __builtin_bit_cast(bf8v, u);
}

// ---- fragment reads of the dual-use image
// A operand, row-wise: lane holds M[row][16*ks + 8*h5 .. +8]
__device__ __forceinline__ bf8v img_row_frag(const unsigned char* img, int row, int ks, int h5) {
  return *(const bf8v*)(img + row * 256 + (((2 * ks + h5) ^ img_f(row)) << 4));
}
// A operand, transposed: element j <- M[rb + 8(j>>2) + 4h + (j&3)][dt*32 + (lane&31)]   (rb multiple of 16)
__device__ __forceinline__ bf8v img_tr_frag(const unsigned char* img, int rb, int dt, int lane) {
  const int i = lane & 15, g1 = (lane >> 4) & 1, h5 = lane >> 5;
  const int row = rb + 4 * h5 + (i >> 2);
  const int ch = 4 * dt + 2 * g1 + ((i & 3) >> 1);
  const unsigned char* a = img + row * 256 + ((ch ^ img_f(row)) << 4) + 8 * (i & 1);
  // second read: row + 8 -> (row&3) unchanged, (row>>2)&3 flips bit 1: f(row+8) = f(row) ^ 2
  const unsigned char* b = img + (row + 8) * 256 + ((ch ^ img_f(row + 8)) << 4) + 8 * (i & 1);
  s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s4v, a));
  s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s4v, b));
  s8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf8v, v);
}

// ---- Per-line key ranges (pero_attention_fwd_keys / pero_attention_bwd_keys): line b attends to the keys [k0, k1) of key_ranges[b] only.  Rule (2) of
// the header comment then reads "P is selected to 0 wherever the key is outside [k0, k1)" - k1 <= S covers the keys >= S - and the key walks
// (forward: 128-key tiles, dQ: 64-key halves) visit only the tiles that intersect the range; rules (1) and (3) stay.  Nothing on the host reads
// the ranges, so the kernels make a bad one harmless: k0 is clamped into [0, S - 1], k1 into [k0 + 1, S] - an empty range means "the key k0".
struct at_key_range { int k0, k1; };
__device__ __forceinline__ at_key_range at_load_key_range(const int* kr, int line, int S) {
  int k0 = kr[2 * line], k1 = kr[2 * line + 1];   // uniform per workgroup: scalar loads
  k0 = k0 < 0 ? 0 : (k0 > S - 1 ? S - 1 : k0);
  k1 = k1 < k0 + 1 ? k0 + 1 : (k1 > S ? S : k1);
  return {k0, k1};
}

// Workgroup -> ((line, head), block) so that the blocks of one (line, head) - which read the same K / V (or Q / dO) rows -
// run on ONE XCD, next to each other in dispatch order (hardware places workgroup b on XCD b & 7): the second reader then
// hits that XCD's L2 instead of fetching the rows again through the fabric.  Needs (lines x heads) % 8 == 0.
__device__ __forceinline__ void attn_block_map(int bid, int nblk, int nlh, int& lh, int& blk) {
  if ((nlh & 7) == 0) {
    const int xcd = bid & 7, u = bid >> 3;
    lh = (u / nblk) * 8 + xcd;
    blk = u % nblk;
  } else {
    lh = bid / nblk;
    blk = bid % nblk;
  }
}

// ---- Software-pipelined operand reads.  hipcc compiles the same loops written with plain LDS reads (the head_dim-64 kernels still are; the
// head_dim-128 forms of that kind were retired) to  read -> s_waitcnt
// lgkmcnt(0) -> MFMA  pairs - one LDS round trip exposed per one or two 32-cycle MFMAs - and, worse, puts an `s_waitcnt vmcnt(0)` in front of
// the first LDS read that follows an LDS-DMA (it cannot tell the DMA's destination from the tile being read), which makes the "prefetch" of
// the next tile a wait in the middle of the current one (an ablation build: the loop's DMA cost 24 % of the backward).  The bodies
// (attn_fwd_p_body, attn_bwd_dq_body_p, attn_bwd_dkv2_body_p) issue every fragment read by inline asm the compiler neither waits
// for nor orders, up to SEVEN fragments ahead of the MFMA that consumes them, each MFMA tied to a counted `s_waitcnt lgkmcnt(n)` through its
// fragment register (LDS operations retire in order, so n = the LDS instructions issued after the fragment's own).  One sequence of reads runs
// through a whole LDS stage: the transposed fragments of the gradient products are in flight while the exponentials run, the next sub-tile's
// row fragments while the gradient products run.  Same MFMAs in the same order as the plain loops.
template <int I, int N, typename F>
__device__ __forceinline__ void at_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    at_static_for<I + 1, N>(f);
  }
}
typedef int at_i2v __attribute__((ext_vector_type(2)));
typedef unsigned at_u2v __attribute__((ext_vector_type(2)));
typedef unsigned at_u4v __attribute__((ext_vector_type(4)));
typedef int at_i4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned at_lds_addr(const void* p) { return (unsigned)(unsigned long long)LDS_PTR(const unsigned char, p); }
// address = per-lane offset (a loop-invariant VGPR) + uniform base (an SGPR: the LDS stage), added right in front of the read: the
// compiler otherwise hoists every (stage + offset) sum out of the loops into its own VGPR and spills (20-80 registers in these bodies)
template <int OFF, typename T>
__device__ __forceinline__ void at_rd128(T& d, unsigned lane_off, unsigned base) {
  static_assert(sizeof(T) == 16, "ds_read_b128");
  unsigned a;
  asm volatile("v_add_u32 %1, %3, %2\n\tds_read_b128 %0, %1 offset:%4" : "=v"(d), "=&v"(a) : "v"(lane_off), "s"(base), "i"(OFF) : "memory");
}
// one transposed fragment = two ds_read_b64_tr_b16 (rows x and x + 8 of the image), joined without register copies
template <int OFFA, int OFFB>
__device__ __forceinline__ void at_rdtr(bf8v& d, unsigned off_a, unsigned off_b, unsigned base) {
  at_i2v lo, hi;
  unsigned a, b;
  asm volatile("v_add_u32 %2, %6, %4\n\tv_add_u32 %3, %6, %5\n\tds_read_b64_tr_b16 %0, %2 offset:%7\n\tds_read_b64_tr_b16 %1, %3 offset:%8"
               : "=&v"(lo), "=&v"(hi), "=&v"(a), "=&v"(b) : "v"(off_a), "v"(off_b), "s"(base), "i"(OFFA), "i"(OFFB) : "memory");
  d = __builtin_bit_cast(bf8v, __builtin_shufflevector(lo, hi, 0, 1, 2, 3));
}
// plain forms: the complete LDS address in a register
template <int OFF, typename T>
__device__ __forceinline__ void at_rd128a(T& d, unsigned addr) {
  static_assert(sizeof(T) == 16, "ds_read_b128");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF) : "memory");
}
template <int OFFA, int OFFB>
__device__ __forceinline__ void at_rdtra(bf8v& d, unsigned addr_a, unsigned addr_b) {
  at_i2v lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%4\n\tds_read_b64_tr_b16 %1, %3 offset:%5"
               : "=&v"(lo), "=&v"(hi) : "v"(addr_a), "v"(addr_b), "i"(OFFA), "i"(OFFB) : "memory");
  d = __builtin_bit_cast(bf8v, __builtin_shufflevector(lo, hi, 0, 1, 2, 3));
}
// the same with the per-lane offset XORed by a compile-time constant first: the swizzled fragment offsets of one lane differ from
// each other only by such a constant (k-step: 32 * ks, head-dim tile: 64 * dt), so ONE register per fragment kind serves all of them
template <int OFF, int KX, typename T>
__device__ __forceinline__ void at_rd128x(T& d, unsigned lane_off, unsigned base) {
  static_assert(sizeof(T) == 16, "ds_read_b128");
  unsigned a;
  asm volatile("v_xor_b32 %1, %4, %2\n\tv_add_u32 %1, %3, %1\n\tds_read_b128 %0, %1 offset:%5" : "=v"(d), "=&v"(a) : "v"(lane_off), "s"(base), "i"(KX), "i"(OFF) : "memory");
}
template <int OFFA, int OFFB, int KX>
__device__ __forceinline__ void at_rdtrx(bf8v& d, unsigned off_a, unsigned off_b, unsigned base) {
  at_i2v lo, hi;
  unsigned a, b;
  asm volatile("v_xor_b32 %2, %7, %4\n\tv_xor_b32 %3, %7, %5\n\tv_add_u32 %2, %6, %2\n\tv_add_u32 %3, %6, %3\n\tds_read_b64_tr_b16 %0, %2 offset:%8\n\tds_read_b64_tr_b16 %1, %3 offset:%9"
               : "=&v"(lo), "=&v"(hi), "=&v"(a), "=&v"(b) : "v"(off_a), "v"(off_b), "s"(base), "i"(KX), "i"(OFFA), "i"(OFFB) : "memory");
  d = __builtin_bit_cast(bf8v, __builtin_shufflevector(lo, hi, 0, 1, 2, 3));
}
template <int N, typename T>
__device__ __forceinline__ void at_wait_lgkm(T& f) {
  static_assert(N >= 0 && N <= 15, "lgkmcnt is a 4-bit counter");
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f) : "i"(N) : "memory");
}
template <int N, typename T>
__device__ __forceinline__ void at_wait_lgkm2(T& f, T& g) {
  static_assert(N >= 0 && N <= 15, "lgkmcnt is a 4-bit counter");
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(f), "+v"(g) : "i"(N) : "memory");
}

// ---- asm vector-memory and LDS wrappers of the forward: loads and stores the compiler neither waits for nor orders.
// Every asm vector-memory instruction that takes an SGPR base opens with wait states: a v_readlane_b32 / v_readfirstlane_b32 that has
// just (re)written the SGPR - a restored spill - needs five of them before a vector-memory instruction reads it, and the compiler pads that
// hazard for its own instructions only (gemm_e_common.hpp's E_BSTORE16 once took stale row offsets that way; tools/check_async_loads.py
// checks the ISA of these kernels too: tests/test_cabi_and_host.py).
template <int IMM, typename T>
__device__ __forceinline__ void at_gload16(T& d, const void* sbase, unsigned voff) {
  static_assert(sizeof(T) == 16 && IMM >= 0 && IMM < 4096, "global_load_dwordx4");
  asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(d) : "v"(voff), "s"(sbase), "i"(IMM) : "memory");
}
// (the trailing wait states: the data registers are rewritten right behind the store - see E_BSTORE16 in gemm_e_common.hpp)
template <int IMM, typename T>
__device__ __forceinline__ void at_gstore16(const T& v, void* sbase, unsigned voff) {
  static_assert(sizeof(T) == 16 && IMM >= 0 && IMM < 4096, "global_store_dwordx4");
  asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 offset:%3\n\ts_nop 2" :: "v"(voff), "v"(v), "s"(sbase), "i"(IMM) : "memory");
}
__device__ __forceinline__ void at_gstore4(float v, void* sbase, unsigned voff) {
  asm volatile("s_nop 4\n\tglobal_store_dword %0, %1, %2\n\ts_nop 2" :: "v"(voff), "v"(v), "s"(sbase) : "memory");
}
__device__ __forceinline__ void at_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <typename T>
__device__ __forceinline__ void at_ds_write8(unsigned addr, const T& v) {
  static_assert(sizeof(T) == 8, "ds_write_b64");
  asm volatile("ds_write_b64 %0, %1" :: "v"(addr), "v"(v) : "memory");
}
template <typename T>
__device__ __forceinline__ void at_ds_read16(T& d, unsigned addr) {
  static_assert(sizeof(T) == 16, "ds_read_b128");
  asm volatile("ds_read_b128 %0, %1" : "=v"(d) : "v"(addr) : "memory");
}
template <int N>
__device__ __forceinline__ void at_wait_lgkm_plain() {
  asm volatile("s_waitcnt lgkmcnt(%0)" :: "i"(N) : "memory");
}

// ---- Bias gradient.  The backward kernels leave partial[which][(lh, blk)][HD] (which = q, k, v; lh = line * nh + head): the column sums of each workgroup's
// output tile.  dbias[which * d + head * HD + c] += their sum over the workgroups (line, block) of a head.
// Grid (heads, 3, slices of the workgroup list): one atomic per address and slice.  64 slices at >= 4096 workgroups per head (16 slices
// were 192 blocks of two waves for 12.6 MB of partial rows: 37 us, latency-bound).
template <int HD>
__global__ __launch_bounds__(HD) void attn_bias_reduce_k(const float* partial, float* dbias, int nlines, int nh, int nblk) {
  const int c = threadIdx.x, head = blockIdx.x, which = blockIdx.y;
  const long long nwg = (long long)nlines * nh * nblk;
  const float* p = partial + (long long)which * nwg * HD;
  const int per_head = nlines * nblk;  // workgroups of this head
  const int chunk = (per_head + gridDim.z - 1) / gridDim.z;
  const int i0 = blockIdx.z * chunk, i1 = i0 + chunk < per_head ? i0 + chunk : per_head;
  // eight rows in flight per thread (two were 27 us for 25 MB of partial rows: one dependent load latency per pair)
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto at = [&](int i) -> float { return p[(((long long)(i / nblk) * nh + head) * nblk + i % nblk) * HD + c]; };
  int i = i0;
  for (; i + 8 <= i1; i += 8) {
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] += at(i + k);
  }
  for (; i < i1; i++) s[0] += at(i);
  if (i0 < i1) atomicAdd(dbias + (long long)which * nh * HD + head * HD + c, ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])));
}
template <int HD>
static inline void attn_bias_reduce_launch(const float* partial, float* dbias, int64_t N, int64_t num_heads, int64_t nb, hipStream_t st) {
  const unsigned slices = (N * nb >= 4096) ? 128 : (N * nb >= 1024) ? 64 : 16;
  hipLaunchKernelGGL(attn_bias_reduce_k<HD>, dim3((unsigned)num_heads, 3, slices), dim3(HD), 0, st, partial, dbias, (int)N, (int)num_heads, (int)nb);
}

// attention_hd64.hip: the head_dim-64 kernels (compiler-scheduled, any S >= 1); kr null: no key ranges.  attn_fwd_run / attn_bwd_run
// (attention_fwd.hip, attention_bwd.hip) validate the arguments, dispatch on head_dim and check the launch.
__attribute__((visibility("hidden"))) void attn64_fwd_launch(const void* qkv, const int* kr, void* out, float* lse, int64_t N, int64_t S, int64_t num_heads, hipStream_t st);
__attribute__((visibility("hidden"))) void attn64_bwd_launch(const void* qkv, const int* kr, const void* out, const void* dout, const float* lse, float* dvec, void* dqkv,
                                                             float* dbias, float* work, int64_t N, int64_t S, int64_t num_heads, hipStream_t st);
