// Tiled backward of the fused attention (two workgroups of four waves per CU) and its host side, attn_bwd_run behind pero_attention_bwd /
// pero_attention_bwd_keys.  Two bodies, each recomputing S^T / P from q, k and the saved base-2 log-sum-exp (no S x S tensor is ever stored):
//   attn_bwd_dq_body_p   : 128 queries of a (line, head), query on the lane, sweeps the keys in 32-key sub-tiles: S^T = K Q^T, dP^T = V dO^T,
//                          dS^T = P^T (dP^T - D) scale, dQ^T += K^T dS^T.  Also writes D[q] = sum_d dO[q][d] O[q][d] for the other body
//                          (unless D is handed in: `out` null).
//   attn_bwd_dkv2_body_p : 128 keys, key on the lane, sweeps the queries in 32-query sub-tiles: S = Q K^T, P, dP = dO V^T, dS;
//                          dV^T += dO^T P, dK^T += Q^T dS.
// both with software-pipelined operand reads (attention_common.hpp), each instantiated for full tiles, RAGGED (S % 128 != 0, the three rules:
// attention_common.hpp) and RAGGED with KEYS (per-line key ranges, at every S).  Kernels: attn_bwd_dq_k<RAGGED> then attn_bwd_dkv2_k<RAGGED> (two
// launches: dq writes D), attn_bwd_pair_k<RAGGED> (both bodies in one launch when D is handed in), their three `_keys_k` forms, then
// attn_bias_reduce_k<128> (attention_common.hpp).  No atomics in dqkv, deterministic; costs 7 MFMA products instead of
// the minimal 5 (attention is ~8 % of the step's FLOPs).  All LDS tiles use the ONE dual-use image of attention_common.hpp.
// Who waits for whom: every stage loop opens with vmcnt(0) + barrier (the stage has landed, every wave is done with the other buffer) and
// issues the next stage's LDS-DMA right behind it, under the current stage's MFMAs; a global load issued in the loop goes out BEFORE the DMA
// (vmcnt retires in order).  attn_store_tile opens with a barrier: the staging region is free.
#include "attention_common.hpp"

// Epilogue of the backward kernels: a 128 x 128 gradient tile held as acc[dt][e] (row = this lane's query / key
// `wave * 32 + r`, columns d = dt*32 + 8*(e>>2) + 4*h5 + (e&3)) goes through LDS as bf16 rows and leaves in 16-byte row
// segments (the direct form was 16 scattered 8-byte stores per lane); the staged rows also give the tile's column sums -
// this (line, head) block's share of in_proj's bias gradient - for 128 (x2) atomics instead of a pass over dqkv.
// Image: 128 rows x 256 B, 8-byte granule index XORed with (row & 31): conflict-free ds_write_b64 and ds_read_b128.
// RAGGED: only the tile's first `nrows` rows exist in the line and are stored; the staged rows behind them are exact zeros (the bodies see to
// that), so the column sums need no change.
template <bool RAGGED = false>
__device__ __forceinline__ void attn_store_tile(const f16v (&acc)[4], unsigned char* stg, bf16raw* out_base, long long ld,
                                                float* colsum, int tid, int wave, int r, int h5, int nrows = 128) {
  __syncthreads();  // the staging region is free (every wave is past its last tile read)
  const int row_w = wave * 32 + r;
#pragma unroll
  for (int dt = 0; dt < 4; dt++)
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {
      uint2 w;
      w.x = pack2bf(acc[dt][4 * g4 + 0], acc[dt][4 * g4 + 1]);
      w.y = pack2bf(acc[dt][4 * g4 + 2], acc[dt][4 * g4 + 3]);
      const int g = dt * 8 + 2 * g4 + h5;
      *(uint2*)(stg + row_w * 256 + ((g ^ (row_w & 31)) << 3)) = w;
    }
  __syncthreads();
  const int ch = tid & 15;
#pragma unroll 2
  for (int i = 0; i < 8; i++) {
    const int row = (tid >> 4) + 16 * i;
    const int x = row & 31;
    uint4 v = *(const uint4*)(stg + row * 256 + ((ch ^ (x >> 1)) << 4));
    if (x & 1) { const unsigned t0 = v.x, t1 = v.y; v.x = v.z; v.y = v.w; v.z = t0; v.w = t1; }
    if (!RAGGED || row < nrows) *(uint4*)(out_base + (long long)row * ld + ch * 8) = v;
  }
  if (colsum) {
    // Column sums of the staged tile (this (line, head) block's share of in_proj's bias gradient) on the MATRIX pipe, which idles through
    // the epilogue: wave w takes the 32 columns 32 w .., ones (32 x 16) times the 16 x 32 block of the
    // image read back TRANSPOSED (ds_read_b64_tr_b16: the row index becomes the MFMA's k - any order of the rows inside a k-step gives the
    // same sum), accumulated over the eight row blocks: every lane n then holds the sum of column 32 w + (n & 31), exact in f32, and writes
    // it - no cross-lane shuffles, no second pass through LDS, no barriers.  (As 128 vector adds + 16 shuffles per thread + an LDS
    // reduction over the four waves behind two barriers the sums were 7 % of the backward, measured by an ablation build.)
    const int lane = tid & 63;
    const int ti = lane & 15, tg = (lane >> 4) & 1;
    const int g = 8 * wave + 4 * tg + (ti & 3);                 // 8-byte granule (4 columns) this lane supplies
    const int q0 = 8 * h5 + (ti >> 2);                          // row inside a 16-row block; the second read takes row + 4
    const __bf16 one = (__bf16)1.0f;
    const bf8v ones = {one, one, one, one, one, one, one, one};
    f16v cs = {0};
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {
      const int ra = 16 * ks + q0, rb = ra + 4;
      const bf8v frag = lds_tr16_pair(stg + ra * 256 + ((g ^ (ra & 31)) << 3), stg + rb * 256 + ((g ^ (rb & 31)) << 3));
      cs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, frag, cs, 0, 0, 0);
    }
    if (lane < 32) colsum[32 * wave + lane] = cs[0];
  }
}

// ---- dQ body.  K / V are staged in 64-key HALF tiles, double-buffered (2 x (16 + 16) KiB): the DMA of the next half runs under the current
// half's 48 MFMAs per wave (whole 128-key tiles in one buffer exposed the DMA's latency once per key tile, twice per workgroup at S = 256).
// Per 64-key half (one LDS stage pair): 48 fragments = 2 sub-tiles x (16 row fragments K0 V0 K1 V1 ... for S^T / dP^T, then 8 transposed K fragments for dQ^T).  Fragment j is issued when fragment j - 7 has been consumed (pool of 8 registers
// sets), so at most 7 fragments (<= 14 LDS instructions) are in flight.
#define DQ_DEPTH 7
// LDS instructions of fragment j of a 64-key half (16 row fragments: one each, 8 transposed ones: two each)
__device__ __forceinline__ constexpr int dq_ninstr(int j) { return (j % 24) < 16 ? 1 : 2; }
__device__ __forceinline__ constexpr int dq_after(int j) {   // LDS instructions issued after fragment j's when it is consumed
  int n = 0;
  for (int k = j + 1; k <= j + DQ_DEPTH && k < 48; k++) n += dq_ninstr(k);
  return n;
}
// KEYS (with RAGGED; pero_attention_bwd_keys): the sweep takes the 64-key halves h0 .. that intersect the line's [k0, k1) only, and the 0 select of dS^T covers
// the dead keys of the first and the last of them.  dQ is computed for every query < S.
template <bool RAGGED, bool KEYS = false>
__device__ __forceinline__ void attn_bwd_dq_body_p(unsigned char* smem, int lh, int qb, const bf16raw* qkv, const bf16raw* out,
                                                   const bf16raw* dout, const float* lse2, float* dvec, bf16raw* dqkv, float* dbias, int S,
                                                   int nh, float c, float scale, const int* kr = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h5 = lane >> 5, r = lane & 31;
  const int nqb = RAGGED ? (S + 127) >> 7 : S >> 7;
  const int line = lh / nh, head = lh % nh;
  const long long d = (long long)nh * 128, ld = 3 * d;
  const bf16raw* base = qkv + (long long)line * S * ld + head * 128;
  const bf16raw* Kg = base + d;
  const bf16raw* Vg = base + 2 * d;
  const int q = qb * 128 + wave * 32 + r;
  const int qc = RAGGED ? (q < S - 1 ? q : S - 1) : q;   // ragged: a query >= S reads the line's last row; its dS is forced to 0 below
  at_key_range rng = {0, S};
  if constexpr (KEYS) rng = at_load_key_range(kr, line, S);
  const int h0 = KEYS ? rng.k0 >> 6 : 0;   // the line's first live 64-key half

  attn_glds_img<4, RAGGED>(Kg + (long long)h0 * 64 * ld, ld, smem, wave, lane, S - 1 - h0 * 64);
  attn_glds_img<4, RAGGED>(Vg + (long long)h0 * 64 * ld, ld, smem + AT_HALF_BYTES, wave, lane, S - 1 - h0 * 64);

  // D[q] = sum_d dO[q][d] O[q][d] (row sums of the output gradient times the output), layout dvec[(line*S + q)*nh + head]:
  // either already there (out == nullptr: written by the epilogue of the product that produced dO, PERO_GEMM_ROWDOT) or
  // computed here from the O rows and stored for the dK / dV kernel.
  bf8v qf[8], gf[8];
  float dsum = 0.f;
  const long long dix = ((long long)line * S + qc) * nh + head;
  {
    const bf16raw* qrow = base + (long long)qc * ld + 8 * h5;
    const bf16raw* grow = dout + ((long long)line * S + qc) * d + head * 128 + 8 * h5;
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {
      qf[ks] = *(const bf8v*)(qrow + 16 * ks);
      gf[ks] = *(const bf8v*)(grow + 16 * ks);
    }
    if (out) {
      const bf16raw* orow = out + ((long long)line * S + qc) * d + head * 128 + 8 * h5;
#pragma unroll
      for (int ks = 0; ks < 8; ks++) {
        const bf8v of = *(const bf8v*)(orow + 16 * ks);
#pragma unroll
        for (int e = 0; e < 8; e++) dsum += (float)gf[ks][e] * (float)of[e];
      }
      dsum += __shfl_xor(dsum, 32, 64);
      if (h5 == 0 && (!RAGGED || q < S)) dvec[dix] = dsum;
    } else {
      dsum = dvec[dix];
    }
  }
  const float lq = lse2[(long long)lh * S + qc];

  // fragment addresses inside a stage (byte offsets from the stage's K image): row fragments per ks, transposed fragments per dt
  const unsigned s0 = at_lds_addr(smem);
  unsigned ra[8], ta[4], tb[4];
  {
    const int f = img_f(r);
#pragma unroll
    for (int ks = 0; ks < 8; ks++) ra[ks] = (unsigned)(r * 256 + (((2 * ks + h5) ^ f) << 4));
    const int i = lane & 15, g1 = (lane >> 4) & 1;
    const int row = 4 * h5 + (i >> 2);
#pragma unroll
    for (int dt = 0; dt < 4; dt++) {
      const int ch = 4 * dt + 2 * g1 + ((i & 3) >> 1);
      ta[dt] = (unsigned)(row * 256 + ((ch ^ img_f(row)) << 4) + 8 * (i & 1));
      tb[dt] = (unsigned)((row + 8) * 256 + ((ch ^ img_f(row + 8)) << 4) + 8 * (i & 1));
    }
  }

  f16v dq[4];
#pragma unroll
  for (int t = 0; t < 4; t++) dq[t] = (f16v){0};
  const int nhalf = KEYS ? ((rng.k1 + 63) >> 6) - h0 : RAGGED ? (S + 63) >> 6 : S >> 6;   // ragged: a last half without a key is not swept; keys: live halves only
  for (int hk = 0; hk < nhalf; hk++) {   // half h0 + hk of the line, in buffer hk & 1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // half hk landed; every wave is done with the other buffer
    const unsigned stage = s0 + (hk & 1) * 2 * AT_HALF_BYTES;
    if (hk + 1 < nhalf) {
      unsigned char* nb = smem + ((hk + 1) & 1) * 2 * AT_HALF_BYTES;
      attn_glds_img<4, RAGGED>(Kg + (long long)(h0 + hk + 1) * 64 * ld, ld, nb, wave, lane, S - 1 - (h0 + hk + 1) * 64);
      attn_glds_img<4, RAGGED>(Vg + (long long)(h0 + hk + 1) * 64 * ld, ld, nb + AT_HALF_BYTES, wave, lane, S - 1 - (h0 + hk + 1) * 64);
    }
    bf8v fr[8];
    f16v s, dp;
    bf8v dsf[2];
    auto issue = [&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      constexpr int t = j / 24, qd = j % 24;
      if constexpr (qd < 16) {
        constexpr int ks = qd >> 1, isv = qd & 1;
        at_rd128<isv * AT_HALF_BYTES + t * 8192>(fr[j & 7], ra[ks], stage);
      } else {
        constexpr int sub = (qd - 16) >> 2, dt = (qd - 16) & 3;
        at_rdtr<t * 8192 + sub * 4096, t * 8192 + sub * 4096>(fr[j & 7], ta[dt], tb[dt], stage);
      }
    };
    at_static_for<0, DQ_DEPTH>(issue);
    AT_PRIO(1);
    at_static_for<0, 48>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      constexpr int qd = j % 24;
      if constexpr (j + DQ_DEPTH < 48) issue(std::integral_constant<int, j + DQ_DEPTH>{});
      if constexpr (qd == 16) {
        // ---- dS^T = P^T (dP^T - D) scale for the sub-tile whose scores are complete; the transposed fragments are in flight
        AT_PRIO(0);
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[e], c, -lq));
          s[e] = p * (dp[e] - dsum) * scale;
        }
        if constexpr (KEYS) {
          if (hk == 0 || hk == nhalf - 1 || qb == nqb - 1) {
            // dS^T selected to 0 for keys outside [k0, k1) (the first and the last live half) and queries >= S (the last query block)
            constexpr int t = j / 24;
            const int lo = rng.k0 - (h0 + hk) * 64 - t * 32 - 4 * h5;
            const int hi = q < S ? rng.k1 - (h0 + hk) * 64 - t * 32 - 4 * h5 : lo;
#pragma unroll
            for (int e = 0; e < 16; e++) {
              const int k = 8 * (e >> 2) + (e & 3);
              s[e] = (k >= lo && k < hi) ? s[e] : 0.f;
            }
          }
        } else if (RAGGED && (hk == nhalf - 1 || qb == nqb - 1)) {
          // dS^T selected to 0 for keys >= S (the line's last half) and queries >= S (its last query block): the staged dQ rows of such
          // queries are exact zeros.  Key of s[e] inside the sub-tile = 8 (e >> 2) + 4 h5 + (e & 3)
          constexpr int t = j / 24;
          const int lim = q < S ? S - hk * 64 - t * 32 - 4 * h5 : 0;
#pragma unroll
          for (int e = 0; e < 16; e++) s[e] = (8 * (e >> 2) + (e & 3) < lim) ? s[e] : 0.f;
        }
        dsf[0] = pack8(s, 0);
        dsf[1] = pack8(s, 1);
        AT_PRIO(1);
      }
      at_wait_lgkm<dq_after(j)>(fr[j & 7]);
      if constexpr (qd < 16) {
        constexpr int ks = qd >> 1;
        if constexpr (qd == 0) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j & 7], qf[0], (f16v){0}, 0, 0, 0);
        else if constexpr (qd == 1) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j & 7], gf[0], (f16v){0}, 0, 0, 0);
        else if constexpr ((qd & 1) == 0) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j & 7], qf[ks], s, 0, 0, 0);
        else dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j & 7], gf[ks], dp, 0, 0, 0);
      } else {
        constexpr int sub = (qd - 16) >> 2, dt = (qd - 16) & 3;
        dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j & 7], dsf[sub], dq[dt], 0, 0, 0);
      }
    });
    AT_PRIO(0);
  }
  attn_store_tile<RAGGED>(dq, smem, dqkv + ((long long)line * S + qb * 128) * ld + head * 128, ld,
                          dbias ? dbias + ((long long)lh * nqb + qb) * 128 : nullptr, tid, wave, r, h5, S - qb * 128);
}
template <bool RAGGED>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_k(const bf16raw* qkv, const bf16raw* out, const bf16raw* dout, const float* lse2,
                                                        float* dvec, bf16raw* dqkv, float* dbias, int S, int nh, float c, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nqb = RAGGED ? (S + 127) >> 7 : S >> 7;
  int lh, qb;
  attn_block_map(blockIdx.x, nqb, gridDim.x / nqb, lh, qb);
  attn_bwd_dq_body_p<RAGGED>(smem, lh, qb, qkv, out, dout, lse2, dvec, dqkv, dbias, S, nh, c, scale);
}

// dK and dV in ONE pass (4 products: S, dP, dV^T += dO^T P, dK^T += Q^T dS; key on the lane).  The two-launch form read
// Q, dO and K twice and computed S twice (605 MB and 5 products per layer at S = 256, d = 512); both launches were HBM-bound
// to about half (row / tile reads of 256 KiB per workgroup for ~2.6 us of MFMA work).  What made the single pass spill before
// was register-resident V next to register-resident K and two accumulator sets; here the workgroup's 128 x 128 V tile
// lives in LDS (read as the B operand of dP) and Q / dO arrive in 32-query stages (8 + 8 KiB, double-buffered), so the
// footprint stays at 64.5 KiB = two workgroups per CU.
// ---- dK / dV body.  Per 32-query stage: 24 row fragments (per ks: Q, dO, V) for S / dP, then the stage's row statistics
// (compiler-visible LDS reads, issued while nothing else is in flight) and the exponentials, with the first transposed fragments of the
// gradient products issued between the four groups of the arithmetic, then 16 transposed fragments (per (sub, dt): dO^T, Q^T).
#ifndef DKV_POOL
#define DKV_POOL 6
#endif
#define DKV_TD (DKV_POOL - 1)        // transposed fragments in flight: 5 .. 7
#define DKV_RDEPTH (DKV_POOL - 2)   // row fragments in flight (a dP product holds two pool entries: dO and V); transposed fragments: 7
                                    // in flight (two LDS instructions each: 14 of the 15 the counter can hold)
// KEYS (with RAGGED; pero_attention_bwd_keys): every query < S is swept; the staged dK / dV rows of the keys outside the line's [k0, k1) are zeroed the way keys >= S
// are (a dead key's P may overflow: it stays in that key's MFMA column and is SELECTED away).  A tile wholly outside the range sweeps nothing and still stores
// zero rows for its real keys (dqkv arrives uninitialised) and zero partial rows of the bias gradient.
template <bool RAGGED, bool KEYS = false>
__device__ __forceinline__ void attn_bwd_dkv2_body_p(unsigned char* smem, int lh, int kb, long long nwg, const bf16raw* qkv, const bf16raw* dout,
                                                     const float* lse2, const float* dvec, bf16raw* dqkv, float* dbias, int S, int nh, float c,
                                                     float scale, const int* kr = nullptr) {
  unsigned char* vimg = smem + 4 * AT_SUB_BYTES;
  float* lds_ld = (float*)(smem + 4 * AT_SUB_BYTES + AT_TILE_BYTES);  // [2 buffers][32 lse2 | 32 D]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h5 = lane >> 5, r = lane & 31;
  const int nkb = RAGGED ? (S + 127) >> 7 : S >> 7;
  const int line = lh / nh, head = lh % nh;
  const long long d = (long long)nh * 128, ld = 3 * d;
  const bf16raw* base = qkv + (long long)line * S * ld + head * 128;
  const bf16raw* Gg = dout + (long long)line * S * d + head * 128;
  const int key = kb * 128 + wave * 32 + r;
  const int kc = RAGGED ? (key < S - 1 ? key : S - 1) : key;   // ragged: a key >= S computes on the line's last row; its dK / dV rows are zeroed below
  // row statistics of a 32-query stage: threads 0-31 load lse2[lh][q], threads 32-63 load D[(line*S + q)*nh + head]   (ragged: q clamped to S - 1)
  const float* stat = tid < 32 ? lse2 + (long long)lh * S + tid : dvec + ((long long)line * S + (tid & 31)) * nh + head;
  const long long stat_step = tid < 32 ? 32 : 32LL * nh;
  // ragged: the queries >= S of the line's LAST stage take the statistics of the line's last row - one per-lane element offset, used in that stage only
  int stat_tail = 0;
  if constexpr (RAGGED) {
    const int qs = (((S + 31) >> 5) - 1) * 32 + (tid & 31);
    stat_tail = qs < S ? 0 : (S - 1 - qs) * (tid < 32 ? 1 : nh);
  }

  if constexpr (RAGGED) { if (tid < 64) lds_ld[tid] = stat[S <= 32 ? stat_tail : 0]; }
  else if (tid < 64) lds_ld[tid] = stat[0];
  attn_glds_img<8, RAGGED>(base + 2 * d + (long long)kb * 128 * ld, ld, vimg, wave, lane, S - 1 - kb * 128);  // this workgroup's V tile, resident
  attn_glds_img<2, RAGGED>(base, ld, smem, wave, lane, S - 1);
  attn_glds_img<2, RAGGED>(Gg, d, smem + AT_SUB_BYTES, wave, lane, S - 1);

  bf8v kf[8];
  {
    const bf16raw* krow = base + d + (long long)kc * ld + 8 * h5;
#pragma unroll
    for (int ks = 0; ks < 8; ks++) kf[ks] = *(const bf8v*)(krow + 16 * ks);
  }
  // fragment addresses (byte offsets inside a stage's Q image; the dO image follows at + AT_SUB_BYTES)
  const unsigned s0 = at_lds_addr(smem);
  const unsigned vbase = s0 + 4 * AT_SUB_BYTES + __builtin_amdgcn_readfirstlane(wave) * 8192;    // this wave's 32 rows of the resident V image
  unsigned ra[8], ta[4], tb[4];
  {
    const int f = img_f(r);
#pragma unroll
    for (int ks = 0; ks < 8; ks++) ra[ks] = (unsigned)(r * 256 + (((2 * ks + h5) ^ f) << 4));
    const int i = lane & 15, g1 = (lane >> 4) & 1;
    const int row = 4 * h5 + (i >> 2);
#pragma unroll
    for (int dt = 0; dt < 4; dt++) {
      const int ch = 4 * dt + 2 * g1 + ((i & 3) >> 1);
      ta[dt] = (unsigned)(row * 256 + ((ch ^ img_f(row)) << 4) + 8 * (i & 1));
      tb[dt] = (unsigned)((row + 8) * 256 + ((ch ^ img_f(row + 8)) << 4) + 8 * (i & 1));
    }
  }
  f16v dv[4], dk[4];
#pragma unroll
  for (int t = 0; t < 4; t++) { dv[t] = (f16v){0}; dk[t] = (f16v){0}; }
  at_key_range rng = {0, S};
  if constexpr (KEYS) rng = at_load_key_range(kr, line, S);
  const bool dead_tile = KEYS && (kb * 128 >= rng.k1 || kb * 128 + 128 <= rng.k0);
  const int nsub = dead_tile ? 0 : RAGGED ? (S + 31) >> 5 : S >> 5;   // ragged: stages without a query are not swept
  for (int sq = 0; sq < nsub; sq++) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage sq (Q / dO rows + statistics) landed; every wave is done with the other buffers
    const unsigned stage = s0 + (sq & 1) * 2 * AT_SUB_BYTES;
    const float* lds_l = lds_ld + (sq & 1) * 64;
    const float* lds_d = lds_l + 32;
    float nstat = 0.f;
    if (sq + 1 < nsub) {
      if constexpr (RAGGED) { if (tid < 64) nstat = stat[(sq + 1) * stat_step + (sq + 2 == nsub ? stat_tail : 0)]; }
      else if (tid < 64) nstat = stat[(sq + 1) * stat_step];  // before the DMA: vmcnt is in-order
      unsigned char* nb = smem + ((sq + 1) & 1) * 2 * AT_SUB_BYTES;
      attn_glds_img<2, RAGGED>(base + (long long)(sq + 1) * 32 * ld, ld, nb, wave, lane, S - 1 - (sq + 1) * 32);
      attn_glds_img<2, RAGGED>(Gg + (long long)(sq + 1) * 32 * d, d, nb + AT_SUB_BYTES, wave, lane, S - 1 - (sq + 1) * 32);
    }
    bf8v fr[DKV_POOL];
    f16v s, dp;
    // ---- S = Q K^T, dP = dO V^T: 24 row fragments
    auto issue_r = [&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      constexpr int ks = j / 3, kind = j % 3;
      if constexpr (kind == 0) at_rd128<0>(fr[j % DKV_POOL], ra[ks], stage);
      else if constexpr (kind == 1) at_rd128<AT_SUB_BYTES>(fr[j % DKV_POOL], ra[ks], stage);
      else at_rd128<0>(fr[j % DKV_POOL], ra[ks], vbase);
    };
    at_static_for<0, DKV_RDEPTH>(issue_r);
    AT_PRIO(1);
    at_static_for<0, 24>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      constexpr int ks = j / 3, kind = j % 3;
      if constexpr (j + DKV_RDEPTH < 24) issue_r(std::integral_constant<int, j + DKV_RDEPTH>{});
      constexpr int after = (24 - 1 - j) < DKV_RDEPTH ? (24 - 1 - j) : DKV_RDEPTH;
      if constexpr (kind == 0) {
        at_wait_lgkm<after>(fr[j % DKV_POOL]);
        if constexpr (ks == 0) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j % DKV_POOL], kf[0], (f16v){0}, 0, 0, 0);
        else s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j % DKV_POOL], kf[ks], s, 0, 0, 0);
      } else if constexpr (kind == 2) {
        at_wait_lgkm<after>(fr[j % DKV_POOL]);   // LDS reads retire in order: the dO fragment (j - 1) has landed too
        asm volatile("" : "+v"(fr[(j - 1) % DKV_POOL]));
        if constexpr (ks == 0) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[(j - 1) % DKV_POOL], fr[j % DKV_POOL], (f16v){0}, 0, 0, 0);
        else dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[(j - 1) % DKV_POOL], fr[j % DKV_POOL], dp, 0, 0, 0);
      }
    });
    AT_PRIO(0);
    // ---- P, dS (rows q = (e&3) + 8(e>>2) + 4*h5 of the stage on the registers); transposed fragments go out group by group
    auto issue_t = [&](auto mc) __attribute__((always_inline)) {
      constexpr int m = decltype(mc)::value;
      constexpr int sub = m >> 3, dt = (m >> 1) & 3, kind = m & 1;   // kind 0: dO^T (-> dV), 1: Q^T (-> dK)
      constexpr int off = sub * 4096 + (kind == 0 ? AT_SUB_BYTES : 0);
      at_rdtr<off, off>(fr[m % DKV_POOL], ta[dt], tb[dt], stage);
    };
    // The stage's row statistics (lse2 and D of the 16 queries a lane holds: four groups of 4 + 4 floats) travel in the same counted stream
    // as the fragments - compiler-visible reads would be waited for with lgkmcnt(0), i.e. together with every transposed fragment
    // issued ahead of them.  Stream: S0 S1 | math 0 | S2 T0 T1 | math 1 | S3 T2 T3 | math 2 | T4 T5 | math 3 | T6   (Sg = 2 reads, Tm = 2)
    f4v l4[4], d4[4];
    const unsigned stb = s0 + 4 * AT_SUB_BYTES + AT_TILE_BYTES + (sq & 1) * 256, sto = 16 * h5;
    auto issue_s = [&](auto gc) __attribute__((always_inline)) {
      constexpr int g = decltype(gc)::value;
      at_rd128<32 * g>(l4[g], sto, stb);
      at_rd128<128 + 32 * g>(d4[g], sto, stb);
    };
    issue_s(std::integral_constant<int, 0>{});
    issue_s(std::integral_constant<int, 1>{});
    bf8v pf[2], dsf[2];
    at_static_for<0, 4>([&](auto gc) __attribute__((always_inline)) {
      constexpr int g4 = decltype(gc)::value;
      // LDS instructions issued after this group's statistics: g0: S1 = 2; g1: S2 T0 T1 = 6; g2: T0 T1 S3 T2 T3 = 10; g3: T2 T3 T4 T5 = 8
      constexpr int after = g4 == 0 ? 2 : g4 == 1 ? 6 : g4 == 2 ? 10 : (DKV_TD >= 6 ? 8 : 4);
      at_wait_lgkm2<after>(l4[g4], d4[g4]);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float p = __builtin_amdgcn_exp2f(fmaf(s[4 * g4 + e], c, -l4[g4][e]));
        if constexpr (RAGGED) p = (sq * 32 + 8 * g4 + 4 * h5 + e < S) ? p : 0.f;   // queries >= S (the last stage): P = 0, so dS = 0 (its other factor is finite)
        s[4 * g4 + e] = p;                                              // P
        dp[4 * g4 + e] = p * (dp[4 * g4 + e] - d4[g4][e]) * scale;     // dS
      }
      if constexpr (g4 == 1) { pf[0] = pack8(s, 0); dsf[0] = pack8(dp, 0); }
      if constexpr (g4 == 3) { pf[1] = pack8(s, 1); dsf[1] = pack8(dp, 1); }
      if constexpr (g4 + 2 < 4) issue_s(std::integral_constant<int, g4 + 2>{});
      if constexpr (2 * g4 < DKV_TD) issue_t(std::integral_constant<int, 2 * g4>{});
      if constexpr (2 * g4 + 1 < DKV_TD) issue_t(std::integral_constant<int, 2 * g4 + 1>{});
    });
    AT_PRIO(1);
    at_static_for<0, 16>([&](auto mc) __attribute__((always_inline)) {
      constexpr int m = decltype(mc)::value;
      constexpr int sub = m >> 3, dt = (m >> 1) & 3, kind = m & 1;
      if constexpr (m + DKV_TD < 16) issue_t(std::integral_constant<int, m + DKV_TD>{});
      constexpr int after = 2 * ((16 - 1 - m) < DKV_TD ? (16 - 1 - m) : DKV_TD);
      at_wait_lgkm<after>(fr[m % DKV_POOL]);
      if constexpr (kind == 0) dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[m % DKV_POOL], pf[sub], dv[dt], 0, 0, 0);    // dV^T += dO^T P
      else dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[m % DKV_POOL], dsf[sub], dk[dt], 0, 0, 0);                     // dK^T += Q^T dS
    });
    AT_PRIO(0);
    if (sq + 1 < nsub && tid < 64) lds_ld[((sq + 1) & 1) * 64 + tid] = nstat;  // visible after the next barrier
  }
  if constexpr (KEYS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // a dead tile ran no stage: its prologue's LDS-DMA must land before the staging writes
  if constexpr (RAGGED) {   // keys >= S computed on a copy of the last key (keys outside the range: on dead operands): their staged dK / dV rows are exact zeros
    const bool live = KEYS ? (key >= rng.k0 && key < rng.k1) : key < S;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) { dk[t][e] = live ? dk[t][e] : 0.f; dv[t][e] = live ? dv[t][e] : 0.f; }
  }
  bf16raw* tile_o = dqkv + ((long long)line * S + kb * 128) * ld + d + head * 128;  // dK tile; dV tile = + d columns
  attn_store_tile<RAGGED>(dk, smem, tile_o, ld, dbias ? dbias + (nwg + (long long)lh * nkb + kb) * 128 : nullptr, tid, wave, r, h5, S - kb * 128);
  attn_store_tile<RAGGED>(dv, smem, tile_o + d, ld, dbias ? dbias + (2 * nwg + (long long)lh * nkb + kb) * 128 : nullptr, tid, wave, r, h5, S - kb * 128);
}
template <bool RAGGED>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv2_k(const bf16raw* qkv, const bf16raw* dout, const float* lse2, const float* dvec,
                                                          bf16raw* dqkv, float* dbias, int S, int nh, float c, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nkb = RAGGED ? (S + 127) >> 7 : S >> 7;
  int lh, kb;
  attn_block_map(blockIdx.x, nkb, gridDim.x / nkb, lh, kb);
  attn_bwd_dkv2_body_p<RAGGED>(smem, lh, kb, gridDim.x, qkv, dout, lse2, dvec, dqkv, dbias, S, nh, c, scale);
}
// Both backward kernels as ONE launch (D already computed: `out` is not read, so no workgroup depends on another): the 2 x (S / 128)
// workgroups of a (line, head) - its dQ blocks and its dK / dV blocks, which all read the same Q, K, V and dO rows - sit next to
// each other in one XCD's dispatch order, so the rows come from HBM once and the other readers find them in that XCD's L2
// (FETCH_SIZE of the backward at 256 lines: 534 MB as two launches, 308 MB paired, 267 MB = each row once; 789 -> 740 us at 1024 lines).
__device__ __forceinline__ void attn_pair_map(int nb, int order, int& lh, int& blk) {
  attn_block_map(blockIdx.x, 2 * nb, gridDim.x / (2 * nb), lh, blk);
  {   // Dispatch order inside an XCD (pero_set_option("attn_order", n); default 32): chunks of 32 units whose 64 dK / dV blocks - one round of the XCD's 64 workgroup
      // places - go out ahead of their 64 dQ blocks, so that the CUs of an XCD run ONE kind of block at a time: medians of six launches (tools/attn_order_ab.py, 2048 lines)
      // 1 406 us side by side, 1 385 / 1 381 with chunks of 4 / 8, 1 414 with 16 (both kinds in one round again), 1 361 with 32, 1 388 with 64.  A chunk's rows are 8 MB:
      // the dQ blocks find half of them in the XCD's L2, the rest in the memory-side cache.
    const int nlh = gridDim.x / (2 * nb);
    if (order && (nlh & 7) == 0) {
      const int xcd = blockIdx.x & 7, u = blockIdx.x >> 3;
      if (order == 1) blk = (blk + nb) % (2 * nb);
      else {
        // order = 100 v + CH: chunks of CH units per XCD; v & 1: the dQ blocks of a chunk first (else the dK / dV blocks); v & 2: block-major inside a role (else unit-major)
        const int CH = order % 100, v = order / 100, per = CH * 2 * nb;
        if (CH > 0 && (nlh >> 3) % CH == 0) {
          const int cch = u / per, i = u % per, first = i / (CH * nb), j = i % (CH * nb);
          const int role_dkv = (v & 1) ? first : 1 - first;
          const int un = (v & 2) ? j % CH : j / nb, bl = (v & 2) ? j / CH : j % nb;
          lh = (cch * CH + un) * 8 + xcd;
          blk = (role_dkv ? nb : 0) + bl;
        }
      }
    }
  }
}
template <bool RAGGED>
__global__ __launch_bounds__(256, 2) void attn_bwd_pair_k(const bf16raw* qkv, const bf16raw* dout, const float* lse2, float* dvec,
                                                          bf16raw* dqkv, float* dbias, int S, int nh, float c, float scale, int order) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nb = RAGGED ? (S + 127) >> 7 : S >> 7;
  int lh, blk;
  attn_pair_map(nb, order, lh, blk);
  if (blk < nb) attn_bwd_dq_body_p<RAGGED>(smem, lh, blk, qkv, nullptr, dout, lse2, dvec, dqkv, dbias, S, nh, c, scale);
  else attn_bwd_dkv2_body_p<RAGGED>(smem, lh, blk - nb, (long long)(gridDim.x >> 1), qkv, dout, lse2, dvec, dqkv, dbias, S, nh, c, scale);
}
// ---- the three launches with per-line key ranges: the KEYS instantiations of the pipelined ragged bodies
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_keys_k(const bf16raw* qkv, const int* kr, const bf16raw* out, const bf16raw* dout, const float* lse2,
                                                             float* dvec, bf16raw* dqkv, float* dbias, int S, int nh, float c, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nqb = (S + 127) >> 7;
  int lh, qb;
  attn_block_map(blockIdx.x, nqb, gridDim.x / nqb, lh, qb);
  attn_bwd_dq_body_p<true, true>(smem, lh, qb, qkv, out, dout, lse2, dvec, dqkv, dbias, S, nh, c, scale, kr);
}
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv2_keys_k(const bf16raw* qkv, const int* kr, const bf16raw* dout, const float* lse2, const float* dvec,
                                                               bf16raw* dqkv, float* dbias, int S, int nh, float c, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nkb = (S + 127) >> 7;
  int lh, kb;
  attn_block_map(blockIdx.x, nkb, gridDim.x / nkb, lh, kb);
  attn_bwd_dkv2_body_p<true, true>(smem, lh, kb, gridDim.x, qkv, dout, lse2, dvec, dqkv, dbias, S, nh, c, scale, kr);
}
__global__ __launch_bounds__(256, 2) void attn_bwd_pair_keys_k(const bf16raw* qkv, const int* kr, const bf16raw* dout, const float* lse2, float* dvec,
                                                               bf16raw* dqkv, float* dbias, int S, int nh, float c, float scale, int order) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nb = (S + 127) >> 7;
  int lh, blk;
  attn_pair_map(nb, order, lh, blk);
  if (blk < nb) attn_bwd_dq_body_p<true, true>(smem, lh, blk, qkv, nullptr, dout, lse2, dvec, dqkv, dbias, S, nh, c, scale, kr);
  else attn_bwd_dkv2_body_p<true, true>(smem, lh, blk - nb, (long long)(gridDim.x >> 1), qkv, dout, lse2, dvec, dqkv, dbias, S, nh, c, scale, kr);
}

constexpr int AT_PAIR_LDS = AT_DKV2_LDS > 2 * AT_TILE_BYTES ? AT_DKV2_LDS : 2 * AT_TILE_BYTES;   // a paired workgroup runs either body

// One host path for both entry points (`who` prefixes the error texts; key_ranges null: none): validate, dispatch on head_dim, launch - two
// launches when D is computed here (`out` given) or "attn_bwd_pair" is 0, the paired launch otherwise ("attn_order" orders its dispatch) -, reduce
// the bias gradient, check.  Key ranges run the KEYS instantiations (ragged bodies) at every S.
static int attn_bwd_run(const char* who, const void* qkv, const int* key_ranges /* null: none */, const void* out, const void* dout, const float* lse,
                        float* dvec, void* dqkv, float* dbias, float* work, int64_t N, int64_t S, int64_t num_heads, int64_t head_dim, int dtype,
                        hipStream_t st) {
  PERO_REQUIRE(qkv && dout && lse && dvec && dqkv, "%s: null pointer", who);
  PERO_REQUIRE(dtype == PERO_BF16 && (head_dim == 64 || head_dim == 128) && S > 0 && N > 0 && num_heads > 0,
               "%s: fused kernel needs bf16, head_dim 64 or 128, S > 0 (got hd=%lld S=%lld)", who, (long long)head_dim, (long long)S);
  PERO_REQUIRE(aligned16(qkv) && (!out || aligned16(out)) && aligned16(dout) && aligned16(dqkv), "%s: 16-byte alignment", who);
  PERO_REQUIRE(!dbias || work, "%s: dbias needs the partial-sum workspace", who);
  if (head_dim == 64) {   // attention_hd64.hip: the same two kernels whether D is computed here or handed in
    attn64_bwd_launch(qkv, key_ranges, out, dout, lse, dvec, dqkv, dbias, work, N, S, num_heads, st);
    PERO_CHECK_LAUNCH(who);
    return PERO_OK;
  }
  PERO_LDS_ATTR(attn_bwd_dq_k<false>, 2 * AT_TILE_BYTES);
  PERO_LDS_ATTR(attn_bwd_dq_k<true>, 2 * AT_TILE_BYTES);
  PERO_LDS_ATTR(attn_bwd_dq_keys_k, 2 * AT_TILE_BYTES);
  PERO_LDS_ATTR(attn_bwd_dkv2_k<false>, AT_DKV2_LDS);
  PERO_LDS_ATTR(attn_bwd_dkv2_k<true>, AT_DKV2_LDS);
  PERO_LDS_ATTR(attn_bwd_dkv2_keys_k, AT_DKV2_LDS);
  PERO_LDS_ATTR(attn_bwd_pair_k<false>, AT_PAIR_LDS);
  PERO_LDS_ATTR(attn_bwd_pair_k<true>, AT_PAIR_LDS);
  PERO_LDS_ATTR(attn_bwd_pair_keys_k, AT_PAIR_LDS);
  const float scale = (float)(1.0 / sqrt((double)head_dim));
  const float c = (float)(1.4426950408889634 / sqrt((double)head_dim));
  const int64_t nb = (S + 127) / 128;   // query blocks = key blocks of a line; the last one is ragged when S % 128 != 0
  const bool ragged = S % 128 != 0;
  const dim3 grid((unsigned)(N * num_heads * nb)), block(256);
  const bf16raw *q_ = (const bf16raw*)qkv, *o_ = (const bf16raw*)out, *g_ = (const bf16raw*)dout;
  bf16raw* dq_ = (bf16raw*)dqkv;
  float* const part = dbias ? work : nullptr;   // the partial-sum workspace of the bias gradient
  const int s_ = (int)S, nh_ = (int)num_heads;
  if (!out && g_opt.attn_bwd_pair) {
    const dim3 grid2(2 * grid.x);
    if (key_ranges) hipLaunchKernelGGL(attn_bwd_pair_keys_k, grid2, block, AT_PAIR_LDS, st, q_, key_ranges, g_, lse, dvec, dq_, part, s_, nh_, c, scale, g_opt.attn_order);
    else hipLaunchKernelGGL((ragged ? attn_bwd_pair_k<true> : attn_bwd_pair_k<false>), grid2, block, AT_PAIR_LDS, st, q_, g_, lse, dvec, dq_, part, s_, nh_, c, scale, g_opt.attn_order);
  } else if (key_ranges) {
    hipLaunchKernelGGL(attn_bwd_dq_keys_k, grid, block, 2 * AT_TILE_BYTES, st, q_, key_ranges, o_, g_, lse, dvec, dq_, part, s_, nh_, c, scale);
    hipLaunchKernelGGL(attn_bwd_dkv2_keys_k, grid, block, AT_DKV2_LDS, st, q_, key_ranges, g_, lse, dvec, dq_, part, s_, nh_, c, scale);
  } else {
    hipLaunchKernelGGL((ragged ? attn_bwd_dq_k<true> : attn_bwd_dq_k<false>), grid, block, 2 * AT_TILE_BYTES, st, q_, o_, g_, lse, dvec, dq_, part, s_, nh_, c, scale);
    hipLaunchKernelGGL((ragged ? attn_bwd_dkv2_k<true> : attn_bwd_dkv2_k<false>), grid, block, AT_DKV2_LDS, st, q_, g_, lse, dvec, dq_, part, s_, nh_, c, scale);
  }
  if (dbias) attn_bias_reduce_launch<128>(work, dbias, N, num_heads, nb, st);
  PERO_CHECK_LAUNCH(who);
  return PERO_OK;
}

extern "C" int pero_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* dvec, void* dqkv,
                                  float* dbias, float* work, int64_t N, int64_t S, int64_t num_heads, int64_t head_dim, int dtype,
                                  void* stream) {
  return attn_bwd_run("pero_attention_bwd", qkv, nullptr, out, dout, lse, dvec, dqkv, dbias, work, N, S, num_heads, head_dim, dtype, (hipStream_t)stream);
}

// The same with per-line key ranges (include/pero_hip.h)
extern "C" int pero_attention_bwd_keys(const void* qkv, const int* key_ranges, const void* out, const void* dout, const float* lse, float* dvec, void* dqkv,
                                       float* dbias, float* work, int64_t N, int64_t S, int64_t num_heads, int64_t head_dim, int dtype, void* stream) {
  PERO_REQUIRE(key_ranges, "pero_attention_bwd_keys: null pointer");
  return attn_bwd_run("pero_attention_bwd_keys", qkv, key_ranges, out, dout, lse, dvec, dqkv, dbias, work, N, S, num_heads, head_dim, dtype, (hipStream_t)stream);
}
