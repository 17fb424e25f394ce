// Fused attention at head_dim 64 (bf16, any S >= 1): forward attn64_fwd_k, backward attn64_bwd_dq_k then attn64_bwd_dkv_k, their `_keys_k`
// forms with per-line key ranges, and the two launchers that attn_fwd_run / attn_bwd_run (attention_fwd.hip, attention_bwd.hip) dispatch to; the bias
// reduction is attn_bias_reduce_k<64> of attention_common.hpp.  The scheme is the one of
// attention_fwd.hip and attention_bwd.hip - everything computed TRANSPOSED (a query, or a key, lives on a lane), P never leaves registers, K / V
// / Q / dO tiles arrive by LDS-DMA, the backward recomputes P from the base-2 lse, no atomics go into dqkv - re-derived for rows of 128 bytes
// (64 bf16): S^T of 32 keys x 32 queries takes 4 k-steps of mfma_f32_32x32x16_bf16, O^T / dQ^T / dK^T / dV^T take 2 head-dim tiles.  The loops
// are compiler-scheduled; "attn_bwd_pair" and "attn_order" have no effect here.
//
// ONE LDS image serves every tile (K and V of the forward, K / V halves of dQ, the Q / dO stages and the V tile of dK / dV).  Rows of 128 B
// in pieces of 1 KiB: piece p = rows 8p .. 8p+7, filled by ONE global_load_lds of 16 bytes per lane, lane -> (row 8p + (lane >> 3), 16-byte
// slot lane & 7).  LDS is filled lane-linearly, so the swizzle sits on the SOURCE address: slot `slot` of row `row` receives the row's chunk
//   slot ^ a64_f(row),   a64_f(row) = (bit 1 of row) << 2 | (bits 3..2 of row)
// Derivation (banks of ds_read_b128 / ds_read_b64_tr_b16: (address / 4) % 64, i.e. a 256-byte bank row = TWO image rows, row parity = the half):
//   * row reads (ds_read_b128, lane = row, all lanes the same chunk): a 16-lane group of the instruction holds 8 even and 8 odd rows whose
//     (row >> 1) & 7 are all different (groups {0-3,12-15,20-27} and {4-11,16-19,28-31} of each 32 lanes).  a64_f is a bijection of
//     (row >> 1) & 7, so the 8 rows of one parity land in 8 different 16-byte slots of their half: conflict-free.
//   * transposed reads (ds_read_b64_tr_b16; banking per 32-lane half): a half reads rows 4k .. 4k+3, 64 contiguous logical bytes each (chunks
//     4 dt .. 4 dt + 3).  Rows 4k and 4k+2 share a parity; bit 2 of a64_f is bit 1 of the row, so their chunks fall into opposite 64-byte blocks
//     of the half (likewise 4k+1 and 4k+3): the 4 x 64 bytes cover the 256-byte bank row once: conflict-free.
// Staging image of the LDS-staged stores (O, dQ, dK, dV: a 128 x 64 tile as bf16 rows of 128 B): 8-byte granule index XORed with (row & 15).
// ds_write_b64 banks are (address / 4) % 32 - one image row - in groups of 16 contiguous lanes (= 16 consecutive rows, one granule): 16
// different granules.  Read back as ds_read_b128, lane -> (row = tid >> 3, chunk tid & 7): a 16-lane group holds four half rows, {0-3} and
// {4-7} XORed with ((row & 15) >> 1) of rows r and r + 2 (complementary), in the two parities: conflict-free.
// Ragged S, the three rules of attention_common.hpp, always on (one instantiation): every row index that feeds a global address is clamped
// to the line's last row; P (dS) is selected to 0 where key >= S or query >= S; every row store is guarded by row < S.
#include "attention_common.hpp"

#define A64_TILE_BYTES 16384   // 128 rows x 128 B
#define A64_HALF_BYTES 8192    // 64 rows
#define A64_SUB_BYTES 4096     // 32 rows
#define A64_FWD_LDS (2 * A64_TILE_BYTES)                         // K tile, V tile
#define A64_DQ_LDS (4 * A64_HALF_BYTES)                          // (K half, V half) x 2
#define A64_DKV_LDS (4 * A64_SUB_BYTES + A64_TILE_BYTES + 512)   // (Q stage, dO stage) x 2, V tile, row statistics x 2

__device__ __forceinline__ int a64_f(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }

// NP pieces per wave: 4 = a 128-row tile, 2 = a 64-row half, 1 = a 32-row stage.  LDS row `row` receives source row min(row, last), last >= 0.
template <int NP>
__device__ __forceinline__ void a64_glds(const bf16raw* g, long long ld, unsigned char* lds, int wave, int lane, int last) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    const int p = wave + 4 * i;
    const int row = 8 * p + (lane >> 3), slot = lane & 7;
    const int chunk = slot ^ a64_f(row);
    const int srow = row < last ? row : last;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + (long long)srow * ld + chunk * 8),
                                     (__attribute__((address_space(3))) void*)(lds + p * 1024), 16, 0, 0);
  }
}
// A / B operand, row-wise: lane holds M[row][16*ks + 8*h5 .. +8]
__device__ __forceinline__ bf8v a64_row_frag(const unsigned char* img, int row, int ks, int h5) {
  return *(const bf8v*)(img + row * 128 + (((2 * ks + h5) ^ a64_f(row)) << 4));
}
// A operand, transposed: element j <- M[rb + 8(j>>2) + 4h + (j&3)][dt*32 + (lane&31)]   (rb multiple of 16)
__device__ __forceinline__ bf8v a64_tr_frag(const unsigned char* img, int rb, int dt, int lane) {
  const int i = lane & 15, g1 = (lane >> 4) & 1, h5 = lane >> 5;
  const int row = rb + 4 * h5 + (i >> 2);
  const int ch = 4 * dt + 2 * g1 + ((i & 3) >> 1);
  return lds_tr16_pair(img + row * 128 + ((ch ^ a64_f(row)) << 4) + 8 * (i & 1),
                       img + (row + 8) * 128 + ((ch ^ a64_f(row + 8)) << 4) + 8 * (i & 1));
}

// A 128 x 64 tile held as acc[dt][e] (row = this lane's query / key `wave * 32 + r`, columns d = dt*32 + 8*(e>>2) + 4*h5 + (e&3)) goes
// through LDS as bf16 rows and leaves in 16-byte row segments: HBM sees whole 128-byte rows.  Only the tile's first `nrows` rows are
// stored.  colsum (64 floats, or null): the staged tile's column sums - this block's share of in_proj's bias gradient - on the matrix pipe
// as in attn_store_tile (attention_bwd.hip): waves 0 and 1 take 32 columns each, ones (32 x 16) times the image read back transposed; the
// rows behind `nrows` are exact zeros (the bodies see to that).  Opens with a barrier: the staging region is free.
__device__ __forceinline__ void a64_store_tile(const f16v (&acc)[2], unsigned char* stg, bf16raw* out_base, long long ld, float* colsum,
                                               int tid, int wave, int r, int h5, int nrows) {
  __syncthreads();
  const int row_w = wave * 32 + r;
#pragma unroll
  for (int dt = 0; dt < 2; dt++)
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {
      uint2 w;
      w.x = pack2bf(acc[dt][4 * g4 + 0], acc[dt][4 * g4 + 1]);
      w.y = pack2bf(acc[dt][4 * g4 + 2], acc[dt][4 * g4 + 3]);
      const int g = dt * 8 + 2 * g4 + h5;  // granule of d = dt*32 + 8*g4 + 4*h5
      *(uint2*)(stg + row_w * 128 + ((g ^ (row_w & 15)) << 3)) = w;
    }
  __syncthreads();
  const int ch = tid & 7;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int row = (tid >> 3) + 32 * i;
    const int x = row & 15;
    uint4 v = *(const uint4*)(stg + row * 128 + ((ch ^ (x >> 1)) << 4));
    if (x & 1) { const unsigned t0 = v.x, t1 = v.y; v.x = v.z; v.y = v.w; v.z = t0; v.w = t1; }
    if (row < nrows) *(uint4*)(out_base + (long long)row * ld + ch * 8) = v;
  }
  if (colsum && wave < 2) {
    const int lane = tid & 63;
    const int ti = lane & 15, tg = (lane >> 4) & 1;
    const int g = 8 * wave + 4 * tg + (ti & 3);   // 8-byte granule (4 columns) this lane supplies
    const int q0 = 8 * h5 + (ti >> 2);            // row inside a 16-row block; the second read takes row + 4
    const __bf16 one = (__bf16)1.0f;
    const bf8v ones = {one, one, one, one, one, one, one, one};
    f16v cs = {0};
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {
      const int ra = 16 * ks + q0, rb = ra + 4;
      const bf8v frag = lds_tr16_pair(stg + ra * 128 + ((g ^ (ra & 15)) << 3), stg + rb * 128 + ((g ^ (rb & 15)) << 3));
      cs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, frag, cs, 0, 0, 0);
    }
    if (lane < 32) colsum[32 * wave + lane] = cs[0];
  }
}

// ---- forward.  One workgroup = 128 queries of hpb heads of a line (a64_heads_per_block), one head after the other; 4 waves x 32 queries; keys in
// tiles of 128, online softmax across tiles.
//   S^T tile (32 keys x 32 q) = mfma(A = K rows from LDS, B = Q^T from registers), 4 k-steps
//   P^T (bf16, packed in place) = the B operand of  O^T (32 d x 32 q) += mfma(A = V^T via ds_read_b64_tr_b16, B = P^T), 2 d-tiles
// Who waits for whom, as written: loop top: K(kt) landed (V(kt), the newest four DMA instructions, may still fly) | barrier | scores |
// vmcnt(0): own part of V(kt) | barrier: every wave is done with the K image | DMA of K(kt + 1) | softmax | O^T += V^T P^T | barrier | DMA of
// V(kt + 1).  As compiled: hipcc cannot tell an LDS-DMA's destination from the image being read and puts an `s_waitcnt vmcnt(0)` in front of the
// first LDS read behind every DMA, here the first V fragment of the P V cluster - so K(kt + 1) is waited for in the middle of tile kt, under
// the softmax only, not under the P V MFMAs (the behaviour of plain loops described in attention_common.hpp, "Software-pipelined operand
// reads").  Correct either way; it is part of the 12-23 % by which these loops trail the inline-asm head_dim-128 ones.
// KEYS (pero_attention_fwd_keys): line b attends to the keys [k0, k1) of `kr` only (at_key_range, attention_common.hpp: clamped).  A head's stream walks the key
// tiles kt0 .. kt_last that intersect the range - a tile without a live key would leave the running maximum at -inf - and the -inf select covers the dead keys
// of the first and the last of them.  With [0, S): the walk, the MFMAs and the bits of the unmasked kernel.
template <bool KEYS>
__device__ __forceinline__ void attn64_fwd_body(const bf16raw* qkv, const int* kr, bf16raw* out, float* lse2, int S, int nh, int hpb, float c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* kimg = smem;
  unsigned char* vimg = smem + A64_TILE_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h5 = lane >> 5, r = lane & 31;
  const int nb = (S + 127) >> 7;
  int lg, qb;
  const int ngrp = nh / hpb;   // hpb heads of a line are walked as ONE stream of (head, key tile) units: the next head's first K / V tiles and Q rows are
                               // requested under the current head's last tile and output stores
  attn_block_map(blockIdx.x, nb, gridDim.x / nb, lg, qb);
  const int line = lg / ngrp, head0 = (lg % ngrp) * hpb;
  const long long d = (long long)nh * 64, ld = 3 * d;
  const bf16raw* lbase = qkv + (long long)line * S * ld;
  const bf16raw* base = lbase + head0 * 64;
  at_key_range rng = {0, S};
  if constexpr (KEYS) rng = at_load_key_range(kr, line, S);
  const int kt0 = KEYS ? rng.k0 >> 7 : 0;                       // the line's first live key tile
  const int nkt = KEYS ? ((rng.k1 + 127) >> 7) - kt0 : nb;      // live key tiles of a head
  const int kt_last = kt0 + nkt - 1;
  const int units = hpb * nkt;  // q ; + d : k ; + 2d : v
  const int q = qb * 128 + wave * 32 + r;  // this lane's query (both lane halves hold the same query)
  const int qc = q < S - 1 ? q : S - 1;    // a query >= S computes on a copy of the line's last row and stores nothing

  a64_glds<4>(base + d + (long long)kt0 * 128 * ld, ld, kimg, wave, lane, S - 1 - kt0 * 128);
  a64_glds<4>(base + 2 * d + (long long)kt0 * 128 * ld, ld, vimg, wave, lane, S - 1 - kt0 * 128);
  bf8v qf[4];
  {
    const bf16raw* qrow = base + (long long)qc * ld + 8 * h5;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) qf[ks] = *(const bf8v*)(qrow + 16 * ks);
  }
  f16v o[2];
  o[0] = (f16v){0};
  o[1] = (f16v){0};
  float m = -INFINITY, l = 0.f;

  for (int u = 0; u < units; u++) {
    const int head = head0 + u / nkt, kt = kt0 + u % nkt;
    if (u > 0) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // K(kt) landed
    f16v s[4];
    AT_PRIO(1);   // this wave's MFMA cluster goes ahead of the other wave's softmax instructions on the same SIMD
#pragma unroll
    for (int t = 0; t < 4; t++) {
      s[t] = (f16v){0};
#pragma unroll
      for (int ks = 0; ks < 4; ks++)
        s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a64_row_frag(kimg, t * 32 + r, ks, h5), qf[ks], s[t], 0, 0, 0);
    }
    AT_PRIO(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // own part of V(kt)
    __syncthreads();  // every wave is done with the K image; V(kt) landed
    const int nhd = head0 + (u + 1) / nkt, nkt_i = kt0 + (u + 1) % nkt;
    if (u + 1 < units) a64_glds<4>(lbase + nhd * 64 + d + (long long)nkt_i * 128 * ld, ld, kimg, wave, lane, S - 1 - nkt_i * 128);

    if constexpr (KEYS) {
      if (kt == kt0 || kt == kt_last) {
        // the first and the last live tile: scores of keys outside [k0, k1) become -inf, so their P is exactly 0; each of the two holds a live key
        const int lo = rng.k0 - kt * 128 - 4 * h5, hi = rng.k1 - kt * 128 - 4 * h5;
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const int k = 32 * t + 8 * (e >> 2) + (e & 3);
            s[t][e] = (k >= lo && k < hi) ? s[t][e] : -INFINITY;
          }
      }
    } else if (kt == nb - 1 && (S & 127)) {
      // the line's ragged last key tile: scores of keys >= S (copies of the last key's) become -inf in front of the running maximum, so their
      // P is exactly 0; the tile holds at least one real key.  Key of s[t][e] = 32 t + 8 (e >> 2) + 4 h5 + (e & 3)
      const int lim = S - kt * 128 - 4 * h5;
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) s[t][e] = (32 * t + 8 * (e >> 2) + (e & 3) < lim) ? s[t][e] : -INFINITY;
    }
    // ---- online softmax, all lane-local except one lane^32 exchange per reduction
    float mx = s[0][0];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) mx = fmaxf(mx, s[t][e]);
    {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
      mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    }
    const float mn = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * c);  // exp2(-inf) = 0 on the first tile
    const float mc = mn * c;
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const float p = __builtin_amdgcn_exp2f(fmaf(s[t][e], c, -mc));
        s[t][e] = p;
        ps += p;
      }
    {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(ps), __float_as_uint(ps), false, false);
      ps = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    l = l * alpha + ps;
    m = mn;
    if (kt != kt0) {  // (the first tile: O is still zero)
#pragma unroll
      for (int t = 0; t < 2; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) o[t][e] *= alpha;
    }

    // ---- O^T += V^T P^T
    AT_PRIO(1);
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
      for (int sub = 0; sub < 2; sub++) {
        const bf8v pf = pack8(s[t], sub);
#pragma unroll
        for (int dt = 0; dt < 2; dt++)
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a64_tr_frag(vimg, t * 32 + sub * 16, dt, lane), pf, o[dt], 0, 0, 0);
      }
    }
    AT_PRIO(0);
    if (kt == kt_last) {
      const float inv = 1.0f / l;
#pragma unroll
      for (int t = 0; t < 2; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) o[t][e] *= inv;
      if (h5 == 0 && q < S) lse2[((long long)line * nh + head) * S + q] = m * c + __builtin_amdgcn_logf(l);
      a64_store_tile(o, vimg, out + ((long long)line * S + qb * 128) * d + head * 64, d, nullptr, tid, wave, r, h5, S - qb * 128);
      if (u + 1 < units) {
        o[0] = (f16v){0};
        o[1] = (f16v){0};
        m = -INFINITY;
        l = 0.f;
        const bf16raw* qrow = lbase + (head + 1) * 64 + (long long)qc * ld + 8 * h5;
#pragma unroll
        for (int ks = 0; ks < 4; ks++) qf[ks] = *(const bf8v*)(qrow + 16 * ks);
      }
    }
    if (u + 1 < units) {
      __syncthreads();  // every wave is done with the V image (and with the O staging reads)
      a64_glds<4>(lbase + nhd * 64 + 2 * d + (long long)nkt_i * 128 * ld, ld, vimg, wave, lane, S - 1 - nkt_i * 128);
    }
  }
}
__global__ __launch_bounds__(256, 2) void attn64_fwd_k(const bf16raw* qkv, bf16raw* out, float* lse2, int S, int nh, int hpb, float c) {
  attn64_fwd_body<false>(qkv, nullptr, out, lse2, S, nh, hpb, c);
}
__global__ __launch_bounds__(256, 2) void attn64_fwd_keys_k(const bf16raw* qkv, const int* kr, bf16raw* out, float* lse2, int S, int nh, int hpb, float c) {
  attn64_fwd_body<true>(qkv, kr, out, lse2, S, nh, hpb, c);
}

// ---- backward, dQ: 128 queries of a (line, head), query on the lane, sweeps the keys in 32-key sub-tiles of 64-key halves (K and V half,
// double-buffered: the DMA of the next half is issued ahead of the current one's MFMAs - as compiled, hipcc's `s_waitcnt vmcnt(0)` in front of
// the first LDS read behind it, inside the first MFMA cluster, waits for it there, so only the issue is early, not the overlap; the same holds
// for the next (Q, dO) stage of the dK / dV kernel): S^T = K Q^T, dP^T = V dO^T, dS^T = P^T (dP^T - D) scale,
// dQ^T += K^T dS^T.  Writes D[q] = sum_d dO[q][d] O[q][d] into dvec[(line*S + q)*nh + head] when `out` is given, reads it when `out` is null.
// KEYS (pero_attention_bwd_keys): the sweep takes the 64-key halves h0 .. that intersect the line's [k0, k1) only; the 0 select of dS^T covers the dead keys of the
// first and the last of them.  dQ is computed for every query < S.
template <bool KEYS>
__device__ __forceinline__ void attn64_bwd_dq_body(unsigned char* smem, const bf16raw* qkv, const int* kr, const bf16raw* out, const bf16raw* dout, const float* lse2,
                                                   float* dvec, bf16raw* dqkv, float* part, int S, int nh, float c, float scale) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h5 = lane >> 5, r = lane & 31;
  const int nb = (S + 127) >> 7;
  int lh, qb;
  attn_block_map(blockIdx.x, nb, gridDim.x / nb, lh, qb);
  const int line = lh / nh, head = lh % nh;
  const long long d = (long long)nh * 64, ld = 3 * d;
  const bf16raw* base = qkv + (long long)line * S * ld + head * 64;
  const bf16raw* Kg = base + d;
  const bf16raw* Vg = base + 2 * d;
  const int q = qb * 128 + wave * 32 + r;
  const int qc = q < S - 1 ? q : S - 1;   // a query >= S reads the line's last row; its dS is forced to 0 below
  at_key_range rng = {0, S};
  if constexpr (KEYS) rng = at_load_key_range(kr, line, S);
  const int h0 = KEYS ? rng.k0 >> 6 : 0;   // the line's first live 64-key half

  a64_glds<2>(Kg + (long long)h0 * 64 * ld, ld, smem, wave, lane, S - 1 - h0 * 64);
  a64_glds<2>(Vg + (long long)h0 * 64 * ld, ld, smem + A64_HALF_BYTES, wave, lane, S - 1 - h0 * 64);

  bf8v qf[4], gf[4];
  float dsum = 0.f;
  const long long dix = ((long long)line * S + qc) * nh + head;
  {
    const bf16raw* qrow = base + (long long)qc * ld + 8 * h5;
    const bf16raw* grow = dout + ((long long)line * S + qc) * d + head * 64 + 8 * h5;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
      qf[ks] = *(const bf8v*)(qrow + 16 * ks);
      gf[ks] = *(const bf8v*)(grow + 16 * ks);
    }
    if (out) {
      const bf16raw* orow = out + ((long long)line * S + qc) * d + head * 64 + 8 * h5;
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        const bf8v of = *(const bf8v*)(orow + 16 * ks);
#pragma unroll
        for (int e = 0; e < 8; e++) dsum += (float)gf[ks][e] * (float)of[e];
      }
      dsum += __shfl_xor(dsum, 32, 64);
      if (h5 == 0 && q < S) dvec[dix] = dsum;
    } else {
      dsum = dvec[dix];
    }
  }
  const float lq = lse2[(long long)lh * S + qc];

  f16v dq[2];
  dq[0] = (f16v){0};
  dq[1] = (f16v){0};
  const int nhalf = KEYS ? ((rng.k1 + 63) >> 6) - h0 : (S + 63) >> 6;   // a last half without a key is not swept; keys: live halves only
  for (int hk = 0; hk < nhalf; hk++) {   // half h0 + hk of the line, in buffer hk & 1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // half hk landed; every wave is done with the other buffer
    const unsigned char* kimg = smem + (hk & 1) * 2 * A64_HALF_BYTES;
    const unsigned char* vimg = kimg + A64_HALF_BYTES;
    if (hk + 1 < nhalf) {
      unsigned char* nbuf = smem + ((hk + 1) & 1) * 2 * A64_HALF_BYTES;
      a64_glds<2>(Kg + (long long)(h0 + hk + 1) * 64 * ld, ld, nbuf, wave, lane, S - 1 - (h0 + hk + 1) * 64);
      a64_glds<2>(Vg + (long long)(h0 + hk + 1) * 64 * ld, ld, nbuf + A64_HALF_BYTES, wave, lane, S - 1 - (h0 + hk + 1) * 64);
    }
#pragma unroll
    for (int t = 0; t < 2; t++) {  // 32-key sub-tile
      f16v s = {0}, dp = {0};
      AT_PRIO(1);
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a64_row_frag(kimg, t * 32 + r, ks, h5), qf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a64_row_frag(vimg, t * 32 + r, ks, h5), gf[ks], dp, 0, 0, 0);
      }
      AT_PRIO(0);
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const float p = __builtin_amdgcn_exp2f(fmaf(s[e], c, -lq));
        s[e] = p * (dp[e] - dsum) * scale;  // dS^T
      }
      if constexpr (KEYS) {
        if (hk == 0 || hk == nhalf - 1 || qb == nb - 1) {
          // dS^T selected to 0 for keys outside [k0, k1) (the first and the last live half) and queries >= S (the last query block)
          const int lo = rng.k0 - (h0 + hk) * 64 - t * 32 - 4 * h5;
          const int hi = q < S ? rng.k1 - (h0 + hk) * 64 - t * 32 - 4 * h5 : lo;
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const int k = 8 * (e >> 2) + (e & 3);
            s[e] = (k >= lo && k < hi) ? s[e] : 0.f;
          }
        }
      } else if (hk == nhalf - 1 || qb == nb - 1) {
        // dS^T selected to 0 for keys >= S (the line's last half) and queries >= S (its last query block): the staged dQ rows of such
        // queries are exact zeros.  Key of s[e] inside the sub-tile = 8 (e >> 2) + 4 h5 + (e & 3)
        const int lim = q < S ? S - hk * 64 - t * 32 - 4 * h5 : 0;
#pragma unroll
        for (int e = 0; e < 16; e++) s[e] = (8 * (e >> 2) + (e & 3) < lim) ? s[e] : 0.f;
      }
      AT_PRIO(1);
#pragma unroll
      for (int sub = 0; sub < 2; sub++) {
        const bf8v dsf = pack8(s, sub);
#pragma unroll
        for (int dt = 0; dt < 2; dt++)
          dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a64_tr_frag(kimg, t * 32 + sub * 16, dt, lane), dsf, dq[dt], 0, 0, 0);
      }
      AT_PRIO(0);
    }
  }
  // partial-sum workspace of the bias gradient [3][workgroups][64] (q, k, v); this kernel fills plane 0
  a64_store_tile(dq, smem, dqkv + ((long long)line * S + qb * 128) * ld + head * 64, ld, part ? part + ((long long)lh * nb + qb) * 64 : nullptr,
                 tid, wave, r, h5, S - qb * 128);
}
__global__ __launch_bounds__(256, 2) void attn64_bwd_dq_k(const bf16raw* qkv, const bf16raw* out, const bf16raw* dout, const float* lse2,
                                                          float* dvec, bf16raw* dqkv, float* part, int S, int nh, float c, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  attn64_bwd_dq_body<false>(smem, qkv, nullptr, out, dout, lse2, dvec, dqkv, part, S, nh, c, scale);
}
__global__ __launch_bounds__(256, 2) void attn64_bwd_dq_keys_k(const bf16raw* qkv, const int* kr, const bf16raw* out, const bf16raw* dout, const float* lse2,
                                                               float* dvec, bf16raw* dqkv, float* part, int S, int nh, float c, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  attn64_bwd_dq_body<true>(smem, qkv, kr, out, dout, lse2, dvec, dqkv, part, S, nh, c, scale);
}

// ---- backward, dK and dV in one pass: 128 keys, key on the lane, the workgroup's V tile resident in LDS, Q / dO in 32-query stages
// (double-buffered) with their row statistics (lse2, D): S = Q K^T, P, dP = dO V^T, dS; dV^T += dO^T P, dK^T += Q^T dS.
// KEYS (pero_attention_bwd_keys): every query < S is swept; the staged dK / dV rows of the keys outside the line's [k0, k1) are zeroed the way keys >= S are (a dead
// key's P may overflow: it stays in that key's MFMA column and is SELECTED away).  A tile wholly outside the range sweeps nothing and still stores zero rows for
// its real keys (dqkv arrives uninitialised) and zero partial rows of the bias gradient.
template <bool KEYS>
__device__ __forceinline__ void attn64_bwd_dkv_body(unsigned char* smem, const bf16raw* qkv, const int* kr, const bf16raw* dout, const float* lse2, const float* dvec,
                                                    bf16raw* dqkv, float* part, int S, int nh, float c, float scale) {
  unsigned char* vimg = smem + 4 * A64_SUB_BYTES;
  float* lds_ld = (float*)(smem + 4 * A64_SUB_BYTES + A64_TILE_BYTES);  // [2 buffers][32 lse2 | 32 D]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h5 = lane >> 5, r = lane & 31;
  const int nb = (S + 127) >> 7;
  int lh, kb;
  attn_block_map(blockIdx.x, nb, gridDim.x / nb, lh, kb);
  const long long nwg = gridDim.x;
  const int line = lh / nh, head = lh % nh;
  const long long d = (long long)nh * 64, ld = 3 * d;
  const bf16raw* base = qkv + (long long)line * S * ld + head * 64;
  const bf16raw* Gg = dout + (long long)line * S * d + head * 64;
  const int key = kb * 128 + wave * 32 + r;
  const int kc = key < S - 1 ? key : S - 1;   // a key >= S computes on the line's last row; its dK / dV rows are zeroed below
  // row statistics of a 32-query stage: threads 0-31 load lse2[lh][q], threads 32-63 load D[(line*S + q)*nh + head], q clamped to S - 1
  auto stat_at = [&](int sq) -> float {
    const int qs0 = sq * 32 + (tid & 31), qs = qs0 < S - 1 ? qs0 : S - 1;
    return tid < 32 ? lse2[(long long)lh * S + qs] : dvec[((long long)line * S + qs) * nh + head];
  };

  if (tid < 64) lds_ld[tid] = stat_at(0);
  a64_glds<4>(base + 2 * d + (long long)kb * 128 * ld, ld, vimg, wave, lane, S - 1 - kb * 128);  // this workgroup's V tile, resident
  a64_glds<1>(base, ld, smem, wave, lane, S - 1);
  a64_glds<1>(Gg, d, smem + A64_SUB_BYTES, wave, lane, S - 1);

  bf8v kf[4];
  {
    const bf16raw* krow = base + d + (long long)kc * ld + 8 * h5;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) kf[ks] = *(const bf8v*)(krow + 16 * ks);
  }
  f16v dv[2], dk[2];  // dV^T, dK^T: 32 d x 32 keys per tile, key on the lane
#pragma unroll
  for (int t = 0; t < 2; t++) { dv[t] = (f16v){0}; dk[t] = (f16v){0}; }
  at_key_range rng = {0, S};
  if constexpr (KEYS) rng = at_load_key_range(kr, line, S);
  const bool dead_tile = KEYS && (kb * 128 >= rng.k1 || kb * 128 + 128 <= rng.k0);
  const int nsub = dead_tile ? 0 : (S + 31) >> 5;   // stages without a query are not swept
  for (int sq = 0; sq < nsub; sq++) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage sq (Q / dO rows + statistics) landed; every wave is done with the other buffers
    const unsigned char* qimg = smem + (sq & 1) * 2 * A64_SUB_BYTES;
    const unsigned char* gimg = qimg + A64_SUB_BYTES;
    const float* lds_l = lds_ld + (sq & 1) * 64;
    const float* lds_d = lds_l + 32;
    float nstat = 0.f;
    if (sq + 1 < nsub) {
      if (tid < 64) nstat = stat_at(sq + 1);  // before the DMA: vmcnt is in-order
      unsigned char* nbuf = smem + ((sq + 1) & 1) * 2 * A64_SUB_BYTES;
      a64_glds<1>(base + (long long)(sq + 1) * 32 * ld, ld, nbuf, wave, lane, S - 1 - (sq + 1) * 32);
      a64_glds<1>(Gg + (long long)(sq + 1) * 32 * d, d, nbuf + A64_SUB_BYTES, wave, lane, S - 1 - (sq + 1) * 32);
    }
    // rows q = (e&3) + 8(e>>2) + 4*h5 of the 32-query stage on the registers, key on the lane
    f16v s = {0}, dp = {0};
    AT_PRIO(1);
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a64_row_frag(qimg, r, ks, h5), kf[ks], s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a64_row_frag(gimg, r, ks, h5), a64_row_frag(vimg, wave * 32 + r, ks, h5), dp, 0, 0, 0);
    }
    AT_PRIO(0);
    const int qlim = S - sq * 32 - 4 * h5;   // queries >= S (the last stage): P = 0, so dS = 0 (its other factor is finite)
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {
      const f4v l4 = *(const f4v*)(lds_l + 8 * g4 + 4 * h5);
      const f4v d4 = *(const f4v*)(lds_d + 8 * g4 + 4 * h5);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float p = __builtin_amdgcn_exp2f(fmaf(s[4 * g4 + e], c, -l4[e]));
        p = (8 * g4 + e < qlim) ? p : 0.f;
        s[4 * g4 + e] = p;                                         // P
        dp[4 * g4 + e] = p * (dp[4 * g4 + e] - d4[e]) * scale;     // dS
      }
    }
    AT_PRIO(1);
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      const bf8v pf = pack8(s, sub), dsf = pack8(dp, sub);
#pragma unroll
      for (int dt = 0; dt < 2; dt++) {
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a64_tr_frag(gimg, sub * 16, dt, lane), pf, dv[dt], 0, 0, 0);   // dV^T += dO^T P
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a64_tr_frag(qimg, sub * 16, dt, lane), dsf, dk[dt], 0, 0, 0);  // dK^T += Q^T dS
      }
    }
    AT_PRIO(0);
    if (sq + 1 < nsub && tid < 64) lds_ld[((sq + 1) & 1) * 64 + tid] = nstat;  // visible after the next barrier
  }
  if constexpr (KEYS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // a dead tile ran no stage: its prologue's LDS-DMA must land before the staging writes
  {   // keys >= S computed on a copy of the last key (keys outside the range: on dead operands): their staged dK / dV rows are exact zeros
    const bool live = KEYS ? (key >= rng.k0 && key < rng.k1) : key < S;
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) { dk[t][e] = live ? dk[t][e] : 0.f; dv[t][e] = live ? dv[t][e] : 0.f; }
  }
  bf16raw* tile_o = dqkv + ((long long)line * S + kb * 128) * ld + d + head * 64;  // dK tile; dV tile = + d columns
  // planes 1 (dK) and 2 (dV) of the partial-sum workspace, nwg = (line, head) x key blocks entries each
  a64_store_tile(dk, smem, tile_o, ld, part ? part + (nwg + (long long)lh * nb + kb) * 64 : nullptr, tid, wave, r, h5, S - kb * 128);
  a64_store_tile(dv, smem, tile_o + d, ld, part ? part + (2 * nwg + (long long)lh * nb + kb) * 64 : nullptr, tid, wave, r, h5, S - kb * 128);
}
__global__ __launch_bounds__(256, 2) void attn64_bwd_dkv_k(const bf16raw* qkv, const bf16raw* dout, const float* lse2, const float* dvec,
                                                           bf16raw* dqkv, float* part, int S, int nh, float c, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  attn64_bwd_dkv_body<false>(smem, qkv, nullptr, dout, lse2, dvec, dqkv, part, S, nh, c, scale);
}
__global__ __launch_bounds__(256, 2) void attn64_bwd_dkv_keys_k(const bf16raw* qkv, const int* kr, const bf16raw* dout, const float* lse2, const float* dvec,
                                                                bf16raw* dqkv, float* part, int S, int nh, float c, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  attn64_bwd_dkv_body<true>(smem, qkv, kr, dout, lse2, dvec, dqkv, part, S, nh, c, scale);
}

// Heads per forward workgroup: the largest divisor of num_heads that keeps >= 4 workgroups per CU - two rounds of the two resident ones.  Measured
// (forward, d = 512, 8 heads, us, 1 / 2 / 4 / 8 heads per workgroup): N = 2048: S = 256 640 / 596 / 581 / 574, S = 260 1094 / 1034 / 1008 / 1012,
// S = 36 160 / 146 / 139 / 138; N = 256: S = 256 77 / 74 / 72 / 72, S = 260 132 / 128 / 129 / 146 - the last one is 768 workgroups, one and a
// half rounds, which is why the bound is 4 per CU and not the 2 of attn_heads_per_block (attention_fwd.hip).  Same bits for every value.
// Lines of more than three key tiles keep one head per workgroup: the stream hides a workgroup's prologue and epilogue, whose share falls with
// the tiles per head, and at N S = 65 536 rows four heads per workgroup measured 143 / 229 / 391 us at S = 512 / 1024 / 2048 against 135 / 216 /
// 366 with one (separate runs).
static int a64_heads_per_block(int64_t N, int64_t S, int64_t nh) {
  const long long num_cus = pero_num_cus();
  if (S > 3 * 128) return 1;
  for (int cand = (int)nh; cand > 1; cand--)
    if (nh % cand == 0 && N * ((S + 127) / 128) * (nh / cand) >= 4 * num_cus) return cand;
  return 1;
}
extern "C" int pero_attention_hd64_heads_per_block(int64_t N, int64_t S, int64_t num_heads) {
  PERO_REQUIRE(N > 0 && S > 0 && num_heads > 0, "pero_attention_hd64_heads_per_block: N, S, num_heads > 0");
  return a64_heads_per_block(N, S, num_heads);
}

// ---- launchers (declared in attention_common.hpp): the callers have validated the arguments and check the launch.  kr null: the plain kernels;
// else the `_keys_k` ones - same grids, same heads per workgroup.
void attn64_fwd_launch(const void* qkv, const int* kr, void* out, float* lse, int64_t N, int64_t S, int64_t num_heads, hipStream_t st) {
  const float c = (float)(1.4426950408889634 / sqrt(64.0));
  const int64_t nb = (S + 127) / 128;
  const int hpb = a64_heads_per_block(N, S, num_heads);
  const dim3 grid((unsigned)(N * (num_heads / hpb) * nb)), block(256);
  if (kr) hipLaunchKernelGGL(attn64_fwd_keys_k, grid, block, A64_FWD_LDS, st, (const bf16raw*)qkv, kr, (bf16raw*)out, lse, (int)S, (int)num_heads, hpb, c);
  else hipLaunchKernelGGL(attn64_fwd_k, grid, block, A64_FWD_LDS, st, (const bf16raw*)qkv, (bf16raw*)out, lse, (int)S, (int)num_heads, hpb, c);
}
// The same two kernels whether D is computed (`out` given) or handed in (`out` null): dqkv is bit-identical between the two forms.
void attn64_bwd_launch(const void* qkv, const int* kr, const void* out, const void* dout, const float* lse, float* dvec, void* dqkv, float* dbias, float* work,
                       int64_t N, int64_t S, int64_t num_heads, hipStream_t st) {
  const float scale = (float)(1.0 / sqrt(64.0));
  const float c = (float)(1.4426950408889634 / sqrt(64.0));
  const int64_t nb = (S + 127) / 128;   // query blocks = key blocks of a line
  const dim3 grid((unsigned)(N * num_heads * nb)), block(256);
  const bf16raw *q_ = (const bf16raw*)qkv, *o_ = (const bf16raw*)out, *g_ = (const bf16raw*)dout;
  bf16raw* dq_ = (bf16raw*)dqkv;
  float* const part = dbias ? work : nullptr;   // 3 * N * num_heads * nb * 64 floats: half of what ops.attention_bwd_fused allocates
  if (kr) {
    hipLaunchKernelGGL(attn64_bwd_dq_keys_k, grid, block, A64_DQ_LDS, st, q_, kr, o_, g_, lse, dvec, dq_, part, (int)S, (int)num_heads, c, scale);
    hipLaunchKernelGGL(attn64_bwd_dkv_keys_k, grid, block, A64_DKV_LDS, st, q_, kr, g_, lse, dvec, dq_, part, (int)S, (int)num_heads, c, scale);
  } else {
    hipLaunchKernelGGL(attn64_bwd_dq_k, grid, block, A64_DQ_LDS, st, q_, o_, g_, lse, dvec, dq_, part, (int)S, (int)num_heads, c, scale);
    hipLaunchKernelGGL(attn64_bwd_dkv_k, grid, block, A64_DKV_LDS, st, q_, g_, lse, dvec, dq_, part, (int)S, (int)num_heads, c, scale);
  }
  if (dbias) attn_bias_reduce_launch<64>(work, dbias, N, num_heads, nb, st);
}
