// Persistent backward of the fused attention at S = 256: attn_bwd_lh_k takes ONE (line, head) per workgroup pass - eight waves, one workgroup
// per CU - and attn_bwd_lh_launch launches it.  Optional (pero_set_option("attn_lh")): pero_attention_bwd (attention_bwd.hip) decides whether
// it runs and launches attn_bias_reduce_k behind it.  This file: the LH_* layout of the workgroup's LDS, the lh_* asm wrappers only this
// kernel uses (the others: attention_common.hpp), lh_store_matrix (the epilogue of one output matrix), the kernel, the launcher.
//
// What the two-workgroups-per-CU kernels of attention_bwd.hip are bound by is neither MFMA nor LDS nor HBM bandwidth: with every MFMA or every
// exponential compiled out they run at the same speed (ablation builds, realistic inputs: -1 %), while without the loop's LDS-DMA
// or without the output tiles they gain 11 % / 20 %.  They move 2.0 GB in ~740 us (2.7 TB/s) with at most one 32 KiB stage in flight per
// workgroup, and every workgroup pays its first loads and its last stores in full: memory-level parallelism is the bound.  Here a
// workgroup owns 128 KiB of LDS as a ring of four 32 KiB slots and streams a whole (line, head) through it with the loads THREE items
// ahead of the MFMAs, every vector-memory instruction issued by inline asm and waited for by a COUNTED vmcnt (the counter retires in
// order; the schedule below is static, so the counts are constants), and it loops over (line, head) units so that the next unit's
// first loads fly under the current unit's last stores:
//
//   phase Q (dQ^T of the 256 queries; wave w owns queries 32w..32w+31 on its lanes; Q / dO row fragments, lse and D in registers):
//       items H0..H3 = 64-key halves (K image 16 KiB + V image 16 KiB) in slots 0..3;   per half: the fragment sequence of attn_bwd_dq_body_p
//   phase K (dK^T / dV^T of the 256 keys; wave w owns keys 32w..32w+31; K row fragments in registers):
//       items V0, V1 = the V block (256 keys x 256 B) in slots 0, 1 (B operand of dP), items T0..T7 = 32-query stages (Q image 8 KiB +
//       dO image 8 KiB + 256 B of row statistics) in the four 16 KiB sub-slots of slots 2, 3;   per stage: the sequence of attn_bwd_dkv2_body_p
//
//   per-thread vector-memory program order of a unit in steady state ([n] = instructions; `newer` = issued after the awaited item):
//       (end of the previous unit)  H0 H1 H2 H3 [4 x 4]   dK rows [8]   F: Q / dO fragments, lse, D [18] (their registers are free once dK has left)   dV rows [8]
//       half 0: wait F - and with it the older H0..H3, which have had the whole epilogue to land - (newer 8) | barrier | previous unit's bias
//               partials [1] | MFMAs          halves 1..3: MFMAs (everything is resident: no barrier, no wave waits for another)
//       (the first unit of a workgroup issues F, then H0..H3, and waits for all of it)
//       barrier | issue V0 V1 [4 + 4], K fragments [8], T0 T1 T2 T3 [4 x 3] | epilogue Q: dQ rows [8]
//       stage 0: wait V0 V1, the K fragments and T0 (newer: T1 T2 T3 9 + 8 = 17) | barrier | MFMAs
//       stage j = 1..3: wait Tj (14) | barrier | issue T(j+3) [3] | MFMAs     stage 4: wait (6) | barrier | issue T7 | MFMAs     stages 5, 6, 7: wait (6, 3, 0)
//       barrier | issue the next unit's H0..H3 | epilogue K: dK rows, the next unit's F, dV rows
//   A slot is refilled only behind the barrier that follows its last reader; LDS reads are asm too (the compiler would put a vmcnt(0)
//   in front of any LDS read it can see behind an LDS-DMA).  The same MFMAs in the same order as the tiled kernels: dqkv is bit-identical.
// Output tiles leave through a wave-private 2 KiB staging block, 16 rows x 64 columns at a time (lh_store_matrix); the
// column sums of the stored values (in_proj's bias gradient) are reduced over the eight waves through LDS: one partial row per unit.
#include "attention_common.hpp"

#define LH_SLOT 32768
#define LH_RING (4 * LH_SLOT)
#define LH_STATS LH_RING                    // 4 sub-slots x 256 B: [32 lse2 | 32 D] of a stage
#define LH_STG (LH_RING + 1024)             // 8 waves x 2 KiB
#define LH_PART (LH_STG + 8 * 2048)         // 8 waves x 3 matrices x 128 floats
#define LH_LDS_BYTES (LH_PART + 8 * 1536)   // 160 768 B of the CU's 163 840

// LDS-DMA, 16 (4) bytes per lane: global address = sbase + voff, LDS address = dst + 16 (4) * lane
// (wait states in front of every asm vector-memory instruction that takes an SGPR base: see attention_common.hpp; with the s_mov the LDS-DMA
// forms have s_nop 3 + 1)
__device__ __forceinline__ void lh_dma16(const void* sbase, unsigned voff, unsigned dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %1, %0" :: "s"(sbase), "v"(voff), "s"(dst) : "memory", "m0");
}
__device__ __forceinline__ void lh_dma4(const float* addr, unsigned dst) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" :: "v"(addr), "s"(dst) : "memory", "m0");
}
__device__ __forceinline__ void lh_gload4(float& d, const void* sbase, unsigned voff) {
  asm volatile("s_nop 4\n\tglobal_load_dword %0, %1, %2" : "=v"(d) : "v"(voff), "s"(sbase) : "memory");
}
template <int N>
__device__ __forceinline__ void lh_wait_vm() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0)" :: "i"(N) : "memory");
}
template <int N_STEADY, int N_FIRST>
__device__ __forceinline__ void lh_wait_vm2(bool first) {
  if (first) lh_wait_vm<N_FIRST>(); else lh_wait_vm<N_STEADY>();
}
template <int OFF>
__device__ __forceinline__ void lh_ds_write4(unsigned addr, float v) {
  asm volatile("ds_write_b32 %0, %1 offset:%2" :: "v"(addr), "v"(v), "i"(OFF) : "memory");
}
__device__ __forceinline__ void lh_ds_read4(float& d, unsigned addr) {
  asm volatile("ds_read_b32 %0, %1" : "=v"(d) : "v"(addr) : "memory");
}

// One 128-column output matrix of a wave (acc[dt][e]: row = this lane's query / key r, columns dt*32 + 8*(e>>2) + 4*h5 + (e&3)) -> global
// rows (pitch `pitch_b` bytes from `obase`) through the wave's private 2 KiB staging block, and its column sums (of the stored bf16
// values) -> the wave's partial row in LDS.  8 stores per thread.
//   * a round = 16 rows x 64 columns, i.e. 128-BYTE row segments on eight adjacent lanes: 64-byte segments (32 rows x 32 columns per round)
//     write at 3.4 TB/s, 128- and 256-byte ones at 5.5 (tools/probe_tilebw.hip) - the first version of this kernel spent 40 % of a unit in
//     its epilogues.  Round order (columns 0-63: rows 0-15, rows 16-31; columns 64-127: ...); the 32 lanes that own a round's rows write.
//   * the rounds are software-pipelined: a wave's LDS operations execute in order, so round r + 1 is written into the SAME block right
//     behind round r's reads without waiting for their data (counted lgkmcnt: S0 S1 | wait S0 | finish 0 | S2 | wait S1 | ...);
//   * the column sums are MFMAs: ones (32 x 16) times the staged 16 x 32 tile read back TRANSPOSED (ds_read_b64_tr_b16: the row index
//     becomes the MFMA's k), accumulated over the two row halves - every lane n then holds the sum of column n, exact in f32.  As
//     cross-lane sums they cost 384 ds_bpermute per wave and unit through the CU's one LDS crossbar (10 us of a 52 us unit,
//     in-kernel stamps), as DPP / v_permlane*_swap arithmetic ~450 vector instructions per matrix (8 us).
__device__ __forceinline__ void lh_store_matrix(const f16v (&acc)[4], unsigned stg, unsigned part, void* obase, unsigned pitch_b, int lane) {
  // (every address below derives from this opaque copy of the lane index: otherwise the compiler computes them once in front of the unit
  //  loop, finds no registers for them and reloads them from scratch inside the epilogue - behind an `s_waitcnt vmcnt(0)` that also waits
  //  for every LDS-DMA in flight)
  asm volatile("" : "+v"(lane));
  const int r = lane & 31, h5 = lane >> 5, rl = r & 15;
  // staging image [16 rows][128 B], 16-byte chunk index XORed with (row & 7)
  const unsigned wa = stg + rl * 128 + 8 * h5;                        // + (((4 * (dt & 1) + g4) ^ (rl & 7)) << 4)
  const int rrow = lane >> 3, rc = lane & 7;                          // read-back: rows rrow, rrow + 8; chunk rc (8 lanes = 128 contiguous bytes)
  const unsigned ra0 = stg + rrow * 128 + ((rc ^ (rrow & 7)) << 4);
  const unsigned ra1 = ra0 + 8 * 128;                                 // (row + 8: same row & 7)
  const unsigned go = (unsigned)rrow * pitch_b + rc * 16;
  // transposed read (B operand, k = row): lane (i = lane & 15, g1, h5) supplies the 8 bytes of row 4 h5 + (i >> 2) (+ 8 for the second
  // read), columns 32 cb + 16 g1 + 4 (i & 3) .. + 3; the hardware hands lane i column 32 cb + 16 g1 + i
  const int ti = lane & 15, tg = (lane >> 4) & 1;
  const int trow = 4 * h5 + (ti >> 2), tch = 2 * tg + ((ti & 3) >> 1);
  const unsigned tq0 = stg + trow * 128 + ((tch ^ (trow & 7)) << 4) + 8 * (ti & 1);          // column block 0, rows trow / trow + 8
  const unsigned tq1 = stg + trow * 128 + (((4 + tch) ^ (trow & 7)) << 4) + 8 * (ti & 1);    // column block 1
  const __bf16 one = (__bf16)1.0f;
  const bf8v ones = {one, one, one, one, one, one, one, one};
  at_u4v v0[4], v1[4];
  bf8v t0[4], t1[4];
  float sums[4];                                                      // column sums of columns 32 b + (lane & 31), b = 0..3
  f16v cs0, cs1;
  auto stage_round = [&](auto rc_) __attribute__((always_inline)) {   // round 2 ch + rh: 8 writes (the 32 lanes of the rows) + 2 reads + 4 transposed reads
    constexpr int rd = decltype(rc_)::value;
    constexpr int ch = rd >> 1, rh = rd & 1;
    if ((r >> 4) == rh) {
#pragma unroll
      for (int dl = 0; dl < 2; dl++)
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) {
          const at_u2v w = {pack2bf(acc[2 * ch + dl][4 * g4 + 0], acc[2 * ch + dl][4 * g4 + 1]),
                            pack2bf(acc[2 * ch + dl][4 * g4 + 2], acc[2 * ch + dl][4 * g4 + 3])};
          lh_ds_write8(wa + (((4 * dl + g4) ^ (rl & 7)) << 4), w);
        }
    }
    lh_ds_read16(v0[rd], ra0);
    lh_ds_read16(v1[rd], ra1);
    at_rdtr<0, 8 * 128>(t0[rd], tq0, tq0, 0u);
    at_rdtr<0, 8 * 128>(t1[rd], tq1, tq1, 0u);
  };
  auto finish_round = [&](auto rc_) __attribute__((always_inline)) {  // 2 global stores; the round's share of the column sums
    constexpr int rd = decltype(rc_)::value;
    constexpr int ch = rd >> 1, rh = rd & 1;
    void* ob = (unsigned char*)obase + (long long)(16 * rh) * pitch_b;
    lh_gstore16<ch * 128>(v0[rd], ob, go);
    lh_gstore16<ch * 128>(v1[rd], (unsigned char*)ob + 8LL * pitch_b, go);
    if constexpr (rh == 0) {
      cs0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, t0[rd], (f16v){0}, 0, 0, 0);
      cs1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, t1[rd], (f16v){0}, 0, 0, 0);
    } else {
      cs0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, t0[rd], cs0, 0, 0, 0);
      cs1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, t1[rd], cs1, 0, 0, 0);
      sums[2 * ch] = cs0[0] + 0.0f;        // (through the vector ALU: the compiler pads the MFMA -> read hazard for its own instructions)
      sums[2 * ch + 1] = cs1[0] + 0.0f;
    }
  };
  stage_round(std::integral_constant<int, 0>{});
  stage_round(std::integral_constant<int, 1>{});
  asm volatile("s_waitcnt lgkmcnt(14)" : "+v"(v0[0]), "+v"(v1[0]), "+v"(t0[0]), "+v"(t1[0]) :: "memory");     // behind S0: S1 = 14
  finish_round(std::integral_constant<int, 0>{});
  stage_round(std::integral_constant<int, 2>{});
  asm volatile("s_waitcnt lgkmcnt(14)" : "+v"(v0[1]), "+v"(v1[1]), "+v"(t0[1]), "+v"(t1[1]) :: "memory");
  finish_round(std::integral_constant<int, 1>{});
  stage_round(std::integral_constant<int, 3>{});
  asm volatile("s_waitcnt lgkmcnt(14)" : "+v"(v0[2]), "+v"(v1[2]), "+v"(t0[2]), "+v"(t1[2]) :: "memory");
  finish_round(std::integral_constant<int, 2>{});
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v0[3]), "+v"(v1[3]), "+v"(t0[3]), "+v"(t1[3]) :: "memory");
  finish_round(std::integral_constant<int, 3>{});
  const unsigned pa = part + r * 4;          // lanes n and n + 32 hold the same sums and write the same address
  lh_ds_write4<0>(pa, sums[0]);
  lh_ds_write4<128>(pa, sums[1]);
  lh_ds_write4<256>(pa, sums[2]);
  lh_ds_write4<384>(pa, sums[3]);
}

#ifndef LH_STAGGER
#define LH_STAGGER 0
#endif
#ifndef LH_STAGGER_K
#define LH_STAGGER_K 0
#endif
#ifndef LH_QPOOL
#define LH_QPOOL 4     // fragment register sets of phase Q (LH_QPOOL - 1 in flight): the kernel is bound by its memory pipeline, not by LDS latency
#endif
#ifndef LH_KPOOL
#define LH_KPOOL 4     // ... of phase K (row fragments LH_KPOOL - 2, transposed fragments LH_KPOOL - 1 in flight)
#endif
__device__ __forceinline__ constexpr int lh_q_after(int j) {   // LDS instructions issued after fragment j's when it is consumed (phase Q)
  int n = 0;
  for (int k = j + 1; k <= j + LH_QPOOL - 1 && k < 48; k++) n += dq_ninstr(k);
  return n;
}
__global__ __launch_bounds__(512, 2) void attn_bwd_lh_k(const bf16raw* qkv, const bf16raw* dout, const float* lse2, const float* dvec, bf16raw* dqkv,
                                                        float* work, int nunits, int nh, float c, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int S = 256;
  const int tid = threadIdx.x, lane = tid & 63, h5 = lane >> 5, r = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = gridDim.x;
  const long long d = (long long)nh * 128, ld = 3 * d;
  const unsigned pq = (unsigned)(ld * 2), pg = (unsigned)(d * 2);    // row pitches in bytes: qkv / dqkv rows, dO rows
  const unsigned s0 = at_lds_addr(smem);

  // ---- per-thread constants
  // LDS-DMA piece of a tile image: row 4 * wave + (lane >> 4) (+ 32 per further piece), 16-byte chunk (lane & 15) ^ img_f(row)
  const int drow = 4 * wave + (lane >> 4);
  const unsigned dq_off = (unsigned)drow * pq + (((lane & 15) ^ img_f(drow)) << 4);   // in q / k / v rows
  const unsigned dg_off = (unsigned)drow * pg + (((lane & 15) ^ img_f(drow)) << 4);   // in dO rows
  const unsigned ddst = wave * 1024;                                                   // piece `wave` of an image (+ 8192 per further piece)
  // row fragments from global memory: this lane's row (query / key 32 * wave + r), 16 bytes at 32 * ks + 16 * h5
  const unsigned fq_off = (unsigned)(32 * wave + r) * pq + 16 * h5;
  const unsigned fg_off = (unsigned)(32 * wave + r) * pg + 16 * h5;
  // fragment read offsets inside an LDS stage (as in the _p bodies of attention_bwd.hip)
  // (one register per kind: the offset of k-step ks is ra0 ^ (32 * ks), that of head-dim tile dt is ta0 ^ (64 * dt) - see at_rd128x)
  unsigned ra0, ta0, tb0;
  {
    ra0 = (unsigned)(r * 256 + ((h5 ^ img_f(r)) << 4));
    const int i = lane & 15, g1 = (lane >> 4) & 1;
    const int row = 4 * h5 + (i >> 2);
    const int ch = 2 * g1 + ((i & 3) >> 1);
    ta0 = (unsigned)(row * 256 + ((ch ^ img_f(row)) << 4) + 8 * (i & 1));
    tb0 = (unsigned)((row + 8) * 256 + ((ch ^ img_f(row + 8)) << 4) + 8 * (i & 1));
  }
  const unsigned stg = s0 + LH_STG + wave * 2048, part = s0 + LH_PART + wave * 1536;

  // ---- unit-dependent bases (uniform)
  const bf16raw *uq, *ug;          // Q rows of the unit's (line, head); dO rows
  const float *ul, *ud;            // lse2 row of the unit; D[(line * S + 0) * nh + head]
  auto set_unit = [&](int u) {
    const int line = u / nh, head = u % nh;
    uq = qkv + (long long)line * S * ld + head * 128;
    ug = dout + (long long)line * S * d + head * 128;
    ul = lse2 + (long long)u * S;
    ud = dvec + (long long)line * S * nh + head;
  };
  bf8v qf[8], gf[8], kf[8];
  float lq, dsum;
  // F: this lane's Q / dO row fragments, lse and D of unit u  [18]
  auto issue_F = [&](const bf16raw* q_, const bf16raw* g_, const float* l_, const float* d_) {
    at_static_for<0, 8>([&](auto kc) __attribute__((always_inline)) { constexpr int ks = decltype(kc)::value; lh_gload16<32 * ks>(qf[ks], q_, fq_off); });
    at_static_for<0, 8>([&](auto kc) __attribute__((always_inline)) { constexpr int ks = decltype(kc)::value; lh_gload16<32 * ks>(gf[ks], g_, fg_off); });
    lh_gload4(lq, l_, (unsigned)(32 * wave + r) * 4);
    lh_gload4(dsum, d_, (unsigned)(32 * wave + r) * (unsigned)nh * 4);
  };
  // H_h: K rows 64h..64h+63 -> slot h + 0, V rows -> slot h + 16384  [4]
  auto issue_H = [&](const bf16raw* q_, int h) {
    const unsigned char* kb = (const unsigned char*)(q_ + d) + (long long)h * 64 * pq;
    const unsigned char* vb = (const unsigned char*)(q_ + 2 * d) + (long long)h * 64 * pq;
    const unsigned dst = s0 + h * LH_SLOT + ddst;
    lh_dma16(kb, dq_off, dst);
    lh_dma16(kb + 32LL * pq, dq_off, dst + 8192);
    lh_dma16(vb, dq_off, dst + 16384);
    lh_dma16(vb + 32LL * pq, dq_off, dst + 16384 + 8192);
  };
  // V_i: V rows 128i..128i+127 -> slot i  [4]
  auto issue_V = [&](int i) {
    const unsigned char* vb = (const unsigned char*)(uq + 2 * d) + (long long)i * 128 * pq;
    const unsigned dst = s0 + i * LH_SLOT + ddst;
#pragma unroll
    for (int k = 0; k < 4; k++) lh_dma16(vb + (long long)k * 32 * pq, dq_off, dst + k * 8192);
  };
  // T_j: Q rows 32j..32j+31 -> sub-slot j & 3, dO rows -> + 8192, statistics -> LH_STATS + 256 (j & 3)  [3]
  const float* stat_lane = nullptr;   // set per unit: lanes 0-31 -> lse2[q], lanes 32-63 -> D[q]
  auto issue_T = [&](int j) {
    const long long stat_step = lane < 32 ? 32 : 32LL * nh;
    const unsigned sub = s0 + 2 * LH_SLOT + (j & 3) * 16384;
    lh_dma16((const unsigned char*)uq + (long long)j * 32 * pq, dq_off, sub + ddst);
    lh_dma16((const unsigned char*)ug + (long long)j * 32 * pg, dg_off, sub + 8192 + ddst);
    lh_dma4(stat_lane + j * stat_step, s0 + LH_STATS + (j & 3) * 256);
  };
  auto issue_KF = [&]() {   // K row fragments of this lane's key  [8]
    at_static_for<0, 8>([&](auto kc) __attribute__((always_inline)) { constexpr int ks = decltype(kc)::value; lh_gload16<32 * ks>(kf[ks], uq + d, fq_off); });
  };

  // bias-gradient partials of a finished unit: the eight waves' rows summed in wave order -> work[which][unit][128]; called behind a barrier
  // that every wave passes after its epilogue K.  One store per thread (threads 384..511 repeat the first 128: one count for all waves).
  auto reduce_partials = [&](int un) {
    int tq = tid;
    asm volatile("" : "+v"(tq));                   // (opaque: see lh_store_matrix)
    const int e = tq < 384 ? tq : tq - 384;
    float v[8];
#pragma unroll
    for (int w = 0; w < 8; w++) lh_ds_read4(v[w], s0 + LH_PART + w * 1536 + e * 4);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]) :: "memory");
    const float acc = ((((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) + v[5]) + v[6]) + v[7];
    const int which = e >> 7, col = e & 127;
    lh_gstore4(acc, work + (long long)un * 128, ((unsigned)which * (unsigned)nunits * 128u + (unsigned)col) * 4u);   // (uniform base + per-thread offset)
  };
  int uprev = 0;
  int u = blockIdx.x;
  if (u >= nunits) return;
  set_unit(u);
  issue_F(uq, ug, ul, ud);
#pragma unroll
  for (int h = 0; h < 4; h++) issue_H(uq, h);
  bool first = true;

  for (;;) {
    const bool has_next = u + G < nunits;
    stat_lane = lane < 32 ? ul + lane : ud + (long long)(lane & 31) * nh;
    // ============================== phase Q ==============================
    f16v dq[4];
#pragma unroll
    for (int t = 0; t < 4; t++) dq[t] = (f16v){0};
    at_static_for<0, 4>([&](auto hc) __attribute__((always_inline)) {
      constexpr int h = decltype(hc)::value;
      if constexpr (h == 0) {
        // F and - older - H0..H3 (steady state: newer are the 8 dV stores; a workgroup's first unit issued H0..H3 behind F: wait for all)
        lh_wait_vm2<8, 0>(first);
        // the fragments are registers the compiler tracks: tie them to the wait
        asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]), "+v"(qf[4]), "+v"(qf[5]), "+v"(qf[6]), "+v"(qf[7]) :: "memory");
        asm volatile("" : "+v"(gf[0]), "+v"(gf[1]), "+v"(gf[2]), "+v"(gf[3]), "+v"(gf[4]), "+v"(gf[5]), "+v"(gf[6]), "+v"(gf[7]), "+v"(lq), "+v"(dsum) :: "memory");
        lh_barrier();            // all four halves of every thread have landed: the halves below need no further barrier
        if (!first) reduce_partials(uprev);   // the previous unit's bias partials: every wave has left its epilogue (this barrier)  [1]
        // the two waves of a SIMD run the same instruction sequence from the same barrier: left alone they want the matrix pipe at the same
        // time and the vector ALU at the same time.  Waves 4-7 start one MFMA cluster late (LH_STAGGER x 64 cycles), so that one wave's
        // exponentials run under the other's MFMAs (s_setprio 1 inside the clusters keeps them apart)
        if (LH_STAGGER && wave >= 4) __builtin_amdgcn_s_sleep(LH_STAGGER);
      }
      unsigned stage = s0 + h * LH_SLOT;
      asm volatile("" : "+s"(stage));       // (opaque: the address registers below belong to this half only)
      // the fragment addresses of this half in registers: computing them in front of every read (xor + add per LDS instruction) made the
      // vector ALU as busy as the matrix pipe (~3 800 of a wave's instructions per unit against 448 MFMAs)
      unsigned ar[8], at4[4], bt4[4];
#pragma unroll
      for (int ks = 0; ks < 8; ks++) ar[ks] = (ra0 ^ (32u * ks)) + stage;
#pragma unroll
      for (int dt = 0; dt < 4; dt++) { at4[dt] = (ta0 ^ (64u * dt)) + stage; bt4[dt] = (tb0 ^ (64u * dt)) + stage; }
      bf8v fr[LH_QPOOL];
      f16v s, dp;
      bf8v dsf[2];
      auto issue = [&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        constexpr int t = j / 24, qd = j % 24;
        if constexpr (qd < 16) {
          constexpr int ks = qd >> 1, isv = qd & 1;
          at_rd128a<isv * AT_HALF_BYTES + t * 8192>(fr[j % LH_QPOOL], ar[ks]);
        } else {
          constexpr int sub = (qd - 16) >> 2, dt = (qd - 16) & 3;
          at_rdtra<t * 8192 + sub * 4096, t * 8192 + sub * 4096>(fr[j % LH_QPOOL], at4[dt], bt4[dt]);
        }
      };
      at_static_for<0, LH_QPOOL - 1>(issue);
      AT_PRIO(1);
      at_static_for<0, 48>([&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        constexpr int qd = j % 24;
        if constexpr (j + LH_QPOOL - 1 < 48) issue(std::integral_constant<int, j + LH_QPOOL - 1>{});
        if constexpr (qd == 16) {
          AT_PRIO(0);
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const float p = __builtin_amdgcn_exp2f(fmaf(s[e], c, -lq));
            s[e] = p * (dp[e] - dsum) * scale;
          }
          dsf[0] = pack8(s, 0);
          dsf[1] = pack8(s, 1);
          AT_PRIO(1);
        }
        at_wait_lgkm<lh_q_after(j)>(fr[j % LH_QPOOL]);
        if constexpr (qd < 16) {
          constexpr int ks = qd >> 1;
          if constexpr (qd == 0) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j % LH_QPOOL], qf[0], (f16v){0}, 0, 0, 0);
          else if constexpr (qd == 1) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j % LH_QPOOL], gf[0], (f16v){0}, 0, 0, 0);
          else if constexpr ((qd & 1) == 0) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j % LH_QPOOL], qf[ks], s, 0, 0, 0);
          else dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j % LH_QPOOL], gf[ks], dp, 0, 0, 0);
        } else {
          constexpr int sub = (qd - 16) >> 2, dt = (qd - 16) & 3;
          dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j % LH_QPOOL], dsf[sub], dq[dt], 0, 0, 0);
        }
      });
      AT_PRIO(0);
    });
    lh_barrier();                    // every wave is done with the four halves
    // phase K's first items go out here, in front of the dQ epilogue (refilling the slots half by half would need a barrier per half:
    // 0.9 us of wave skew each, measured by in-kernel stamps)
    issue_V(0); issue_V(1);
    issue_KF();
    issue_T(0); issue_T(1); issue_T(2); issue_T(3);
    // dQ rows of this wave: dqkv[(line * S + 32 * wave + row)][head * 128 ..]
    bf16raw* uo = dqkv + (uq - qkv);
    lh_store_matrix(dq, stg, part, (unsigned char*)uo + (long long)(32 * wave) * pq, pq, lane);   // [8]

    // ============================== phase K ==============================
    f16v dv[4], dk[4];
#pragma unroll
    for (int t = 0; t < 4; t++) { dv[t] = (f16v){0}; dk[t] = (f16v){0}; }
    const unsigned vbase = s0 + wave * 8192;     // this wave's 32 rows of the V block (slots 0, 1)
    // (a run-time loop: one copy of the stage's code; the waits and the issues are uniform branches on j8)
    lh_wait_vm<17>();            // V0 V1, the K fragments, T0 (newer: T1 T2 T3 9 + dQ rows 8)
    asm volatile("" : "+v"(kf[0]), "+v"(kf[1]), "+v"(kf[2]), "+v"(kf[3]), "+v"(kf[4]), "+v"(kf[5]), "+v"(kf[6]), "+v"(kf[7]) :: "memory");
#pragma unroll 1
    for (int j8 = 0; j8 < 8; j8++) {
      if (j8 == 0) lh_wait_vm<17>();
      else if (j8 <= 3) lh_wait_vm<14>();
      else if (j8 <= 5) lh_wait_vm<6>();
      else if (j8 == 6) lh_wait_vm<3>();
      else lh_wait_vm<0>();
      lh_barrier();
      if (j8 >= 1 && j8 <= 4) issue_T(j8 + 3);
      if (LH_STAGGER_K && wave >= 4) __builtin_amdgcn_s_sleep(LH_STAGGER_K);
      const unsigned stage = s0 + 2 * LH_SLOT + (j8 & 3) * 16384;
      const unsigned stb = s0 + LH_STATS + (j8 & 3) * 256, sto = 16 * h5;
      bf8v fr[LH_KPOOL];
      f16v s, dp;
      auto issue_r = [&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        constexpr int ks = j / 3, kind = j % 3;
        if constexpr (kind == 0) at_rd128x<0, 32 * ks>(fr[j % LH_KPOOL], ra0, stage);
        else if constexpr (kind == 1) at_rd128x<AT_SUB_BYTES, 32 * ks>(fr[j % LH_KPOOL], ra0, stage);
        else at_rd128x<0, 32 * ks>(fr[j % LH_KPOOL], ra0, vbase);
      };
      at_static_for<0, (LH_KPOOL - 2)>(issue_r);
      AT_PRIO(1);
      at_static_for<0, 24>([&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        constexpr int ks = j / 3, kind = j % 3;
        if constexpr (j + (LH_KPOOL - 2) < 24) issue_r(std::integral_constant<int, j + (LH_KPOOL - 2)>{});
        constexpr int after = (24 - 1 - j) < (LH_KPOOL - 2) ? (24 - 1 - j) : (LH_KPOOL - 2);
        if constexpr (kind == 0) {
          at_wait_lgkm<after>(fr[j % LH_KPOOL]);
          if constexpr (ks == 0) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j % LH_KPOOL], kf[0], (f16v){0}, 0, 0, 0);
          else s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j % LH_KPOOL], kf[ks], s, 0, 0, 0);
        } else if constexpr (kind == 2) {
          at_wait_lgkm<after>(fr[j % LH_KPOOL]);
          asm volatile("" : "+v"(fr[(j - 1) % LH_KPOOL]));
          if constexpr (ks == 0) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[(j - 1) % LH_KPOOL], fr[j % LH_KPOOL], (f16v){0}, 0, 0, 0);
          else dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[(j - 1) % LH_KPOOL], fr[j % LH_KPOOL], dp, 0, 0, 0);
        }
      });
      AT_PRIO(0);
      auto issue_t = [&](auto mc) __attribute__((always_inline)) {
        constexpr int m = decltype(mc)::value;
        constexpr int sub = m >> 3, dt = (m >> 1) & 3, kind = m & 1;
        constexpr int off = sub * 4096 + (kind == 0 ? AT_SUB_BYTES : 0);
        at_rdtrx<off, off, 64 * dt>(fr[m % LH_KPOOL], ta0, tb0, stage);
      };
      f4v l4[4], d4[4];
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
        // LDS instructions issued after this group's statistics (S = 2 reads, T = 2 reads, T m issued only while m < LH_KPOOL - 1):
        //   g0: S1;  g1: S2 T0 T1;  g2: T0 T1 S3 T2 T3;  g3: T2 T3 T4 T5
        constexpr int TDK = LH_KPOOL - 1;
        constexpr int nt01 = 2 * ((0 < TDK) + (1 < TDK)), nt23 = 2 * ((2 < TDK) + (3 < TDK)), nt45 = 2 * ((4 < TDK) + (5 < TDK));
        constexpr int after = g4 == 0 ? 2 : g4 == 1 ? 2 + nt01 : g4 == 2 ? nt01 + 2 + nt23 : nt23 + nt45;
        at_wait_lgkm2<after>(l4[g4], d4[g4]);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[4 * g4 + e], c, -l4[g4][e]));
          s[4 * g4 + e] = p;
          dp[4 * g4 + e] = p * (dp[4 * g4 + e] - d4[g4][e]) * scale;
        }
        if constexpr (g4 == 1) { pf[0] = pack8(s, 0); dsf[0] = pack8(dp, 0); }
        if constexpr (g4 == 3) { pf[1] = pack8(s, 1); dsf[1] = pack8(dp, 1); }
        if constexpr (g4 + 2 < 4) issue_s(std::integral_constant<int, g4 + 2>{});
        if constexpr (2 * g4 < (LH_KPOOL - 1)) issue_t(std::integral_constant<int, 2 * g4>{});
        if constexpr (2 * g4 + 1 < (LH_KPOOL - 1)) issue_t(std::integral_constant<int, 2 * g4 + 1>{});
      });
      AT_PRIO(1);
      at_static_for<0, 16>([&](auto mc) __attribute__((always_inline)) {
        constexpr int m = decltype(mc)::value;
        constexpr int sub = m >> 3, dt = (m >> 1) & 3, kind = m & 1;
        if constexpr (m + (LH_KPOOL - 1) < 16) issue_t(std::integral_constant<int, m + (LH_KPOOL - 1)>{});
        constexpr int after = 2 * ((16 - 1 - m) < (LH_KPOOL - 1) ? (16 - 1 - m) : (LH_KPOOL - 1));
        at_wait_lgkm<after>(fr[m % LH_KPOOL]);
        if constexpr (kind == 0) dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[m % LH_KPOOL], pf[sub], dv[dt], 0, 0, 0);
        else dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[m % LH_KPOOL], dsf[sub], dk[dt], 0, 0, 0);
      });
      AT_PRIO(0);
    }
    lh_barrier();                    // every wave is done with the ring
    const int ucur = u;
    set_unit(has_next ? u + G : u);
    if (has_next) {
#pragma unroll
      for (int h = 0; h < 4; h++) issue_H(uq, h);
    }
    // dK / dV rows of this wave; the next unit's fragment loads go out between the two (their 64 registers become free with dK).  They
    // are issued unconditionally (a workgroup's last unit re-reads its own rows): a definition under `if (has_next)` keeps the old
    // fragments alive through phase K in the register allocator's eyes - 64 registers spilled and reloaded per unit
    lh_store_matrix(dk, stg, part + 512, (unsigned char*)(uo + d) + (long long)(32 * wave) * pq, pq, lane);       // [8]
    issue_F(uq, ug, ul, ud);
    lh_store_matrix(dv, stg, part + 1024, (unsigned char*)(uo + 2 * d) + (long long)(32 * wave) * pq, pq, lane);  // [8]
    lh_wait_lgkm_plain<0>();         // this wave's partial rows are in LDS: the next barrier publishes them (reduce_partials)
    uprev = ucur;
    if (!has_next) break;
    u += G;
    first = false;
  }
  lh_barrier();
  reduce_partials(uprev);
  lh_wait_vm<0>();
}

void attn_bwd_lh_launch(const void* qkv, const void* dout, const float* lse, const float* dvec, void* dqkv, float* work, int64_t N,
                        int64_t num_heads, float c, float scale, hipStream_t st) {
  PERO_LDS_ATTR(attn_bwd_lh_k, LH_LDS_BYTES);
  const long long units = N * num_heads;
  const int cus = pero_num_cus();
  hipLaunchKernelGGL(attn_bwd_lh_k, dim3((unsigned)(units < cus ? units : cus)), dim3(512), LH_LDS_BYTES, st, (const bf16raw*)qkv, (const bf16raw*)dout, lse,
                     dvec, (bf16raw*)dqkv, work, (int)units, (int)num_heads, c, scale);
}
