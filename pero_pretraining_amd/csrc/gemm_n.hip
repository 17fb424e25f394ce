// ROW-COMPLETE tile for the N = 512 products (DESIGN.md "what comes next"; opt-in: pero_set_option("gemm_nw", 1)): one workgroup owns 128 rows x
// ALL 512 columns, so that an epilogue can see whole rows (the residual LayerNorm of the out-projection / linear2 products, the LayerNorm
// backward behind linear1's / in_proj's input gradients).  The eight-phase compute code of gemm_bf16_e256 with another operand assignment:
//  * the two wave GROUPS take the two N-tiles of the same 128 rows: wave (g, wc) = all 128 rows (the two 64-row parts of ONE A half tile, which
//    both groups read: part 0 in phase 1, part 1 in phase 3) x the 32 wc columns of each half of N-tile g.  The same 128 x 64 outputs, the same
//    fragment reads and MFMAs per wave and K-tile as in the 256 x 256 tile.
//  * a K-tile is FIVE half tiles (A, B00, B10, B01, B11; Bgh = half h of N-tile g): A - the HBM stream - has its own ring of three slots, the four
//    B half tiles - the 512-row weight matrix, which every workgroup streams from L2 - roll through six: nine slots = 144 KiB + 16 KiB of epilogue
//    staging = all of the CU's LDS; the bias comes by side loads.  A slot is restaged two phases after its last read (B00 / B10: one phase,
//    their reads are retired by the lgkmcnt(8) in front of phase 1's first barrier):
//        phase 1 of K-tile t: A(t+2) -> A(t-1)'s slot          phase 2: B01(t+1), B11(t+1) -> the slots of B00(t), B10(t)
//        phase 4:             B00(t+2), B10(t+2) -> the slots of B01(t), B11(t)
//    (slots: A(t) = t % 3; with gb = 4 t % 6: B00 gb, B10 gb + 1, B01 gb + 2, B11 gb + 3, all mod 6 - every index has period three K-tiles).
//  * counted waits, two per K-tile: W2 in phase 1 (B01 / B11 of THIS K-tile, read from phase 2 on: newer are B00 / B10 of t + 1 and A(t+2) = 6
//    instructions) and W1 in phase 4 (A, B00, B10 of t + 1: newer are A(t+2), B01 / B11(t+1), B00 / B10(t+2) = 10); in a tile's first K-tile the
//    previous epilogue's side loads and stores, in its last the side loads of its own epilogue are counted out (constants at the waits).
// Epilogue: gemm_bf16_e256's plain / residual epilogue with `128 wr` gone from the row offsets and `256 wr` added to the columns.
#include "gemm_e_common.hpp"
#include "options.hpp"
#include <type_traits>

#define N_BM 128
#define N_ASLOTS 3
#define N_BSLOTS 6
#define N_RING ((N_ASLOTS + N_BSLOTS) * E_HALF)     // 147 456
#define N_XSTG N_RING                                // 8 x 2 KiB: each wave's staging image of the epilogue's lane transpose
#define N_LDS_BYTES (N_XSTG + 8 * 2048)              // 163 840 = the CU's 160 KiB

template <int EPI, bool BIAS>
__global__ __launch_bounds__(512, 2) void gemm_bf16_n512(GemmP p, LnP q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  static_assert(EPI == EP_PLAIN || EPI == EP_RESID || EPI == EP_RESID_LN || EPI == EP_RESID_LN_T || EPI == EP_RESID_LNB,
                "the row-complete tile has the plain, the residual, the residual + LayerNorm and the residual + LayerNorm-backward epilogue");
  static_assert(EPI != EP_RESID_LNB || !BIAS, "an input-gradient product has no bias");
  constexpr bool LN = EPI == EP_RESID_LN || EPI == EP_RESID_LN_T;
  constexpr bool LNB = EPI == EP_RESID_LNB;
  constexpr bool STORE_Y = EPI != EP_RESID_LN_T;
  constexpr bool RES = EPI == EP_RESID || LN || LNB;
  constexpr int LB = BIAS ? 4 : 0;                        // bias side loads (16 B per lane each)
  constexpr int L0 = LB + (RES ? 8 : 0);                  // side loads issued in phase 4 of the last K-tile: bias + residual rows 0-63
  constexpr int L1 = RES ? 8 : 0;                         // residual rows 64-127, issued halfway through rows 0-63
  constexpr int SH = STORE_Y ? 8 : 0;                     // stores per half of the epilogue
  constexpr int LNX = LN ? 8 + 2 + 16 : 0;                // LayerNorm: gamma / beta loads, mean / rstd stores, the 16 stores of t
  // vector-memory operations of an epilogue behind its phase-4 side loads.  LayerNorm backward: residual rows 64-127 (8), t rows 0-63 (8), gamma, beta,
  // rstd, t rows 64-127 (4 + 4 + 8 + 8), the rows of t again for pass 2 (16), the 16 stores of dx
  constexpr int EPO = LNB ? (8 + 8 + 8 + 8 + 16 + 16) : (L1 + 2 * SH + LNX);
  constexpr int cap63 = 63;                               // s_waitcnt vmcnt takes six bits: a larger count only asks for more than needed
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;                // wr: N-tile (columns 256 wr ...), wc: its 64-column strip
  const int nt = (int)(p.M / N_BM);
  const int G = gridDim.x;                                // multiple of 8
  const int q8 = nt >> 3, r8 = nt & 7;
  const int nk = (int)(p.K / E_BK);                       // >= 3 (launcher)
  const unsigned offA = elane_off<false, true>(p.lda, tid), offB = elane_off<false, false>(p.ldb, tid);
  auto tile_of = [&](int T) -> long long {
    const int xcd = T & 7, loc = T >> 3;
    const int id = E_XCD_TILE(xcd, loc, q8, r8);
    return (long long)id * N_BM;
  };
  int T = blockIdx.x;
  if (T >= nt) return;
  long long tm0 = tile_of(T);
  bool has_next = T + G < nt;
  long long nm0 = tile_of(has_next ? T + G : T);

  const unsigned rc0 = E_FRAG_OFF(lane);
  const int li = lane & 15, lq = lane >> 4;
  auto rdA = [&](const unsigned char* base, int ha, int i, int s) -> bf8v {   // rows 64 ha + 16 i of the A half tile
    return *(const bf8v*)(base + (64 * ha + 16 * i) * 128 + (rc0 ^ (s << 6)));
  };
  auto rdB = [&](const unsigned char* base, int j, int s) -> bf8v {           // rows 32 wc + 16 j of a B half tile
    return *(const bf8v*)(base + (32 * wc + 16 * j) * 128 + (rc0 ^ (s << 6)));
  };
  f4v acc[2][2][4][2];  // [A part][B half][i][j]
  bf8v fa[4][2], fb0[2][2], fb1[2][2];
#define N_RD_A(HA_)                                                           \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; i_++) {                          \
    fa[i_][0] = rdA(kA, (HA_), i_, 0);                                        \
    fa[i_][1] = rdA(kA, (HA_), i_, 1);                                        \
  }
#define N_RD_B(F_, BASE_)                                                     \
  _Pragma("unroll") for (int j_ = 0; j_ < 2; j_++) {                          \
    F_[j_][0] = rdB(BASE_, j_, 0);                                            \
    F_[j_][1] = rdB(BASE_, j_, 1);                                            \
  }

  // the two LDS-DMA streams (u >= nk: the K-tile u - nk of the workgroup's next tile; its last tile prefetches its own again)
  const unsigned char* cA = (const unsigned char*)p.A + tm0 * p.lda * 2;
  const unsigned char* nA = (const unsigned char*)p.A + nm0 * p.lda * 2;
  const unsigned char* const Bp = (const unsigned char*)p.B;
  const long long pieceA = 64 * p.lda * 2, pieceB = 128 * p.ldb * 2;
  unsigned char* const aring = smem;
  unsigned char* const bring = smem + N_ASLOTS * E_HALF;
  // LDS-DMA with a UNIFORM 64-bit base and a 32-bit lane offset (the builtin form keeps a 64-bit address pair per stream in VGPRs and adds
  // into it with the vector ALU; the compiler does not count these either)
  auto dma2 = [&](const unsigned char* sbase, long long piece, unsigned voff, unsigned char* dst) {
    const unsigned d0 = (unsigned)(unsigned long long)LDS_PTR(unsigned char, dst);
    const unsigned char* s1 = sbase + piece;
    // (s_nop 3: with the s_mov five wait states between a v_readlane_b32 that restores a spilled base and the load that reads it - the
    //  compiler pads that hazard for its own instructions only, tools/check_async_loads.py finds the unpadded ones)
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %1, %0" :: "s"(sbase), "v"(voff), "s"(d0) : "memory", "m0");
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %1, %0" :: "s"(s1), "v"(voff), "s"(d0 + 8192u) : "memory", "m0");
  };
  auto issueA = [&](int u, int slot) {
    const bool nx = u >= nk;
    const long long uu = nx ? u - nk : u;
    dma2((nx ? nA : cA) + uu * (E_BK * 2), pieceA, offA, aring + slot * E_HALF + wave * 1024);
  };
  auto issueB = [&](int u, int g, int h, int slot) {
    const long long uu = u >= nk ? u - nk : u;
    dma2(Bp + uu * (E_BK * 2) + (long long)(256 * g + 32 * h) * p.ldb * 2, pieceB, offB, bring + slot * E_HALF + wave * 1024);
  };
  auto mod6 = [](int x) -> int { return x >= 6 ? x - 6 : x; };
  auto mod3 = [](int x) -> int { return x >= 3 ? x - 3 : x; };

  // ---- prologue: K-tile 0 and A, B00, B10 of K-tile 1 (stream order as in the steady state)
  issueA(0, 0); issueB(0, 0, 0, 0); issueB(0, 1, 0, 1); issueB(0, 0, 1, 2); issueB(0, 1, 1, 3);
  issueA(1, 1); issueB(1, 0, 0, 4); issueB(1, 1, 0, 5);
  E_VMCNT(6);
  E_BAR();
  if (wr == 1) { E_BAR(); }  // the stagger: waves 4-7 run one barrier behind

  int ga = 0, gb = 0;        // ring positions of the current K-tile
  bool first = true;

  unsigned char* const xstg = smem + N_XSTG + wave * 2048;
  const ei4v brs = ersrc(BIAS ? (const void*)(p.bias + 256 * wr) : (const void*)p.B, 256 * 4);
  eu4v side0[8], side1[8];   // residual rows 0-63 / 64-127 (EP_RESID)
  eu4v tside0[8], tside1[8]; // EP_RESID_LNB: the rows of t (the LayerNorm's output), same layout
  eu4v biasr[4];             // the lane's 16 bias values as the accumulators hold them: [hb * 2 + j]
  float run_g = 0.f, run_b = 0.f, run_x = 0.f;   // EP_RESID_LNB: the wave's column sums (dgamma, dbeta, sum of dx), one column per lane, over the workgroup's tiles
  (void)tside0; (void)tside1; (void)run_g; (void)run_b; (void)run_x;

  for (;;) {
    E_ACC_ZERO();
    const int spitch = (int)(p.ldr * 2);
    const ei4v srs = ersrc(RES ? (const void*)((const bf16raw*)p.resid + tm0 * p.ldr) : (const void*)p.B, (unsigned)(128 * (RES ? spitch : 2)));
    const int tpitch_l = (int)(q.ldt * 2);
    const ei4v trs_l = ersrc(LNB ? (const void*)((const bf16raw*)q.t + tm0 * q.ldt) : (const void*)p.B, (unsigned)(128 * (LNB ? tpitch_l : 2)));
    (void)tpitch_l;

    auto ktile = [&](auto last_c, auto t0_c, const int t) __attribute__((always_inline)) {
      constexpr bool last = decltype(last_c)::value, t0 = decltype(t0_c)::value;
      unsigned char* const kA = aring + ga * E_HALF;
      unsigned char* const kB0 = bring + (gb + wr) * E_HALF;             // B(wr, 0): gb + wr <= 5
      unsigned char* const kB1 = bring + mod6(gb + 2 + wr) * E_HALF;     // B(wr, 1)
      // P1: A part 0 x B half 0
      N_RD_B(fb0, kB0);
      __builtin_amdgcn_sched_barrier(0);
      N_RD_A(0);
      issueA(t + 2, mod3(ga + 2));
      asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");   // the B half 0 reads (issued first) are done: their slots are restaged in P2
      // W2: B01 / B11 of this K-tile have landed (this wave's pieces).  Newer: B00 / B10 of t + 1, A(t+2); in a tile's first K-tile also the
      // previous tile's side loads and stores
      if (t0 && !first) E_VMCNT((6 + L0 + EPO) < cap63 ? (6 + L0 + EPO) : cap63);
      else E_VMCNT(6);
      E_BAR();
      E_LGKM0();
      E_MFMA(0, 0, fb0);
      E_BAR();
      // P2: A part 0 x B half 1
      N_RD_B(fb1, kB1);
      issueB(t + 1, 0, 1, gb);
      issueB(t + 1, 1, 1, gb + 1);
      E_BAR();
      E_LGKM0();
      E_MFMA(0, 1, fb1);
      E_BAR();
      // P3: A part 1 x B half 1
      N_RD_A(1);
      E_BAR();
      E_LGKM0();
      E_MFMA(1, 1, fb1);
      E_BAR();
      // P4: A part 1 x B half 0
      int lane_p = lane;   // (opaque copy: the side-load offsets are computed here, not carried through the main loop)
      if (last) asm volatile("" : "+v"(lane_p));
      const unsigned bvo = (unsigned)((64 * wc + 4 * (lane_p >> 4)) * 4);        // bias of the lane's accumulator columns: + (32 hb + 16 j) * 4
      const unsigned gvo = (unsigned)(((lane_p >> 2) * p.ldr + 256 * wr + 64 * wc + 8 * (lane_p & 3)) * 2);
      (void)bvo; (void)gvo;
      if (last && BIAS) {   // the epilogue's bias values and residual rows 0-63
        E_BLOAD16(biasr[0], bvo, brs, 0, 0);      // [hb * 2 + j]: columns + 32 hb + 16 j
        E_BLOAD16(biasr[1], bvo, brs, 0, 64);
        E_BLOAD16(biasr[2], bvo, brs, 0, 128);
        E_BLOAD16(biasr[3], bvo, brs, 0, 192);
      }
      if (last && RES) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int so = 16 * i * spitch;
          E_BLOAD16(side0[2 * i], gvo, srs, so, 0);
          E_BLOAD16(side0[2 * i + 1], gvo, srs, so, 64);
        }
      }
      issueB(t + 2, 0, 0, mod6(gb + 2));
      issueB(t + 2, 1, 0, mod6(gb + 3));
      // W1: A, B00, B10 of K-tile t + 1 have landed.  Newer: A(t+2), B01 / B11(t+1), B00 / B10(t+2) = 10; in a tile's first K-tile also the
      // previous epilogue's second-half side loads and its stores, in its last the side loads just issued
      if (t0 && !first) E_VMCNT((10 + EPO) < cap63 ? (10 + EPO) : cap63);
      else if (last) E_VMCNT(10 + L0);
      else E_VMCNT(10);
      E_BAR();
      E_MFMA(1, 0, fb0);
      E_BAR();
      ga = mod3(ga + 1);
      gb = mod6(gb + 4);
    };
    ktile(std::false_type{}, std::true_type{}, 0);
    for (int t = 1; t < nk - 1; t++) ktile(std::false_type{}, std::false_type{}, t);
    ktile(std::true_type{}, std::false_type{}, nk - 1);

    // ---- epilogue, straight from the accumulators
    first = false;
    if (wr == 0) { E_BAR(); }   // undo the stagger: both groups run their epilogues side by side
    if constexpr (LNB) {
      // ---- Linear input gradient + residual gradient = dt (rows complete in this workgroup) -> LayerNorm backward of the upstream norm, from its
      // output t and rstd (layernorm_bwd_pf_k<true>'s arithmetic on the ROUNDED dt, as the unfused pair has it): xhat = (t - beta) / gamma,
      // g = dt gamma, c1 = mean(g), c2 = mean(g xhat), dx = rstd (g - c1 - xhat c2); dgamma += dt xhat, dbeta += dt, dxsum += dx per column.
      //   pass 1a  accumulators + residual rows -> dt through the lane transpose, rounded and PACKED (the accumulators die here)
      //   pass 1b  the two row sums of the lane's 16 columns, all eight rows;  partials of the eight waves -> the A slot this tile's last K-tile has
      //            left free (the next tile's third K-tile refills it), ONE barrier
      //   pass 2   four chunks (32-column block hb, row half ha) of four rows: per row the totals from the exchange area, dx stored; per block the
      //            column sums, reduced over the wave's 16 row indices at once.
      // Vector-memory order (per lane): [phase 4 of the last K-tile: residual rows 0-63 x8] | t rows 0-63 x8 | residual rows 64-127 x8 (halfway through pass 1a of rows
      // 0-63) | gamma x4, beta x4 (in the last quarter of pass 1a) | t rows 64-127 x8 | rstd of chunks 0, 1, 2 (4 each) | 4 stores | rstd of chunk 3 | 4 + 4 + 4 stores.
      int lane_e = lane;
      asm volatile("" : "+v"(lane_e));
      const int li_e = lane_e & 15, lq_e = lane_e >> 4;
      const int er = lane_e >> 2, ep = lane_e & 3;
      const unsigned cvo = (unsigned)((er * p.ldc + 256 * wr + 64 * wc + 8 * ep) * 2);
      const unsigned gvo = (unsigned)((er * p.ldr + 256 * wr + 64 * wc + 8 * ep) * 2);
      const unsigned tvo = (unsigned)((er * q.ldt + 256 * wr + 64 * wc + 8 * ep) * 2);
      const int xsw = (li_e ^ ((li_e >> 1) & 1)) & 7, xsr = (er ^ ((er >> 1) & 1)) & 7;
      const unsigned xw32 = (unsigned)(li_e * 128), xr32 = (unsigned)(er * 128);
      const ei4v crs = ersrc((bf16raw*)p.C + tm0 * p.ldc, (unsigned)(128 * p.ldc * 2));
      const int cpitch = (int)(p.ldc * 2);
      float* const X = (float*)(aring + mod3(ga + 2) * E_HALF);   // exchange area: [8 waves][2 sums][128 rows] floats, 260 per wave (4 of padding: the 32 addresses of a half wave's ds_read_b32 fall on 32 banks)
      auto quad = [&](float v) -> float {
        v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, false));
        v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, false));
        return v;
      };
      auto lo2 = [](unsigned w) -> ef2v { return (ef2v){__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)}; };
      eu4v dtp[2][4][2];
      // gamma / beta of the lane's 16 columns ([2 hb + half]), rstd of its eight rows
      const ei4v grs = ersrc(q.gamma + 256 * wr + 64 * wc, 64 * 4), ers = ersrc(q.beta + 256 * wr + 64 * wc, 64 * 4);
      const ei4v rrs = ersrc(q.rstd + tm0, 128 * 4);
      const unsigned gvoff = (unsigned)(8 * ep * 4), rvo = (unsigned)(er * 4);
      eu4v cg[4], cb[4];
      auto pass1a = [&](auto ha_c) __attribute__((always_inline)) {
        constexpr int ha = decltype(ha_c)::value;
        auto& side1_ = side1;   // (hipcc does not capture a variable that a generic lambda names only as an asm operand)
        auto& cg_ = cg; auto& cb_ = cb;
        const unsigned gvo_ = gvo, gvoff_ = gvoff;
        const ei4v srs_ = srs, grs_ = grs, ers_ = ers;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          if (ha == 0 && i == 2) {
            // residual rows 64-127 go out HALFWAY through rows 0-63: half of that half's accumulators and residual registers are free by now
            // (requested at the epilogue's start they sat beside all 128 accumulators: 16 spilled registers)
#pragma unroll
            for (int i2 = 0; i2 < 4; i2++) {
              const int so = (64 + 16 * i2) * spitch;
              E_BLOAD16(side1_[2 * i2], gvo_, srs_, so, 0);
              E_BLOAD16(side1_[2 * i2 + 1], gvo_, srs_, so, 64);
            }
          }
          if (ha == 1 && i == 3) {
            // the constants go out when three quarters of the accumulators are packed (40 registers; pass 1b needs them first thing)
            E_BLOAD16(cg_[0], gvoff_, grs_, 0, 0); E_BLOAD16(cg_[1], gvoff_, grs_, 0, 16); E_BLOAD16(cg_[2], gvoff_, grs_, 0, 128); E_BLOAD16(cg_[3], gvoff_, grs_, 0, 144);
            E_BLOAD16(cb_[0], gvoff_, ers_, 0, 0); E_BLOAD16(cb_[1], gvoff_, ers_, 0, 16); E_BLOAD16(cb_[2], gvoff_, ers_, 0, 128); E_BLOAD16(cb_[3], gvoff_, ers_, 0, 144);
          }
#pragma unroll
          for (int hb = 0; hb < 2; hb++) {
            const f4v x = acc[ha][hb][i][0], y = acc[ha][hb][i][1];
            *(f4v*)(xstg + xw32 + ((lq_e ^ xsw) << 4)) = x;
            *(f4v*)(xstg + xw32 + (((4 + lq_e) ^ xsw) << 4)) = y;
            const f4v r0 = *(const f4v*)(xstg + xr32 + (((2 * ep) ^ xsr) << 4));
            const f4v r1 = *(const f4v*)(xstg + xr32 + (((2 * ep + 1) ^ xsr) << 4));
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; e++) { v[e] = r0[e]; v[4 + e] = r1[e]; }
            const eu4v r4 = ha ? side1[2 * i + hb] : side0[2 * i + hb];
#pragma unroll
            for (int e = 0; e < 4; e++) { v[2 * e] += __uint_as_float(r4[e] << 16); v[2 * e + 1] += __uint_as_float(r4[e] & 0xffff0000u); }
            dtp[ha][i][hb] = (eu4v){pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
            // (the packed rows are made opaque HERE: left alone the compiler sinks the adds and conversions down to the rows' first use in pass 1b and
            //  parks the f32 rows of all eight units - 64 registers - in scratch meanwhile)
            asm volatile("" : "+v"(dtp[ha][i][hb]));
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      // t rows 0-63 first (they are needed after BOTH halves of pass 1a: issued behind rows 0-63 they had one half to arrive and the wave waited
      // for HBM; with every arithmetic instruction of this epilogue compiled out it still cost 128 us per launch over the plain residual
      // epilogue (an ablation build): its loads' latency, not its 1 900 vector-ALU instructions, is what the epilogue costs)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int so = 16 * i * tpitch_l;
        E_BLOAD16(tside0[2 * i], tvo, trs_l, so, 0);
        E_BLOAD16(tside0[2 * i + 1], tvo, trs_l, so, 64);
      }
      E_WAIT8(12, side0);   // residual rows 0-63 (phase 4 of the last K-tile): newer are B00 / B10 (4) and the 8 loads above
      pass1a(std::integral_constant<int, 0>{});
      E_WAIT8(0, side1);    // residual rows 64-127 (issued halfway through pass 1a of rows 0-63): nothing newer
      pass1a(std::integral_constant<int, 1>{});
#pragma unroll
      for (int i = 0; i < 4; i++) {   // t rows 64-127 (beside rows 64-127 of the accumulators they spill 13 registers: they arrive under pass 1b of rows 0-63)
        const int so = (64 + 16 * i) * tpitch_l;
        E_BLOAD16(tside1[2 * i], tvo, trs_l, so, 0);
        E_BLOAD16(tside1[2 * i + 1], tvo, trs_l, so, 64);
      }
      // t rows 0-63 and the constants (issued in pass 1a's last quarter): newer are the 8 loads just issued
      E_WAIT8(8, tside0);
      E_WAIT4(8, cg);
      E_WAIT4(8, cb);
      // pair e of block hb <-> columns 32 hb + 8 ep + 2 e, + 1
      auto Gp = [&](int hb, int e) -> ef2v { return (ef2v){__uint_as_float(cg[2 * hb + (e >> 1)][2 * (e & 1)]), __uint_as_float(cg[2 * hb + (e >> 1)][2 * (e & 1) + 1])}; };
      auto Bp = [&](int hb, int e) -> ef2v { return (ef2v){__uint_as_float(cb[2 * hb + (e >> 1)][2 * (e & 1)]), __uint_as_float(cb[2 * hb + (e >> 1)][2 * (e & 1) + 1])}; };
      // ---- pass 1b: s1 = sum dt gamma, s2 = sum dt (t - beta) (= dt gamma xhat) over the lane's 16 columns of each of its eight rows
#pragma unroll
      for (int ha = 0; ha < 2; ha++) {
        if (ha == 1) E_WAIT8(0, tside1);   // (nothing newer; the older LDS-DMA of the next tile's first K-tiles has had the whole epilogue so far)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          ef2v a1 = {0.f, 0.f}, a2 = {0.f, 0.f};
#pragma unroll
          for (int hb = 0; hb < 2; hb++) {
            const eu4v tw = ha ? tside1[2 * i + hb] : tside0[2 * i + hb];
#pragma unroll
            for (int e = 0; e < 4; e++) {
              const ef2v d = lo2(dtp[ha][i][hb][e]);
              const ef2v u = lo2(tw[e]) - Bp(hb, e);
              a1 = __builtin_elementwise_fma(d, Gp(hb, e), a1);
              a2 = __builtin_elementwise_fma(d, u, a2);
            }
          }
          const float q1 = quad(a1[0] + a1[1]), q2 = quad(a2[0] + a2[1]);
          if (ep == 0) {
            X[wave * 260 + 64 * ha + 16 * i + er] = q1;
            X[wave * 260 + 128 + 64 * ha + 16 * i + er] = q2;
          }
        }
      }
      // ---- pass 2.  The rows of t again, chunk by chunk (c = 2 hb + ha: rows 64 ha + 16 i + er, the 16-byte piece of block hb), one chunk ahead
      unsigned rsc[3][4];   // rstd of a chunk's four rows, loaded two chunks ahead (held from pass 1a on they were 8 registers too many)
      auto tload = [&](auto c_c) __attribute__((always_inline)) {
        constexpr int c = decltype(c_c)::value, ha = c & 1;
        auto& rsc_ = rsc;   // (hipcc does not capture a variable that a generic lambda names only as an asm operand)
        const unsigned rvo_ = rvo;
        const ei4v rrs_ = rrs;
        E_BLOAD4(rsc_[c % 3][0], rvo_, rrs_, 256 * ha, 0); E_BLOAD4(rsc_[c % 3][1], rvo_, rrs_, 256 * ha, 64);
        E_BLOAD4(rsc_[c % 3][2], rvo_, rrs_, 256 * ha, 128); E_BLOAD4(rsc_[c % 3][3], rvo_, rrs_, 256 * ha, 192);
      };
      tload(std::integral_constant<int, 0>{});
      tload(std::integral_constant<int, 1>{});
      tload(std::integral_constant<int, 2>{});
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      E_BAR();
      auto colred8 = [&](const ef2v (&A)[4]) -> float {
        // 8 values per lane (columns 8 ep + j) summed over the wave's 16 row indices (lane bits 2-5): a halving butterfly over lanes 32, 16 and 8
        // apart (each step a lane keeps half of its values and adds the partner's copy of them), then lane ^ 4; lane (er, ep) ends with the
        // total of column 8 ep + (er >> 1)
        float w4[4], w2[2];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(A[j >> 1][j & 1]), __float_as_uint(A[2 + (j >> 1)][j & 1]), false, false);
          w4[j] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);      // er & 8 == 0: values j of both; else values j + 4 of both
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
          auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(w4[j]), __float_as_uint(w4[j + 2]), false, false);
          w2[j] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);      // er & 4 == 0: w4[j] of both; else w4[j + 2] of both
        }
        const float s0 = w2[0] + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(w2[0]), 0x128, 0xf, 0xf, false));   // row_ror:8 = lane ^ 8
        const float s1 = w2[1] + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(w2[1]), 0x128, 0xf, 0xf, false));
        const float w1 = (er & 2) ? s1 : s0;
        int r = __builtin_amdgcn_update_dpp(0, __float_as_int(w1), 0x104, 0xf, 0x5, false);    // lane ^ 4 (see gemm_bf16_e256's column sums)
        r = __builtin_amdgcn_update_dpp(r, __float_as_int(w1), 0x114, 0xf, 0xa, false);
        return w1 + __int_as_float(r);
      };
      float tot_g[2], tot_b[2], tot_x[2];
      ef2v G[4], Bt[4], IG[4], AG[4], AB[4], AX[4];
      auto chunk = [&](auto c_c) __attribute__((always_inline)) {
        constexpr int c = decltype(c_c)::value, hb = c >> 1, ha = c & 1;
        const unsigned cvo_ = cvo;
        const ei4v crs_ = crs;
        if constexpr (ha == 0) {
#pragma unroll
          for (int e = 0; e < 4; e++) {
            G[e] = Gp(hb, e); Bt[e] = Bp(hb, e);
            asm volatile("" : "+v"(G[e]));   // (opaque here: the compiler otherwise takes the reciprocals of BOTH blocks in front of pass 1b and spills them)
            // (v_rcp_f32, one ulp: the correctly rounded quotient is a dozen instructions per column and tile)
            IG[e][0] = G[e][0] != 0.f ? __builtin_amdgcn_rcpf(G[e][0]) : 0.f;
            IG[e][1] = G[e][1] != 0.f ? __builtin_amdgcn_rcpf(G[e][1]) : 0.f;
            AG[e] = (ef2v){0.f, 0.f}; AB[e] = (ef2v){0.f, 0.f}; AX[e] = (ef2v){0.f, 0.f};
          }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int r = 64 * ha + 16 * i + er;
          const float c1 = quad(X[(2 * ep) * 260 + r] + X[(2 * ep + 1) * 260 + r]) * (1.0f / 512.f);
          const float c2 = quad(X[(2 * ep) * 260 + 128 + r] + X[(2 * ep + 1) * 260 + 128 + r]) * (1.0f / 512.f);
          const float rs = __uint_as_float(rsc[c % 3][i]);
          const ef2v c1v = {-c1, -c1}, c2v = {-c2, -c2}, rsv = {rs, rs};
          const int so = (64 * ha + 16 * i) * cpitch;
          // The rows of t stay in their registers from pass 1b (a second load of them was a second trip to HBM - a round of tiles sweeps the
          // XCD's L2 - and the launch runs at the memory system's rate: it was what the epilogue cost).  Both packed rows are made opaque again:
          // otherwise the unpacked f32 pairs of pass 1b are KEPT for this pass - in scratch - instead of two shifts per pair here
          if (ha) asm volatile("" : "+v"(tside1[2 * i + hb])); else asm volatile("" : "+v"(tside0[2 * i + hb]));
          const eu4v tw = ha ? tside1[2 * i + hb] : tside0[2 * i + hb];
          asm volatile("" : "+v"(dtp[ha][i][hb]));
          eu4v od;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const ef2v d = lo2(dtp[ha][i][hb][e]);
            const ef2v xh = (lo2(tw[e]) - Bt[e]) * IG[e];
            ef2v o = __builtin_elementwise_fma(d, G[e], c1v);
            o = __builtin_elementwise_fma(xh, c2v, o) * rsv;
            AX[e] += o;
            AG[e] = __builtin_elementwise_fma(d, xh, AG[e]);
            AB[e] += d;
            od[e] = pack2bf(o[0], o[1]);
          }
          if (hb) E_BSTORE16(od, cvo_, crs_, so, 64); else E_BSTORE16(od, cvo_, crs_, so, 0);
        }
        if constexpr (ha == 1) {
          tot_g[hb] = colred8(AG);
          tot_b[hb] = colred8(AB);
          tot_x[hb] = colred8(AX);
        }
      };
      E_WAIT4(8, rsc[0]);                                  // chunk 0's rstd: newer are chunks 1 and 2 (4 + 4)
      chunk(std::integral_constant<int, 0>{});
      tload(std::integral_constant<int, 3>{});             // (chunk 0's registers)
      E_WAIT4(12, rsc[1]);                                 // chunk 1: newer are chunk 2 (4), chunk 0's stores (4), chunk 3 (4)
      chunk(std::integral_constant<int, 1>{});
      E_WAIT4(12, rsc[2]);                                 // chunk 2: newer are chunk 0's stores, chunk 3, chunk 1's stores
      chunk(std::integral_constant<int, 2>{});
      E_WAIT4(8, rsc[0]);                                  // chunk 3: newer are chunk 1's and chunk 2's stores
      chunk(std::integral_constant<int, 3>{});
      // every wave has read the exchange area before any wave's next tile refills the slot (LDS-DMA in phase 1 of its first K-tile)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      E_BAR();
      // lane (er, ep) keeps column 32 (er & 1) + 8 ep + (er >> 1) of the wave's 64: three registers run on over the workgroup's tiles
      run_g += (er & 1) ? tot_g[1] : tot_g[0];
      run_b += (er & 1) ? tot_b[1] : tot_b[0];
      run_x += (er & 1) ? tot_x[1] : tot_x[0];
    } else
    {
      // epilogue addressing (see gemm_bf16_e256): after the column swap lane (li, lq) holds 8 columns of a 32-column block of row li; the values
      // go through one lane transpose in LDS so that four adjacent lanes store 64 contiguous bytes of a row.  Derived HERE from an opaque copy of
      // the lane index: as loop invariants the compiler parked two dozen of them in scratch across the main loop and reloaded them in the
      // epilogue - every reload a vector-memory operation in the counted queue with a vmcnt(0) behind it
      int lane_e = lane;
      asm volatile("" : "+v"(lane_e));
      const int li_e = lane_e & 15, lq_e = lane_e >> 4;
      const int cq = ((lq_e & 1) << 1) | (lq_e >> 1);
      const int er = lane_e >> 2, ep = lane_e & 3;
      const unsigned cvo = (unsigned)((er * p.ldc + 256 * wr + 64 * wc + 8 * ep) * 2);
      const unsigned gvo = (unsigned)((er * p.ldr + 256 * wr + 64 * wc + 8 * ep) * 2);
      const unsigned xw16 = (unsigned)(li_e * 64 + ((cq ^ ((li_e >> 1) & 3)) << 4));
      const unsigned xr16 = (unsigned)(er * 64 + ((ep ^ ((er >> 1) & 3)) << 4));
      const int xsw = (li_e ^ ((li_e >> 1) & 1)) & 7, xsr = (er ^ ((er >> 1) & 1)) & 7;
      const unsigned xw32 = (unsigned)(li_e * 128), xr32 = (unsigned)(er * 128);
      (void)xw16; (void)xr16; (void)xsw; (void)xsr; (void)xw32; (void)xr32; (void)gvo; (void)cq;
      const ei4v crs = ersrc((bf16raw*)p.C + tm0 * p.ldc, (unsigned)(128 * p.ldc * 2));
      const int cpitch = (int)(p.ldc * 2);
      unsigned ones2 = 0x3f803f80u;   // the bf16 pair (1, 1), in a register the compiler cannot fold into an inline constant (see the gate epilogue of gemm_bf16_e256)
      asm volatile("" : "+s"(ones2));
      (void)ones2;
      eu4v yk[2][4][2];   // LN: the packed rows of y, kept for the statistics and the normalisation (the accumulators die as they are consumed)
      float rsum[2][4];   // LN: this lane's share of the row sums (rows 64 ha + 16 i + er, its 16 columns)
      eu4v gb[8];         // LN: gamma / beta of the lane's 16 columns: [hb][half] then + 4
      (void)yk; (void)rsum; (void)gb;
#pragma unroll
      for (int ha = 0; ha < 2; ha++) {
        if (ha == 0) {
          // bias and rows 0-63: issued in phase 4 of the last K-tile; newer: B00 / B10 (4 instructions)
          if (BIAS) E_WAIT4(4, biasr);
          if (L1) E_WAIT8(4, side0);
        }
        if (L1 && ha == 1) E_WAIT8(SH / 2, side1);   // newer: the four stores of rows 32-63
        f4v bx[2][2];
#pragma unroll
        for (int hb = 0; hb < 2; hb++)
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const eu4v b4 = biasr[hb * 2 + j];
            bx[hb][j] = BIAS ? (f4v){__uint_as_float(b4[0]), __uint_as_float(b4[1]), __uint_as_float(b4[2]), __uint_as_float(b4[3])} : (f4v){0.f, 0.f, 0.f, 0.f};
          }
        constexpr int NI = RES ? 1 : 2;
#pragma unroll
        for (int ib = 0; ib < 4; ib += NI) {
          if (L1 && ha == 0 && ib == 2) {
            // rows 64-127 of the residual go out HALFWAY through rows 0-63: by then half of that half's accumulators and side registers are free
            // (requested at the epilogue's start they sat beside everything else: 30-40 spilled registers and a vmcnt(0) at every reload)
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int so = (64 + 16 * i) * spitch;
              E_BLOAD16(side1[2 * i], gvo, srs, so, 0);
              E_BLOAD16(side1[2 * i + 1], gvo, srs, so, 64);
            }
          }
          if (LN && ha == 1 && ib == 2) {   // (three quarters of the accumulators and side registers are free by now; only the four stores of rows 96-127 follow)
            // gamma / beta of the lane's columns 256 wr + 64 wc + 32 hb + 8 ep .. + 7 (two 16-byte halves each): needed in pass 2
            const ei4v grs = ersrc(q.gamma + 256 * wr + 64 * wc, 64 * 4), ers = ersrc(q.beta + 256 * wr + 64 * wc, 64 * 4);
            const unsigned gvoff = (unsigned)(8 * ep * 4);
            E_BLOAD16(gb[0], gvoff, grs, 0, 0); E_BLOAD16(gb[1], gvoff, grs, 0, 16); E_BLOAD16(gb[2], gvoff, grs, 0, 128); E_BLOAD16(gb[3], gvoff, grs, 0, 144);
            E_BLOAD16(gb[4], gvoff, ers, 0, 0); E_BLOAD16(gb[5], gvoff, ers, 0, 16); E_BLOAD16(gb[6], gvoff, ers, 0, 128); E_BLOAD16(gb[7], gvoff, ers, 0, 144);
          }
          eu4v o[NI][2];
#pragma unroll
          for (int ii = 0; ii < NI; ii++)
#pragma unroll
            for (int hb = 0; hb < 2; hb++) {
              const int i = ib + ii;
              const f4v x = acc[ha][hb][i][0] + bx[hb][0];
              const f4v y = acc[ha][hb][i][1] + bx[hb][1];
              if (RES) {
                float v[8];
                *(f4v*)(xstg + xw32 + ((lq_e ^ xsw) << 4)) = x;
                *(f4v*)(xstg + xw32 + (((4 + lq_e) ^ xsw) << 4)) = y;
                const f4v r0 = *(const f4v*)(xstg + xr32 + (((2 * ep) ^ xsr) << 4));
                const f4v r1 = *(const f4v*)(xstg + xr32 + (((2 * ep + 1) ^ xsr) << 4));
#pragma unroll
                for (int e = 0; e < 4; e++) { v[e] = r0[e]; v[4 + e] = r1[e]; }
                const eu4v r4 = ha ? side1[2 * i + hb] : side0[2 * i + hb];
#pragma unroll
                for (int e = 0; e < 4; e++) { v[2 * e] += __uint_as_float(r4[e] << 16); v[2 * e + 1] += __uint_as_float(r4[e] & 0xffff0000u); }
                o[ii][hb][0] = pack2bf(v[0], v[1]); o[ii][hb][1] = pack2bf(v[2], v[3]); o[ii][hb][2] = pack2bf(v[4], v[5]); o[ii][hb][3] = pack2bf(v[6], v[7]);
                if (LN) {
                  yk[ha][i][hb] = o[ii][hb];
                  float sacc = hb ? rsum[ha][i] : 0.f;   // the LayerNorm kernel sums the ROUNDED values (layernorm_fwd4_k); (x, y) . (1, 1): one instruction per pair
#pragma unroll
                  for (int e = 0; e < 4; e++) sacc = edot2(o[ii][hb][e], ones2, sacc);
                  rsum[ha][i] = sacc;
                }
              } else {
                const unsigned px0 = pack2bf(x[0], x[1]), px1 = pack2bf(x[2], x[3]);
                const unsigned py0 = pack2bf(y[0], y[1]), py1 = pack2bf(y[2], y[3]);
                auto s0 = __builtin_amdgcn_permlane16_swap(px0, py0, false, false);
                auto s1 = __builtin_amdgcn_permlane16_swap(px1, py1, false, false);
                *(eu4v*)(xstg + hb * 1024 + xw16) = (eu4v){s0[0], s1[0], s0[1], s1[1]};
                o[ii][hb] = *(const eu4v*)(xstg + hb * 1024 + xr16);
              }
            }
#pragma unroll
          for (int ii = 0; ii < NI; ii++) {
            const int i = ib + ii;
            const int so = (64 * ha + 16 * i) * cpitch;
#pragma unroll
            for (int hb = 0; hb < 2; hb++) {
              eu4v& ou = o[ii][hb];
              if (!STORE_Y) continue;
              if (hb) E_BSTORE16(ou, cvo, crs, so, 64); else E_BSTORE16(ou, cvo, crs, so, 0);
            }
          }
        }
      }
      if (LN) {
        // ---- the LayerNorm of the stored rows (layernorm_fwd4_k's arithmetic: mean, then the centred squares, both over the rounded values).
        // A row's 512 columns are spread over the eight waves: every wave leaves its 128 row partials in its own staging block (idle now),
        // one workgroup barrier, and lane (er, ep) adds the partials of waves 2 ep, 2 ep + 1 for its eight rows; a quad sum gives the total.
        float* const mine = (float*)xstg;                                    // [2][128] floats of this wave
        const float* const all = (const float*)(smem + N_XSTG);              // wave w: + 512 w floats
        auto quad = [&](float v) -> float {
          v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, false));
          v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, false));
          return v;
        };
        auto exchange = [&](float (&part)[2][4], int which) {   // in: this lane's shares; out: the totals of its eight rows
#pragma unroll
          for (int ha = 0; ha < 2; ha++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const float w = quad(part[ha][i]);
              if (ep == 0) mine[which * 128 + 64 * ha + 16 * i + er + 4 * wave] = w;   // (+ 4 floats per wave: see the read below)
            }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          E_BAR();
#pragma unroll
          for (int ha = 0; ha < 2; ha++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
              // wave w's partials sit 4 w floats into its 2 KiB block: the four waves 2 ep a half wave reads from then fall on four different
              // groups of 8 banks (at the bare 512-float pitch all of them hit the same 8: 4-way conflicts, 6.3 M conflict cycles per launch)
              const int r = which * 128 + 64 * ha + 16 * i + er;
              part[ha][i] = quad(all[(2 * ep) * 512 + r + 8 * ep] + all[(2 * ep + 1) * 512 + r + 8 * ep + 4]);
            }
        };
        exchange(rsum, 0);
        float mu[2][4], qs[2][4];
        float xc[2][4][2][8];   // the centred values: unpacked and centred ONCE, used by the variance and by the normalisation (the accumulators are dead: 128 registers)
#pragma unroll
        for (int ha = 0; ha < 2; ha++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            mu[ha][i] = rsum[ha][i] / 512.f;
            float a = 0.f;
#pragma unroll
            for (int hb = 0; hb < 2; hb++)
#pragma unroll
              for (int e = 0; e < 4; e++) {
                const float t0 = __uint_as_float(yk[ha][i][hb][e] << 16) - mu[ha][i], t1 = __uint_as_float(yk[ha][i][hb][e] & 0xffff0000u) - mu[ha][i];
                xc[ha][i][hb][2 * e] = t0; xc[ha][i][hb][2 * e + 1] = t1;
                a += t0 * t0; a += t1 * t1;
              }
            qs[ha][i] = a;
          }
        exchange(qs, 1);
        // mean / rstd of the tile's rows: wave w writes the 16 rows of its (ha, i) = (w >> 2, w & 3)
        E_WAIT8(SH / 2, gb);   // gamma / beta: newer are the four stores of rows 96-127
        const ei4v trs = ersrc((bf16raw*)q.t + tm0 * q.ldt, (unsigned)(128 * q.ldt * 2));
        const int tpitch = (int)(q.ldt * 2);
        const unsigned tvo = (unsigned)((er * q.ldt + 256 * wr + 64 * wc + 8 * ep) * 2);
#pragma unroll
        for (int ha = 0; ha < 2; ha++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const float rs = 1.0f / sqrtf(qs[ha][i] / 512.f + q.eps);
            if (wave == ha * 4 + i && ep == 0) {
              q.mean[tm0 + 64 * ha + 16 * i + er] = mu[ha][i];
              q.rstd[tm0 + 64 * ha + 16 * i + er] = rs;
            }
#pragma unroll
            for (int hb = 0; hb < 2; hb++) {
              eu4v ot;
#pragma unroll
              for (int e = 0; e < 4; e++) {
                const float g0 = __uint_as_float(gb[2 * hb + (e >> 1)][2 * (e & 1)]), g1 = __uint_as_float(gb[2 * hb + (e >> 1)][2 * (e & 1) + 1]);
                const float b0 = __uint_as_float(gb[4 + 2 * hb + (e >> 1)][2 * (e & 1)]), b1 = __uint_as_float(gb[4 + 2 * hb + (e >> 1)][2 * (e & 1) + 1]);
                ot[e] = pack2bf(xc[ha][i][hb][2 * e] * rs * g0 + b0, xc[ha][i][hb][2 * e + 1] * rs * g1 + b1);
              }
              const int so = (64 * ha + 16 * i) * tpitch;
              if (hb) E_BSTORE16(ot, tvo, trs, so, 64); else E_BSTORE16(ot, tvo, trs, so, 0);
            }
          }
      }
    }
    if (!has_next) break;
    T += G;
    tm0 = nm0; cA = nA;
    has_next = T + G < nt;
    nm0 = tile_of(has_next ? T + G : T);
    nA = (const unsigned char*)p.A + nm0 * p.lda * 2;
    if (wr == 1) { E_BAR(); }  // the stagger again
  }
  if constexpr (LNB) {
    // this workgroup's partial column sums -> work[which][workgroup][512] (plain stores; layernorm_bwd_reduce_k adds the workgroups' rows)
    const int er = lane >> 2, ep = lane & 3;
    const int col = 256 * wr + 64 * wc + 32 * (er & 1) + 8 * ep + (er >> 1);
    float* w = q.work + (size_t)blockIdx.x * 512 + col;
    w[0] = run_g;
    w[(size_t)gridDim.x * 512] = run_b;
    w[(size_t)2 * gridDim.x * 512] = run_x;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last tile's surplus prefetches land before the LDS is released
#undef N_RD_A
#undef N_RD_B
}
// "gemm_nw" = 1: N = 512 stored products with the plain / residual epilogue on the row-complete tile
bool pero_gemm_n512_takes(const GemmP& p0, long long batch, bool out_f32) {
  if (!g_opt.gemm_nw || batch != 1 || out_f32 || p0.N != 512 || p0.M % N_BM || p0.K % E_BK || p0.K < 3 * E_BK) return false;
  if (p0.alpha != 1.0f || p0.gate || (p0.flags & ~(PERO_GEMM_TILE256))) return false;   // bias and residual only, K-contiguous operands
  return pero_ld_fits32({p0.lda, p0.ldb, p0.ldc, p0.resid ? p0.ldr : 0});
}
void pero_gemm_n512_launch(const GemmP& p, hipStream_t st) {
  const unsigned G = pero_persistent_grid(p.M / N_BM);
  const LnP q = {nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr};
#define LAUNCH_N(EP_, BI_)                                                                          \
  do {                                                                                              \
    PERO_LDS_ATTR((gemm_bf16_n512<EP_, BI_>), N_LDS_BYTES);                                          \
    hipLaunchKernelGGL((gemm_bf16_n512<EP_, BI_>), dim3(G), dim3(512), N_LDS_BYTES, st, p, q);       \
  } while (0)
  if (p.resid) { if (p.bias) LAUNCH_N(EP_RESID, true); else LAUNCH_N(EP_RESID, false); }
  else { if (p.bias) LAUNCH_N(EP_PLAIN, true); else LAUNCH_N(EP_PLAIN, false); }
}
// y = A W^T + bias + resid (bf16, stored), t = LayerNorm(y) * gamma + beta (bf16), mean / rstd of every row: one launch on the row-complete
// tile.  false: the shape does not take it (N must be 512).
bool pero_launch_gemm_n512_ln(const GemmP& p0, void* t, long long ldt, float* mean, float* rstd, const float* gamma, const float* beta, float eps,
                              hipStream_t st) {
  if (p0.N != 512 || p0.M % N_BM || p0.K % E_BK || p0.K < 3 * E_BK || !p0.resid || !t || !mean || !rstd || !gamma || !beta) return false;
  if (!pero_ld_fits32({p0.lda, p0.ldb, p0.C ? p0.ldc : 0, p0.ldr, ldt})) return false;
  const long long nt = p0.M / N_BM;
  const unsigned G = pero_persistent_grid(nt);
  GemmP p = p0;
  const LnP q = {t, ldt, mean, rstd, gamma, beta, eps, nullptr};
  if (!p0.C) { if (p0.bias) LAUNCH_N(EP_RESID_LN_T, true); else LAUNCH_N(EP_RESID_LN_T, false); }   // y not stored
  else if (p0.bias) LAUNCH_N(EP_RESID_LN, true); else LAUNCH_N(EP_RESID_LN, false);
#undef LAUNCH_N
  return true;
}

// dx = LayerNorm backward (from the norm's output t and rstd) of dt = A W^T + R, column sums -> work [3][grid][512]; *grid_out = the rows of work that
// layernorm_bwd_reduce_k has to add.  false: the shape does not take it.
bool pero_launch_gemm_n512_lnb(const GemmP& p0, const void* t, long long ldt, const float* rstd, const float* gamma, const float* beta, float* work,
                               int* grid_out, hipStream_t st) {
  if (p0.N != 512 || p0.M % N_BM || p0.K % E_BK || p0.K < 3 * E_BK || !p0.resid || p0.bias || !p0.C || !t || !rstd || !gamma || !beta || !work) return false;
  if (!pero_ld_fits32({p0.lda, p0.ldb, p0.ldc, p0.ldr, ldt})) return false;
  const long long nt = p0.M / N_BM;
  const unsigned G = pero_persistent_grid(nt);
  // (workgroups beyond the tile count return at once: their rows of `work` are cleared first - the reduce kernel adds all G rows)
  if (nt < (long long)G) hipMemsetAsync(work, 0, (size_t)3 * G * 512 * sizeof(float), st);
  GemmP p = p0;
  const LnP q = {const_cast<void*>(t), ldt, nullptr, const_cast<float*>(rstd), gamma, beta, 0.f, work};
  PERO_LDS_ATTR((gemm_bf16_n512<EP_RESID_LNB, false>), N_LDS_BYTES);
  hipLaunchKernelGGL((gemm_bf16_n512<EP_RESID_LNB, false>), dim3(G), dim3(512), N_LDS_BYTES, st, p, q);
  *grid_out = (int)G;
  return true;
}
