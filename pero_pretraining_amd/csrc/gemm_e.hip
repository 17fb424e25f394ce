// PERSISTENT 256 x 256 x 64 bf16 tile GEMM on the EIGHT-PHASE PING-PONG schedule (cdna_hip_programming.md section 5, "The 256^2
// 8-phase template"): eight waves as 2 (M) x 4 (N), 128 x 64 outputs per wave, one workgroup per CU.
//
//  * A K-tile (256 x 64 of A, 256 x 64 of B) lives in LDS as FOUR half tiles of 16 KiB (A0, A1, B0, B1 = 128 rows x 64 k);
//    a wave owns 64 rows of each A half and 32 columns of each B half, i.e. its 128 x 64 outputs are 2 x 2 blocks of
//    64 x 32 = (A half) x (B half).  One PHASE = one block x K = 64 = 16 MFMAs; four phases per K-tile:
//        P1: read B0 (4 ds_read_b128), A0 (8)  -> A0 x B0        P3: read A1 (8) -> A1 x B1
//        P2: read B1 (4)                       -> A0 x B1        P4: (nothing)   -> A1 x B0
//    so a half tile is read exactly once per wave and at most 64 fragment registers are live beside the 128 accumulators.
//  * Every phase is  { fragment reads ; LDS-DMA of ONE half tile (2 x global_load_lds_dwordx4) ; s_barrier ; lgkmcnt(0) ;
//    s_setprio 1 ; 16 MFMA ; s_setprio 0 ; s_barrier }.  Waves 4-7 take one extra barrier before the loop: the two waves of
//    a SIMD run half a phase apart, one in its MFMA cluster while the other reads / stages (the ping-pong).
//  * The LDS-DMA stream is ONE sequence over (tile, K-tile) pairs, three half tiles ahead of the reads, never drained:
//    a counted s_waitcnt vmcnt once per K-tile (phase 4), raw s_barrier, lgkmcnt only.  Issue order B0(t+2) [P2], A0(t+2)
//    [P3], B1(t+2) [P4], A1(t+2) [P1 of t+1]: a slot is restaged two phases after its last read (B0: one phase, its reads are
//    retired by the lgkmcnt(8) in front of P1's first barrier); the wait in P4 of K-tile t retires everything up to
//    A1(t+1), read from P1 of t+1 on (one phase after the wait: staggered waves need the extra barrier).
//  * Persistent: one workgroup per CU walks tiles bid, bid + G, ...; the next tile's first K-tiles are part of the same
//    stream, so the pipeline never refills.  vmcnt is ONE in-order counter for LDS-DMA, loads and stores: the last
//    half tile the next tile needs before its second K-tile (A1 of K-tile 1) is issued AHEAD of the epilogue's stores, and
//    the first K-tile's wait counts them out - the stores then have two K-tiles of main loop to drain.
//  * Epilogue straight from the accumulators: operands are swapped in the MFMA so that a lane owns 4 consecutive
//    output columns of one row; v_permlane16_swap between the two 16 x 16 tiles of a 32-column block gives it 8 consecutive
//    columns (16 bytes), and ONE lane transpose (through a wave-private LDS staging image) moves the four 16-byte pieces of a
//    row from lanes 16 apart onto four ADJACENT lanes before the store: the memory pipeline merges adjacent lanes only, and a
//    1 KiB store whose adjacent lanes sit on different rows is 64 separate requests (64 instead of 16 cycles of the CU's store
//    path; tools/probe_store3.hip).
//    Side inputs (residual rows, the second matrix of the row dots, the ReLU bit mask) are fetched in that transposed layout by
//    inline-asm buffer loads the compiler does not count: half of them in phase 4 of the tile's last K-tile, half at the start
//    of the epilogue, each waited for by a counted vmcnt.  The bias comes from a per-wave 1 KiB LDS copy of the tile's bias row,
//    fetched by one more LDS-DMA of the same stream at the tile's start (an ordinary load would have to wait for every LDS-DMA
//    issued before it) and added in f32 before the rounding, exactly as the other tile kernels do (acc * alpha + bias): results
//    are bit-identical across kernels, i.e. across batch sizes.
//  * Both wave groups run their epilogues side by side: waves 0-3 take one extra barrier at the epilogue's start (waves 4-7 finish
//    their last MFMA cluster meanwhile), waves 4-7 one in front of the next tile, which staggers the groups again.  Staggered
//    through the epilogue, each group sat at a barrier through the other's epilogue.
#include "gemm_e_common.hpp"
#include "options.hpp"
#include <type_traits>

#define E_BM 256
#define E_BN 256
#define E_KTILE (4 * E_HALF)       // A0 A1 B0 B1
#define E_RING (2 * E_KTILE)       // 128 KiB: two K-tiles
#define E_BIAS E_RING              // 8 x 1 KiB: each wave's copy of the tile's 256 bias floats
#define E_PAD (E_BIAS + 8192)      // 512 B unused: the layout below is the one every measurement was taken with
#define E_LUT (E_PAD + 512)        // EP_GATE_BITS: 256 x 16 B, mask byte -> the four AND masks of its 8 bf16 columns
#define E_XSTG (E_LUT + 4096)      // 8 x 2 KiB: each wave's staging image of the epilogue's lane transpose
#define E_LDS_BYTES (E_XSTG + 8 * 2048)

template <int EPI> struct ECnt {
  // vector-memory operations of the epilogue, in issue order: side loads of rows 0-63 (phase 4 of the last K-tile), [A1 of the
  // next tile's K-tile 1], side loads of rows 64-127, then the stores / atomics of the two halves
  static constexpr int L0 = (EPI == EP_RESID || EPI == EP_ROWDOT) ? 8 : 0;  // (EP_GATE_BITS: its 8 mask loads go out in phase 1 of the last K-tile, ahead of A1(t+1): every later wait retires them)
  static constexpr int L1 = L0;
  static constexpr int S_HALF = 8 + (EPI == EP_RELU_BITS ? 4 : 0) + (EPI == EP_ROWDOT ? 4 : 0);
};

// Work-item order for split-K slice counts that are no multiple of 8 (e.g. 12 tiles x 21 slices).  Workgroup T runs on XCD T & 7;
// slice z belongs to XCD z % 8, and an XCD takes the (tile, slice) items of its own slices first, slice by slice, so that the tiles
// which stream the same operand panels meet in one L2; what an XCD has too many of (an XCD with three slices has 36 items for 31-32
// workgroups) goes to the XCDs with room.  In plain order (item = T) every XCD fetched every panel: K-tiles of 4.2 k cycles against
// 3.6 k with aligned slices.  Computed per workgroup from (tiles, slices) alone - a few scalar loops - so no table, no allocation
// and no host copy stand behind the product (round 2 kept a device table per shape in a process-wide cache).
__device__ __forceinline__ void esplitk_xcd_item(int T, int tiles, int nsl, int& id, int& z) {
  const int n = tiles * nsl, x = T & 7, k = T >> 3;
  auto cnt = [&](int xx) { return tiles * ((nsl - xx + 7) / 8); };   // items of the slices z = xx, xx + 8, ... < nsl
  auto cap = [&](int xx) { return (n - xx + 7) / 8; };               // workgroups T = xx, xx + 8, ... < n
  int kk = k, xo = x;
  if (k >= cnt(x)) {
    // one of this XCD's free places: the q-th of all free places (in XCD order) takes the q-th surplus item (in XCD order)
    int q = k - cnt(x);
    for (int xx = 0; xx < x; xx++) { const int dfc = cap(xx) - cnt(xx); q += dfc > 0 ? dfc : 0; }
    for (int xx = 0; xx < 8; xx++) {
      const int sp = cnt(xx) - cap(xx);
      if (sp <= 0) continue;
      if (q < sp) { xo = xx; kk = cap(xx) + q; break; }
      q -= sp;
    }
  }
  z = xo + 8 * (kk / tiles);
  id = kk % tiles;
}

template <bool TA, bool TB, int EPI>
__global__ __launch_bounds__(512, 2) void gemm_bf16_e256(GemmP p, int ks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef ECnt<EPI> CN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int ntn = (int)(p.N / E_BN);
  const int nt = (int)(p.M / E_BM) * ntn;
  const int G = gridDim.x;  // multiple of 8
  const int q8 = nt >> 3, r8 = nt & 7;
  const bf16raw* A = (const bf16raw*)p.A;
  const bf16raw* B = (const bf16raw*)p.B;
  int nk = (int)(p.K / E_BK);  // >= 2 (launcher); split-K: the work item's K-tiles (set below)
  const unsigned offA = elane_off<TA, true>(p.lda, tid), offB = elane_off<TB, false>(p.ldb, tid);
  const bool colsum = EPI == EP_GATE_BITS && (p.flags & PERO_GEMM_COLSUM);

  // stored products: `ks` = N-tiles of one row panel a workgroup walks ONE AFTER THE OTHER (0 / 1: none - the ntn workgroups of an XCD that share a row panel
  // run its ntn N-tiles side by side and all wait for the SAME bytes from HBM; `seq` > 1 leaves ntn / seq sharers per panel and seq x as many panels in flight)
  const int ksq = ks & 15;
  const bool inter = ks & 16;   // the side-by-side workgroups take ADJACENT N-tiles (n = r * sharers + j instead of j * seq + r)
  const int seq = (EPI != EP_SPLITK && ksq > 1 && r8 == 0 && ntn % ksq == 0 && (G >> 3) % (ntn / ksq) == 0 && q8 % (((G >> 3) / (ntn / ksq)) * ntn) == 0) ? ksq : 1;
  auto tile_of = [&](int T, long long& tm0, long long& tn0) {
    const int xcd = T & 7;
    int loc = T >> 3;
    if (seq > 1) {
      const int per = G >> 3, sh = ntn / seq, l = loc % per, k = loc / per;
      loc = ((k / seq) * (per / sh) + l / sh) * ntn + (inter ? (k % seq) * sh + l % sh : (l % sh) * seq + k % seq);
    }
    const int id = E_XCD_TILE(xcd, loc, q8, r8);
    tm0 = (long long)(id / ntn) * E_BM;
    tn0 = (long long)(id % ntn) * E_BN;
  };
  int T = blockIdx.x;
  long long tm0, tn0, nm0, nn0, kbeg = 0;
  bool has_next = false;
  long long ws_slot = 0;   // split-K with a workspace: this work item's place among the partial tiles, (tile, slice) -> tile * slices + slice
  if (EPI == EP_SPLITK) {
    // work item = (tile, k-slice); the slices of one XCD's workgroups are the same few (operand panels fetched once per L2)
    const int xcd = T & 7, r = T >> 3;
    int id, z;
    if (ks < 0 && p.kchunk) esplitk_xcd_item(T, ntn * (int)(p.M / E_BM), -ks, id, z);  // any slice count, XCD by XCD
    else if (ks < 0) { id = T / (-ks); z = T % (-ks); }  // any slice count: plain order
    else if (ks >= 8) { const int per = ks >> 3; z = xcd * per + (r % per); id = r / per; }
    else { z = xcd % ks; id = r * (8 / ks) + xcd / ks; }
    tm0 = (long long)(id / ntn) * E_BM; tn0 = (long long)(id % ntn) * E_BN;
    nm0 = tm0; nn0 = tn0;
    // K-tiles are dealt evenly: the first (steps % slices) slices take one more
    const int steps = (int)(p.K / E_BK), nsl = ks < 0 ? -ks : ks, base = steps / nsl, rem = steps % nsl;
    nk = base + (z < rem ? 1 : 0);
    kbeg = (long long)(z * base + (z < rem ? z : rem)) * E_BK;
    ws_slot = (long long)id * nsl + z;
  } else {
    if (T >= nt) return;
    tile_of(T, tm0, tn0);
    has_next = T + G < nt;
    tile_of(has_next ? T + G : T, nm0, nn0);
  }

  // fragment read addresses (per lane, relative to a half tile's base)
  //  K-contiguous image [128 rows][128 B]: row = row0 + (lane & 15), 16-byte chunk (4 s + (lane >> 4)) ^ (row & 7)
  const unsigned rc0 = E_FRAG_OFF(lane);
  //  K-major image [64 k-rows][256 B]: see frag_kmajor (gemm.hip); 32-byte block (col >> 4) ^ fk(krow)
  const int li = lane & 15, lq = lane >> 4;
  const int kf = (li >> 2) | ((lq & 1) << 2);
  const unsigned rk0 = (unsigned)((8 * lq + (li >> 2)) * 256 + 8 * (li & 3));
  // Transposed fragments are read by inline asm: behind an LDS-DMA hipcc (ROCm 7.2) puts `s_waitcnt vmcnt(0)` in front of every
  // ds_read_b64_tr_b16 it can see (three per K-tile in the K-major kernels: each phase's reads then waited for the half tile
  // issued a quarter of a K-tile earlier, i.e. for the whole memory latency, and the counted vmcnt(6) of phase 4 never mattered).
  // The ds_read_b128 of the K-contiguous images do not get that wait.  Every read here is retired by the phase's own
  // `s_waitcnt lgkmcnt(0)` in front of its MFMAs (E_LGKM0_F ties the fragment registers to that wait).
  auto rd_tr = [&](const unsigned char* a) -> bf8v {
    typedef int i2v_ __attribute__((ext_vector_type(2)));
    i2v_ lo, hi;
    const unsigned addr = (unsigned)(unsigned long long)LDS_PTR(const unsigned char, a);
    asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:1024" : "=&v"(lo), "=&v"(hi) : "v"(addr) : "memory");
    return __builtin_bit_cast(bf8v, __builtin_shufflevector(lo, hi, 0, 1, 2, 3));
  };
  auto rdA = [&](const unsigned char* base, int i, int s) -> bf8v {  // rows 64 wr + 16 i of an A half
    if (!TA) return *(const bf8v*)(base + (64 * wr + 16 * i) * 128 + (rc0 ^ (s << 6)));
    return rd_tr(base + rk0 + s * 32 * 256 + (((4 * wr + i) ^ kf) << 5));
  };
  auto rdB = [&](const unsigned char* base, int j, int s) -> bf8v {  // rows 32 wc + 16 j of a B half
    if (!TB) return *(const bf8v*)(base + (32 * wc + 16 * j) * 128 + (rc0 ^ (s << 6)));
    return rd_tr(base + rk0 + s * 32 * 256 + (((2 * wc + j) ^ kf) << 5));
  };

  f4v acc[2][2][4][2];  // [A half][B half][i][j]
  bf8v fa[4][2], fb0[2][2], fb1[2][2];

#define E_RD_A(H_)                                                            \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; i_++) {                          \
    fa[i_][0] = rdA(kt + (H_) * E_HALF, i_, 0);                               \
    fa[i_][1] = rdA(kt + (H_) * E_HALF, i_, 1);                               \
  }
#define E_RD_B(F_, H_)                                                        \
  _Pragma("unroll") for (int j_ = 0; j_ < 2; j_++) {                          \
    F_[j_][0] = rdB(kt + (2 + (H_)) * E_HALF, j_, 0);                         \
    F_[j_][1] = rdB(kt + (2 + (H_)) * E_HALF, j_, 1);                         \
  }
// the same, with the fragments read by asm in this phase tied to the wait (an MFMA cannot move in front of it)
#define E_LGKM0_A()                                                                                                       \
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fa[1][0]), "+v"(fa[1][1]), "+v"(fa[2][0]), \
               "+v"(fa[2][1]), "+v"(fa[3][0]), "+v"(fa[3][1]) :: "memory");                                              \
  __builtin_amdgcn_sched_barrier(0);
#define E_LGKM0_B(F_)                                                                                                     \
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(F_[0][0]), "+v"(F_[0][1]), "+v"(F_[1][0]), "+v"(F_[1][1]) :: "memory");     \
  __builtin_amdgcn_sched_barrier(0);

  // the LDS-DMA stream: half tile `which` (0 A0, 1 A1, 2 B0, 3 B1) of K-tile u of the current tile (u >= nk: of the next
  // one; a workgroup's last tile "prefetches" its own first K-tiles again: the stream keeps its shape, no branches)
  const EStep<TA, 64> sa(p.lda);
  const EStep<TB, 32> sb(p.ldb);
  const unsigned char* cA = (const unsigned char*)A + tm0 * sa.tile + (kbeg / E_BK) * sa.ktile;
  const unsigned char* cB = (const unsigned char*)B + tn0 * sb.tile + (kbeg / E_BK) * sb.ktile;
  const unsigned char* nA = (const unsigned char*)A + nm0 * sa.tile;
  const unsigned char* nB = (const unsigned char*)B + nn0 * sb.tile;
  auto issue = [&](int u, int which, unsigned char* ktbase) {
    if (EPI == EP_SPLITK && u >= nk) return;  // one work item: nothing follows (the ring is the epilogue's staging area)
    const bool nx = u >= nk;
    const long long uu = nx ? u - nk : u;
    unsigned char* dst = ktbase + which * E_HALF + wave * 1024;
    if (which < 2) eglds2((nx ? nA : cA) + uu * sa.ktile + which * sa.half, sa.piece, offA, dst);
    else eglds2((nx ? nB : cB) + uu * sb.ktile + (which - 2) * sb.half, sb.piece, offB, dst);
  };
  const bool use_bias = (EPI <= EP_RELU_BITS) && p.bias;
  unsigned char* const biasl = smem + E_BIAS + wave * 1024;
  auto issue_bias = [&](long long bn) {  // 256 floats = 64 lanes x 16 B, this wave's private copy
    const float* src = use_bias ? p.bias + bn : (const float*)p.B;  // (no bias: any readable address; the copy is not used)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((const unsigned char*)src + lane * 16),
                                     (__attribute__((address_space(3))) void*)(biasl), 16, 0, 0);
  };

  if (EPI == EP_GATE_BITS) {
    // bit e of a mask byte keeps column e of the lane's 8: dword k holds columns 2k (low half) and 2k + 1
    if (tid < 256) {
      eu4v m;
#pragma unroll
      for (int k = 0; k < 4; k++) m[k] = (((tid >> (2 * k)) & 1) ? 0x0000ffffu : 0u) | (((tid >> (2 * k + 1)) & 1) ? 0xffff0000u : 0u);
      *(eu4v*)(smem + E_LUT + tid * 16) = m;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // visible to every wave behind the prologue's barrier
  }
  // ---- prologue: K-tile 0 and all of K-tile 1 (a tile's A1(1) is always issued ahead of its first K-tile)
  issue(0, 2, smem); issue(0, 0, smem); issue(0, 3, smem); issue(0, 1, smem);
  issue(1, 2, smem + E_KTILE); issue(1, 0, smem + E_KTILE); issue(1, 3, smem + E_KTILE); issue(1, 1, smem + E_KTILE);
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  E_BAR();
  if (wr == 1) { E_BAR(); }  // the stagger: waves 4-7 run one barrier behind

  int d = 0;  // ring slot of the current K-tile
  bool first = true;

  // Epilogue addressing.  After the column swap lane (li, lq) holds the 8 columns 8 cq .. 8 cq + 7 of a 32-column block of row li:
  // the four 16-byte pieces of a row sit in lanes 16 apart and ADJACENT lanes belong to different rows.  The memory pipeline merges
  // the addresses of adjacent lanes only: stored (or loaded) like that, a 1 KiB wave-instruction is 64 separate 16-byte requests and
  // takes 64 cycles of the CU's store path instead of 16 (tools/probe_store3.hip: 128 KiB tile 7.5 k cycles against 2.1 k, at any
  // row pitch, with nothing else running).  So the packed values go through ONE lane transpose first (see below): lane L then holds
  // piece L & 3 of row L >> 2 and four adjacent lanes cover 64 contiguous bytes; side inputs and the bit mask are addressed in that
  // layout as well.
  const int cq = ((lq & 1) << 1) | (lq >> 1);
  const int er = lane >> 2, ep = lane & 3;                                          // row and 16-byte piece of the transposed layout
  const unsigned cvo = (unsigned)(((128 * wr + er) * p.ldc + 64 * wc + 8 * ep) * 2);   // C
  const unsigned gvo = (unsigned)(((128 * wr + er) * (EPI == EP_RESID ? p.ldr : p.ldg) + 64 * wc + 8 * ep) * 2);  // residual / row-dot matrix
  // bit mask (EP_RELU_BITS out, EP_GATE_BITS in): 8 bytes per row and wave; row pitch ldg, or - PERO_GEMM_MASK_TILED - 32 bytes inside the N-tile's own M x 32 plane
  const bool mtiled = (EPI == EP_RELU_BITS || EPI == EP_GATE_BITS) && (p.flags & PERO_GEMM_MASK_TILED);
  const long long mld = mtiled ? 32 : p.ldg;
  auto mask_base = [&](long long tm, long long tn) -> const unsigned char* {
    return (const unsigned char*)p.gate + (mtiled ? (tn >> 8) * p.M * 32 + tm * 32 : tm * p.ldg + (tn >> 3));
  };
  const unsigned mvo = (unsigned)((128 * wr + er) * mld + 8 * wc);
  // The transpose goes through LDS memory: a unit is written as the lanes hold it (one ds_write_b128: row li, piece cq) and read back
  // in the transposed layout (one ds_read_b128: row er, piece ep) - 13 + 4 cycles of the LDS pipeline per unit against 4 x 6 for
  // four ds_bpermute_b32 (tools/probe_bperm.hip); the f32 sums of EP_RESID 2 x (13 + 4) against 8 x 6, and without their lane
  // swaps.  A wave's LDS instructions execute in order, so the read needs no wait of its own and a slot is reused without one.
  // Pieces are XOR-swizzled so that both directions are conflict-free (bf16: [16 rows][64 B], 2 slots; f32: [16][128 B]).
  unsigned char* const xstg = smem + E_XSTG + wave * 2048;
  const unsigned xw16 = (unsigned)(li * 64 + ((cq ^ ((li >> 1) & 3)) << 4));
  const unsigned xr16 = (unsigned)(er * 64 + ((ep ^ ((er >> 1) & 3)) << 4));
  const int xsw = (li ^ ((li >> 1) & 1)) & 7, xsr = (er ^ ((er >> 1) & 1)) & 7;
  const unsigned xw32 = (unsigned)(li * 128), xr32 = (unsigned)(er * 128);
  (void)xw16; (void)xr16; (void)xsw; (void)xsr; (void)xw32; (void)xr32;
  const unsigned char* const lutp = smem + E_LUT;
  // bf16 pairs (1, 0) and (0, 1) in registers the compiler cannot fold: as a constant operand hipcc (ROCm 7.2) prints the pair (1, 0) as the
  // inline constant `1.0`, which v_dot2c_f32_bf16 reads as the f32 pattern 0x3f800000 = the pair (0, 1) (measured: both sums took the odd column)
  unsigned sel_lo = 0x00003f80u, sel_hi = 0x3f800000u;
  asm volatile("" : "+s"(sel_lo), "+s"(sel_hi));
  float cs_run = 0.f;        // EP_GATE_BITS + column sums: the wave's running sums of its current N-tile (see the epilogue)
  long long cs_tn0 = -1;
  eu4v side0[8], side1[8];   // side inputs of rows 0-63 / 64-127 (EP_RESID, EP_ROWDOT: 16 B per unit)
  eu2v sm0[4], sm1[4];       // EP_GATE_BITS: the 8 mask bytes of a row (this wave's 64 columns), per row group

  for (;;) {
    E_ACC_ZERO();
    issue_bias(tn0);  // this tile's bias row for its epilogue: part of the stream (older than everything a later wait counts)

    // side-input descriptor of this tile
    const int spitch = (int)(EPI == EP_RESID ? p.ldr * 2 : EPI == EP_ROWDOT ? p.ldg * 2 : mld);  // bytes per row
    const ei4v srs = ersrc(EPI == EP_RESID ? (const void*)((const bf16raw*)p.resid + tm0 * p.ldr + tn0)
                           : EPI == EP_ROWDOT ? (const void*)((const bf16raw*)p.gate + tm0 * p.ldg + tn0)
                           : (const void*)mask_base(tm0, tn0),
                           (unsigned)(256 * spitch));

    // one K-tile; LAST = the tile's last one (peeled: the side loads of the epilogue start in its phase 4 and their registers
    // are live from there only)
    auto ktile = [&](auto last_c, const int t) __attribute__((always_inline)) {
      constexpr bool last = decltype(last_c)::value;
      unsigned char* const kt = smem + d * E_KTILE;         // K-tile t
      unsigned char* const kn = smem + (d ^ 1) * E_KTILE;   // K-tiles t + 1 (being completed) and, slot by slot, t + 2
      // P1
      E_RD_B(fb0, 0);
      __builtin_amdgcn_sched_barrier(0);
      E_RD_A(0);
      if (EPI == EP_GATE_BITS && last) {  // the tile's mask bytes (8 per row and wave): 8 small loads, four phases ahead of the epilogue
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int so0 = 16 * i * spitch, so1 = (64 + 16 * i) * spitch;
          E_BLOAD8(sm0[i], mvo, srs, so0, 0);
          E_BLOAD8(sm1[i], mvo, srs, so1, 0);
        }
      }
      if (last || t > 0) issue(t + 1, 1, kn);                       // A1(t+1)  (a tile's A1(1) went out ahead of the previous epilogue)
      if (TA) asm volatile("s_waitcnt lgkmcnt(15)" ::: "memory");  // the B0 reads (issued first) are done: B0 may be restaged in P2
      else asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
      E_BAR();
      E_LGKM0_B(fb0);
      E_LGKM0_A();
      E_MFMA(0, 0, fb0);
      E_BAR();
      // P2
      E_RD_B(fb1, 1);
      issue(t + 2, 2, kt);                                  // B0(t+2)
      E_BAR();
      E_LGKM0_B(fb1);
      E_MFMA(0, 1, fb1);
      E_BAR();
      // P3
      E_RD_A(1);
      issue(t + 2, 0, kt);                                  // A0(t+2)
      E_BAR();
      E_LGKM0_A();
      E_MFMA(1, 1, fb1);
      E_BAR();
      // P4
      if (CN::L0 && last) {  // side inputs of the wave's rows 0-63
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int so = 16 * i * spitch;
          E_BLOAD16(side0[2 * i], gvo, srs, so, 0);
          E_BLOAD16(side0[2 * i + 1], gvo, srs, so, 64);
        }
      }
      issue(t + 2, 3, kt);                                  // B1(t+2)
      // K-tile t+1 has landed (this wave's pieces).  What was issued after its last half tile A1(t+1) stays in flight:
      // normally the three half tiles of t+2; in a tile's first K-tile also the previous epilogue (side loads of rows 64-127,
      // stores) and the bias row; in its last K-tile the side loads issued just above.
      if (!last && t == 0 && first) E_VMCNT(7);  // + the bias row
      // (the column-sum atomic of EP_GATE_BITS leaves only when the workgroup's N-tile changes: on that one tile the count below asks for
      //  one operation more than needed to have retired - never for one less)
      else if (!last && t == 0 && !first) E_VMCNT(6 + 1 + CN::L1 + 2 * CN::S_HALF);
      else if (CN::L0 && last) E_VMCNT(6 + CN::L0);
      else if (EPI == EP_SPLITK && t + 2 >= nk) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stream has ended
      else E_VMCNT(6);
      E_BAR();
      E_MFMA(1, 0, fb0);
      E_BAR();
      d ^= 1;
    };
    // (the first K-tile is its own copy of the code: its MFMAs take the zero accumulators as an inline constant, so the 128 registers
    //  are never cleared by moves, and its t == 0 cases fold)
    ktile(std::false_type{}, 0);
    for (int t = 1; t < nk - 1; t++) ktile(std::false_type{}, t);
    ktile(std::true_type{}, nk - 1);

    // ---- epilogue, straight from the accumulators
    first = false;
    issue(nk + 1, 1, smem + (d ^ 1) * E_KTILE);  // A1 of the next tile's K-tile 1: ahead of the stores in the in-order counter
    // Undo the stagger for the epilogue.  Staggered, waves 4-7 sit at the barrier behind their last MFMA
    // cluster until waves 0-3 reach the next tile's first barrier, i.e. through the whole epilogue of waves 0-3, and waves 0-3 then
    // sit through the epilogue of waves 4-7: the two epilogues ran one after the other (stamps at K = 512: 4.5 k + 5.3 k cycles of a
    // 40 k-cycle tile).  With one extra barrier here waves 0-3 wait the 256 cycles of that last cluster and both epilogues run
    // side by side; waves 4-7 take the extra barrier in front of the next tile, which staggers the groups again.
    if (EPI != EP_SPLITK && wr == 0) { E_BAR(); }
    if (EPI == EP_SPLITK) {
      // f32 tile added into C with atomics whose wave-instructions cover 256 contiguous bytes (full atomic rate): two rounds
      // through the (now free) 128 KiB ring, [128 rows][256 f32], 16-byte chunk index XORed with (row & 15)
      if (wr == 0) { E_BAR(); }  // undo the stagger: every wave has finished its last reads and MFMAs
      if (p.resid) {
        // partial tile -> workspace with plain 16-byte stores, accumulator by accumulator: every wave-instruction writes 1 KiB of
        // contiguous bytes ([accumulator][wave][lane] float4; pero_splitk_reduce_k knows the layout).  The slices of a tile are summed
        // by that kernel in slice order: deterministic, and 6 TB/s of stores + one pass over the partials instead of f32 atomics, which
        // the chip executes at 1.3 TB/s of added bytes (MI355X_MICROARCH.md): 64 MB per launch were ~49 us of every weight gradient.
        f4v* const W = (f4v*)p.resid + ws_slot * (E_BM * E_BN / 4) + wave * 64 + lane;
#pragma unroll
        for (int ha = 0; ha < 2; ha++)
#pragma unroll
          for (int hb = 0; hb < 2; hb++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
              for (int j = 0; j < 2; j++) W[(((ha * 2 + hb) * 4 + i) * 2 + j) * 512] = acc[ha][hb][i][j];
        return;
      }
      float* const C = (float*)p.C;
#pragma unroll
      for (int ha = 0; ha < 2; ha++) {
        if (ha) { E_LGKM0(); E_BAR(); }
#pragma unroll
        for (int hb = 0; hb < 2; hb++)
#pragma unroll
          for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
              const int row = 64 * wr + 16 * i + li, chunk = 16 * wc + 8 * hb + 4 * j + lq;
              *(f4v*)(smem + row * 1024 + ((chunk ^ (row & 15)) << 4)) = acc[ha][hb][i][j];
            }
        E_LGKM0();
        E_BAR();
        // staged row r = 64 * wr' + rr  <->  tile row 128 * wr' + 64 * ha + rr
#pragma unroll 4
        for (int it = 0; it < 64; it++) {
          const int item = it * 8 + wave, row = item >> 2, seg = item & 3;
          const int col = 64 * seg + lane;
          const float v = *(const float*)(smem + row * 1024 + ((((col >> 2)) ^ (row & 15)) << 4) + (col & 3) * 4);
          const long long grow = tm0 + 128 * (row >> 6) + 64 * ha + (row & 63);
          atomicAdd(C + grow * p.ldc + tn0 + col, v * p.alpha);
        }
      }
      return;
    }
    {
      const ei4v crs = ersrc((bf16raw*)p.C + tm0 * p.ldc + tn0, (unsigned)(256 * p.ldc * 2));
      const int cpitch = (int)(p.ldc * 2);
      // bias of the lane's columns as the accumulators hold them: 64 wc + 32 hb + 16 j + 4 (lane >> 4) .. + 3
      f4v bx[2][2];
#pragma unroll
      for (int hb = 0; hb < 2; hb++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
          bx[hb][j] = (f4v){0.f, 0.f, 0.f, 0.f};
          if (use_bias) bx[hb][j] = *(const f4v*)(biasl + (64 * wc + 32 * hb + 16 * j + 4 * lq) * 4);
        }
      float cs[2][8];  // EP_GATE_BITS + column sums
      float rd[4];     // EP_ROWDOT: row dots of one row group
#pragma unroll
      for (int hb = 0; hb < 2; hb++)
#pragma unroll
        for (int e = 0; e < 8; e++) cs[hb][e] = 0.f;
#pragma unroll
      for (int ha = 0; ha < 2; ha++) {
        if (CN::L1 && ha == 0) {  // side inputs of rows 64-127, then wait for those of rows 0-63
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int so = (64 + 16 * i) * spitch;
            E_BLOAD16(side1[2 * i], gvo, srs, so, 0);
            E_BLOAD16(side1[2 * i + 1], gvo, srs, so, 64);
          }
          E_WAIT8(2 + 2 + CN::L1, side0);
        }
        if (CN::L1 && ha == 1) E_WAIT8(CN::S_HALF, side1);
        if (EPI == EP_GATE_BITS && ha == 0) {
          // retired by phase 4's wait of the last K-tile long ago (the statements tie the registers to a wait)
          E_WAIT4(63, sm0);
          E_WAIT4(63, sm1);
        }
        // Units (row group i, B half hb) are computed NI row groups at a time, instruction kind by instruction kind: one unit's chain
        // (add -> convert -> lane swap -> store, each waiting for the one before, and the next unit reusing the same registers)
        // took ~190 cycles of a wave that had the SIMD to itself (stamps); independent chains side by side fill those gaps.
        constexpr int NI = (EPI == EP_RESID || EPI == EP_ROWDOT) ? 1 : 2;
#pragma unroll
        for (int ib = 0; ib < 4; ib += NI) {
          eu4v o[NI][2];
          eu4v kp[NI][2];   // EP_GATE_BITS: the AND masks of the unit's 8 columns, requested with the staging reads (not in front of their use)
          (void)kp;
#pragma unroll
          for (int ii = 0; ii < NI; ii++)
#pragma unroll
            for (int hb = 0; hb < 2; hb++) {
              const int i = ib + ii;
              if (EPI == EP_GATE_BITS) {
                const eu2v mm = ha ? sm1[i] : sm0[i];
                const unsigned byte = __builtin_amdgcn_ubfe(hb ? mm[1] : mm[0], 8u * (unsigned)ep, 8u);
                kp[ii][hb] = *(const eu4v*)(lutp + (byte << 4));
              }
              // (alpha = 1: the other kernels' acc * alpha + bias, bit for bit; the modes that never take a bias skip the add of zero)
              const f4v x = EPI <= EP_RELU_BITS ? acc[ha][hb][i][0] + bx[hb][0] : acc[ha][hb][i][0];
              const f4v y = EPI <= EP_RELU_BITS ? acc[ha][hb][i][1] + bx[hb][1] : acc[ha][hb][i][1];
              if (EPI == EP_RESID) {
                // f32 columns first (one rounding), through the staging image: x = columns 4 lq .. + 3 (piece lq), y = columns 16 + 4 lq ..
                // (piece 4 + lq) of the row's 32 f32; read: columns 8 ep .. + 7
                float v[8];
                *(f4v*)(xstg + xw32 + ((lq ^ xsw) << 4)) = x;
                *(f4v*)(xstg + xw32 + (((4 + lq) ^ xsw) << 4)) = y;
                const f4v r0 = *(const f4v*)(xstg + xr32 + (((2 * ep) ^ xsr) << 4));
                const f4v r1 = *(const f4v*)(xstg + xr32 + (((2 * ep + 1) ^ xsr) << 4));
#pragma unroll
                for (int e = 0; e < 4; e++) { v[e] = r0[e]; v[4 + e] = r1[e]; }
                const eu4v r4 = ha ? side1[2 * i + hb] : side0[2 * i + hb];
#pragma unroll
                for (int e = 0; e < 4; e++) { v[2 * e] += __uint_as_float(r4[e] << 16); v[2 * e + 1] += __uint_as_float(r4[e] & 0xffff0000u); }
                o[ii][hb][0] = pack2bf(v[0], v[1]); o[ii][hb][1] = pack2bf(v[2], v[3]); o[ii][hb][2] = pack2bf(v[4], v[5]); o[ii][hb][3] = pack2bf(v[6], v[7]);
              } else {
                unsigned px0 = pack2bf(x[0], x[1]), px1 = pack2bf(x[2], x[3]);
                unsigned py0 = pack2bf(y[0], y[1]), py1 = pack2bf(y[2], y[3]);
                if (EPI == EP_RELU || EPI == EP_RELU_BITS) {
                  // ReLU on the ROUNDED pairs: one v_pk_max_i16 per dword instead of two v_max_f32 (rounding keeps the sign, so
                  // max(round(x), 0) == round(max(x, 0)); a negative value or -0 is a negative int16 and becomes +0)
                  px0 = epk_relu(px0); px1 = epk_relu(px1); py0 = epk_relu(py0); py1 = epk_relu(py1);
                }
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
            unsigned mL = 0, mH = 0;
            if (EPI == EP_ROWDOT) rd[i] = 0.f;
#pragma unroll
            for (int hb = 0; hb < 2; hb++) {
              eu4v& ou = o[ii][hb];
              if (EPI == EP_RELU_BITS) {
                // bit e = (stored column e > 0); after the ReLU every half word is +0, -0 or positive
                unsigned z = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                  const unsigned m = epk_nonzero(ou[k]);  // bit 0: low half > 0, bit 16: high half (one v_pk_min_u16: the halves are >= +0)
                  z |= m << (2 * k);
                }
                const unsigned byte = (z & 0x55u) | ((z >> 15) & 0xaau);
                if (hb == 0) mL = byte << (8 * ep); else mH = byte << (8 * ep);
              }
              if (EPI == EP_GATE_BITS) {
                // column sums always (no branch per dword on the runtime flag; only the final atomic is conditional): one
                // v_dot2c_f32_bf16 per column pair and half, (x, y) . (1, 0) and (x, y) . (0, 1) - exact products, exact sums with zero
#pragma unroll
                for (int k = 0; k < 4; k++) {
                  ou[k] &= kp[ii][hb][k];
                  cs[hb][2 * k] = edot2(ou[k], sel_lo, cs[hb][2 * k]);
                  cs[hb][2 * k + 1] = edot2(ou[k], sel_hi, cs[hb][2 * k + 1]);
                }
              }
              if (EPI == EP_ROWDOT) {
                const eu4v g4 = ha ? side1[2 * i + hb] : side0[2 * i + hb];
#pragma unroll
                for (int k = 0; k < 4; k++) rd[i] = edot2(ou[k], g4[k], rd[i]);   // one v_dot2c_f32_bf16 instead of 4 unpacks, 2 multiplies, 2 adds
              }
              if (hb) E_BSTORE16(ou, cvo, crs, so, 64); else E_BSTORE16(ou, cvo, crs, so, 0);
            }
            if (EPI == EP_RELU_BITS) {
              // OR over the four lanes of a row (one quad): every one of them then holds the row's 8 bytes
              mL |= (unsigned)__builtin_amdgcn_mov_dpp((int)mL, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
              mH |= (unsigned)__builtin_amdgcn_mov_dpp((int)mH, 0xB1, 0xf, 0xf, false);
              mL |= (unsigned)__builtin_amdgcn_mov_dpp((int)mL, 0x4E, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
              mH |= (unsigned)__builtin_amdgcn_mov_dpp((int)mH, 0x4E, 0xf, 0xf, false);
              const eu2v mo = {mL, mH};
              const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc((unsigned char*)mask_base(tm0, tn0), 0, (int)(256 * mld), 0x00020000);
              // all four store them (same address, same data): one instruction, no branch (storing from the quad's first lane only
              // measured no faster)
              __builtin_amdgcn_raw_buffer_store_b64(mo, mrs, mvo, (64 * ha + 16 * i) * (int)mld, 0);
            }
            if (EPI == EP_ROWDOT) {
              // sum over the four lanes of a row (one quad), then its first lane adds into [m][n / 128] (two waves per 128-column block)
              float s = rd[i];
              s += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s), 0xB1, 0xf, 0xf, false));
              s += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s), 0x4E, 0xf, 0xf, false));
              float* dst = (float*)p.bias + (tm0 + 128 * wr + 64 * ha + 16 * i + er) * (p.N >> 7) + ((tn0 + 64 * wc) >> 7);
              if (ep == 0) atomicAdd(dst, s);
            }
          }
        }
      }
      if (colsum) {
        // column sums of the tile's 128 rows of this wave.  A lane holds 16 partial sums (its 8 columns x 2 B halves) of its
        // rows; a halving butterfly over the 16 row indices of the wave (lane bits 2-5: xor 32, 16, 8, 4; each step a lane keeps half of
        // its values and adds the partner's copy of them - 15 exchanges instead of 64) leaves the total of value `er` on the lane,
        // and ONE atomic instruction with all 64 lanes adds the wave's 64 column sums
        // The exchanges stay in the vector ALU (round 3; as 15 ds_bpermute_b32 the four dependent LDS round trips at the very end of the
        // epilogue were ~1 us per tile = 6 % of the gated product): lanes 32 / 16 apart trade by v_permlane32_swap / v_permlane16_swap - the
        // swap of (a, b) followed by a + b IS "keep one, add the partner's copy of it" for both partners at once - lanes 8 / 4 apart by DPP
        // row rotations / shifts; a + partner(a) is the same on both partners, each then keeps the sum that is its to keep.
        float w8[8], w4[4], w2[2];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(cs[0][j]), __float_as_uint(cs[1][j]), false, false);
          w8[j] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);      // lanes 0-31 (er & 8 == 0): cs[0][j] of both; lanes 32-63: cs[1][j] of both
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(w8[j]), __float_as_uint(w8[j + 4]), false, false);
          w4[j] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);      // er & 4 == 0: w8[j] of both; else w8[j + 4] of both
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const float s0 = w4[j] + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(w4[j]), 0x128, 0xf, 0xf, false));          // row_ror:8 = lane ^ 8
          const float s1 = w4[j + 2] + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(w4[j + 2]), 0x128, 0xf, 0xf, false));
          w2[j] = (er & 2) ? s1 : s0;
        }
        // lane ^ 4 inside a row of 16: lanes with bit 2 clear take lane + 4 (row_shl:4 into banks 0, 2), the others lane - 4 (row_shr:4 into banks 1, 3)
        auto x4 = [&](float v) -> float {
          int r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x104, 0xf, 0x5, false);
          r = __builtin_amdgcn_update_dpp(r, __float_as_int(v), 0x114, 0xf, 0xa, false);
          return __int_as_float(r);
        };
        const float t0 = w2[0] + x4(w2[0]), t1 = w2[1] + x4(w2[1]);
        const float tot = (er & 1) ? t1 : t0;     // value index er = 8 * hb + e, of the lane's piece ep
        // A persistent workgroup keeps ONE N-tile while ntn divides its stride (ntn = 8 at N = 2048: always): the wave's 64 column sums run
        // on in ONE register over its tiles and leave by one atomic when the N-tile changes or the kernel ends (per tile: 131 072
        // wave-atomics per 2048-line launch onto 2048 addresses, each of them in the in-order vmcnt queue for ~3 k cycles)
        if (tn0 != cs_tn0) {
          if (cs_tn0 >= 0) atomicAdd((float*)p.bias + cs_tn0 + 64 * wc + 32 * (er >> 3) + 8 * ep + (er & 7), cs_run);
          cs_run = 0.f; cs_tn0 = tn0;
        }
        cs_run += tot;
      }
    }
    if (!has_next) break;
    T += G;
    tm0 = nm0; tn0 = nn0; cA = nA; cB = nB;
    has_next = T + G < nt;
    tile_of(has_next ? T + G : T, nm0, nn0);
    nA = (const unsigned char*)A + nm0 * sa.tile;
    nB = (const unsigned char*)B + nn0 * sb.tile;
    if (wr == 1) { E_BAR(); }  // the stagger again
  }
  if (EPI == EP_GATE_BITS && colsum && cs_tn0 >= 0) atomicAdd((float*)p.bias + cs_tn0 + 64 * wc + 32 * (lane >> 5) + 8 * (lane & 3) + ((lane >> 2) & 7), cs_run);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last tile's surplus prefetches land before the LDS is released
#undef E_RD_A
#undef E_RD_B
}

// C[tile] += alpha * sum over the slices (in slice order) of the partial tiles the split-K work items left in the workspace.
// One thread per float4 position of a tile: consecutive threads read consecutive 16 bytes of every partial tile.
__global__ __launch_bounds__(256) void pero_splitk_reduce_k(const f4v* ws, float* C, long long ldc, int ntn, int nsl, float alpha, bool vec4) {
  const int tile = blockIdx.x >> 6;                                   // 64 blocks of 256 threads per 256 x 256 tile
  const int pos = ((blockIdx.x & 63) << 8) + threadIdx.x;             // (accumulator * 8 + wave) * 64 + lane
  const f4v* src = ws + (long long)tile * nsl * (E_BM * E_BN / 4) + pos;
  f4v sum = src[0];
  int z = 1;
  for (; z + 8 <= nsl; z += 8) {   // eight partial tiles requested together, added in slice order
    f4v v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = src[(long long)(z + k) * (E_BM * E_BN / 4)];
#pragma unroll
    for (int k = 0; k < 8; k++) sum += v[k];
  }
  for (; z < nsl; z++) sum += src[(long long)z * (E_BM * E_BN / 4)];
  const int lane = pos & 63, wave = (pos >> 6) & 7, idx = pos >> 9;
  const int ha = idx >> 4, hb = (idx >> 3) & 1, i = (idx >> 1) & 3, j = idx & 1;
  const long long row = (long long)(tile / ntn) * E_BM + 128 * (wave >> 2) + 64 * ha + 16 * i + (lane & 15);
  const long long col = (long long)(tile % ntn) * E_BN + 64 * (wave & 3) + 32 * hb + 16 * j + 4 * (lane >> 4);
  // plain read-modify-write, 16 bytes per thread when C allows it: C must have ONE writer at a time in this mode (pero_hip.h,
  // PERO_GEMM_ATOMIC with a workspace).  As four f32 atomics per thread the pass took 21 us instead of 14 per launch (50 launches a step).
  float* dst = C + row * ldc + col;
  if (vec4) {
    f4v* d4 = (f4v*)dst;
    *d4 = *d4 + sum * alpha;
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) dst[e] += sum[e] * alpha;
  }
}
__global__ __launch_bounds__(256) void pero_zero16_k(f4v* p, long long n16) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) p[i] = (f4v){0.f, 0.f, 0.f, 0.f};
}

// Slice count of a split-K product on this kernel (k_split <= 0: the library chooses) and whether the slices can be aligned to the XCDs.
static int e256_splitk_slices(long long tiles, long long steps, int k_split, bool* xcd_ok) {
  int ks = k_split;
  if (ks <= 0) {  // the library chooses: one round of workgroups over the CUs
    ks = (int)(256 / tiles);
    if (ks >= 8) ks = (ks / 8) * 8; else if (ks >= 4) ks = 4; else if (ks >= 2) ks = 2; else ks = 1;
    // an XCD-aligned slice count (one slice set per XCD: operand panels fetched once per L2) when it fills >= 90 % of the CUs
    // that the plain count fills, else the plain count
    int kx = (int)(256 / tiles);
    kx = kx < 1 ? 1 : kx;
    if (ks * tiles * 10 < kx * tiles * 9) ks = kx;
  }
  while (ks > 1 && steps / ks < 2) ks--;
  if (xcd_ok) *xcd_ok = pero_xcd_slices(tiles, ks);
  return ks;
}
// Bytes of caller-owned workspace with which a split-K product of this shape runs DETERMINISTICALLY on this kernel: every (tile, slice)
// work item leaves its f32 partial tile there by plain stores and pero_splitk_reduce_k adds the slices of a tile in slice order.  0: one
// slice.  Without (enough) workspace the product falls back to f32 atomics.
long long pero_gemm_e256_splitk_ws_bytes(long long M, long long N, int slices) {
  return slices > 1 ? (M / E_BM) * (N / E_BN) * slices * (long long)(E_BM * E_BN * sizeof(float)) : 0;
}

// EP_* epilogue mode of a stored bf16 product on this kernel, from its flags and pointers; -1: that combination (or a side input whose stride does not
// fit 32-bit byte offsets) is another kernel's.
static int e256_stored_epilogue(const GemmP& p) {
  const bool relu = p.flags & PERO_GEMM_RELU, bits = p.flags & PERO_GEMM_RELU_BITS, rowdot = p.flags & PERO_GEMM_ROWDOT, cs = p.flags & PERO_GEMM_COLSUM;
  int epi;
  if (rowdot) { if (relu || bits || cs || p.resid || !p.gate || !p.bias) return -1; epi = EP_ROWDOT; }
  else if (bits) {
    if (!p.gate || p.resid || (relu && cs)) return -1;
    // the gate epilogue has no input-bias path (its `bias` is the column-sum OUTPUT under PERO_GEMM_COLSUM): a gated product WITH an
    // input bias goes to gemm_bf16_r256, which adds it - both kernels then give the same bits at every tile count
    if (!relu && p.bias && !cs) return -1;
    epi = relu ? EP_RELU_BITS : EP_GATE_BITS;
  }
  else if (cs || p.gate) return -1;                  // column sums without the bit mask, bf16 gate rows: other kernels
  else if (p.resid) { if (relu) return -1; epi = EP_RESID; }
  else epi = relu ? EP_RELU : EP_PLAIN;
  if (!pero_ld_fits32({epi == EP_RESID ? p.ldr : 0, (epi == EP_ROWDOT || bits) ? p.ldg : 0})) return -1;
  return epi;
}

// Qualifies: one problem (batch 1), bf16 operands; stored bf16 output (alpha == 1) or a split-K f32 product; M % 256 == N % 256 == K % 64 == 0, K >= 128.
bool pero_gemm_e256_takes(const GemmP& p0, long long batch, int k_split, bool out_f32, int* slices) {
  if (p0.M % E_BM || p0.N % E_BN || p0.K % E_BK || p0.K < 2 * E_BK || batch != 1) return false;
  if (p0.flags & PERO_GEMM_ATOMIC) {
    // split-K: f32 C, plain product
    if (!out_f32 || p0.bias || p0.resid || p0.gate || (p0.flags & ~(PERO_GEMM_ATOMIC | PERO_GEMM_TRANS_A | PERO_GEMM_TRANS_B | PERO_GEMM_TILE_V | PERO_GEMM_TILE256))) return false;
    if (!pero_ld_fits32({p0.lda, p0.ldb})) return false;
    *slices = e256_splitk_slices((p0.M / E_BM) * (p0.N / E_BN), p0.K / E_BK, k_split, nullptr);
    return true;
  }
  if (k_split > 1 || out_f32 || (p0.flags & PERO_GEMM_ACCUM)) return false;
  if (p0.alpha != 1.0f) return false;
  if (!pero_ld_fits32({p0.lda, p0.ldb, p0.ldc})) return false;
  const int epi = e256_stored_epilogue(p0);
  if (epi < 0) return false;
  if (epi != EP_PLAIN && (p0.flags & (PERO_GEMM_TRANS_A | PERO_GEMM_TRANS_B))) return false;   // the fused epilogues exist for the K-contiguous products only
  *slices = 1;
  return true;
}
// ws / ws_bytes: the caller's workspace for the split-K partial tiles (pero_gemm's `workspace`); never allocated here.
void pero_gemm_e256_launch(const GemmP& p0, int k_split, hipStream_t st, void* ws, long long ws_bytes) {
  const bool ta = p0.flags & PERO_GEMM_TRANS_A, tb = p0.flags & PERO_GEMM_TRANS_B;
  int ks = 0;
  if (p0.flags & PERO_GEMM_ATOMIC) {
    // equal slices of whole K-tiles, one slice set per XCD
    const long long tiles = (p0.M / E_BM) * (p0.N / E_BN), steps = p0.K / E_BK;
    bool xcd_ok = false;
    ks = e256_splitk_slices(tiles, steps, k_split, &xcd_ok);
    GemmP p = p0;
    p.kchunk = 0;
    dim3 grid((unsigned)(tiles * ks)), block(512);
    const int nsl = ks;
    const bool ws_ok = ws && (((size_t)ws) & 15) == 0 && ws_bytes >= pero_gemm_e256_splitk_ws_bytes(p.M, p.N, nsl);
    p.resid = (g_opt.splitk_workspace && ws_ok && nsl > 1) ? ws : nullptr;
    if (!xcd_ok) {
      ks = -ks;
      p.kchunk = g_opt.splitk_table ? 1 : 0;   // work items handed out XCD by XCD (esplitk_xcd_item)
    }
#define LAUNCH_ES(TA_, TB_, OF_)                                                                                           \
  do {                                                                                                                     \
    PERO_LDS_ATTR((gemm_bf16_e256<TA_, TB_, EP_SPLITK>), E_LDS_BYTES);                                                     \
    hipLaunchKernelGGL((gemm_bf16_e256<TA_, TB_, EP_SPLITK>), grid, block, E_LDS_BYTES, st, p, ks);                       \
  } while (0)
    PERO_LAYOUT_LADDER(LAUNCH_ES, ta, tb, true);
#undef LAUNCH_ES
    if (p.resid)
      hipLaunchKernelGGL(pero_splitk_reduce_k, dim3((unsigned)(tiles * 64)), dim3(256), 0, st, (const f4v*)p.resid, (float*)p.C, (long long)p.ldc,
                         (int)(p.N / E_BN), nsl, p.alpha, p.ldc % 4 == 0 && (((size_t)p.C) & 15) == 0);
    return;
  }
  const int epi = e256_stored_epilogue(p0);
  GemmP p = p0;
  p.kchunk = p.K;
  const long long nt = (p.M / E_BM) * (p.N / E_BN);
  const unsigned G = pero_persistent_grid(nt);
  dim3 grid(G), block(512);
  // Walk of the stored K <= 512 products (the kernel's tile_of): by default the ntn workgroups of an XCD that share a 256-row panel of A run its ntn N-tiles side
  // by side and wait for the same bytes from HBM together.  With each workgroup taking `seq` N-tiles of its panel one after the other, seq x as many panels are in
  // flight per XCD and the panel's later passes come from the caches: 524 288 x 2048 x 512 plain / ReLU 1 056 -> 1 010 us, bit-mask gate 1 086 -> 1 054, N = 1536
  // 784 -> 772, N = 4096 2 117 -> 1 926 (seq 4 / 3; profiles/r04_e256_store_probes.txt).  NOT for the epilogue that writes the ReLU bit mask in ROWS (its 32 bytes per row and tile are a
  // quarter of a line: written rounds apart they cost more than the walk gains, 1 095 -> 1 147; with PERO_GEMM_MASK_TILED a tile's mask is whole lines), not at K = 2048 (+- 1 %).  Same tiles, same bits.
  if (g_opt.gemm_e_walk && p.K <= 512 && (epi == EP_PLAIN || epi == EP_RELU || epi == EP_GATE_BITS || (epi == EP_RELU_BITS && (p.flags & PERO_GEMM_MASK_TILED))) && nt >= 2LL * G) {
    const long long ntn = p.N / E_BN;
    ks = (ntn >= 8 && ntn % 4 == 0) ? 4 : (ntn >= 6 && ntn % 3 == 0) ? 3 : 0;
  }
  if (epi == EP_ROWDOT) {  // the two waves of a 128-column block add into it: cleared first (hipMemsetAsync's fill kernel took 27 us for these 4 MB)
    const long long n = p.M * (p.N >> 7);
    if (n % 4 == 0 && aligned16(p.bias))
      hipLaunchKernelGGL(pero_zero16_k, dim3((unsigned)((n / 4 + 255) / 256 < 2048 ? (n / 4 + 255) / 256 : 2048)), dim3(256), 0, st, (f4v*)p.bias, n / 4);
    else
      hipMemsetAsync((void*)p.bias, 0, (size_t)n * sizeof(float), st);
  }
#define LAUNCH_E(TA_, TB_, EP_)                                                               \
  do {                                                                                        \
    PERO_LDS_ATTR((gemm_bf16_e256<TA_, TB_, EP_>), E_LDS_BYTES);                              \
    hipLaunchKernelGGL((gemm_bf16_e256<TA_, TB_, EP_>), grid, block, E_LDS_BYTES, st, p, ks); \
  } while (0)
  if (!ta && !tb) {
    switch (epi) {
      case EP_RELU: LAUNCH_E(false, false, EP_RELU); break;
      case EP_RESID: LAUNCH_E(false, false, EP_RESID); break;
      case EP_RELU_BITS: LAUNCH_E(false, false, EP_RELU_BITS); break;
      case EP_GATE_BITS: LAUNCH_E(false, false, EP_GATE_BITS); break;
      case EP_ROWDOT: LAUNCH_E(false, false, EP_ROWDOT); break;
      default: LAUNCH_E(false, false, EP_PLAIN); break;
    }
  }
  else if (!ta && tb) LAUNCH_E(false, true, EP_PLAIN);
  else if (ta && tb) LAUNCH_E(true, true, EP_PLAIN);
  else LAUNCH_E(true, false, EP_PLAIN);
#undef LAUNCH_E
}
