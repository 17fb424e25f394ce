// Shared by the bf16 tile GEMM kernels (gemm.hip, gemm_o.hip, gemm_r.hip and, through gemm_e_common.hpp, gemm_e.hip, gemm_n.hip).
#pragma once
#include "common.hpp"
#include <initializer_list>

struct GemmP {
  const void* A; const void* B; void* C;
  const float* bias; const void* resid; const void* gate;
  long long M, N, K, lda, ldb, ldc, ldr, ldg;
  long long sAo, sAi, sBo, sBi, sCo, sCi;
  int binner; float alpha; int flags; long long kchunk;
};


// K-major LDS images: 32-byte blocks of a k-row are XORed with fk(krow) so that the two transposed 8-byte reads of
// a fragment (k-rows 8g+q and 8g+q+4 of the 4 lane groups) hit 32 distinct 8-byte slots of the 256-byte bank row.
__device__ __forceinline__ int fk(int krow) { return (krow & 3) | (((krow >> 3) & 1) << 2); }

template <int N_>
__device__ __forceinline__ void wait_vmcnt() {
  if (N_ == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
}
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");  // keep later LDS accesses below the barrier
}

// ---- host entries of the tile kernels.  Each family has a pure predicate `_takes` (the shape / epilogue restrictions of its kernel; no HIP call, no
// pointer dereferenced) and a `_launch` that cannot refuse: gemm_plan (gemm.hip) asks the predicates, pero_gemm launches what the plan names.
// ta / tb are p.flags' PERO_GEMM_TRANS_A / _B; `k_split` of a launch is the slice count the plan settled on (p.kchunk set to match).
// one-tile-per-workgroup 128x128x64 kernel (gemm_o.hip): split-K weight gradients of short reductions
bool pero_gemm_o128_takes(const GemmP& p);
void pero_gemm_o128_launch(const GemmP& p, long long batch, int k_split, bool out_f32, hipStream_t st);
// 256x128x32 eight-wave kernel (gemm_r.hip): stored products of small batches
bool pero_gemm_r256_takes(const GemmP& p);
void pero_gemm_r256_launch(const GemmP& p, long long batch, int k_split, bool out_f32, hipStream_t st);
// eight-phase ping-pong persistent 256x256x64 kernel (gemm_e.hip); k_split: as the caller asked (<= 0: the library chooses), *slices: the slice count
// the kernel runs with (1: a stored product).  ws / ws_bytes: the caller's workspace for split-K partial tiles (pero_gemm's `workspace`); null: f32 atomics
bool pero_gemm_e256_takes(const GemmP& p, long long batch, int k_split, bool out_f32, int* slices);
void pero_gemm_e256_launch(const GemmP& p, int k_split, hipStream_t st, void* ws, long long ws_bytes);
long long pero_gemm_e256_splitk_ws_bytes(long long M, long long N, int slices);
// row-complete 128 x 512 tile (gemm_n.hip, opt-in "gemm_nw"): N = 512 stored products with the plain / residual epilogue
bool pero_gemm_n512_takes(const GemmP& p, long long batch, bool out_f32);
void pero_gemm_n512_launch(const GemmP& p, hipStream_t st);
// ... and its fused LayerNorm forms, which have no other kernel to fall back to (false: the shape is not theirs, nothing was launched)
bool pero_launch_gemm_n512_ln(const GemmP& p, void* t, long long ldt, float* mean, float* rstd, const float* gamma, const float* beta, float eps,
                              hipStream_t st);
bool pero_launch_gemm_n512_lnb(const GemmP& p, const void* t, long long ldt, const float* rstd, const float* gamma, const float* beta, float* work,
                               int* grid_out, hipStream_t st);

// ---- host arithmetic shared by the split-K launchers
constexpr int PERO_BK128 = 64;   // K-step of both 128x128 kernels (T_BK, O_BK): gemm_plan chunks K for either
// `*k_split` slices of whole bk-wide K-steps: returns the chunk length and leaves in *k_split the slice count those chunks really make (<= 1: one slice, K)
static inline long long pero_k_chunk(long long K, int bk, int* k_split) {
  if (*k_split <= 1) { *k_split = 1; return K; }
  const long long steps = K / bk, per = (steps + *k_split - 1) / *k_split;
  *k_split = (int)((steps + per - 1) / per);
  return per * bk;
}
// can `tiles` x `ks` work items be dealt so that every XCD (workgroup index % 8) keeps the same few k-slices?
static inline bool pero_xcd_slices(long long tiles, int ks) {
  return (ks == 1 || ks == 2 || ks == 4 || ks % 8 == 0) && (tiles * ks) % 8 == 0 && (ks >= 8 || tiles % (8 / ks) == 0);
}
// LAUNCH_(TA, TB, OUTF32) with the three template arguments as constants
#define PERO_LAYOUT_LADDER(LAUNCH_, ta_, tb_, of_)                                                                  \
  do {                                                                                                              \
    if (!(ta_) && !(tb_)) { if (of_) LAUNCH_(false, false, true); else LAUNCH_(false, false, false); }              \
    else if (!(ta_) && (tb_)) { if (of_) LAUNCH_(false, true, true); else LAUNCH_(false, true, false); }            \
    else if ((ta_) && (tb_)) { if (of_) LAUNCH_(true, true, true); else LAUNCH_(true, true, false); }               \
    else { if (of_) LAUNCH_(true, false, true); else LAUNCH_(true, false, false); }                                 \
  } while (0)

// ---- host helpers of the persistent launchers
// CU count rounded down to a multiple of 8 (a grid is dealt to the 8 XCDs in turn), at least 8
static inline int pero_num_cus8() {
  const int n = (pero_num_cus() / 8) * 8;
  return n < 8 ? 8 : n;
}
// persistent grid over nt tiles: one workgroup per CU; fewer tiles: their count rounded up to a multiple of 8
static inline unsigned pero_persistent_grid(long long nt) {
  const int num_cus = pero_num_cus8();
  return (unsigned)(nt < num_cus ? ((nt + 7) / 8) * 8 : num_cus);
}
// every row stride (in elements) leaves the byte offsets inside a tile in 32 bits
static inline bool pero_ld_fits32(std::initializer_list<long long> lds) {
  for (const long long ld : lds)
    if (ld >= (1LL << 22)) return false;
  return true;
}
// rowops.hip: dgamma / dbeta / dxsum (each may be null) += the sum of the `nblocks` partial rows of work [3][nblocks][d]
void pero_ln_bwd_reduce_launch(const float* work, float* dgamma, float* dbeta, float* dxsum, int nblocks, int d, hipStream_t st);
