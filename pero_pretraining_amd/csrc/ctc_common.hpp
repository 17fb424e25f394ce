// What the CTC kernels share (ctc.hip: loss, gradient, greedy; ctc_decode.hip: beam search; ctc_align.hip: forced alignment): the limits, the
// helpers of the extended-state lattice, the wave-level row log-sum-exp, the per-thread state table and the frame loop of alpha and beta.  Every
// piece of arithmetic that include/pero_hip.h promises to be the same between loss, decoder and aligner exists here, once.  Derivation: DESIGN.md
// section 11 "Kernels".
#pragma once
#include "dispatch.hpp"

#define CTC_THREADS 256
#define CTC_MAX_S 512
#define CTC_MAX_C 8192
#define CTC_MAXK 5   // ceil((2 * CTC_MAX_S + 1) / CTC_THREADS): extended states of one thread
#define CTC_NEG_INF (-__builtin_huge_valf())

static __device__ __forceinline__ int ctc_clamp_len(int64_t v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// class of extended state s (even: blank); -1 for a label outside [0, C): such a state emits with probability 0
static __device__ __forceinline__ int ctc_state_class(const int64_t* tg, int s, int C, int blank) {
  if (!(s & 1)) return blank;
  const int64_t l = tg[s >> 1];
  return (l >= 0 && l < C) ? (int)l : -1;
}

// log(exp(a) + exp(b) + exp(c)); an all -inf triple stays -inf (no inf - inf)
static __device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == CTC_NEG_INF) return CTC_NEG_INF;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}
// x - lse; a -inf logit has log-probability -inf whatever the row's lse is
static __device__ __forceinline__ float ctc_logp(float x, float lse) { return x == CTC_NEG_INF ? CTC_NEG_INF : x - lse; }

// One wave, one logit row: max + log sum exp(x - max), an xor butterfly for the max and one for the sum; a row of -inf stays -inf.  Every lane
// gets the value.
template <typename T>
static __device__ __forceinline__ float ctc_wave_row_lse(const T* __restrict__ x, int C, int lane) {
  float mx = CTC_NEG_INF;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, Elem<T>::ld(x + c));
  mx = wave_max(mx);
  float sum = 0.f;
  if (mx != CTC_NEG_INF)
    for (int c = lane; c < C; c += 64) sum += expf(Elem<T>::ld(x + c) - mx);
  sum = wave_sum(sum);
  return mx == CTC_NEG_INF ? CTC_NEG_INF : mx + logf(sum);
}

// The states of thread tid: s = tid + k CTC_THREADS < Lp, their classes (-1: none, or a label outside [0, C)) and whether the transition over
// two states exists (from s - 2 forwards, to s + 2 backwards).
template <bool BACKWARD>
static __device__ __forceinline__ void ctc_state_table(const int64_t* __restrict__ tg, int Lp, int C, int blank, int (&cls)[CTC_MAXK],
                                                       bool (&skip)[CTC_MAXK]) {
#pragma unroll
  for (int k = 0; k < CTC_MAXK; k++) {
    const int s = threadIdx.x + k * CTC_THREADS;
    cls[k] = -1;
    skip[k] = false;
    if (s < Lp) {
      cls[k] = ctc_state_class(tg, s, C, blank);
      skip[k] = (BACKWARD ? s + 2 < Lp : s >= 2) && cls[k] != ctc_state_class(tg, BACKWARD ? s + 2 : s - 2, C, blank);
    }
  }
}
// the logits of one frame (x: its row) at the thread's states
template <typename T>
static __device__ __forceinline__ void ctc_emissions(const T* __restrict__ x, const int (&cls)[CTC_MAXK], float (&xe)[CTC_MAXK]) {
#pragma unroll
  for (int k = 0; k < CTC_MAXK; k++) xe[k] = cls[k] >= 0 ? Elem<T>::ld(x + cls[k]) : CTC_NEG_INF;
}

// The recursion over one line's lattice, frame by frame (BACKWARD: from frame Tn - 1 down), by one workgroup of CTC_THREADS threads; Tn >= 1.
// ctc_alpha_k and ctc_beta_k are this function with CtcSumCell (ctc.hip).
// Thread j owns the states j, j + 256, .. with class and skip flag in registers.  lds: two rows of W + 4 floats in ping-pong, frame t in row
// t & 1; row entry s + 2 holds state s, and the two entries in front of state 0 (BACKWARD: behind state Lp - 1) stay -inf: the neighbours
// that do not exist.  A frame's emissions (and what cell.frame loads) are issued ahead of the ONE barrier per frame and needed only after the
// three LDS reads.  The cell decides what a state's value is and what is stored per (t, s):
//   cell.frame(t)                            the frame's own scalars
//   cell.first(v, t, s, live, xe)            v = the value in the initial frame; live: s < 2 (BACKWARD: s >= Lp - 2)
//   cell.next(v, t, s, same, one, two, xe)   v = the value from those of states s, s -+ 1, s -+ 2 (-inf where that transition does not exist)
// v is the state's row entry: the cell writes it, then stores what it keeps of (t, s).
// Returns the row of the last frame processed; it is complete for the other threads after a barrier.
template <typename T, bool BACKWARD, typename Cell>
static __device__ __forceinline__ const float* ctc_lattice_sweep(const T* __restrict__ x, const int64_t* __restrict__ tg, float* lds, int W, int Tn,
                                                                 int Lp, int C, int blank, Cell& cell) {
  const int tid = threadIdx.x;
  float* rows[2] = {lds, lds + W + 4};
  int cls[CTC_MAXK];
  bool skip[CTC_MAXK];
  ctc_state_table<BACKWARD>(tg, Lp, C, blank, cls, skip);
  if (tid < 2) rows[0][(BACKWARD ? Lp + 2 : 0) + tid] = rows[1][(BACKWARD ? Lp + 2 : 0) + tid] = CTC_NEG_INF;

  const int t0 = BACKWARD ? Tn - 1 : 0, d = BACKWARD ? 1 : -1;
  float xe[CTC_MAXK];
  cell.frame(t0);
  ctc_emissions(x + (long long)t0 * C, cls, xe);
#pragma unroll
  for (int k = 0; k < CTC_MAXK; k++) {
    const int s = tid + k * CTC_THREADS;
    if (s < Lp) cell.first(rows[t0 & 1][s + 2], t0, s, BACKWARD ? s >= Lp - 2 : s < 2, xe[k]);
  }
  for (int i = 1; i < Tn; i++) {
    const int t = BACKWARD ? t0 - i : i;
    cell.frame(t);
    ctc_emissions(x + (long long)t * C, cls, xe);
    __syncthreads();   // the previous frame's row is complete; everyone is done reading this frame's row (the previous frame read it)
    const float* prev = rows[(t & 1) ^ 1];
    float* cur = rows[t & 1];
#pragma unroll
    for (int k = 0; k < CTC_MAXK; k++) {
      const int s = tid + k * CTC_THREADS;
      if (s < Lp) cell.next(cur[s + 2], t, s, prev[s + 2], prev[s + 2 + d], skip[k] ? prev[s + 2 + 2 * d] : CTC_NEG_INF, xe[k]);
    }
  }
  return rows[(BACKWARD ? 0 : Tn - 1) & 1];
}

// ---------------------------------------------------------------------------------------------- host side (defined in ctc.hip)
// The refusals every entry point over the lattice shares: PERO_OK, PERO_E_INVALID (dtype, sizes, blank, N S >= 2^31) or PERO_E_UNSUPPORTED (above
// the limits).  Lmax = 0 where there are no targets.
int ctc_check(const char* name, int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int dtype);
// Launches ctc_row_lse_k: row_lse[n S + t] of every row (input_lengths null) or of the rows t < T alone (the others neither read nor written).
int ctc_launch_row_lse(const void* logits, const int64_t* input_lengths, float* row_lse, int64_t N, int64_t S, int64_t C, int dtype, hipStream_t st);
