// CTC forced alignment on the device: the best state path of a line's label string (Viterbi), its character spans and its
// log-probabilities.  Contract and arithmetic: include/pero_hip.h; derivation, tie rule and error bounds: DESIGN.md "CTC forced alignment".
//
//   pero_ctc_align  ctc_row_lse_k    (ctc.hip, through ctc_launch_row_lse) one wave per logit row t < T: the kernel pero_ctc_fwd launches
//                   ctc_align_k      one workgroup per line: the max-recursion over the extended states, on ctc_common.hpp's state table
//                                    and emission prefetch (two LDS rows in ping-pong, ONE barrier per frame), one backpointer byte per
//                                    (t, s); then one thread walks the T backpointers, one thread per frame finds the span ends, one
//                                    thread per label sums its own frames in order.  The frame loop is the kernel's own: through
//                                    ctc_lattice_sweep the compiler scheduled it differently, and the call with the backpointers in
//                                    global memory measured 2 % longer
// The backpointers of a line live in dynamic LDS when S (2 Lmax + 1) <= ALIGN_LDS_BACK_MAX bytes (the walk back is T DEPENDENT reads: out
// of LDS it pays no global round trip per frame), else in the caller's `back` workspace.  Only f32 additions and comparisons touch the
// path: with -ffp-contract=off every bit of states, spans and path_logit is fixed by the header's formulas.
#include "ctc_common.hpp"

#define ALIGN_LDS_BACK_MAX (96 * 1024)   // bytes of backpointers kept in LDS (PERO_CTC_ALIGN_LDS_BACK_BYTES of the header)

// Dynamic LDS: two rows of W + 2 floats, W = 2 Lmax + 1 (row entry s + 2 holds state s; entries 0, 1 stay -inf: the predecessors of states
// 0 and 1) | path[S] ints, the state of every frame | span[2 Lmax] ints | with LDS_BACK: S W backpointer bytes, entry t W + s.
template <typename T, bool LDS_BACK>
__global__ __launch_bounds__(CTC_THREADS) void ctc_align_k(const T* __restrict__ logits, const int64_t* __restrict__ targets,
                                                             const int64_t* __restrict__ input_lengths, const int64_t* __restrict__ target_lengths,
                                                             const float* __restrict__ row_lse, uint8_t* __restrict__ back,
                                                             int32_t* __restrict__ states, int32_t* __restrict__ spans,
                                                             float* __restrict__ path_logit, float* __restrict__ score,
                                                             float* __restrict__ label_logp, int S, int C, int Lmax, int blank) {
  extern __shared__ float align_lds[];
  __shared__ float lse_sum, path_v;
  __shared__ int feasible;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int W = 2 * Lmax + 1;
  const int Tn = ctc_clamp_len(input_lengths[n], S), L = ctc_clamp_len(target_lengths[n], Lmax), Lp = 2 * L + 1;
  float* rows[2] = {align_lds, align_lds + W + 2};
  int* path = (int*)(align_lds + 2 * (W + 2));
  int* span = path + S;
  uint8_t* lback = (uint8_t*)(span + 2 * Lmax);
  uint8_t* gback = back + (long long)n * S * W;
  int32_t* so = states + (long long)n * S;
  int32_t* po = spans + (long long)n * Lmax * 2;
  float* lo = label_logp + (long long)n * Lmax;

  if (Tn == 0) {   // no frame: the empty path spells the empty string
    for (int t = tid; t < S; t += CTC_THREADS) so[t] = -1;
    for (int i = tid; i < 2 * Lmax; i += CTC_THREADS) po[i] = -1;
    for (int k = tid; k < Lmax; k += CTC_THREADS) lo[k] = 0.f;
    if (tid == 0) path_logit[n] = score[n] = L == 0 ? 0.f : CTC_NEG_INF;
    return;
  }
  const int64_t* tg = targets + (long long)n * Lmax;
  const T* x = logits + (long long)n * S * C;
  const float* lse = row_lse + (long long)n * S;

  int cls[CTC_MAXK];
  bool skip[CTC_MAXK];
  ctc_state_table<false>(tg, Lp, C, blank, cls, skip);
  if (tid < 2) rows[0][tid] = rows[1][tid] = CTC_NEG_INF;
  for (int i = tid; i < 2 * Lmax; i += CTC_THREADS) span[i] = -1;

  float xe[CTC_MAXK];
  ctc_emissions(x, cls, xe);
#pragma unroll
  for (int k = 0; k < CTC_MAXK; k++) {
    const int s = tid + k * CTC_THREADS;
    if (s < Lp) rows[0][s + 2] = s < 2 ? xe[k] : CTC_NEG_INF;
  }
  for (int t = 1; t < Tn; t++) {
    ctc_emissions(x + (long long)t * C, cls, xe);   // this frame's emissions: issued before the barrier, needed after the three LDS reads
    __syncthreads();   // row (t - 1) & 1 is complete; everyone is done reading row t & 1 (frame t - 1 read it as "previous")
    const float* prev = rows[(t - 1) & 1];
    float* cur = rows[t & 1];
#pragma unroll
    for (int k = 0; k < CTC_MAXK; k++) {
      const int s = tid + k * CTC_THREADS;
      if (s < Lp) {
        float best = prev[s + 2];
        int step = 0;
        const float a1 = prev[s + 1], a2 = skip[k] ? prev[s] : CTC_NEG_INF;
        if (a1 > best) { best = a1; step = 1; }   // strict: equal values keep the smaller step
        if (a2 > best) { best = a2; step = 2; }
        cur[s + 2] = xe[k] + best;
        if (LDS_BACK) lback[t * W + s] = (uint8_t)step;
        else gback[(long long)t * W + s] = (uint8_t)step;
      }
    }
  }
  __syncthreads();   // the last row and every backpointer of the line (LDS, or global memory written by this workgroup) are visible
  if (tid == 0) {
    const float* last = rows[(Tn - 1) & 1];
    int s = (Lp == 1 || last[Lp - 1 + 2] >= last[Lp - 2 + 2]) ? Lp - 1 : Lp - 2;
    const float v = last[s + 2];
    const bool ok = v > CTC_NEG_INF && v < __builtin_huge_valf();
    feasible = ok;
    path_v = v;
    path_logit[n] = ok ? v : CTC_NEG_INF;
    if (ok) {
      path[Tn - 1] = s;
      for (int t = Tn - 1; t > 0; t--) {
        s -= LDS_BACK ? lback[t * W + s] : gback[(long long)t * W + s];
        path[t - 1] = s;
      }
    }
  }
  if (tid == 64) {   // a second wave, beside the walk back: the rows' lse in frame order
    float sum = 0.f;
    for (int t = 0; t < Tn; t++) sum += lse[t];
    lse_sum = sum;
  }
  __syncthreads();
  const bool ok = feasible;
  for (int t = tid; t < S; t += CTC_THREADS) so[t] = ok && t < Tn ? path[t] : -1;
  if (ok)
    for (int t = tid; t < Tn; t += CTC_THREADS) {   // a label's frames are consecutive: its first and last frame each have one owner
      const int s = path[t];
      if (s & 1) {
        if (t == 0 || path[t - 1] != s) span[s - 1] = t;
        if (t == Tn - 1 || path[t + 1] != s) span[s] = t + 1;
      }
    }
  if (tid == 0) score[n] = ok ? path_v - lse_sum : CTC_NEG_INF;
  __syncthreads();
  for (int k = tid; k < Lmax; k += CTC_THREADS) {
    const int a = span[2 * k], b = span[2 * k + 1];
    po[2 * k] = a;
    po[2 * k + 1] = b;
    float acc = 0.f;
    if (a >= 0) {   // k < L on a feasible line: the label is a class
      const int c = (int)tg[k];
      for (int t = a; t < b; t++) acc += Elem<T>::ld(x + (long long)t * C + c) - lse[t];
    }
    lo[k] = acc;
  }
}

// ---------------------------------------------------------------------------------------------- host side
extern "C" int pero_ctc_align(const void* logits, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths,
                              int32_t* states, int32_t* spans, float* path_logit, float* score, float* label_logp, float* row_lse, void* back,
                              int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int flags, int dtype, void* stream) {
  const int rc = ctc_check("pero_ctc_align", N, S, C, Lmax, blank, dtype);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE((flags & ~PERO_CTC_ALIGN_GLOBAL_BACK) == 0, "pero_ctc_align: unknown flags %d", flags);
  PERO_REQUIRE(logits && input_lengths && target_lengths && states && path_logit && score && row_lse && back &&
                   ((targets && spans && label_logp) || Lmax == 0),
               "pero_ctc_align: null pointer");
  static_assert(ALIGN_LDS_BACK_MAX == PERO_CTC_ALIGN_LDS_BACK_BYTES, "the header states the constant");
  hipStream_t st = (hipStream_t)stream;
  const int64_t W = 2 * Lmax + 1;
  ctc_launch_row_lse(logits, input_lengths, row_lse, N, S, C, dtype, st);   // the rows t < T alone
  PERO_CHECK_LAUNCH("pero_ctc_align (row lse)");
  const bool lds_back = S * W <= ALIGN_LDS_BACK_MAX && !(flags & PERO_CTC_ALIGN_GLOBAL_BACK);   // host-known sizes only
  const size_t fixed = (2 * ((size_t)W + 2) + (size_t)S + 2 * (size_t)Lmax) * sizeof(float);
  const size_t lds = fixed + (lds_back ? (size_t)(S * W) : 0);
  const size_t lds_max = (2 * (2 * (size_t)CTC_MAX_S + 3) + 3 * (size_t)CTC_MAX_S) * sizeof(float) + ALIGN_LDS_BACK_MAX;
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(lds_back, [&](auto B) {
    constexpr bool LDS_BACK = decltype(B)::value;
    if (LDS_BACK) PERO_LDS_ATTR((ctc_align_k<T, LDS_BACK>), lds_max);
    hipLaunchKernelGGL((ctc_align_k<T, LDS_BACK>), dim3((unsigned)N), dim3(CTC_THREADS), lds, st, (const T*)logits, targets, input_lengths,
                       target_lengths, (const float*)row_lse, (uint8_t*)back, states, spans, path_logit, score, label_logp, (int)S, (int)C,
                       (int)Lmax, (int)blank); }); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_ctc_align (alignment)");
  return PERO_OK;
}
