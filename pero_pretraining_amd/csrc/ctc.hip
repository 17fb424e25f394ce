// CTC on the head's own (N*S, C) logit rows: loss (log-domain alpha recursion over a fused log-softmax), gradient with respect to the LOGITS
// (beta recursion + a per-row class sum without float atomics) and greedy decoding.  Contract: include/pero_hip.h; derivation: DESIGN.md.
//
//   pero_ctc_fwd    ctc_row_lse_k  one wave per logit row: ctc_wave_row_lse (N*S rows, all of them parallel); pero_ctc_align launches it too,
//                                  through ctc_launch_row_lse, for the rows t < T alone
//                   ctc_alpha_k    one workgroup per line: ctc_lattice_sweep (ctc_common.hpp: states across the threads, two LDS rows in
//                                  ping-pong, ONE barrier per frame) forwards with the log-sum-exp cell, then the line's nll
//   pero_ctc_bwd    ctc_beta_k     the same sweep and cell backwards in time; also builds the line's "next occurrence of the same label" chain
//                   ctc_grad_k     one workgroup per logit row: per-state posteriors -> LDS, class sums by ONE writer per class walking its
//                                  chain in label order (blank: per-thread strided sum, wave shuffle, four partials in wave order) -> the row
//   pero_ctc_greedy ctc_greedy_k   one workgroup per line: a wave per row for the argmax (first maximum), one thread collapses the line
#include "ctc_common.hpp"

template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_row_lse_k(const T* __restrict__ logits, const int64_t* __restrict__ input_lengths,
                                                             float* __restrict__ row_lse, long long rows, int S, int C) {
  const long long row = (long long)blockIdx.x * (CTC_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  if (input_lengths && (int)(row % S) >= ctc_clamp_len(input_lengths[row / S], S)) return;   // a row behind the line's frames is never read
  const int lane = threadIdx.x & 63;
  const float lse = ctc_wave_row_lse(logits + row * C, C, lane);
  if (lane == 0) row_lse[row] = lse;
}

// The cell of ctc_lattice_sweep for alpha and beta: (+) of the three neighbours, times the state's own emission probability; every (t, s) goes
// to out (alpha or beta of the line), entry t W + s.
struct CtcSumCell {
  const float* lse;
  float* out;
  int W;
  float le;
  __device__ __forceinline__ void frame(int t) { le = lse[t]; }
  __device__ __forceinline__ void first(float& v, int t, int s, bool live, float xe) {
    const float a = live ? xe - le : CTC_NEG_INF;
    v = a;
    out[(long long)t * W + s] = a;
  }
  __device__ __forceinline__ void next(float& v, int t, int s, float same, float one, float two, float xe) {
    const float m = ctc_lse3(same, one, two);
    const float a = m == CTC_NEG_INF ? CTC_NEG_INF : m + (xe - le);
    v = a;
    out[(long long)t * W + s] = a;
  }
};

// LDS: the two rows of ctc_lattice_sweep
template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_alpha_k(const T* __restrict__ logits, const int64_t* __restrict__ targets,
                                                           const int64_t* __restrict__ input_lengths, const int64_t* __restrict__ target_lengths,
                                                           const float* __restrict__ row_lse, float* __restrict__ alpha, float* __restrict__ nll,
                                                           int S, int C, int Lmax, int blank) {
  extern __shared__ float ctc_lds[];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int W = 2 * Lmax + 1;
  const int Tn = ctc_clamp_len(input_lengths[n], S), L = ctc_clamp_len(target_lengths[n], Lmax), Lp = 2 * L + 1;
  if (Tn == 0) {   // no frame: the empty path spells the empty string
    if (tid == 0) nll[n] = L == 0 ? 0.f : __builtin_huge_valf();
    return;
  }
  CtcSumCell cell{row_lse + (long long)n * S, alpha + (long long)n * S * W, W, 0.f};
  const float* last = ctc_lattice_sweep<T, false>(logits + (long long)n * S * C, targets + (long long)n * Lmax, ctc_lds, W, Tn, Lp, C, blank, cell);
  __syncthreads();
  if (tid == 0) {
    const float v = ctc_lse3(last[Lp - 1 + 2], last[Lp - 2 + 2], CTC_NEG_INF);   // Lp == 1: entry 1 is the -inf pad
    nll[n] = -v;
  }
}

// chain[n][i] for label i of line n: bit 0 = i is the first occurrence of its label, bits 1.. = (index of the next occurrence) + 1, 0 = none.
// Labels equal to blank or outside [0, C) get 0: the former are summed with the blank states, the latter emit nothing.
// LDS: the two rows of ctc_lattice_sweep | lab[Lmax] label classes
template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_beta_k(const T* __restrict__ logits, const int64_t* __restrict__ targets,
                                                          const int64_t* __restrict__ input_lengths, const int64_t* __restrict__ target_lengths,
                                                          const float* __restrict__ row_lse, float* __restrict__ beta, int32_t* __restrict__ chain,
                                                          int S, int C, int Lmax, int blank) {
  extern __shared__ float ctc_lds[];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int W = 2 * Lmax + 1;
  const int Tn = ctc_clamp_len(input_lengths[n], S), L = ctc_clamp_len(target_lengths[n], Lmax), Lp = 2 * L + 1;
  int* lab = (int*)(ctc_lds + 2 * (W + 4));
  const int64_t* tg = targets + (long long)n * Lmax;

  for (int i = tid; i < L; i += CTC_THREADS) lab[i] = ctc_state_class(tg, 2 * i + 1, C, blank);
  __syncthreads();
  for (int i = tid; i < L; i += CTC_THREADS) {
    const int c = lab[i];
    int v = 0;
    if (c >= 0 && c != blank) {
      int first = 1, next = -1;
      for (int j = 0; j < i; j++) first &= lab[j] != c;
      for (int j = i + 1; j < L; j++)
        if (lab[j] == c) { next = j; break; }
      v = ((next + 1) << 1) | first;
    }
    chain[(long long)n * Lmax + i] = v;
  }
  if (Tn == 0) return;
  CtcSumCell cell{row_lse + (long long)n * S, beta + (long long)n * S * W, W, 0.f};
  ctc_lattice_sweep<T, true>(logits + (long long)n * S * C, tg, ctc_lds, W, Tn, Lp, C, blank, cell);
}

// LDS: occ[C] class sums | w[W] per-state posteriors | part[4] blank partials of the waves
template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_grad_k(const T* __restrict__ logits, const int64_t* __restrict__ targets,
                                                          const int64_t* __restrict__ input_lengths, const int64_t* __restrict__ target_lengths,
                                                          const float* __restrict__ row_lse, const float* __restrict__ alpha,
                                                          const float* __restrict__ beta, const float* __restrict__ nll, const float* __restrict__ g,
                                                          const int32_t* __restrict__ chain, T* __restrict__ dlogits, int S, int C, int Lmax,
                                                          int blank, int zero_infinity) {
  extern __shared__ float ctc_lds[];
  const long long row = blockIdx.x;
  const int n = (int)(row / S), t = (int)(row % S), tid = threadIdx.x;
  const int W = 2 * Lmax + 1;
  const int Tn = ctc_clamp_len(input_lengths[n], S), L = ctc_clamp_len(target_lengths[n], Lmax), Lp = 2 * L + 1;
  T* dx = dlogits + row * C;
  const float loss = nll[n];
  if (t >= Tn || (zero_infinity && !(fabsf(loss) < __builtin_huge_valf()))) {
    for (int c = tid; c < C; c += CTC_THREADS) Elem<T>::st(dx + c, 0.f);
    return;
  }
  float* occ = ctc_lds;
  float* w = ctc_lds + C;
  float* part = w + W;
  const int64_t* tg = targets + (long long)n * Lmax;
  const int32_t* ch = chain + (long long)n * Lmax;
  const T* x = logits + row * C;
  const float le = row_lse[row], gn = g[n];
  const float* al = alpha + row * W;
  const float* be = beta + row * W;

  for (int c = tid; c < C; c += CTC_THREADS) occ[c] = 0.f;
  float blank_sum = 0.f;   // this thread's blank-class states, in state order
  for (int s = tid; s < Lp; s += CTC_THREADS) {
    const int c = ctc_state_class(tg, s, C, blank);
    float v = 0.f;
    if (c >= 0) v = expf(((al[s] + be[s]) + loss) - (Elem<T>::ld(x + c) - le));
    w[s] = v;
    if (c == blank) blank_sum += v;
  }
  blank_sum = wave_sum(blank_sum);
  if ((tid & 63) == 0) part[tid >> 6] = blank_sum;
  __syncthreads();
  for (int i = tid; i < L; i += CTC_THREADS) {
    const int v = ch[i];
    if (v & 1) {   // first occurrence: the one writer of its class
      float sum = w[2 * i + 1];
      for (int j = (v >> 1) - 1; j >= 0; j = (ch[j] >> 1) - 1) sum += w[2 * j + 1];
      occ[tg[i]] = sum;
    }
  }
  if (tid == 0) occ[blank] = ((part[0] + part[1]) + part[2]) + part[3];
  __syncthreads();
  for (int c = tid; c < C; c += CTC_THREADS) Elem<T>::st(dx + c, gn * (expf(Elem<T>::ld(x + c) - le) - occ[c]));
}

// LDS: S ints, the rows' argmax classes | the line's decoded length
template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_greedy_k(const T* __restrict__ logits, const int64_t* __restrict__ input_lengths,
                                                            int64_t* __restrict__ out, int64_t* __restrict__ out_lengths, int S, int C, int blank) {
  extern __shared__ float ctc_lds[];
  int* arg = (int*)ctc_lds;
  int& n_out = arg[S];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int Tn = ctc_clamp_len(input_lengths[n], S);
  for (int t = tid >> 6; t < Tn; t += CTC_THREADS / 64) {
    const T* x = logits + ((long long)n * S + t) * C;
    float best = CTC_NEG_INF;
    int at = C;   // no candidate yet
    for (int c = lane; c < C; c += 64) {
      const float v = Elem<T>::ld(x + c);
      if (at == C || v > best) { best = v; at = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oa = __shfl_xor(at, o, 64);
      if (oa < C && (at == C || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    if (lane == 0) arg[t] = at;
  }
  __syncthreads();
  int64_t* o = out + (long long)n * S;
  if (tid == 0) {
    int k = 0, last = -1;
    for (int t = 0; t < Tn; t++) {
      const int c = arg[t];
      if (c != last && c != blank) o[k++] = c;
      last = c;
    }
    out_lengths[n] = k;
    n_out = k;
  }
  __syncthreads();
  for (int k = n_out + tid; k < S; k += CTC_THREADS) o[k] = -1;
}

// ---------------------------------------------------------------------------------------------- host side
int ctc_check(const char* name, int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int dtype) {
  PERO_REQUIRE(dtype == PERO_F32 || dtype == PERO_BF16, "%s: bad dtype", name);
  PERO_REQUIRE(N > 0 && N < (1LL << 31) && S > 0 && C >= 2, "%s: bad sizes (N %lld, S %lld, C %lld)", name, (long long)N, (long long)S, (long long)C);
  PERO_REQUIRE(Lmax >= 0, "%s: Lmax %lld is negative", name, (long long)Lmax);
  PERO_REQUIRE(blank >= 0 && blank < C, "%s: blank %lld outside [0, C = %lld)", name, (long long)blank, (long long)C);
  if (S > CTC_MAX_S || Lmax > CTC_MAX_S || C > CTC_MAX_C) {   // Lmax may exceed S (a padded target matrix); a line with L > T is infeasible
    pero_set_error("%s: supported up to S = %d, Lmax = %d and C = %d (got S %lld, Lmax %lld, C %lld)", name, CTC_MAX_S, CTC_MAX_S, CTC_MAX_C, (long long)S,
                   (long long)Lmax, (long long)C);
    return PERO_E_UNSUPPORTED;
  }
  PERO_REQUIRE(N * S < (1LL << 31), "%s: N * S must be below 2^31", name);
  return PERO_OK;
}

int ctc_launch_row_lse(const void* logits, const int64_t* input_lengths, float* row_lse, int64_t N, int64_t S, int64_t C, int dtype, hipStream_t st) {
  const int64_t rows = N * S;
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t);
    hipLaunchKernelGGL((ctc_row_lse_k<T>), dim3((unsigned)((rows + 3) / 4)), dim3(CTC_THREADS), 0, st, (const T*)logits, input_lengths, row_lse,
                       (long long)rows, (int)S, (int)C); }), "bad dtype");
  return PERO_OK;
}

extern "C" int pero_ctc_fwd(const void* logits, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths, float* row_lse,
                            float* alpha, float* nll, int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int dtype, void* stream) {
  const int rc = ctc_check("pero_ctc_fwd", N, S, C, Lmax, blank, dtype);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE(logits && input_lengths && target_lengths && row_lse && alpha && nll && (targets || Lmax == 0), "pero_ctc_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  ctc_launch_row_lse(logits, nullptr, row_lse, N, S, C, dtype, st);   // every row, as the header promises
  PERO_CHECK_LAUNCH("pero_ctc_fwd (row lse)");
  const size_t lds = 2 * (2 * (size_t)Lmax + 5) * sizeof(float);
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t);
    hipLaunchKernelGGL((ctc_alpha_k<T>), dim3((unsigned)N), dim3(CTC_THREADS), lds, st, (const T*)logits, targets, input_lengths, target_lengths,
                       (const float*)row_lse, alpha, nll, (int)S, (int)C, (int)Lmax, (int)blank); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_ctc_fwd (alpha)");
  return PERO_OK;
}

extern "C" int pero_ctc_bwd(const void* logits, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths,
                            const float* row_lse, const float* alpha, const float* nll, const float* g, float* beta, int32_t* chain, void* dlogits,
                            int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int zero_infinity, int dtype, void* stream) {
  const int rc = ctc_check("pero_ctc_bwd", N, S, C, Lmax, blank, dtype);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE(logits && input_lengths && target_lengths && row_lse && alpha && nll && g && beta && dlogits && ((targets && chain) || Lmax == 0),
               "pero_ctc_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds_b = (2 * (2 * (size_t)Lmax + 5) + (size_t)Lmax) * sizeof(float);
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t);
    hipLaunchKernelGGL((ctc_beta_k<T>), dim3((unsigned)N), dim3(CTC_THREADS), lds_b, st, (const T*)logits, targets, input_lengths, target_lengths,
                       row_lse, beta, chain, (int)S, (int)C, (int)Lmax, (int)blank); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_ctc_bwd (beta)");
  const size_t lds_g = ((size_t)C + 2 * (size_t)Lmax + 1 + 4) * sizeof(float);
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t);
    hipLaunchKernelGGL((ctc_grad_k<T>), dim3((unsigned)(N * S)), dim3(CTC_THREADS), lds_g, st, (const T*)logits, targets, input_lengths,
                       target_lengths, row_lse, alpha, (const float*)beta, nll, g, (const int32_t*)chain, (T*)dlogits, (int)S, (int)C, (int)Lmax,
                       (int)blank, zero_infinity); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_ctc_bwd (gradient)");
  return PERO_OK;
}

extern "C" int pero_ctc_greedy(const void* logits, const int64_t* input_lengths, int64_t* out, int64_t* out_lengths, int64_t N, int64_t S, int64_t C,
                               int64_t blank, int dtype, void* stream) {
  const int rc = ctc_check("pero_ctc_greedy", N, S, C, 0, blank, dtype);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE(logits && input_lengths && out && out_lengths, "pero_ctc_greedy: null pointer");
  hipStream_t st = (hipStream_t)stream;
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t);
    hipLaunchKernelGGL((ctc_greedy_k<T>), dim3((unsigned)N), dim3(CTC_THREADS), ((size_t)S + 1) * sizeof(int), st, (const T*)logits, input_lengths, out,
                       out_lengths, (int)S, (int)C, (int)blank); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_ctc_greedy");
  return PERO_OK;
}
