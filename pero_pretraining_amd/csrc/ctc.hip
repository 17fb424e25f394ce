// CTC on the head's own (N*S, C) logit rows: loss (log-domain alpha recursion over a fused log-softmax), gradient with respect to the LOGITS
// (beta recursion + a per-row class sum without float atomics) and greedy decoding.  Contract: include/pero_hip.h; derivation: DESIGN.md.
//
//   pero_ctc_fwd    ctc_row_lse_k  one wave per logit row: lse = max + log sum exp(x - max)               (N*S rows, all of them parallel)
//                   ctc_alpha_k    one workgroup per line: extended states across the threads (in strides of 256 for L' > 256), two LDS rows
//                                  in ping-pong, ONE barrier per time step, the next step's emissions loaded ahead of the barrier
//   pero_ctc_bwd    ctc_beta_k     the same recursion backwards in time; also builds the line's "next occurrence of the same label" chain
//                   ctc_grad_k     one workgroup per logit row: per-state posteriors -> LDS, class sums by ONE writer per class walking its
//                                  chain in label order (blank: per-thread strided sum, wave shuffle, four partials in wave order) -> the row
//   pero_ctc_greedy ctc_greedy_k   one workgroup per line: a wave per row for the argmax (first maximum), one thread collapses the line
#include "losses_common.hpp"

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

template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_row_lse_k(const T* __restrict__ logits, float* __restrict__ row_lse, long long rows, int C) {
  const long long row = (long long)blockIdx.x * (CTC_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const T* x = logits + row * C;
  float mx = CTC_NEG_INF;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, Elem<T>::ld(x + c));
  mx = wave_max(mx);
  float sum = 0.f;
  if (mx != CTC_NEG_INF)
    for (int c = lane; c < C; c += 64) sum += expf(Elem<T>::ld(x + c) - mx);
  sum = wave_sum(sum);
  if (lane == 0) row_lse[row] = mx == CTC_NEG_INF ? CTC_NEG_INF : mx + logf(sum);
}

// LDS: two rows of W + 2 floats, W = 2 Lmax + 1.  Row entry s + 2 holds state s; entries 0, 1 stay -inf (the predecessors of states 0 and 1).
template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_alpha_k(const T* __restrict__ logits, const int64_t* __restrict__ targets,
                                                           const int64_t* __restrict__ input_lengths, const int64_t* __restrict__ target_lengths,
                                                           const float* __restrict__ row_lse, float* __restrict__ alpha, float* __restrict__ nll,
                                                           int S, int C, int Lmax, int blank) {
  extern __shared__ float ctc_lds[];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int W = 2 * Lmax + 1;
  const int Tn = ctc_clamp_len(input_lengths[n], S), L = ctc_clamp_len(target_lengths[n], Lmax), Lp = 2 * L + 1;
  float* rows[2] = {ctc_lds, ctc_lds + W + 2};
  if (Tn == 0) {   // no frame: the empty path spells the empty string
    if (tid == 0) nll[n] = L == 0 ? 0.f : __builtin_huge_valf();
    return;
  }
  const int64_t* tg = targets + (long long)n * Lmax;
  const T* x = logits + (long long)n * S * C;
  const float* lse = row_lse + (long long)n * S;
  float* al = alpha + (long long)n * S * W;

  int cls[CTC_MAXK];
  bool skip[CTC_MAXK];
#pragma unroll
  for (int k = 0; k < CTC_MAXK; k++) {
    const int s = tid + k * CTC_THREADS;
    cls[k] = -1;
    skip[k] = false;
    if (s < Lp) {
      cls[k] = ctc_state_class(tg, s, C, blank);
      skip[k] = s >= 2 && cls[k] != ctc_state_class(tg, s - 2, C, blank);
    }
  }
  if (tid < 2) rows[0][tid] = rows[1][tid] = CTC_NEG_INF;

  float xe[CTC_MAXK], le = lse[0];
#pragma unroll
  for (int k = 0; k < CTC_MAXK; k++) xe[k] = cls[k] >= 0 ? Elem<T>::ld(x + cls[k]) : CTC_NEG_INF;
#pragma unroll
  for (int k = 0; k < CTC_MAXK; k++) {
    const int s = tid + k * CTC_THREADS;
    if (s < Lp) {
      const float a = s < 2 ? xe[k] - le : CTC_NEG_INF;
      rows[0][s + 2] = a;
      al[s] = a;
    }
  }
  for (int t = 1; t < Tn; t++) {
    // this step's emissions: issued before the barrier, needed after the three LDS reads
    le = lse[t];
#pragma unroll
    for (int k = 0; k < CTC_MAXK; k++) xe[k] = cls[k] >= 0 ? Elem<T>::ld(x + (long long)t * C + cls[k]) : CTC_NEG_INF;
    __syncthreads();   // row (t - 1) & 1 is complete; everyone is done reading row t & 1 (step t - 1 read it as "previous")
    const float* prev = rows[(t - 1) & 1];
    float* cur = rows[t & 1];
#pragma unroll
    for (int k = 0; k < CTC_MAXK; k++) {
      const int s = tid + k * CTC_THREADS;
      if (s < Lp) {
        const float v = ctc_lse3(prev[s + 2], prev[s + 1], skip[k] ? prev[s] : CTC_NEG_INF);
        const float a = v == CTC_NEG_INF ? CTC_NEG_INF : v + (xe[k] - le);
        cur[s + 2] = a;
        al[(long long)t * W + s] = a;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    const float* last = rows[(Tn - 1) & 1];
    const float v = ctc_lse3(last[Lp - 1 + 2], last[Lp - 2 + 2], CTC_NEG_INF);   // Lp == 1: entry 1 is the -inf pad
    nll[n] = -v;
  }
}

// chain[n][i] for label i of line n: bit 0 = i is the first occurrence of its label, bits 1.. = (index of the next occurrence) + 1, 0 = none.
// Labels equal to blank or outside [0, C) get 0: the former are summed with the blank states, the latter emit nothing.
// LDS: two rows of W + 2 floats; row entry s holds state s, entries Lp, Lp + 1 stay -inf (the successors of the last two states).
template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_beta_k(const T* __restrict__ logits, const int64_t* __restrict__ targets,
                                                          const int64_t* __restrict__ input_lengths, const int64_t* __restrict__ target_lengths,
                                                          const float* __restrict__ row_lse, float* __restrict__ beta, int32_t* __restrict__ chain,
                                                          int S, int C, int Lmax, int blank) {
  extern __shared__ float ctc_lds[];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int W = 2 * Lmax + 1;
  const int Tn = ctc_clamp_len(input_lengths[n], S), L = ctc_clamp_len(target_lengths[n], Lmax), Lp = 2 * L + 1;
  float* rows[2] = {ctc_lds, ctc_lds + W + 2};
  int* lab = (int*)(ctc_lds + 2 * (W + 2));   // Lmax label classes
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

  const T* x = logits + (long long)n * S * C;
  const float* lse = row_lse + (long long)n * S;
  float* be = beta + (long long)n * S * W;
  int cls[CTC_MAXK];
  bool skip[CTC_MAXK];   // s -> s + 2 is a transition
#pragma unroll
  for (int k = 0; k < CTC_MAXK; k++) {
    const int s = tid + k * CTC_THREADS;
    cls[k] = -1;
    skip[k] = false;
    if (s < Lp) {
      cls[k] = ctc_state_class(tg, s, C, blank);
      skip[k] = s + 2 < Lp && cls[k] != ctc_state_class(tg, s + 2, C, blank);
    }
  }
  if (tid < 2) rows[0][Lp + tid] = rows[1][Lp + tid] = CTC_NEG_INF;

  float xe[CTC_MAXK], le = lse[Tn - 1];
#pragma unroll
  for (int k = 0; k < CTC_MAXK; k++) xe[k] = cls[k] >= 0 ? Elem<T>::ld(x + (long long)(Tn - 1) * C + cls[k]) : CTC_NEG_INF;
#pragma unroll
  for (int k = 0; k < CTC_MAXK; k++) {
    const int s = tid + k * CTC_THREADS;
    if (s < Lp) {
      const float b = s >= Lp - 2 ? xe[k] - le : CTC_NEG_INF;
      rows[(Tn - 1) & 1][s] = b;
      be[(long long)(Tn - 1) * W + s] = b;
    }
  }
  for (int t = Tn - 2; t >= 0; t--) {
    le = lse[t];
#pragma unroll
    for (int k = 0; k < CTC_MAXK; k++) xe[k] = cls[k] >= 0 ? Elem<T>::ld(x + (long long)t * C + cls[k]) : CTC_NEG_INF;
    __syncthreads();
    const float* nxt = rows[(t + 1) & 1];
    float* cur = rows[t & 1];
#pragma unroll
    for (int k = 0; k < CTC_MAXK; k++) {
      const int s = tid + k * CTC_THREADS;
      if (s < Lp) {
        const float v = ctc_lse3(nxt[s], nxt[s + 1], skip[k] ? nxt[s + 2] : CTC_NEG_INF);
        const float b = v == CTC_NEG_INF ? CTC_NEG_INF : v + (xe[k] - le);
        cur[s] = b;
        be[(long long)t * W + s] = b;
      }
    }
  }
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
static int ctc_check(const char* name, int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int dtype) {
  PERO_REQUIRE(dtype == PERO_F32 || dtype == PERO_BF16, "%s: bad dtype", name);
  PERO_REQUIRE(N > 0 && N < (1LL << 31) && S > 0 && C >= 2, "%s: bad sizes (N %lld, S %lld, C %lld)", name, (long long)N, (long long)S, (long long)C);
  PERO_REQUIRE(Lmax >= 0, "%s: Lmax %lld is negative", name, (long long)Lmax);
  PERO_REQUIRE(blank >= 0 && blank < C, "%s: blank %lld outside [0, C = %lld)", name, (long long)blank, (long long)C);
  if (S > CTC_MAX_S || Lmax > CTC_MAX_S || C > CTC_MAX_C) {   // Lmax may exceed S (a padded target matrix); a line with L > T is infeasible
    pero_set_error("%s: supported up to S = %d, Lmax = %d and C = %d (got S %lld, Lmax %lld, C %lld)", name, CTC_MAX_S, CTC_MAX_S, CTC_MAX_C, (long long)S,
                   (long long)Lmax, (long long)C);
    return PERO_E_UNSUPPORTED;
  }
  return PERO_OK;
}

#define CTC_LAUNCH_LSE(T, ...) \
  hipLaunchKernelGGL((ctc_row_lse_k<T>), dim3((unsigned)((rows + 3) / 4)), dim3(CTC_THREADS), 0, st, (const T*)logits, row_lse, (long long)rows, (int)C)
#define CTC_LAUNCH_ALPHA(T, ...)                                                                                                            \
  hipLaunchKernelGGL((ctc_alpha_k<T>), dim3((unsigned)N), dim3(CTC_THREADS), lds, st, (const T*)logits, targets, input_lengths, target_lengths, \
                     (const float*)row_lse, alpha, nll, (int)S, (int)C, (int)Lmax, (int)blank)

extern "C" int pero_ctc_fwd(const void* logits, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths, float* row_lse,
                            float* alpha, float* nll, int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int dtype, void* stream) {
  const int rc = ctc_check("pero_ctc_fwd", N, S, C, Lmax, blank, dtype);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE(logits && input_lengths && target_lengths && row_lse && alpha && nll && (targets || Lmax == 0), "pero_ctc_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = N * S;
  DISPATCH_T(dtype, CTC_LAUNCH_LSE, 0);
  PERO_CHECK_LAUNCH("pero_ctc_fwd (row lse)");
  const size_t lds = 2 * (2 * (size_t)Lmax + 3) * sizeof(float);
  DISPATCH_T(dtype, CTC_LAUNCH_ALPHA, 0);
  PERO_CHECK_LAUNCH("pero_ctc_fwd (alpha)");
  return PERO_OK;
}

#define CTC_LAUNCH_BETA(T, ...)                                                                                                            \
  hipLaunchKernelGGL((ctc_beta_k<T>), dim3((unsigned)N), dim3(CTC_THREADS), lds_b, st, (const T*)logits, targets, input_lengths, target_lengths, \
                     row_lse, beta, chain, (int)S, (int)C, (int)Lmax, (int)blank)
#define CTC_LAUNCH_GRAD(T, ...)                                                                                                             \
  hipLaunchKernelGGL((ctc_grad_k<T>), dim3((unsigned)(N * S)), dim3(CTC_THREADS), lds_g, st, (const T*)logits, targets, input_lengths,          \
                     target_lengths, row_lse, alpha, (const float*)beta, nll, g, (const int32_t*)chain, (T*)dlogits, (int)S, (int)C, (int)Lmax, \
                     (int)blank, zero_infinity)

extern "C" int pero_ctc_bwd(const void* logits, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths,
                            const float* row_lse, const float* alpha, const float* nll, const float* g, float* beta, int32_t* chain, void* dlogits,
                            int64_t N, int64_t S, int64_t C, int64_t Lmax, int64_t blank, int zero_infinity, int dtype, void* stream) {
  const int rc = ctc_check("pero_ctc_bwd", N, S, C, Lmax, blank, dtype);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE(logits && input_lengths && target_lengths && row_lse && alpha && nll && g && beta && dlogits && ((targets && chain) || Lmax == 0),
               "pero_ctc_bwd: null pointer");
  PERO_REQUIRE(N * S < (1LL << 31), "pero_ctc_bwd: N * S must be below 2^31");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds_b = (2 * (2 * (size_t)Lmax + 3) + (size_t)Lmax) * sizeof(float);
  DISPATCH_T(dtype, CTC_LAUNCH_BETA, 0);
  PERO_CHECK_LAUNCH("pero_ctc_bwd (beta)");
  const size_t lds_g = ((size_t)C + 2 * (size_t)Lmax + 1 + 4) * sizeof(float);
  DISPATCH_T(dtype, CTC_LAUNCH_GRAD, 0);
  PERO_CHECK_LAUNCH("pero_ctc_bwd (gradient)");
  return PERO_OK;
}

#define CTC_LAUNCH_GREEDY(T, ...)                                                                                                       \
  hipLaunchKernelGGL((ctc_greedy_k<T>), dim3((unsigned)N), dim3(CTC_THREADS), ((size_t)S + 1) * sizeof(int), st, (const T*)logits, input_lengths, out, \
                     out_lengths, (int)S, (int)C, (int)blank)

extern "C" int pero_ctc_greedy(const void* logits, const int64_t* input_lengths, int64_t* out, int64_t* out_lengths, int64_t N, int64_t S, int64_t C,
                               int64_t blank, int dtype, void* stream) {
  const int rc = ctc_check("pero_ctc_greedy", N, S, C, 0, blank, dtype);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE(logits && input_lengths && out && out_lengths, "pero_ctc_greedy: null pointer");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, CTC_LAUNCH_GREEDY, 0);
  PERO_CHECK_LAUNCH("pero_ctc_greedy");
  return PERO_OK;
}
