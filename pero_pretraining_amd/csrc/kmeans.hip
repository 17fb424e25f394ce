// Mini-batch k-means fit (Feature-Quantization centroids, scripts/fit_kmeans.py) in f32: the centre update of one
// mini-batch, the per-centre work of greedy k-means++ seeding and the early-stopping state.  The nearest-centre search
// is pero_vq_argmin (vq.hip); nothing here repeats it.
//
// Every sum below has a fixed order that depends on the shapes and the labels only - no float atomics - so the same
// inputs give the same bits from run to run.
#include "common.hpp"

// ---------------------------------------------------------------------------------------------------------------
// Centre update (sklearn _minibatch_update_dense):  for every centre k with n_k > 0 members in the batch
//   centers[k] = (centers[k] * weight_sums[k] + sum of member rows) / (weight_sums[k] + n_k);  weight_sums[k] += n_k.
// The caller sorts the labels (stable): `order` lists the batch rows centre by centre, each centre's rows in batch order.
//   km_bounds_k   start[k] = first sorted position whose label is >= k   (k = 0..K; every entry written exactly once)
//   km_update_k   one workgroup per centre.  Thread (g, c) owns column slot c (4 floats, 16-byte loads; 1 float on the
//                 generic path) of row group g: it adds the member rows g, g+G, g+2G, ... in that order; the G partial sums
//                 of a column are then added in the order g = 0..G-1.  A heavy centre is thereby split over the G row
//                 groups (waves, for D >= 256), and its tree is a function of n_k alone.  The quotient is formed in f64
//                 (weight_sums is f64: exact counts beyond 2^24) and rounded once to f32.
// Centres without members are not touched.  shift[k] = |c_new - c_old|^2 (0 for untouched centres), summed over k in a
// fixed order by sum_scale_k.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void km_bounds_k(const int64_t* sorted_labels, int* start, long long B, int K) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i > B) return;
  long long prev = i == 0 ? -1 : sorted_labels[i - 1];
  long long cur = i == B ? K : sorted_labels[i];
  prev = prev < -1 ? -1 : (prev > K - 1 ? K - 1 : prev);   // labels outside [0, K) cannot index outside start[0..K]
  cur = cur < 0 ? 0 : (cur > K ? K : cur);
  for (long long k = prev + 1; k <= cur; k++) start[k] = (int)i;
}

template <bool VEC> struct KmCol;
template <> struct KmCol<true> {
  typedef f4v T;
  static constexpr int W = 4;
  static __device__ __forceinline__ T zero() { return (f4v){0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ T ld(const float* p) { return *(const f4v*)p; }
  static __device__ __forceinline__ void st(float* p, T v) { *(f4v*)p = v; }
  static __device__ __forceinline__ float get(const T& v, int e) { return v[e]; }
  static __device__ __forceinline__ void set(T& v, int e, float f) { v[e] = f; }
};
template <> struct KmCol<false> {
  typedef float T;
  static constexpr int W = 1;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, T v) { *p = v; }
  static __device__ __forceinline__ float get(const T& v, int) { return v; }
  static __device__ __forceinline__ void set(T& v, int, float f) { v = f; }
};

template <bool VEC>
__global__ __launch_bounds__(256) void km_update_k(const float* x, const int64_t* order, const int* start, float* centers, double* weight_sums,
                                                   float* shift, long long B, int D, int CW) {
  typedef KmCol<VEC> C;
  typedef typename C::T T;
  __shared__ __attribute__((aligned(16))) float part[256 * C::W];
  __shared__ float red[4];
  const int tid = threadIdx.x, k = blockIdx.x;
  const int s0 = start[k], s1 = start[k + 1], n = s1 - s0;
  if (n <= 0) {
    if (tid == 0) shift[k] = 0.f;
    return;
  }
  const int c = tid & (CW - 1), g = tid / CW, G = 256 / CW;
  const int cols = D / C::W;
  const double w_old = weight_sums[k], w_new = w_old + (double)n;
  float sh = 0.f;
  for (int c0 = 0; c0 < cols; c0 += CW) {
    const int col = c0 + c;
    const bool act = col < cols;
    T acc = C::zero();
    if (act) {
      const float* xc = x + (long long)col * C::W;
      int j = s0 + g;
      for (; j + 3 * G < s1; j += 4 * G) {   // four independent loads in flight, added in row order
        const long long r0 = order[j], r1 = order[j + G], r2 = order[j + 2 * G], r3 = order[j + 3 * G];
        const bool ok = (unsigned long long)r0 < (unsigned long long)B && (unsigned long long)r1 < (unsigned long long)B &&
                        (unsigned long long)r2 < (unsigned long long)B && (unsigned long long)r3 < (unsigned long long)B;
        if (!ok) continue;   // `order` is a permutation of [0, B): anything else is skipped, never dereferenced
        const T v0 = C::ld(xc + r0 * D), v1 = C::ld(xc + r1 * D), v2 = C::ld(xc + r2 * D), v3 = C::ld(xc + r3 * D);
        acc += v0;
        acc += v1;
        acc += v2;
        acc += v3;
      }
      for (; j < s1; j += G) {
        const long long r0 = order[j];
        if ((unsigned long long)r0 < (unsigned long long)B) acc += C::ld(xc + r0 * D);
      }
    }
    C::st(part + tid * C::W, acc);
    __syncthreads();
    if (g == 0 && act) {
      T sum = C::ld(part + c * C::W);
      for (int gg = 1; gg < G; gg++) sum += C::ld(part + (gg * CW + c) * C::W);
      float* cp = centers + (long long)k * D + (long long)col * C::W;
      const T old = C::ld(cp);
      T neu;
#pragma unroll
      for (int e = 0; e < C::W; e++) {
        const float o = C::get(old, e);
        const float v = (float)(((double)o * w_old + (double)C::get(sum, e)) / w_new);
        C::set(neu, e, v);
        const float d = v - o;
        sh += d * d;
      }
      C::st(cp, neu);
    }
    __syncthreads();
  }
  sh = wave_sum(sh);
  if ((tid & 63) == 0) red[tid >> 6] = sh;
  __syncthreads();
  if (tid == 0) {
    shift[k] = ((red[0] + red[1]) + red[2]) + red[3];
    weight_sums[k] = w_new;
  }
}

__global__ __launch_bounds__(256) void km_sum_k(const float* partial, float* out, long long n) {
  __shared__ float sm[4];
  float s = 0.f;
  for (long long i = threadIdx.x; i < n; i += 256) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

extern "C" int pero_kmeans_update(const float* x, const int64_t* order, const int64_t* sorted_labels, float* centers, double* weight_sums,
                                  float* shift_out, void* work, int64_t B, int64_t K, int64_t D, void* stream) {
  PERO_REQUIRE(x && order && sorted_labels && centers && weight_sums && shift_out && work, "pero_kmeans_update: null pointer");
  PERO_REQUIRE(B > 0 && K > 0 && D > 0 && B < 2147483647LL && K < 2147483647LL && D < 2147483647LL, "pero_kmeans_update: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  int* start = (int*)work;                  // K + 1
  float* shift = (float*)work + (K + 1);    // K
  hipLaunchKernelGGL(km_bounds_k, dim3((unsigned)((B + 1 + 255) / 256)), dim3(256), 0, st, sorted_labels, start, (long long)B, (int)K);
  const bool vec = D % 4 == 0 && aligned16(x) && aligned16(centers);
  const long long cols = vec ? D / 4 : D;
  int CW = 1;
  while (CW < 256 && CW < cols) CW <<= 1;
  if (vec)
    hipLaunchKernelGGL(km_update_k<true>, dim3((unsigned)K), dim3(256), 0, st, x, order, start, centers, weight_sums, shift, (long long)B, (int)D, CW);
  else
    hipLaunchKernelGGL(km_update_k<false>, dim3((unsigned)K), dim3(256), 0, st, x, order, start, centers, weight_sums, shift, (long long)B, (int)D, CW);
  hipLaunchKernelGGL(km_sum_k, dim3(1), dim3(256), 0, st, shift, shift_out, (long long)K);
  PERO_CHECK_LAUNCH("pero_kmeans_update");
  return PERO_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Greedy k-means++ (sklearn _kmeans_plusplus), the work for ONE new centre: for each of the t candidate rows
//   newd[j][i] = min(closest[i], max(0, |x_i|^2 + |x_cand_j|^2 - 2 x_i . x_cand_j)),   pot[j] = sum_i newd[j][i]
// then the candidate with the lowest potential (first one on a tie) is committed: chosen[0] = its row index,
// pot_out[0] = its potential, closest <- newd[best].  Nothing returns to the host.
//   kpp_dist_k    64 rows per workgroup, 16 per wave in groups of 4; lanes run along D; a row's distance is a lane-partial
//                 fmaf chain + an xor butterfly; a wave adds its rows in row order, the 4 waves are added in wave order.
//   kpp_commit_k  one workgroup: block partials added in a fixed strided order (f64), argmin over t.
//   kpp_apply_k   closest <- newd[best].
// work (f32 units): [0, 4) selection, then t*n distances, then t*ceil(n/64) block partials.
// ---------------------------------------------------------------------------------------------------------------
#define KPP_TMAX 32
#define KPP_ROWS 64

template <bool VEC>
__global__ __launch_bounds__(256) void kpp_dist_k(const float* X, const float* sqn, const float* closest, const int64_t* cand, float* newd,
                                                  float* partial, long long n, int D, int t) {
  __shared__ float ps[4][KPP_TMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int W = VEC ? 4 : 1;
  if (tid < 4 * KPP_TMAX) ps[tid / KPP_TMAX][tid % KPP_TMAX] = 0.f;
  __syncthreads();
  const long long base = (long long)blockIdx.x * KPP_ROWS + wave * 16;
  for (int j = 0; j < t; j++) {
    long long ci = cand[j];
    ci = ci < 0 ? 0 : (ci >= n ? n - 1 : ci);
    const float* cr = X + ci * D;
    const float sc = sqn[ci];
    float wsum = 0.f;
    for (int q = 0; q < 4; q++) {
      const long long r0 = base + 4 * q;
      if (r0 >= n) break;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int c = lane * W; c < D; c += 64 * W) {
        if (VEC) {
          const f4v cv = *(const f4v*)(cr + c);
#pragma unroll
          for (int r = 0; r < 4; r++) {
            if (r0 + r < n) {
              const f4v xv = *(const f4v*)(X + (r0 + r) * D + c);
              acc[r] = fmaf(xv[0], cv[0], acc[r]);
              acc[r] = fmaf(xv[1], cv[1], acc[r]);
              acc[r] = fmaf(xv[2], cv[2], acc[r]);
              acc[r] = fmaf(xv[3], cv[3], acc[r]);
            }
          }
        } else {
          const float cv = cr[c];
#pragma unroll
          for (int r = 0; r < 4; r++)
            if (r0 + r < n) acc[r] = fmaf(X[(r0 + r) * D + c], cv, acc[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float dot = wave_sum(acc[r]);
        const long long row = r0 + r;
        if (row < n) {
          float d = fmaxf((sqn[row] + sc) - 2.0f * dot, 0.f);
          if (row == ci) d = 0.f;
          const float m = fminf(d, closest[row]);
          if (lane == 0) newd[(long long)j * n + row] = m;
          wsum += m;
        }
      }
    }
    if (lane == 0) ps[wave][j] = wsum;
  }
  __syncthreads();
  if (tid < t) partial[(long long)tid * gridDim.x + blockIdx.x] = ((ps[0][tid] + ps[1][tid]) + ps[2][tid]) + ps[3][tid];
}

__global__ __launch_bounds__(256) void kpp_commit_k(const float* partial, const int64_t* cand, int* sel, int64_t* chosen, double* pot_out,
                                                    long long nblk, long long n, int t) {
  __shared__ double red[4];
  __shared__ double pot[KPP_TMAX];
  const int tid = threadIdx.x;
  for (int j = 0; j < t; j++) {
    double s = 0.0;
    for (long long b = tid; b < nblk; b += 256) s += (double)partial[(long long)j * nblk + b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) pot[j] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
  }
  if (tid == 0) {
    int best = 0;
    for (int j = 1; j < t; j++)
      if (pot[j] < pot[best]) best = j;
    long long ci = cand[best];
    ci = ci < 0 ? 0 : (ci >= n ? n - 1 : ci);
    sel[0] = best;
    chosen[0] = ci;
    pot_out[0] = pot[best];
  }
}

__global__ __launch_bounds__(256) void kpp_apply_k(const float* newd, const int* sel, float* closest, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) closest[i] = newd[(long long)sel[0] * n + i];
}

extern "C" int pero_kmeans_pp_step(const float* x, const float* sqnorm, float* closest_dist_sq, const int64_t* candidates, int64_t* chosen,
                                   double* potential, float* work, int64_t n, int64_t D, int64_t t, void* stream) {
  PERO_REQUIRE(x && sqnorm && closest_dist_sq && candidates && chosen && potential && work, "pero_kmeans_pp_step: null pointer");
  PERO_REQUIRE(n > 0 && D > 0 && D < 2147483647LL && t > 0 && t <= KPP_TMAX, "pero_kmeans_pp_step: bad sizes (1 <= t <= 32)");
  hipStream_t st = (hipStream_t)stream;
  const long long nblk = (n + KPP_ROWS - 1) / KPP_ROWS;
  PERO_REQUIRE(nblk < 2147483647LL, "pero_kmeans_pp_step: too many rows");
  int* sel = (int*)work;
  float* newd = work + 4;
  float* partial = newd + t * n;
  if (D % 4 == 0 && aligned16(x))
    hipLaunchKernelGGL(kpp_dist_k<true>, dim3((unsigned)nblk), dim3(256), 0, st, x, sqnorm, closest_dist_sq, candidates, newd, partial, (long long)n,
                       (int)D, (int)t);
  else
    hipLaunchKernelGGL(kpp_dist_k<false>, dim3((unsigned)nblk), dim3(256), 0, st, x, sqnorm, closest_dist_sq, candidates, newd, partial, (long long)n,
                       (int)D, (int)t);
  hipLaunchKernelGGL(kpp_commit_k, dim3(1), dim3(256), 0, st, partial, candidates, sel, chosen, potential, nblk, (long long)n, (int)t);
  hipLaunchKernelGGL(kpp_apply_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, newd, sel, closest_dist_sq, (long long)n);
  PERO_CHECK_LAUNCH("pero_kmeans_pp_step");
  return PERO_OK;
}

// out[r] = |x_r|^2 with the lane-strided order of the argmin's row norms (vq.hip sqnorm_k)
__global__ __launch_bounds__(256) void km_sqnorm_k(const float* x, float* out, long long rows, int d) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float s = 0.f;
  for (int c = threadIdx.x & 63; c < d; c += 64) { const float v = x[row * d + c]; s += v * v; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) out[row] = s;
}
extern "C" int pero_kmeans_sqnorm(const float* x, float* out, int64_t rows, int64_t D, void* stream) {
  PERO_REQUIRE(x && out && rows > 0 && D > 0 && D < 2147483647LL && (rows + 3) / 4 < 2147483647LL, "pero_kmeans_sqnorm: bad arguments");
  hipLaunchKernelGGL(km_sqnorm_k, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, out, (long long)rows, (int)D);
  PERO_CHECK_LAUNCH("pero_kmeans_sqnorm");
  return PERO_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Early stopping on the device (sklearn MiniBatchKMeans._mini_batch_convergence), one thread.
// state (f64[6]): 0 EWA of the batch inertia, 1 its running minimum, 2 steps without improvement, 3 stop flag,
//                 4 steps seen, 5 the step (1-based) at which the flag was raised.  Zero it before the first step.
// ---------------------------------------------------------------------------------------------------------------
__global__ void km_converge_k(const float* batch_inertia, const float* shift, double* state, double n_samples, double batch_size, double tol,
                              long long max_no_improvement) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double step = state[4] + 1.0;
  state[4] = step;
  if (step == 1.0) return;   // the first batch is scored against the seeding, not against a fitted centre set
  const double bi = (double)batch_inertia[0] / batch_size;
  double ewa;
  if (step == 2.0) {
    ewa = bi;
  } else {
    double alpha = batch_size * 2.0 / (n_samples + 1.0);
    alpha = alpha < 1.0 ? alpha : 1.0;
    ewa = state[0] * (1.0 - alpha) + bi * alpha;
  }
  state[0] = ewa;
  bool stop = false;
  if (tol > 0.0 && (double)shift[0] <= tol) stop = true;
  if (!stop) {
    if (step == 2.0 || ewa < state[1]) {
      state[2] = 0.0;
      state[1] = ewa;
    } else {
      state[2] += 1.0;
    }
    if (max_no_improvement >= 0 && state[2] >= (double)max_no_improvement) stop = true;
  }
  if (stop && state[3] == 0.0) {
    state[3] = 1.0;
    state[5] = step;
  }
}

extern "C" int pero_kmeans_converge(const float* batch_inertia, const float* shift, double* state, int64_t n_samples, int64_t batch_size,
                                    double tol, int64_t max_no_improvement, void* stream) {
  PERO_REQUIRE(batch_inertia && shift && state && n_samples > 0 && batch_size > 0, "pero_kmeans_converge: bad arguments");
  hipLaunchKernelGGL(km_converge_k, dim3(1), dim3(64), 0, (hipStream_t)stream, batch_inertia, shift, state, (double)n_samples, (double)batch_size, tol,
                     (long long)max_no_improvement);
  PERO_CHECK_LAUNCH("pero_kmeans_converge");
  return PERO_OK;
}
