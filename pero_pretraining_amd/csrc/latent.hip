// Latent-target self-distillation: the EMA of a whole model in one launch, the normalised layer-averaged targets at the listed rows, and
// the regression loss (smooth L1 / MSE) with its gradient.  All HBM-bound, no float atomics, every sum in a fixed order.  Formulas,
// operation order and layouts: include/pero_hip.h ("latent-target self-distillation").
#include "flat_tiles.hpp"
#include "dispatch.hpp"

// ---------------------------------------------------------------------------------------------
// EMA.  table[s] = {source address, destination offset, count, first tile}.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ema_update_k(float* avg, bf16raw* avg_bf16, const long long* table, int n, float w) {
  const TileSeg s = tile_segment<4>(table, n, blockIdx.x);
  const int count = tile_count(table[s.seg * 4 + 2], s.local);
  const float* src = (const float*)(uintptr_t)table[s.seg * 4] + s.local * LT;
  float* a = avg + table[s.seg * 4 + 1] + s.local * LT;
  bf16raw* ab = avg_bf16 ? avg_bf16 + table[s.seg * 4 + 1] + s.local * LT : nullptr;
  const bool vec = (((uintptr_t)src) & 15) == 0;   // uniform over the workgroup: a source that is not 16-byte aligned takes scalar loads
  f4v pp[4], aa[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
    aa[k] = load4_tail(a, e, count);
    pp[k] = load4_tail(src, e, count, vec);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) aa[k][j] = aa[k][j] + w * (pp[k][j] - aa[k][j]);
    store4_tail(a, e, count, aa[k]);
    if (ab) store4_tail(ab, e, count, aa[k]);
  }
}

// ---------------------------------------------------------------------------------------------
// Targets.  One wave per output row, the row of one matrix in registers: NCH chunks of 256 columns, lane l holding columns
// (c * 64 + l) * 4 .. + 3 of chunk c.  d <= 256 * NCH.
// ---------------------------------------------------------------------------------------------
struct LatentMats { const void* p[PERO_LATENT_MAX_K]; };

template <typename T, int NCH>
__global__ __launch_bounds__(256) void latent_targets_k(LatentMats mats, int K, const long long* index, float* y, long long rows,
                                                        long long n, long long n_pad, int d, float eps, float inv_k) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_pad) return;
  float* out = y + i * d;
  const long long r = i < n ? index[i] : 0;
  if (i >= n || r < 0 || r >= rows) {   // padding: exact zeros; an index outside the matrices: NaN, nothing read
    const float fill = i >= n ? 0.f : __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      const int col = (c * 64 + lane) * 4;
      if (col < d) *(f4v*)(out + col) = (f4v){fill, fill, fill, fill};
    }
    return;
  }
  f4v acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; c++) acc[c] = (f4v){0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < K; k++) {
    const T* x = (const T*)mats.p[k] + r * d;
    f4v v[NCH];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      const int col = (c * 64 + lane) * 4;
      v[c] = (f4v){0.f, 0.f, 0.f, 0.f};
      if (col < d) v[c] = load4<T>(x + col);
    }
#pragma unroll
    for (int c = 0; c < NCH; c++)
      if ((c * 64 + lane) * 4 < d) {
#pragma unroll
        for (int j = 0; j < 4; j++) s += v[c][j];
      }
    const float mu = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; c++)
      if ((c * 64 + lane) * 4 < d) {
#pragma unroll
        for (int j = 0; j < 4; j++) { const float t = v[c][j] - mu; q += t * t; }
      }
    const float rs = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[c][j] = acc[c][j] + (v[c][j] - mu) * rs;
  }
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    const int col = (c * 64 + lane) * 4;
    if (col < d) *(f4v*)(out + col) = (f4v){acc[c][0] * inv_k, acc[c][1] * inv_k, acc[c][2] * inv_k, acc[c][3] * inv_k};
  }
}

// ---------------------------------------------------------------------------------------------
// Loss.  MSE: beta == 0.
// ---------------------------------------------------------------------------------------------
template <bool MSE> __device__ __forceinline__ float latent_l(float e, float beta) {
  if (MSE) return e * e;
  const float ae = fabsf(e);
  return ae < beta ? ((0.5f * e) * e) / beta : ae - 0.5f * beta;
}
template <bool MSE> __device__ __forceinline__ float latent_dl(float e, float beta) {
  if (MSE) return 2.0f * e;
  return fabsf(e) < beta ? e / beta : (e > 0.f ? 1.0f : (e < 0.f ? -1.0f : e));   // (|e| >= beta > 0 leaves no zero here; a NaN stays a NaN)
}

template <typename T, bool MSE>
__global__ __launch_bounds__(256) void latent_loss_rows_k(const T* pred, const float* y, float* rowsum, long long n, int d, float beta) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const T* p = pred + i * d;
  const float* t = y + i * d;
  float s = 0.f;
  for (int col = lane * 4; col < d; col += 256) {
    const f4v a = load4<T>(p + col), b = load4<float>(t + col);
#pragma unroll
    for (int j = 0; j < 4; j++) s += latent_l<MSE>(a[j] - b[j], beta);
  }
  s = wave_sum(s);
  if (lane == 0) rowsum[i] = s;
}

// one workgroup: the row sums in f64 (run_sum_f64)
__global__ __launch_bounds__(256) void latent_loss_finish_k(const float* rowsum, float* loss, long long n, int d) {
  double s[1];
  run_sum_f64<1, 1>(rowsum, n, s);
  if (threadIdx.x == 0) loss[0] = (float)(s[0] / ((double)n * (double)d));
}

template <typename T, bool MSE>
__global__ __launch_bounds__(256) void latent_loss_bwd_k(const T* pred, const float* y, const float* dloss, T* dpred, long long n_live,
                                                         long long n_all, float coef, float beta) {
  // n_live, n_all: pieces of four elements inside the first n rows / inside all n_pad rows
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= n_all) return;
  f4v o = {0.f, 0.f, 0.f, 0.f};
  if (q < n_live) {
    const float g = (dloss ? dloss[0] : 1.0f) * coef;
    const f4v a = load4<T>(pred + q * 4), b = load4<float>(y + q * 4);
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = g * latent_dl<MSE>(a[j] - b[j], beta);
  }
  store4<T>(dpred + q * 4, o);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
extern "C" int pero_ema_update(float* avg, void* avg_bf16, const int64_t* table, int64_t n_segments, int64_t total_tiles, float w,
                               void* stream) {
  PERO_REQUIRE(avg && table, "pero_ema_update: null pointer");
  PERO_REQUIRE(n_segments > 0 && n_segments < (1LL << 31) && total_tiles >= n_segments && total_tiles < (1LL << 31),
               "pero_ema_update: segment count / tile count (every segment has a tile; fewer than 2^31 tiles)");
  PERO_REQUIRE(aligned16(avg) && (!avg_bf16 || (((uintptr_t)avg_bf16) & 7) == 0), "pero_ema_update: alignment");
  hipLaunchKernelGGL(ema_update_k, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, avg, (bf16raw*)avg_bf16,
                     (const long long*)table, (int)n_segments, w);
  PERO_CHECK_LAUNCH("pero_ema_update");
  return PERO_OK;
}

template <typename T>
static void launch_targets(int nch, dim3 grid, hipStream_t st, const LatentMats& m, int K, const int64_t* index, float* y, int64_t rows,
                           int64_t n, int64_t n_pad, int d, float eps, float inv_k) {
  auto launch = [&](auto N) {
    hipLaunchKernelGGL((latent_targets_k<T, decltype(N)::value>), grid, dim3(256), 0, st, m, K, (const long long*)index, y, (long long)rows, (long long)n,
                       (long long)n_pad, d, eps, inv_k);
  };
  if (nch <= 1) launch(std::integral_constant<int, 1>());
  else if (nch <= 2) launch(std::integral_constant<int, 2>());
  else if (nch <= 4) launch(std::integral_constant<int, 4>());
  else if (nch <= 8) launch(std::integral_constant<int, 8>());
  else launch(std::integral_constant<int, 16>());
}

extern "C" int pero_latent_targets(const void** mats, int64_t K, const int64_t* index, float* y, int64_t rows, int64_t n, int64_t n_pad,
                                   int64_t d, float eps, int dtype, void* stream) {
  PERO_REQUIRE(mats && y && (index || n == 0), "pero_latent_targets: null pointer");
  PERO_REQUIRE(K >= 1 && K <= PERO_LATENT_MAX_K, "pero_latent_targets: 1 <= K <= %d matrices, got %lld", PERO_LATENT_MAX_K, (long long)K);
  PERO_REQUIRE(dtype == PERO_F32 || dtype == PERO_BF16, "pero_latent_targets: dtype");
  PERO_REQUIRE(d >= 4 && d % 4 == 0 && d <= PERO_LATENT_MAX_D, "pero_latent_targets: d must be a multiple of 4 in [4, %d], got %lld",
               PERO_LATENT_MAX_D, (long long)d);
  PERO_REQUIRE(rows >= 1 && n >= 0 && n_pad >= n && n_pad < (1LL << 32), "pero_latent_targets: rows / n / n_pad");
  PERO_REQUIRE(aligned16(y), "pero_latent_targets: y must be 16-byte aligned");
  LatentMats m;
  for (int k = 0; k < PERO_LATENT_MAX_K; k++) m.p[k] = k < K ? mats[k] : nullptr;
  for (int k = 0; k < K; k++) PERO_REQUIRE(m.p[k] && aligned16(m.p[k]), "pero_latent_targets: matrix %d is null or not 16-byte aligned", k);
  if (n_pad == 0) return PERO_OK;
  const dim3 grid((unsigned)((n_pad + 3) / 4));
  const int nch = (int)((d + 255) / 256);
  const float inv_k = (float)(1.0 / (double)K);
  with_elem(dtype, [&](auto t) { launch_targets<decltype(t)>(nch, grid, (hipStream_t)stream, m, (int)K, index, y, rows, n, n_pad, (int)d, eps, inv_k); });
  PERO_CHECK_LAUNCH("pero_latent_targets");
  return PERO_OK;
}

#define LATENT_REQUIRE_LOSS(name)                                                                                              \
  PERO_REQUIRE(dtype == PERO_F32 || dtype == PERO_BF16, name ": dtype");                                                       \
  PERO_REQUIRE(d >= 4 && d % 4 == 0 && d < (1LL << 31), name ": d must be a multiple of 4, got %lld", (long long)d);            \
  PERO_REQUIRE(beta >= 0.f, name ": beta must not be negative (0 = MSE)")

extern "C" int pero_latent_loss_fwd(const void* pred, const float* y, float* work, float* loss, int64_t n, int64_t d, float beta, int dtype,
                                    void* stream) {
  PERO_REQUIRE(loss && n >= 0 && n < (1LL << 32) && (n == 0 || (pred && y && work)), "pero_latent_loss_fwd: null pointer or row count");
  LATENT_REQUIRE_LOSS("pero_latent_loss_fwd");
  PERO_REQUIRE(aligned16(pred) && aligned16(y), "pero_latent_loss_fwd: 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    const dim3 grid((unsigned)((n + 3) / 4));
    const bool mse = beta == 0.f;
    with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(mse, [&](auto M) {
      hipLaunchKernelGGL((latent_loss_rows_k<T, decltype(M)::value>), grid, dim3(256), 0, st, (const T*)pred, y, work, (long long)n, (int)d, beta); }); });
    PERO_CHECK_LAUNCH("pero_latent_loss_fwd");
  }
  hipLaunchKernelGGL(latent_loss_finish_k, dim3(1), dim3(256), 0, st, work, loss, (long long)n, (int)d);
  PERO_CHECK_LAUNCH("pero_latent_loss_fwd");
  return PERO_OK;
}

extern "C" int pero_latent_loss_bwd(const void* pred, const float* y, const float* dloss, void* dpred, int64_t n, int64_t n_pad, int64_t d,
                                    float beta, int dtype, void* stream) {
  PERO_REQUIRE(n >= 0 && n_pad >= n && (n_pad == 0 || dpred) && (n == 0 || (pred && y)), "pero_latent_loss_bwd: null pointer or row counts");
  LATENT_REQUIRE_LOSS("pero_latent_loss_bwd");
  PERO_REQUIRE(aligned16(pred) && aligned16(y) && aligned16(dpred), "pero_latent_loss_bwd: 16-byte alignment");
  const long long n_live = n * (d / 4), n_all = n_pad * (d / 4);
  PERO_REQUIRE((n_all + 255) / 256 < (1LL << 31), "pero_latent_loss_bwd: too many elements for one launch");
  if (n_all == 0) return PERO_OK;
  const float coef = n > 0 ? (float)(1.0 / ((double)n * (double)d)) : 0.f;
  const dim3 grid((unsigned)((n_all + 255) / 256));
  const bool mse = beta == 0.f;
  with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(mse, [&](auto M) {
    hipLaunchKernelGGL((latent_loss_bwd_k<T, decltype(M)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)pred, y, dloss, (T*)dpred, n_live,
                       n_all, coef, beta); }); });
  PERO_CHECK_LAUNCH("pero_latent_loss_bwd");
  return PERO_OK;
}
