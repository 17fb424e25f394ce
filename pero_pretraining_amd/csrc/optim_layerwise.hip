// LAMB and LARS over the flat buffers of optim.FusedAdam: layer-wise trust ratios ||p|| / ||u|| per parameter tensor, in three launches per
// group and step without float atomics, without waiting between workgroups and without a buffer for the update u (stage 2 computes it again
// from the same operands with the same operations: -ffp-contract=off, the same bits).  All HBM-bound.  Formulas, operation order and the
// tile / partial layout: include/pero_hip.h ("layer-wise optimizers").
#include "flat_tiles.hpp"

// ---------------------------------------------------------------------------------------------
// Workgroup -> tile.  table[t] = {offset, numel, first tile}.  Piece k of lane t holds the elements (k * 256 + t) * 4 .. + 3 of the tile.
// ---------------------------------------------------------------------------------------------
struct LayerTile {
  long long start;   // first element in the flat buffer
  int count;         // 1 .. LT elements (0: nothing)
  int tensor;
};
__device__ __forceinline__ LayerTile layer_tile(const long long* table, int n, long long bid) {
  const TileSeg s = tile_segment<3>(table, n, bid);
  LayerTile r;
  r.tensor = s.seg;
  r.start = table[s.seg * 3] + s.local * LT;
  r.count = tile_count(table[s.seg * 3 + 1], s.local);
  return r;
}

// ---------------------------------------------------------------------------------------------
// One element, in the header's order.  `g` arrives as grad * grad_scale.
// ---------------------------------------------------------------------------------------------
template <bool MAXI, bool CLIP>
__device__ __forceinline__ float layer_grad(float g, float coef) {
  if (CLIP) g = g * coef;
  if (MAXI) g = -g;
  return g;
}
__device__ __forceinline__ float clip_coef(const float* gnorm, float max_norm) {   // as adam_ex_k: a NaN norm gives a NaN coefficient
  const float c = max_norm / (*gnorm + 1e-6f);
  return c > 1.0f ? 1.0f : c;
}
__device__ __forceinline__ float lamb_update(float p, float m, float v, float rbc1, float rsb2, float eps, float wd) {
  const float denom = sqrtf(v) * rsb2 + eps;
  return (m * rbc1) / denom + wd * p;
}
__device__ __forceinline__ float lars_update(float p, float g, float wd) { return g + wd * p; }

template <bool MAXI, bool CLIP>
__global__ __launch_bounds__(256) void lamb_stage1_k(const float* p, const float* g, float* m, float* v, const long long* table, int n,
                                                     float* partials, float b1, float b2, float omb1, float omb2, float eps, float rbc1,
                                                     float rsb2, float gscale, float wd, const float* gnorm, float max_norm) {
  const float coef = CLIP ? clip_coef(gnorm, max_norm) : 1.0f;
  const LayerTile T = layer_tile(table, n, blockIdx.x);
  f4v pp[4], gg[4], mm[4], vv[4];   // sixteen loads in flight per lane
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
    pp[k] = load4_tail(p + T.start, e, T.count); gg[k] = load4_tail(g + T.start, e, T.count);
    mm[k] = load4_tail(m + T.start, e, T.count); vv[k] = load4_tail(v + T.start, e, T.count);
  }
  f4v ap = {0.f, 0.f, 0.f, 0.f}, au = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float pe = pp[k][j];
      const float ge = layer_grad<MAXI, CLIP>(gg[k][j] * gscale, coef);
      const float me = mm[k][j] * b1 + omb1 * ge;
      const float ve = vv[k][j] * b2 + omb2 * ge * ge;
      const float u = lamb_update(pe, me, ve, rbc1, rsb2, eps, wd);
      const bool live = e + j < T.count;   // an element behind the tile's end adds an exact zero
      ap[j] = ap[j] + (live ? pe * pe : 0.f);
      au[j] = au[j] + (live ? u * u : 0.f);
      mm[k][j] = me; vv[k][j] = ve;
    }
    store4_tail(m + T.start, e, T.count, mm[k]);
    store4_tail(v + T.start, e, T.count, vv[k]);
  }
  block_fold<2>({ap, au}, partials + 2 * (long long)blockIdx.x);
}

__global__ __launch_bounds__(256) void lamb_stage2_k(float* p, const float* m, const float* v, bf16raw* pb, const long long* table, int n,
                                                     const float* stats, float lr, float eps, float rbc1, float rsb2, float wd) {
  const LayerTile T = layer_tile(table, n, blockIdx.x);
  const float step = lr * stats[T.tensor * 3 + 2];   // one float per workgroup (a uniform load)
  f4v pp[4], mm[4], vv[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
    pp[k] = load4_tail(p + T.start, e, T.count); mm[k] = load4_tail(m + T.start, e, T.count); vv[k] = load4_tail(v + T.start, e, T.count);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) pp[k][j] = pp[k][j] - step * lamb_update(pp[k][j], mm[k][j], vv[k][j], rbc1, rsb2, eps, wd);
    store4_tail(p + T.start, e, T.count, pp[k]);
    if (pb) store4_tail(pb + T.start, e, T.count, pp[k]);
  }
}

template <bool MAXI, bool CLIP>
__global__ __launch_bounds__(256) void lars_stage1_k(const float* p, const float* g, const long long* table, int n, float* partials,
                                                     float gscale, float wd, const float* gnorm, float max_norm) {
  const float coef = CLIP ? clip_coef(gnorm, max_norm) : 1.0f;
  const LayerTile T = layer_tile(table, n, blockIdx.x);
  f4v pp[4], gg[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
    pp[k] = load4_tail(p + T.start, e, T.count); gg[k] = load4_tail(g + T.start, e, T.count);
  }
  f4v ap = {0.f, 0.f, 0.f, 0.f}, au = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float pe = pp[k][j];
      const float u = lars_update(pe, layer_grad<MAXI, CLIP>(gg[k][j] * gscale, coef), wd);
      const bool live = e + j < T.count;
      ap[j] = ap[j] + (live ? pe * pe : 0.f);
      au[j] = au[j] + (live ? u * u : 0.f);
    }
  }
  block_fold<2>({ap, au}, partials + 2 * (long long)blockIdx.x);
}

template <bool MAXI, bool CLIP>
__global__ __launch_bounds__(256) void lars_stage2_k(float* p, const float* g, float* buf, bf16raw* pb, const long long* table, int n,
                                                     const float* stats, float lr, float mu, float gscale, float wd, const float* gnorm,
                                                     float max_norm) {
  const float coef = CLIP ? clip_coef(gnorm, max_norm) : 1.0f;
  const LayerTile T = layer_tile(table, n, blockIdx.x);
  const float r = stats[T.tensor * 3 + 2];
  f4v pp[4], gg[4], bb[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
    pp[k] = load4_tail(p + T.start, e, T.count); gg[k] = load4_tail(g + T.start, e, T.count); bb[k] = load4_tail(buf + T.start, e, T.count);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float u = lars_update(pp[k][j], layer_grad<MAXI, CLIP>(gg[k][j] * gscale, coef), wd);
      bb[k][j] = mu * bb[k][j] + r * u;
      pp[k][j] = pp[k][j] - lr * bb[k][j];
    }
    store4_tail(buf + T.start, e, T.count, bb[k]);
    store4_tail(p + T.start, e, T.count, pp[k]);
    if (pb) store4_tail(pb + T.start, e, T.count, pp[k]);
  }
}

// One workgroup per tensor: the two sums of its tiles' partials in f64 (run_sum_f64).
__global__ __launch_bounds__(256) void layer_ratio_finish_k(const float* partials, const long long* table, float c, int adapt, float* stats) {
  const long long t = blockIdx.x;
  const long long first = table[t * 3 + 2], count = (table[t * 3 + 1] + LT - 1) / LT;
  double s[2];   // sum p^2, sum u^2
  run_sum_f64<2, 2>(partials + 2 * first, count, s);
  if (threadIdx.x == 0) {
    const float pn = (float)sqrt(s[0]), un = (float)sqrt(s[1]);
    float r = 1.0f;
    if (adapt && pn > 0.f && un > 0.f) r = (c * pn) / un;   // a NaN norm fails both comparisons: r = 1, the NaN reaches p through u
    stats[t * 3] = pn; stats[t * 3 + 1] = un; stats[t * 3 + 2] = r;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
#define LAYER_REQUIRE_TABLE(name)                                                                                                       \
  PERO_REQUIRE(table && n_tensors > 0 && n_tensors < (1LL << 31) && total_tiles >= n_tensors && total_tiles < (1LL << 31),            \
               name ": table / tensor count / tile count (every tensor has a tile; fewer than 2^31 tiles)")
#define LAYER_REQUIRE_GRAD(name)                                                                                                        \
  PERO_REQUIRE(maximize == 0 || maximize == 1, name ": maximize must be 0 or 1");                                                       \
  PERO_REQUIRE(!grad_norm || max_norm >= 0.0, name ": max_norm must not be negative")
#define LAYER_PICK(kernel, maxi, clip) \
  ((maxi) ? ((clip) ? kernel<true, true> : kernel<true, false>) : ((clip) ? kernel<false, true> : kernel<false, false>))

extern "C" int pero_lamb_stage1(const float* p, const float* g, float* m, float* v, const int64_t* table, int64_t n_tensors,
                                int64_t total_tiles, float* partials, double beta1, double beta2, int64_t step, double eps,
                                double grad_scale, double weight_decay, int maximize, const float* grad_norm, double max_norm, void* stream) {
  PERO_REQUIRE(p && g && m && v && partials && step >= 1, "pero_lamb_stage1: null pointer or step < 1");
  LAYER_REQUIRE_TABLE("pero_lamb_stage1");
  PERO_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), "pero_lamb_stage1: 16-byte alignment");
  LAYER_REQUIRE_GRAD("pero_lamb_stage1");
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  auto k = LAYER_PICK(lamb_stage1_k, maximize != 0, grad_norm != nullptr);
  hipLaunchKernelGGL(k, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (const long long*)table, (int)n_tensors,
                     partials, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)(1.0 / bc1),
                     (float)(1.0 / sqrt(bc2)), (float)grad_scale, (float)weight_decay, grad_norm, (float)max_norm);
  PERO_CHECK_LAUNCH("pero_lamb_stage1");
  return PERO_OK;
}

extern "C" int pero_lamb_stage2(float* p, const float* m, const float* v, void* p_bf16, const int64_t* table, int64_t n_tensors,
                                int64_t total_tiles, const float* stats, double lr, double beta1, double beta2, int64_t step, double eps,
                                double weight_decay, void* stream) {
  PERO_REQUIRE(p && m && v && stats && step >= 1, "pero_lamb_stage2: null pointer or step < 1");
  LAYER_REQUIRE_TABLE("pero_lamb_stage2");
  PERO_REQUIRE(aligned16(p) && aligned16(m) && aligned16(v) && (!p_bf16 || (((uintptr_t)p_bf16) & 7) == 0), "pero_lamb_stage2: alignment");
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  hipLaunchKernelGGL(lamb_stage2_k, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, p, m, v, (bf16raw*)p_bf16,
                     (const long long*)table, (int)n_tensors, stats, (float)lr, (float)eps, (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)),
                     (float)weight_decay);
  PERO_CHECK_LAUNCH("pero_lamb_stage2");
  return PERO_OK;
}

extern "C" int pero_lars_stage1(const float* p, const float* g, const int64_t* table, int64_t n_tensors, int64_t total_tiles,
                                float* partials, double grad_scale, double weight_decay, int maximize, const float* grad_norm,
                                double max_norm, void* stream) {
  PERO_REQUIRE(p && g && partials, "pero_lars_stage1: null pointer");
  LAYER_REQUIRE_TABLE("pero_lars_stage1");
  PERO_REQUIRE(aligned16(p) && aligned16(g), "pero_lars_stage1: 16-byte alignment");
  LAYER_REQUIRE_GRAD("pero_lars_stage1");
  auto k = LAYER_PICK(lars_stage1_k, maximize != 0, grad_norm != nullptr);
  hipLaunchKernelGGL(k, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, p, g, (const long long*)table, (int)n_tensors,
                     partials, (float)grad_scale, (float)weight_decay, grad_norm, (float)max_norm);
  PERO_CHECK_LAUNCH("pero_lars_stage1");
  return PERO_OK;
}

extern "C" int pero_lars_stage2(float* p, const float* g, float* buf, void* p_bf16, const int64_t* table, int64_t n_tensors,
                                int64_t total_tiles, const float* stats, double lr, double momentum, double grad_scale,
                                double weight_decay, int maximize, const float* grad_norm, double max_norm, void* stream) {
  PERO_REQUIRE(p && g && buf && stats, "pero_lars_stage2: null pointer");
  LAYER_REQUIRE_TABLE("pero_lars_stage2");
  PERO_REQUIRE(aligned16(p) && aligned16(g) && aligned16(buf) && (!p_bf16 || (((uintptr_t)p_bf16) & 7) == 0), "pero_lars_stage2: alignment");
  LAYER_REQUIRE_GRAD("pero_lars_stage2");
  auto k = LAYER_PICK(lars_stage2_k, maximize != 0, grad_norm != nullptr);
  hipLaunchKernelGGL(k, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, p, g, buf, (bf16raw*)p_bf16, (const long long*)table,
                     (int)n_tensors, stats, (float)lr, (float)momentum, (float)grad_scale, (float)weight_decay, grad_norm, (float)max_norm);
  PERO_CHECK_LAUNCH("pero_lars_stage2");
  return PERO_OK;
}

extern "C" int pero_layer_ratio_finish(const float* partials, const int64_t* table, int64_t n_tensors, double coefficient, int adapt,
                                       float* stats, void* stream) {
  PERO_REQUIRE(partials && table && stats && n_tensors > 0 && n_tensors < (1LL << 31), "pero_layer_ratio_finish: null pointer or tensor count");
  PERO_REQUIRE(adapt == 0 || adapt == 1, "pero_layer_ratio_finish: adapt must be 0 or 1");
  hipLaunchKernelGGL(layer_ratio_finish_k, dim3((unsigned)n_tensors), dim3(256), 0, (hipStream_t)stream, partials, (const long long*)table,
                     (float)coefficient, adapt, stats);
  PERO_CHECK_LAUNCH("pero_layer_ratio_finish");
  return PERO_OK;
}
