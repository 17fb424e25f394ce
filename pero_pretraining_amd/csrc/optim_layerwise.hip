// LAMB and LARS over the flat buffers of optim.FusedAdam: layer-wise trust ratios ||p|| / ||u|| per parameter tensor, in three launches per
// group and step without float atomics, without waiting between workgroups and without a buffer for the update u (stage 2 computes it again
// from the same operands with the same operations: -ffp-contract=off, the same bits).  All HBM-bound.  Formulas, operation order and the
// tile / partial layout: include/pero_hip.h ("layer-wise optimizers").
#include "common.hpp"

#define LT PERO_LAYER_TILE   // elements of a tile = 256 lanes x 4 pieces of 16 bytes

// ---------------------------------------------------------------------------------------------
// Workgroup -> tile.  table[t] = {offset, numel, first tile}; the tensor of tile `bid` is the last one whose first tile is <= bid (binary
// search: a model has a few hundred tensors).  A tile that lies behind its tensor's end (a table and a tile count that do not belong
// together) has count 0 and touches no element.
// ---------------------------------------------------------------------------------------------
struct LayerTile {
  long long start;   // first element in the flat buffer
  int count;         // 1 .. LT elements (0: nothing)
  int tensor;
};
__device__ __forceinline__ LayerTile layer_tile(const long long* table, int n, long long bid) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid * 3 + 2] <= bid) lo = mid; else hi = mid - 1;
  }
  const long long local = bid - table[lo * 3 + 2];
  const long long left = local >= 0 ? table[lo * 3 + 1] - local * LT : 0;
  LayerTile r;
  r.tensor = lo;
  r.start = table[lo * 3] + local * LT;
  r.count = left >= LT ? LT : (left > 0 ? (int)left : 0);
  return r;
}
// piece k of lane t holds the elements (k * 256 + t) * 4 .. + 3 of the tile; only a tensor's last tile has a piece cut short (scalar tail)
__device__ __forceinline__ f4v tile_load(const float* x, int e, int count) {
  if (e + 4 <= count) return *(const f4v*)(x + e);
  f4v r = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < 4; j++)
    if (e + j < count) r[j] = x[e + j];
  return r;
}
__device__ __forceinline__ void tile_store(float* x, int e, int count, f4v val) {
  if (e + 4 <= count) { *(f4v*)(x + e) = val; return; }
  for (int j = 0; j < 4; j++)
    if (e + j < count) x[e + j] = val[j];
}
__device__ __forceinline__ void tile_store_bf16(bf16raw* x, int e, int count, f4v val) {
  if (e + 4 <= count) { uint2 o; o.x = pack2bf(val[0], val[1]); o.y = pack2bf(val[2], val[3]); *(uint2*)(x + e) = o; return; }
  for (int j = 0; j < 4; j++)
    if (e + j < count) x[e + j] = f2bf(val[j]);
}
// the two sums of a tile: the lane's four running sums folded ((a0+a1)+(a2+a3)), the wave butterfly, the four waves in order - the fixed
// places of sumsq_partials_k (optim.hip)
__device__ __forceinline__ void tile_sums(f4v ap, f4v au, float* out) {
  __shared__ float waves[2][4];
  float sp = (ap[0] + ap[1]) + (ap[2] + ap[3]);
  float su = (au[0] + au[1]) + (au[2] + au[3]);
  sp = wave_sum(sp);
  su = wave_sum(su);
  if ((threadIdx.x & 63) == 0) { waves[0][threadIdx.x >> 6] = sp; waves[1][threadIdx.x >> 6] = su; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = ((waves[0][0] + waves[0][1]) + waves[0][2]) + waves[0][3];
    out[1] = ((waves[1][0] + waves[1][1]) + waves[1][2]) + waves[1][3];
  }
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
    pp[k] = tile_load(p + T.start, e, T.count); gg[k] = tile_load(g + T.start, e, T.count);
    mm[k] = tile_load(m + T.start, e, T.count); vv[k] = tile_load(v + T.start, e, T.count);
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
    tile_store(m + T.start, e, T.count, mm[k]);
    tile_store(v + T.start, e, T.count, vv[k]);
  }
  tile_sums(ap, au, partials + 2 * (long long)blockIdx.x);
}

__global__ __launch_bounds__(256) void lamb_stage2_k(float* p, const float* m, const float* v, bf16raw* pb, const long long* table, int n,
                                                     const float* stats, float lr, float eps, float rbc1, float rsb2, float wd) {
  const LayerTile T = layer_tile(table, n, blockIdx.x);
  const float step = lr * stats[T.tensor * 3 + 2];   // one float per workgroup (a uniform load)
  f4v pp[4], mm[4], vv[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
    pp[k] = tile_load(p + T.start, e, T.count); mm[k] = tile_load(m + T.start, e, T.count); vv[k] = tile_load(v + T.start, e, T.count);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = (k * 256 + threadIdx.x) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) pp[k][j] = pp[k][j] - step * lamb_update(pp[k][j], mm[k][j], vv[k][j], rbc1, rsb2, eps, wd);
    tile_store(p + T.start, e, T.count, pp[k]);
    if (pb) tile_store_bf16(pb + T.start, e, T.count, pp[k]);
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
    pp[k] = tile_load(p + T.start, e, T.count); gg[k] = tile_load(g + T.start, e, T.count);
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
  tile_sums(ap, au, partials + 2 * (long long)blockIdx.x);
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
    pp[k] = tile_load(p + T.start, e, T.count); gg[k] = tile_load(g + T.start, e, T.count); bb[k] = tile_load(buf + T.start, e, T.count);
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
    tile_store(buf + T.start, e, T.count, bb[k]);
    tile_store(p + T.start, e, T.count, pp[k]);
    if (pb) tile_store_bf16(pb + T.start, e, T.count, pp[k]);
  }
}

// One workgroup per tensor: its tiles' partials in index order in f64, contiguous runs per lane and then the run sums (grad_norm_finish_k).
__global__ __launch_bounds__(256) void layer_ratio_finish_k(const float* partials, const long long* table, float c, int adapt, float* stats) {
  __shared__ double runs[2][256];
  const long long t = blockIdx.x;
  const long long first = table[t * 3 + 2], count = (table[t * 3 + 1] + LT - 1) / LT;
  const long long per = (count + 255) / 256;
  const long long a = threadIdx.x * per, b = a + per < count ? a + per : count;
  double tp = 0.0, tu = 0.0;
  for (long long i = a; i < b; i++) { tp += (double)partials[2 * (first + i)]; tu += (double)partials[2 * (first + i) + 1]; }
  runs[0][threadIdx.x] = tp; runs[1][threadIdx.x] = tu;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sp = 0.0, su = 0.0;
    for (int i = 0; i < 256; i++) { sp += runs[0][i]; su += runs[1][i]; }
    const float pn = (float)sqrt(sp), un = (float)sqrt(su);
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
