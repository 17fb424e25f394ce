// Adam with torch.optim.Adam's remaining arguments (weight decay coupled / decoupled, amsgrad, maximize) and a fused global-norm
// clip, plus the two launches that produce that norm on the device.  All HBM-bound.  pero_adam_step (misc.hip) is the plain
// kernel without these arguments: the benchmark times it, and the tests hold adam_ex_k with every flag off to its bits.
#include "flat_tiles.hpp"

// ---------------------------------------------------------------------------------------------
// One element, in torch's order (torch/optim/adam.py _single_tensor_adam; clip_grad_norm_ in front of it).  `g` arrives as
// grad * grad_scale.  `wd` is the weight decay itself (WD == 1, coupled: g += wd * p) or the factor 1 - lr * wd (WD == 2,
// decoupled: p *= factor).  With WD == 0 and every flag false this is the arithmetic of adam_k, operation for operation.
// ---------------------------------------------------------------------------------------------
template <int WD, bool AMS, bool MAXI, bool CLIP>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& vm, float coef, float wd, float lr_bc1, float b1,
                                          float b2, float omb1, float omb2, float eps, float inv_sqrt_bc2) {
  if (CLIP) g = g * coef;
  if (MAXI) g = -g;
  if (WD == 1) g = g + wd * p;
  if (WD == 2) p = p * wd;
  m = m * b1 + omb1 * g;
  v = v * b2 + omb2 * g * g;
  float root;
  if (AMS) { vm = (v > vm || v != v) ? v : vm; root = sqrtf(vm); }  // torch.maximum: a NaN wins (fmaxf would drop it)
  else root = sqrtf(v);
  const float denom = root * inv_sqrt_bc2 + eps;
  p = p - lr_bc1 * (m / denom);
}

template <int WD, bool AMS, bool MAXI, bool CLIP>
__global__ __launch_bounds__(256) void adam_ex_k(float* p, const float* g, float* m, float* v, bf16raw* pb, long long n, float lr_bc1,
                                                 float b1, float b2, float omb1, float omb2, float eps, float inv_sqrt_bc2, float gscale,
                                                 float wd, float* vmax, const float* gnorm, float max_norm) {
  // the clip coefficient of torch.nn.utils.clip_grad_norm_, from the ONE device float every thread reads (a uniform load); written so
  // that a NaN norm gives a NaN coefficient, as torch's clamp does
  float coef = 1.0f;
  if (CLIP) {
    const float c = max_norm / (*gnorm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;
  }
  const long long stride = (long long)gridDim.x * 256 * 4;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      f4v pp = *(f4v*)(p + i), gg = *(const f4v*)(g + i), mm = *(f4v*)(m + i), vv = *(f4v*)(v + i);
      f4v xx = {0.f, 0.f, 0.f, 0.f};
      if (AMS) xx = *(f4v*)(vmax + i);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float pe = pp[e], me = mm[e], ve = vv[e], xe = xx[e];
        adam_elem<WD, AMS, MAXI, CLIP>(pe, gg[e] * gscale, me, ve, xe, coef, wd, lr_bc1, b1, b2, omb1, omb2, eps, inv_sqrt_bc2);
        pp[e] = pe; mm[e] = me; vv[e] = ve; xx[e] = xe;
      }
      *(f4v*)(p + i) = pp; *(f4v*)(m + i) = mm; *(f4v*)(v + i) = vv;
      if (AMS) *(f4v*)(vmax + i) = xx;
      if (pb) { uint2 o; o.x = pack2bf(pp[0], pp[1]); o.y = pack2bf(pp[2], pp[3]); *(uint2*)(pb + i) = o; }
    } else {
      for (long long j = i; j < n; j++) {
        float pe = p[j], me = m[j], ve = v[j], xe = AMS ? vmax[j] : 0.f;
        adam_elem<WD, AMS, MAXI, CLIP>(pe, g[j] * gscale, me, ve, xe, coef, wd, lr_bc1, b1, b2, omb1, omb2, eps, inv_sqrt_bc2);
        m[j] = me; v[j] = ve; p[j] = pe;
        if (AMS) vmax[j] = xe;
        if (pb) pb[j] = f2bf(pe);
      }
    }
  }
}

// the grid of pero_adam_step (misc.hip grid_for(n, 4)): the same elements in the same threads
static unsigned adam_grid(long long n) {
  long long b = (n + 1023) / 1024;
  if (b > 4096) b = 4096;
  return (unsigned)(b < 1 ? 1 : b);
}

typedef void (*adam_ex_fn)(float*, const float*, float*, float*, bf16raw*, long long, float, float, float, float, float, float, float, float,
                           float, float*, const float*, float);
template <int WD, bool AMS, bool MAXI>
static adam_ex_fn adam_ex_pick1(bool clip) { return clip ? adam_ex_k<WD, AMS, MAXI, true> : adam_ex_k<WD, AMS, MAXI, false>; }
template <int WD, bool AMS>
static adam_ex_fn adam_ex_pick2(bool maxi, bool clip) { return maxi ? adam_ex_pick1<WD, AMS, true>(clip) : adam_ex_pick1<WD, AMS, false>(clip); }
template <int WD>
static adam_ex_fn adam_ex_pick3(bool ams, bool maxi, bool clip) { return ams ? adam_ex_pick2<WD, true>(maxi, clip) : adam_ex_pick2<WD, false>(maxi, clip); }

extern "C" int pero_adam_step_ex(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, double lr, double beta1,
                                 double beta2, double eps, int64_t step, double grad_scale, double weight_decay, int decoupled, float* vmax,
                                 int maximize, const float* grad_norm, double max_norm, void* stream) {
  PERO_REQUIRE(p && g && m && v && n > 0 && step >= 1, "pero_adam_step_ex: bad arguments");
  PERO_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(vmax) && (!p_bf16 || (((uintptr_t)p_bf16) & 7) == 0),
               "pero_adam_step_ex: alignment");
  PERO_REQUIRE((decoupled == 0 || decoupled == 1) && (maximize == 0 || maximize == 1), "pero_adam_step_ex: decoupled / maximize must be 0 or 1");
  PERO_REQUIRE(!grad_norm || max_norm >= 0.0, "pero_adam_step_ex: max_norm must not be negative");
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const int wdm = weight_decay == 0.0 ? 0 : (decoupled ? 2 : 1);
  const float wd = wdm == 2 ? (float)(1.0 - lr * weight_decay) : (float)weight_decay;
  const bool ams = vmax != nullptr, maxi = maximize != 0, clip = grad_norm != nullptr;
  const adam_ex_fn k = wdm == 0 ? adam_ex_pick3<0>(ams, maxi, clip) : wdm == 1 ? adam_ex_pick3<1>(ams, maxi, clip) : adam_ex_pick3<2>(ams, maxi, clip);
  hipLaunchKernelGGL(k, dim3(adam_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16raw*)p_bf16, (long long)n,
                     (float)(lr / bc1), (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)(1.0 / sqrt(bc2)),
                     (float)grad_scale, wd, vmax, grad_norm, (float)max_norm);
  PERO_CHECK_LAUNCH("pero_adam_step_ex");
  return PERO_OK;
}

// ---------------------------------------------------------------------------------------------
// Global L2 norm of flat f32 buffers without float atomics, in two launches.
//
// Layout (ops.py mirrors the three constants for the tests' error bound).  The buffer is cut into nv = ceil(n / 4) 16-byte pieces (the last
// one zero-filled); W = min(ceil(nv / 1024), SUMSQ_MAX_BLOCKS) workgroups of 256 lanes - a function of n alone, never of the device.  Lane
// t of workgroup b squares pieces b*256 + t + j * W*256, j = 0, 1, ... into four running f32 sums (one per element of the piece: a chain
// of at most ceil(nv / (W*256)) additions), folds the four ((a0+a1)+(a2+a3): 2 more), the 64 lanes of a wave by a butterfly (6 more), the
// four waves in order (3 more), and writes partials[b].  The second launch is ONE workgroup: lane t adds a contiguous run of partials in
// index order in f64, lane 0 adds the 256 run sums in index order, and norm = scale * sqrt(sum) is rounded to f32 once.  Every addition
// has a fixed place, so the same input gives the same bits on every run and on every device.
// ---------------------------------------------------------------------------------------------
#define SUMSQ_MAX_BLOCKS 2048
static long long sumsq_blocks(long long n) {
  const long long nv = (n + 3) / 4;
  long long b = (nv + 1023) / 1024;
  if (b > SUMSQ_MAX_BLOCKS) b = SUMSQ_MAX_BLOCKS;
  return b < 1 ? 1 : b;
}
__global__ __launch_bounds__(256) void sumsq_partials_k(const float* x, long long n, float* partials) {
  const long long nv = (n + 3) >> 2;
  const long long stride = (long long)gridDim.x * 256;
  f4v acc = {0.f, 0.f, 0.f, 0.f};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += 4 * stride) {
    f4v a[4];  // four loads in flight per lane
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const long long idx = i + k * stride;
      a[k] = (f4v){0.f, 0.f, 0.f, 0.f};
      if (idx < nv) a[k] = load4_tail(x, idx * 4, n);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) acc = acc + a[k] * a[k];
  }
  block_fold<1>({acc}, partials + blockIdx.x);
}
__global__ __launch_bounds__(256) void grad_norm_finish_k(const float* partials, long long count, double scale, float* norm) {
  double total[1];
  run_sum_f64<1, 1>(partials, count, total);
  if (threadIdx.x == 0) norm[0] = (float)(scale * sqrt(total[0]));
}

extern "C" int pero_sumsq_num_partials(int64_t n) { return n > 0 ? (int)sumsq_blocks(n) : 0; }
extern "C" int pero_sumsq_partials(const float* x, int64_t n, float* partials, void* stream) {
  PERO_REQUIRE(x && partials && n > 0, "pero_sumsq_partials: bad arguments");
  PERO_REQUIRE(aligned16(x), "pero_sumsq_partials: alignment");
  hipLaunchKernelGGL(sumsq_partials_k, dim3((unsigned)sumsq_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, (long long)n, partials);
  PERO_CHECK_LAUNCH("pero_sumsq_partials");
  return PERO_OK;
}
extern "C" int pero_grad_norm_finish(const float* partials, int64_t count, double scale, float* norm, void* stream) {
  PERO_REQUIRE(partials && norm && count > 0, "pero_grad_norm_finish: bad arguments");
  hipLaunchKernelGGL(grad_norm_finish_k, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (long long)count, scale, norm);
  PERO_CHECK_LAUNCH("pero_grad_norm_finish");
  return PERO_OK;
}
