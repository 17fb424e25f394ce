// Device-side helpers of the HBM-bound row and column kernels: one column walk for both access widths, the row arithmetic shared by the
// dense and the collated NT-Xent kernels, and the four-wave workgroup sum.
#pragma once
#include "common.hpp"

// W consecutive elements as f32 values: W = 8 through load8 / store8 (16-byte accesses; the row is 16-byte aligned and d % 8 == 0),
// W = 1 through Elem<T>
template <int W, typename T>
__device__ __forceinline__ void load_w(const T* p, float (&v)[W]) {
  static_assert(W == 8 || W == 1, "access width");
  if constexpr (W == 8) load8<T>(p, v);
  else v[0] = Elem<T>::ld(p);
}
template <int W, typename T>
__device__ __forceinline__ void store_w(T* p, const float (&v)[W]) {
  static_assert(W == 8 || W == 1, "access width");
  if constexpr (W == 8) store8<T>(p, v);
  else Elem<T>::st(p, v[0]);
}
// f(c) for the chunks of W columns that belong to `lane` of LANES: c = lane * W, then steps of LANES * W, while c < d
template <int W, int LANES = 64, typename F>
__device__ __forceinline__ void row_walk(int lane, int d, F&& f) {
  for (int c = lane * W; c < d; c += LANES * W) f(c);
}

// 8 consecutive columns col .. col + 7 of a row of d columns: one 16-byte (bf16) / two 16-byte (f32) accesses, or element by element with
// the columns behind d left out (loads give 0 there)
template <typename T, bool V8>
__device__ __forceinline__ void ld8(const T* row, int col, int d, float (&v)[8]) {
  if (V8) { load8<T>(row + col, v); return; }
#pragma unroll
  for (int e = 0; e < 8; e++) v[e] = col + e < d ? Elem<T>::ld(row + col + e) : 0.f;
}
template <typename T, bool V8>
__device__ __forceinline__ void st8(T* row, int col, int d, const float (&v)[8]) {
  if (V8) { store8<T>(row + col, v); return; }
#pragma unroll
  for (int e = 0; e < 8; e++)
    if (col + e < d) Elem<T>::st(row + col + e, v[e]);
}

// ---- one wave per row ----------------------------------------------------------------------------------------------------------------
#define PERO_NORMALIZE_EPS 1e-12f   // F.normalize eps

// dst = src / max(|src|_2, eps); returns 1 / max(|src|_2, eps) in every lane
template <typename T, bool V8>
__device__ __forceinline__ float row_l2_normalize(const T* src, T* dst, int lane, int d) {
  constexpr int W = V8 ? 8 : 1;
  float s = 0.f;
  row_walk<W>(lane, d, [=, &s](int c) {
    float v[W];
    load_w<W>(src + c, v);
#pragma unroll
    for (int e = 0; e < W; e++) s += v[e] * v[e];
  });
  s = wave_sum(s);
  const float r = 1.0f / fmaxf(sqrtf(s), PERO_NORMALIZE_EPS);
  row_walk<W>(lane, d, [=](int c) {
    float v[W];
    load_w<W>(src + c, v);
#pragma unroll
    for (int e = 0; e < W; e++) v[e] *= r;
    store_w<W>(dst + c, v);
  });
  return r;
}
// its backward: dx = (dxn - xn * <xn, dxn>) * inv[0] * (g ? g[0] : 1)
template <typename T, bool V8>
__device__ __forceinline__ void row_l2_normalize_bwd(const T* xn, const T* dxn, const float* inv, const float* g, T* dx, int lane, int d) {
  constexpr int W = V8 ? 8 : 1;
  float s = 0.f;
  row_walk<W>(lane, d, [=, &s](int c) {
    float a[W], b[W];
    load_w<W>(xn + c, a); load_w<W>(dxn + c, b);
#pragma unroll
    for (int e = 0; e < W; e++) s += a[e] * b[e];
  });
  s = wave_sum(s);
  const float r = inv[0] * (g ? g[0] : 1.f);
  row_walk<W>(lane, d, [=](int c) {
    float a[W], b[W];
    load_w<W>(xn + c, a); load_w<W>(dxn + c, b);
#pragma unroll
    for (int e = 0; e < W; e++) b[e] = (b[e] - a[e] * s) * r;
    store_w<W>(dx + c, b);
  });
}
template <typename T, bool V8>
__device__ __forceinline__ void row_zero(T* dst, int lane, int d) {
  constexpr int W = V8 ? 8 : 1;
  float z[W];
#pragma unroll
  for (int e = 0; e < W; e++) z[e] = 0.f;
  row_walk<W>(lane, d, [=](int c) { store_w<W>(dst + c, z); });
}

// The two halves of a column's log-sum-exp in the NT-Xent column kernels.
// One thread: max and sum of exp(. - max) over the first `rows` entries of column j of a row-major f32 block of pitch ld
__device__ __forceinline__ void col_max_sumexp(const float* s, int j, int rows, int ld, float& mx, float& sum) {
  mx = -INFINITY;
  for (int r = 0; r < rows; r++) mx = fmaxf(mx, s[(long long)r * ld + j]);
  sum = 0.f;
  for (int r = 0; r < rows; r++) sum += expf(s[(long long)r * ld + j] - mx);
}
// One wave: the L entries of `row` without entry `own` join a column's (max m1, sum csum); the joint log-sum-exp in every lane
__device__ __forceinline__ float row_join_lse(const float* row, int L, int own, int lane, float m1, float csum) {
  float mx = -INFINITY;
  for (int c = lane; c < L; c += 64) if (c != own) mx = fmaxf(mx, row[c]);
  mx = wave_max(mx);
  const float m = fmaxf(m1, mx);
  float sum = 0.f;
  for (int c = lane; c < L; c += 64) if (c != own) sum += expf(row[c] - m);
  sum = wave_sum(sum);
  return logf(csum * expf(m1 - m) + sum) + m;
}

// ---- one workgroup of four waves --------------------------------------------------------------------------------------------------------
// The sum of v over the 256 threads, folded as ((w0 + w1) + (w2 + w3)) of the four wave sums; every thread gets it.  One barrier; sm
// (4 floats of LDS) must not be in use by a thread that has not reached the call.
__device__ __forceinline__ float block_sum4(float v, float* sm) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
// two values behind one barrier
__device__ __forceinline__ void block_sum4(float& a, float& b, float (*sm)[4]) {
  a = wave_sum(a); b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = a; sm[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  a = (sm[0][0] + sm[0][1]) + (sm[0][2] + sm[0][3]);
  b = (sm[1][0] + sm[1][1]) + (sm[1][2] + sm[1][3]);
}
