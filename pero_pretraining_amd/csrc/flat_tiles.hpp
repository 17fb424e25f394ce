// What the kernels over flat buffers share (optim.hip, optim_layerwise.hip, latent.hip, misc.hip): the workgroup's segment in a device
// table, 16-byte pieces with a scalar tail, the fixed-order f32 fold of a workgroup and the fixed-order f64 sum of its partials.  Every
// order here is pinned bit for bit by the f64 restatements of the tests (tests/optim_ref.py, layerwise_ref.py, latent_ref.py).
#pragma once
#include "common.hpp"

#define LT PERO_LAYER_TILE   // elements of a tile = 256 lanes x 4 pieces of 16 bytes

// ---------------------------------------------------------------------------------------------
// Workgroup -> segment.  A table has W int64 columns, the last one the segment's first tile; the segment of tile `bid` is the last one
// whose first tile is <= bid (binary search: a model has a few hundred tensors).  n >= 1.
// ---------------------------------------------------------------------------------------------
struct TileSeg {
  int seg;           // row of the table
  long long local;   // index of the tile inside its segment
};
template <int W>
__device__ __forceinline__ TileSeg tile_segment(const long long* table, int n, long long bid) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid * W + W - 1] <= bid) lo = mid; else hi = mid - 1;
  }
  TileSeg r;
  r.seg = lo;
  r.local = bid - table[lo * W + W - 1];
  return r;
}
// elements of tile `local` of a segment of `numel` elements cut into tiles of LT: 1 .. LT, or 0 for a tile that lies behind the segment's
// end (a table and a tile count that do not belong together): such a tile touches no element
__device__ __forceinline__ int tile_count(long long numel, long long local) {
  const long long left = local >= 0 ? numel - local * LT : 0;
  return left >= LT ? LT : (left > 0 ? (int)left : 0);
}

// ---------------------------------------------------------------------------------------------
// Four consecutive elements as one 16-byte (f32) or 8-byte (bf16) access ...
// ---------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ f4v load4(const T* p);
template <> __device__ __forceinline__ f4v load4<float>(const float* p) { return *(const f4v*)p; }
template <> __device__ __forceinline__ f4v load4<bf16raw>(const bf16raw* p) {
  const uint2 r = *(const uint2*)p;
  return (f4v){__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u)};
}
template <typename T> __device__ __forceinline__ void store4(T* p, f4v v);
template <> __device__ __forceinline__ void store4<float>(float* p, f4v v) { *(f4v*)p = v; }
template <> __device__ __forceinline__ void store4<bf16raw>(bf16raw* p, f4v v) {
  uint2 o;
  o.x = pack2bf(v[0], v[1]); o.y = pack2bf(v[2], v[3]);
  *(uint2*)p = o;
}
// ... and the piece x[e .. e + 3] of a run of `count` elements: only the run's last piece is cut short (scalar tail; a load fills it with
// zeros).  vec = false takes the scalar path for a whole piece too (a pointer that is not 16-byte aligned).
template <typename I>
__device__ __forceinline__ f4v load4_tail(const float* x, I e, I count, bool vec = true) {
  if (vec && e + 4 <= count) return load4<float>(x + e);
  f4v r = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < 4; j++)
    if (e + j < count) r[j] = x[e + j];
  return r;
}
template <typename T, typename I>
__device__ __forceinline__ void store4_tail(T* x, I e, I count, f4v val) {
  if (e + 4 <= count) { store4<T>(x + e, val); return; }
  for (int j = 0; j < 4; j++)
    if (e + j < count) Elem<T>::st(&x[e + j], val[j]);   // one 32-bit index: `x + e + j` widens both (a wave per SIMD in lamb_stage1_k)
}

// ---------------------------------------------------------------------------------------------
// The N sums of a workgroup of 256 lanes in f32, every addition in a fixed place: the lane's four running sums folded ((a0+a1)+(a2+a3)),
// the 64 lanes of a wave by a butterfly, the four waves in order; lane 0 writes out[0 .. N).
// ---------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void block_fold(const f4v (&acc)[N], float* out) {
  __shared__ float waves[N][4];
  float s[N];
#pragma unroll
  for (int i = 0; i < N; i++) s[i] = (acc[i][0] + acc[i][1]) + (acc[i][2] + acc[i][3]);
#pragma unroll
  for (int i = 0; i < N; i++) s[i] = wave_sum(s[i]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; i++) waves[i][threadIdx.x >> 6] = s[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = ((waves[i][0] + waves[i][1]) + waves[i][2]) + waves[i][3];
  }
}

// ---------------------------------------------------------------------------------------------
// N interleaved sums over partials[STRIDE * i + j], i < count, by one workgroup of 256 lanes in f64: lane t adds the contiguous run
// [t * per, (t + 1) * per) with per = ceil(count / 256) in index order, lane 0 adds the 256 run sums in index order.  total[] is valid in
// lane 0 only.
// ---------------------------------------------------------------------------------------------
template <int N, int STRIDE>
__device__ __forceinline__ void run_sum_f64(const float* partials, long long count, double (&total)[N]) {
  __shared__ double runs[N][256];
  const long long per = (count + 255) / 256;
  const long long a = threadIdx.x * per, b = a + per < count ? a + per : count;
  double t[N];
#pragma unroll
  for (int j = 0; j < N; j++) t[j] = 0.0;
  for (long long i = a; i < b; i++) {
#pragma unroll
    for (int j = 0; j < N; j++) t[j] += (double)partials[STRIDE * i + j];
  }
#pragma unroll
  for (int j = 0; j < N; j++) runs[j][threadIdx.x] = t[j];
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < N; j++) total[j] = 0.0;
    for (int i = 0; i < 256; i++) {
#pragma unroll
      for (int j = 0; j < N; j++) total[j] += runs[j][i];
    }
  }
}
