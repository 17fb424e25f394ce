// Barlow Twins loss (Zbontar et al., 2021; BarlowTwinsLoss in joint_embedding_pretraining/losses.py): the HBM-bound
// passes around the three products, which run on pero_gemm.  Both views go through every launch (blockIdx.z / blockIdx.y = view).  Column
// statistics are reduced without atomics: a row tile of PERO_BARLOW_TILE_ROWS rows leaves one partial per column, a finishing launch merges
// the partials in tile order in f64 - a second run on the same input gives the same bits.
#include "dispatch.hpp"
#include "rows.hpp"

#define TR PERO_BARLOW_TILE_ROWS
#define RB 64  // rows of a workgroup of the two row-wise kernels: 8 per lane, four in flight

// --------------------------------------------------------------------------------------------
// Column partials of a row tile.  Workgroup = 256 columns x one tile x one view; lane (cg, rl) owns 8 columns and the rows r0 + rl + 8k.
// MODE 0 (pero_barlow_stats): rows gathered through the index list; per column (mean, M2) by Welford's update, the 8 row lanes merged in
//   lane order with the parallel-variance formula.  The count of a partial follows from its tile, so it is not stored.
// MODE 1 (pero_barlow_bwd_stats): compact rows; per column (sum dz, sum dz * z), lanes added in lane order.
// part: f32 [view][tile][2][d].
// --------------------------------------------------------------------------------------------
template <typename T, bool V8, int MODE>
__global__ __launch_bounds__(256) void barlow_tile_k(const T* p0, const int64_t* i0, const T* p1, const int64_t* i1, const T* q, float* part,
                                                     long long n, long long view_pitch, int d) {
  __shared__ float red[2][8][256 + 8];
  const int view = blockIdx.z, cg = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int col = (blockIdx.x * 32 + cg) * 8;
  const long long r0 = (long long)blockIdx.y * TR;
  const long long r1 = r0 + TR < n ? r0 + TR : n;
  const T* src = MODE == 0 ? (view ? p1 : p0) : p0 + view * view_pitch;
  const T* src2 = MODE == 0 ? nullptr : q + view * view_pitch;
  const int64_t* idx = view ? i1 : i0;
  float s0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, s1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  if (col < d) {
    for (long long r = r0 + rl; r < r1; r += 32) {   // four rows in flight per lane
      float v[4][8], w[4][8];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const long long rr = r + 8 * u;
        if (rr < r1) {
          ld8<T, V8>(src + (MODE == 0 ? idx[rr] : rr) * d, col, d, v[u]);
          if (MODE == 1) ld8<T, V8>(src2 + rr * d, col, d, w[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (r + 8 * u < r1) {
          if (MODE == 0) {
            cnt++;
            const float inv = 1.0f / (float)cnt;
#pragma unroll
            for (int e = 0; e < 8; e++) {
              const float dl = v[u][e] - s0[e];
              s0[e] += dl * inv;
              s1[e] += dl * (v[u][e] - s0[e]);
            }
          } else {
#pragma unroll
            for (int e = 0; e < 8; e++) { s0[e] += v[u][e]; s1[e] += v[u][e] * w[u][e]; }
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; e++) { red[0][rl][cg * 8 + e] = s0[e]; red[1][rl][cg * 8 + e] = s1[e]; }
  __syncthreads();
  const int c = threadIdx.x;
  const long long gc = (long long)blockIdx.x * 256 + c;
  if (gc >= d) return;
  float a0 = red[0][0][c], a1 = red[1][0][c];
  if (MODE == 0) {
    const long long rows = r1 - r0;
    float na = rows > 0 ? (float)((rows + 7) / 8) : 0.f;   // rows of lane 0
#pragma unroll
    for (int k = 1; k < 8; k++) {
      const float nb = rows > k ? (float)((rows - k + 7) / 8) : 0.f;
      if (nb > 0.f) {
        const float nab = na + nb, dl = red[0][k][c] - a0;
        a0 += dl * (nb / nab);
        a1 += red[1][k][c] + dl * dl * (na * nb / nab);
        na = nab;
      }
    }
  } else {
#pragma unroll
    for (int k = 1; k < 8; k++) { a0 += red[0][k][c]; a1 += red[1][k][c]; }
  }
  float* o = part + (((long long)view * gridDim.y + blockIdx.y) * 2) * d + gc;
  o[0] = a0;
  o[d] = a1;
}

// The partials of a column in tile order, in f64.  Workgroup = 64 columns x one view; wave w merges the contiguous run of tiles
// [w * per, (w + 1) * per), per = ceil(tiles / 4), wave 0's lanes then merge the four runs in order.
// MODE 0: (count, mean, M2) merged with the parallel-variance formula -> out0 = mean, out1 = 1 / sqrt(M2 / n + eps).
// MODE 1: plain sums -> out0 = a, out1 = b.       out0, out1: f32 [view][d].
template <int MODE>
__global__ __launch_bounds__(256) void barlow_finish_k(const float* part, float* out0, float* out1, long long n, int d, int tiles, float eps) {
  __shared__ double run[3][4][64];
  const int view = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long gc = (long long)blockIdx.x * 64 + lane;
  const int per = (tiles + 3) / 4;
  const int t0 = w * per, t1 = t0 + per < tiles ? t0 + per : tiles;
  double cn = 0.0, a0 = 0.0, a1 = 0.0;
  if (gc < d) {
    for (int t = t0; t < t1; t++) {
      const float* p = part + (((long long)view * tiles + t) * 2) * d + gc;
      const double b0 = (double)p[0], b1 = (double)p[d];
      if (MODE == 0) {
        const long long left = n - (long long)t * TR;
        const double nb = (double)(left < TR ? left : TR), nab = cn + nb, dl = b0 - a0;
        a0 += dl * (nb / nab);
        a1 += b1 + dl * dl * (cn * nb / nab);
        cn = nab;
      } else { a0 += b0; a1 += b1; }
    }
  }
  run[0][w][lane] = cn; run[1][w][lane] = a0; run[2][w][lane] = a1;
  __syncthreads();
  if (w != 0 || gc >= d) return;
  for (int k = 1; k < 4; k++) {
    const double nb = run[0][k][lane], b0 = run[1][k][lane], b1 = run[2][k][lane];
    if (MODE == 0) {
      if (nb > 0.0) {
        const double nab = cn + nb, dl = b0 - a0;
        a0 += dl * (nb / nab);
        a1 += b1 + dl * dl * (cn * nb / nab);
        cn = nab;
      }
    } else { a0 += b0; a1 += b1; }
  }
  out0[(long long)view * d + gc] = (float)a0;
  out1[(long long)view * d + gc] = MODE == 0 ? (float)(1.0 / sqrt(a1 / (double)n + (double)eps)) : (float)a1;
}

// zh[view][r] = (z[idx[r]] - mean) * rstd for r < n, explicit zeros for n <= r < n_pad.  Workgroup = RB rows x 256 columns x one view, lane
// (cg, rl) owns 8 columns - their mean and rstd stay in registers - and the rows r0 + rl + 8k.  (One wave per row read the 8 bytes of
// statistics per column again for every row: four times the bytes of the bf16 row itself through the vector cache.)
template <typename T, bool V8>
__global__ __launch_bounds__(256) void barlow_standardize_k(const T* __restrict__ x, const int64_t* ix, const T* __restrict__ y, const int64_t* iy,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd, T* __restrict__ zh,
                                                            long long n, long long n_pad, int d) {
  const int view = blockIdx.z, cg = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int col = (blockIdx.y * 32 + cg) * 8;
  if (col >= d) return;
  float mu[8], rs[8];
  ld8<float, V8>(mean + (long long)view * d, col, d, mu);
  ld8<float, V8>(rstd + (long long)view * d, col, d, rs);
  const T* src = view ? y : x;
  const int64_t* idx = view ? iy : ix;
  T* out = zh + (long long)view * n_pad * d;
  const long long r0 = (long long)blockIdx.x * RB;
  const long long r1 = r0 + RB < n_pad ? r0 + RB : n_pad;
  for (long long r = r0 + rl; r < r1; r += 32) {
    float v[4][8];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const long long rr = r + 8 * u;
      if (rr < r1 && rr < n) ld8<T, V8>(src + idx[rr] * d, col, d, v[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const long long rr = r + 8 * u;
      if (rr < r1) {
#pragma unroll
        for (int e = 0; e < 8; e++) {
          if (rr < n) v[u][e] = (v[u][e] - mu[e]) * rs[e];
          else v[u][e] = 0.f;
        }
        st8<T, V8>(out + rr * d, col, d, v[u]);
      }
    }
  }
}

// One pass over c (d x d, f32), one workgroup per row i: the row's parts of on = sum_i (c_ii - 1)^2 and off = sum_{i != j} c_ij^2, and
// row i of the backward operand G (compute dtype): G_ii = 2 (c_ii - 1) / n, G_ij = 2 lambda c_ij / n.   rowpart: f32 [2][d].
template <typename T, bool V8>
__global__ __launch_bounds__(256) void barlow_corr_k(const float* c, T* G, float* rowpart, int d, float g_on, float g_off) {
  __shared__ float sm[2][4];
  const int i = blockIdx.x;
  const float* row = c + (long long)i * d;
  T* o = G + (long long)i * d;
  constexpr int W = V8 ? 8 : 1;
  float on = 0.f, off = 0.f;
  row_walk<W, 256>(threadIdx.x, d, [=, &on, &off](int j) {
    float v[W];
    load_w<W>(row + j, v);
#pragma unroll
    for (int e = 0; e < W; e++) {
      if (j + e == i) { const float t = v[e] - 1.0f; on += t * t; v[e] = g_on * t; }
      else { off += v[e] * v[e]; v[e] = g_off * v[e]; }
    }
    store_w<W>(o + j, v);
  });
  block_sum4(on, off, sm);
  if (threadIdx.x == 0) { rowpart[i] = on; rowpart[d + i] = off; }
}
// out = {on + lambda * off, on, off} from the row parts (single workgroup, fixed order)
__global__ __launch_bounds__(256) void barlow_fold_k(const float* rowpart, float* out, int d, float lambda) {
  __shared__ float sm[2][4];
  float on = 0.f, off = 0.f;
  for (int i = threadIdx.x; i < d; i += 256) { on += rowpart[i]; off += rowpart[d + i]; }
  block_sum4(on, off, sm);
  if (threadIdx.x == 0) { out[0] = on + lambda * off; out[1] = on; out[2] = off; }
}

// dz = g * rstd_j * (dzh - a_j / n - zh * b_j / n), stored to dx[ix[r]] / dy[iy[r]] (the indices are unique: a store).  The layout of
// barlow_standardize_k: the lane's 8 columns of g * rstd, a / n and b / n stay in registers.
template <typename T, bool V8>
__global__ __launch_bounds__(256) void barlow_standardize_bwd_k(const T* __restrict__ dzh, const T* __restrict__ zh, const float* __restrict__ rstd,
                                                                const float* __restrict__ a, const float* __restrict__ b, const int64_t* ix,
                                                                const int64_t* iy, T* __restrict__ dx, T* __restrict__ dy, const float* g,
                                                                long long n, long long n_pad, int d) {
  const int view = blockIdx.z, cg = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int col = (blockIdx.y * 32 + cg) * 8;
  if (col >= d) return;
  const float gs = g ? g[0] : 1.f, inv_n = 1.0f / (float)n;
  float rs[8], av[8], bv[8];
  ld8<float, V8>(rstd + (long long)view * d, col, d, rs);
  ld8<float, V8>(a + (long long)view * d, col, d, av);
  ld8<float, V8>(b + (long long)view * d, col, d, bv);
#pragma unroll
  for (int e = 0; e < 8; e++) { rs[e] = gs * rs[e]; av[e] = av[e] * inv_n; bv[e] = bv[e] * inv_n; }
  const T* dz = dzh + (long long)view * n_pad * d;
  const T* z = zh + (long long)view * n_pad * d;
  T* out = view ? dy : dx;
  const int64_t* idx = view ? iy : ix;
  const long long r0 = (long long)blockIdx.x * RB;
  const long long r1 = r0 + RB < n ? r0 + RB : n;
  for (long long r = r0 + rl; r < r1; r += 32) {
    float v[4][8], w[4][8];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const long long rr = r + 8 * u;
      if (rr < r1) { ld8<T, V8>(dz + rr * d, col, d, v[u]); ld8<T, V8>(z + rr * d, col, d, w[u]); }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const long long rr = r + 8 * u;
      if (rr < r1) {
#pragma unroll
        for (int e = 0; e < 8; e++) v[u][e] = rs[e] * (v[u][e] - av[e] - w[u][e] * bv[e]);
        st8<T, V8>(out + idx[rr] * d, col, d, v[u]);
      }
    }
  }
}

static inline int64_t barlow_tiles(int64_t n) { return (n + TR - 1) / TR; }

extern "C" int pero_barlow_stats(const void* x, const int64_t* ix, const void* y, const int64_t* iy, float* part, float* mean, float* rstd,
                                 int64_t n, int64_t d, float eps, int dtype, void* stream) {
  PERO_REQUIRE(x && y && ix && iy && part && mean && rstd && n > 0 && d > 0 && d < (1ll << 31) && eps >= 0.f, "pero_barlow_stats: bad arguments");
  const int64_t tiles = barlow_tiles(n);
  PERO_REQUIRE(tiles <= 65535, "pero_barlow_stats: more than 65535 row tiles");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)((d + 255) / 256), (unsigned)tiles, 2), block(256);
  const bool v8 = v8_ok(d, dtype, {x, y});
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(v8, [&](auto V) {
    hipLaunchKernelGGL((barlow_tile_k<T, decltype(V)::value, 0>), grid, block, 0, st, (const T*)x, ix, (const T*)y, iy, (const T*)nullptr, part, (long long)n, 0ll, (int)d); }); }), "bad dtype");
  hipLaunchKernelGGL((barlow_finish_k<0>), dim3((unsigned)((d + 63) / 64), 2), block, 0, st, part, mean, rstd, (long long)n, (int)d, (int)tiles, eps);
  PERO_CHECK_LAUNCH("pero_barlow_stats");
  return PERO_OK;
}

extern "C" int pero_barlow_standardize(const void* x, const int64_t* ix, const void* y, const int64_t* iy, const float* mean, const float* rstd,
                                       void* zh, int64_t n, int64_t n_pad, int64_t d, int dtype, void* stream) {
  PERO_REQUIRE(x && y && ix && iy && mean && rstd && zh && n > 0 && n_pad >= n && d > 0 && (d + 255) / 256 <= 65535 && (n_pad + RB - 1) / RB < (1ll << 31),
               "pero_barlow_standardize: bad arguments");
  dim3 grid((unsigned)((n_pad + RB - 1) / RB), (unsigned)((d + 255) / 256), 2), block(256);
  const bool v8 = v8_ok(d, dtype, {x, y, zh, mean, rstd});
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(v8, [&](auto V) {
    hipLaunchKernelGGL((barlow_standardize_k<T, decltype(V)::value>), grid, block, 0, (hipStream_t)stream, (const T*)x, ix, (const T*)y, iy, mean, rstd, (T*)zh, (long long)n, (long long)n_pad, (int)d); }); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_barlow_standardize");
  return PERO_OK;
}

extern "C" int pero_barlow_corr(const float* c, void* G, float* rowpart, float* out, int64_t d, int64_t n, float lambda, int dtype, void* stream) {
  PERO_REQUIRE(c && G && rowpart && out && d > 0 && d < (1ll << 31) && n > 0, "pero_barlow_corr: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const float g_on = 2.0f / (float)n, g_off = 2.0f * lambda / (float)n;
  const bool v8 = d % 8 == 0 && aligned16(c) && aligned16(G);
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(v8, [&](auto V) {
    hipLaunchKernelGGL((barlow_corr_k<T, decltype(V)::value>), dim3((unsigned)d), dim3(256), 0, st, c, (T*)G, rowpart, (int)d, g_on, g_off); }); }), "bad dtype");
  hipLaunchKernelGGL(barlow_fold_k, dim3(1), dim3(256), 0, st, rowpart, out, (int)d, lambda);
  PERO_CHECK_LAUNCH("pero_barlow_corr");
  return PERO_OK;
}

extern "C" int pero_barlow_bwd_stats(const void* dzh, const void* zh, float* part, float* a, float* b, int64_t n, int64_t n_pad, int64_t d,
                                     int dtype, void* stream) {
  PERO_REQUIRE(dzh && zh && part && a && b && n > 0 && n_pad >= n && d > 0 && d < (1ll << 31), "pero_barlow_bwd_stats: bad arguments");
  const int64_t tiles = barlow_tiles(n);
  PERO_REQUIRE(tiles <= 65535, "pero_barlow_bwd_stats: more than 65535 row tiles");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)((d + 255) / 256), (unsigned)tiles, 2), block(256);
  const bool v8 = v8_ok(d, dtype, {dzh, zh});
  const long long pitch = (long long)n_pad * d;
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(v8, [&](auto V) {
    hipLaunchKernelGGL((barlow_tile_k<T, decltype(V)::value, 1>), grid, block, 0, st, (const T*)dzh, (const int64_t*)nullptr, (const T*)nullptr, (const int64_t*)nullptr, (const T*)zh, part, (long long)n, pitch, (int)d); }); }), "bad dtype");
  hipLaunchKernelGGL((barlow_finish_k<1>), dim3((unsigned)((d + 63) / 64), 2), block, 0, st, part, a, b, (long long)n, (int)d, (int)tiles, 0.f);
  PERO_CHECK_LAUNCH("pero_barlow_bwd_stats");
  return PERO_OK;
}

extern "C" int pero_barlow_standardize_bwd(const void* dzh, const void* zh, const float* rstd, const float* a, const float* b, const int64_t* ix,
                                           const int64_t* iy, void* dx, void* dy, const float* g, int64_t n, int64_t n_pad, int64_t d, int dtype,
                                           void* stream) {
  PERO_REQUIRE(dzh && zh && rstd && a && b && ix && iy && dx && dy && n > 0 && n_pad >= n && d > 0 && (d + 255) / 256 <= 65535 && (n + RB - 1) / RB < (1ll << 31),
               "pero_barlow_standardize_bwd: bad arguments");
  dim3 grid((unsigned)((n + RB - 1) / RB), (unsigned)((d + 255) / 256), 2), block(256);
  const bool v8 = v8_ok(d, dtype, {dzh, zh, dx, dy, rstd, a, b});
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(v8, [&](auto V) {
    hipLaunchKernelGGL((barlow_standardize_bwd_k<T, decltype(V)::value>), grid, block, 0, (hipStream_t)stream, (const T*)dzh, (const T*)zh, rstd, a, b, ix, iy, (T*)dx, (T*)dy, g, (long long)n, (long long)n_pad, (int)d); }); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_barlow_standardize_bwd");
  return PERO_OK;
}
