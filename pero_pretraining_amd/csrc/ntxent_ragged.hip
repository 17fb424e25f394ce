// NT-Xent on collated batches (NTXentLoss(apply_masks=True)): every line keeps only the positions its shift mask AND its image mask
// mark with 1.  The selected rows of a line are compacted to the front of a block of Sp >= S rows (Sp a multiple of 128 in bf16, so
// that the three per-line products meet pero_gemm's tile conditions at every S); rows behind the line's count m are zero, and the
// column kernel writes zeros outside the m x m block of its gradient, so the products may read whole padded blocks.
// Everything here is HBM-bound row / column work in f32 statistics; the row arithmetic and the halves of the column log-sum-exp are the
// functions of rows.hpp that the dense kernels of losses.hip call too.
#include "dispatch.hpp"
#include "rows.hpp"

// One wave per line: rank of every selected position among the line's selected positions (ballot + popcount prefix over chunks of 64
// positions), -1 elsewhere; count[l] = the number of selected positions, -1 when the two views select different numbers.
__global__ __launch_bounds__(256) void ntxent_slots_k(const unsigned char* im1, const unsigned char* im2, const unsigned char* sm1,
                                                      const unsigned char* sm2, int* slot1, int* slot2, int* count, int lines, int S) {
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= lines) return;
  const int lane = threadIdx.x & 63;
  const long long o = (long long)l * S;
  const unsigned long long below = (1ull << lane) - 1ull;
  int c1 = 0, c2 = 0;
  for (int base = 0; base < S; base += 64) {
    const int p = base + lane;
    const bool a = p < S && sm1[o + p] == 1 && im1[o + p] == 1;
    const bool b = p < S && sm2[o + p] == 1 && im2[o + p] == 1;
    const unsigned long long ma = __ballot(a), mb = __ballot(b);
    if (p < S) {
      slot1[o + p] = a ? c1 + __popcll(ma & below) : -1;
      slot2[o + p] = b ? c2 + __popcll(mb & below) : -1;
    }
    c1 += __popcll(ma);
    c2 += __popcll(mb);
  }
  if (lane == 0) count[l] = c1 == c2 ? c1 : -1;
}

// One wave per (line, r), r < Sp.  Position r of the line, when selected (slot k >= 0), is L2-normalised into compact row k
// (row_l2_normalize, as in rownorm_fwd_k); compact row r >= m is written as zeros (inv 0).  A line with count <= 0 becomes an all-zero block.
template <typename T, bool V8>
__global__ __launch_bounds__(256) void ntxent_rows_fwd_k(const T* x, const int* slot, const int* count, T* xn, float* inv, long long lines,
                                                         int ncount, int S, int Sp, int d) {
  const long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= lines * Sp) return;
  const long long l = idx / Sp;
  const int r = (int)(idx - l * Sp), lane = threadIdx.x & 63;
  const int cnt = count[l % ncount];
  const int m = cnt > 0 ? (cnt < Sp ? cnt : Sp) : 0;
  if (r >= m) {
    row_zero<T, V8>(xn + idx * d, lane, d);
    if (lane == 0) inv[idx] = 0.f;
  }
  if (r >= S) return;
  const int k = slot[l * S + r];
  if (k < 0 || k >= m) return;
  const float rn = row_l2_normalize<T, V8>(x + (l * S + r) * d, xn + (l * Sp + k) * d, lane, d);
  if (lane == 0) inv[l * Sp + k] = rn;
}

// One wave per (line, position): a selected position reads its compact row k: dx = (dxn_k - xn_k <xn_k, dxn_k>) inv_k g
// (row_l2_normalize_bwd, as in rownorm_bwd_k); every other position, and every position of a line with count <= 0, is written as zeros.
template <typename T, bool V8>
__global__ __launch_bounds__(256) void ntxent_rows_bwd_k(const T* xn, const T* dxn, const float* inv, const int* slot, const int* count,
                                                         const float* g, T* dx, long long lines, int ncount, int S, int Sp, int d) {
  const long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= lines * S) return;
  const long long l = idx / S;
  const int lane = threadIdx.x & 63;
  const int k = slot[idx], m = count[l % ncount];
  T* o = dx + idx * d;
  if (k < 0 || k >= m || k >= Sp) { row_zero<T, V8>(o, lane, d); return; }
  const long long row = l * Sp + k;
  row_l2_normalize_bwd<T, V8>(xn + row * d, dxn + row * d, inv + row, g, o, lane, d);
}

// One workgroup per line; m = count[l].  ntxent_cols_k / ntxent_cols_cross_k (losses.hip) restricted to the leading m x m block of the line's
// Sp x Sp similarity block and to the first m rows of its part of `cross` (null: no pooled negatives):
//   lse_j = log( sum_{i<m} exp(sim[i][j]) + sum_{l' != own} exp(cross[j][l']) ),   line_loss = mean_{j<m} (lse_j - sim[j][j]),   w = 1 / (m lines),
//   dsim[i][j] = (exp(sim[i][j] - lse_j) - [i == j]) w  (i, j < m),   dcross[j][l'] = exp(cross[j][l'] - lse_j) w  (j < m, l' != own),
// and ZERO everywhere else in the padded blocks.  m <= 0: line_loss = NaN, all gradients zero.
template <typename T>
__global__ __launch_bounds__(256) void ntxent_cols_ragged_k(const float* sim, const int* count, const float* cross, float* line_loss, T* dsim,
                                                            T* dcross, int Sp, int L, int lines, int own0) {
  extern __shared__ float sh[];          // [Sp] max, [Sp] sum, [Sp] lse
  float* cmx = sh; float* csum = sh + Sp; float* clse = sh + 2 * Sp;
  __shared__ float red[4];
  const long long l = blockIdx.x;
  const int m = count[l] < Sp ? count[l] : Sp;
  const float* s = sim + l * Sp * (long long)Sp;
  const float* cr = cross ? cross + l * Sp * (long long)L : nullptr;
  T* od = dsim ? dsim + l * Sp * (long long)Sp : nullptr;
  T* oc = dcross ? dcross + l * Sp * (long long)L : nullptr;
  const int own = own0 + (int)l;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (m <= 0) {
    if (od) for (long long i = tid; i < (long long)Sp * Sp; i += 256) Elem<T>::st(od + i, 0.f);
    if (oc) for (long long i = tid; i < (long long)Sp * L; i += 256) Elem<T>::st(oc + i, 0.f);
    if (tid == 0) line_loss[l] = __builtin_nanf("");
    return;
  }
  for (int j = tid; j < m; j += 256) {
    float mx, sum;
    col_max_sumexp(s, j, m, Sp, mx, sum);
    cmx[j] = mx; csum[j] = sum;
    if (!cr) clse[j] = logf(sum) + mx;
  }
  __syncthreads();
  if (cr) {
    for (int j = wave; j < m; j += 4) {
      const float lse = row_join_lse(cr + (long long)j * L, L, own, lane, cmx[j], csum[j]);
      if (lane == 0) clse[j] = lse;
    }
    __syncthreads();
  }
  const float w = 1.0f / ((float)m * (float)lines);
  float acc = 0.f;
  for (int j = tid; j < Sp; j += 256) {
    const bool in = j < m;
    const float lse = in ? clse[j] : 0.f;
    if (in) acc += lse - s[(long long)j * Sp + j];
    if (od) {
      const int rows = in ? m : 0;
      for (int r = 0; r < rows; r++) Elem<T>::st(od + (long long)r * Sp + j, (expf(s[(long long)r * Sp + j] - lse) - (r == j ? 1.f : 0.f)) * w);
      for (int r = rows; r < Sp; r++) Elem<T>::st(od + (long long)r * Sp + j, 0.f);
    }
  }
  if (oc) {
    for (int j = wave; j < Sp; j += 4) {
      T* o = oc + (long long)j * L;
      if (j < m) {
        const float* row = cr + (long long)j * L;
        const float lse = clse[j];
        for (int c = lane; c < L; c += 64) Elem<T>::st(o + c, c == own ? 0.f : expf(row[c] - lse) * w);
      } else {
        for (int c = lane; c < L; c += 64) Elem<T>::st(o + c, 0.f);
      }
    }
  }
  acc = block_sum4(acc, red);
  if (tid == 0) line_loss[l] = acc / (float)m;
}

// pooled[l][c] = mean over the first count[l] rows of the line's compact block (f32 out; zeros for count <= 0)
template <typename T>
__global__ __launch_bounds__(256) void line_mean_ragged_k(const T* x, const int* count, float* out, int Sp, int d) {
  const long long l = blockIdx.y;
  const int c = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (c >= d) return;
  const int m = count[l] < Sp ? count[l] : Sp;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const T* p = x + l * Sp * (long long)d + c;
  for (int s = 0; s < m; s++) {
    float v[8];
    load8<T>(p + (long long)s * d, v);
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] += v[e];
  }
  const float w = m > 0 ? 1.0f / (float)m : 0.f;
#pragma unroll
  for (int e = 0; e < 8; e++) acc[e] *= w;
  store8<float>(out + l * d + c, acc);
}
// dst[(l*Sp + s)][c] += src[l][c] / count[l] for s < count[l]   (the backward of the mean)
template <typename T>
__global__ __launch_bounds__(256) void add_line_rows_ragged_k(T* dst, const float* src, const int* count, int Sp, int d) {
  const long long l = blockIdx.y;
  const int c = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (c >= d) return;
  const int m = count[l] < Sp ? count[l] : Sp;
  if (m <= 0) return;
  const float scale = 1.0f / (float)m;
  float g[8];
  load8<float>(src + l * d + c, g);
  T* p = dst + l * Sp * (long long)d + c;
  for (int s = 0; s < m; s++) {
    float v[8];
    load8<T>(p + (long long)s * d, v);
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] += scale * g[e];
    store8<T>(p + (long long)s * d, v);
  }
}

extern "C" int pero_ntxent_slots(const void* image_mask1, const void* image_mask2, const void* shift_mask1, const void* shift_mask2, int* slot1,
                                 int* slot2, int* count, int64_t lines, int64_t S, void* stream) {
  PERO_REQUIRE(image_mask1 && image_mask2 && shift_mask1 && shift_mask2 && slot1 && slot2 && count && lines > 0 && S > 0 && S <= 4096 &&
               lines < (1ll << 31), "pero_ntxent_slots: bad arguments (1 <= S <= 4096)");
  hipLaunchKernelGGL(ntxent_slots_k, dim3((unsigned)((lines + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)image_mask1,
                     (const unsigned char*)image_mask2, (const unsigned char*)shift_mask1, (const unsigned char*)shift_mask2, slot1, slot2, count,
                     (int)lines, (int)S);
  PERO_CHECK_LAUNCH("pero_ntxent_slots");
  return PERO_OK;
}
extern "C" int pero_ntxent_rows_fwd(const void* x, const int* slot, const int* count, void* xn, float* inv, int64_t lines, int64_t count_lines,
                                    int64_t S, int64_t Sp, int64_t d, int dtype, void* stream) {
  PERO_REQUIRE(x && slot && count && xn && inv && lines > 0 && count_lines > 0 && lines % count_lines == 0 && S > 0 && Sp >= S && Sp <= 4096 &&
               d > 0 && d < (1ll << 31) && lines * Sp < (1ll << 32), "pero_ntxent_rows_fwd: bad arguments (S <= Sp <= 4096, lines a multiple of count_lines)");
  dim3 grid((unsigned)((lines * Sp + 3) / 4)), block(256);
  const bool v8 = v8_ok(d, dtype, {x, xn});
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(v8, [&](auto V) {
    hipLaunchKernelGGL((ntxent_rows_fwd_k<T, decltype(V)::value>), grid, block, 0, (hipStream_t)stream, (const T*)x, slot, count, (T*)xn, inv, (long long)lines, (int)count_lines, (int)S, (int)Sp, (int)d); }); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_ntxent_rows_fwd");
  return PERO_OK;
}
extern "C" int pero_ntxent_rows_bwd(const void* xn, const void* dxn, const float* inv, const int* slot, const int* count, const float* g, void* dx,
                                    int64_t lines, int64_t count_lines, int64_t S, int64_t Sp, int64_t d, int dtype, void* stream) {
  PERO_REQUIRE(xn && dxn && inv && slot && count && dx && lines > 0 && count_lines > 0 && lines % count_lines == 0 && S > 0 && Sp >= S &&
               Sp <= 4096 && d > 0 && d < (1ll << 31) && lines * S < (1ll << 32), "pero_ntxent_rows_bwd: bad arguments (S <= Sp <= 4096, lines a multiple of count_lines)");
  dim3 grid((unsigned)((lines * S + 3) / 4)), block(256);
  const bool v8 = v8_ok(d, dtype, {xn, dxn, dx});
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(v8, [&](auto V) {
    hipLaunchKernelGGL((ntxent_rows_bwd_k<T, decltype(V)::value>), grid, block, 0, (hipStream_t)stream, (const T*)xn, (const T*)dxn, inv, slot, count, g, (T*)dx, (long long)lines, (int)count_lines, (int)S, (int)Sp, (int)d); }); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_ntxent_rows_bwd");
  return PERO_OK;
}
extern "C" int pero_ntxent_cols_ragged(const float* sim, const int* count, const float* cross, float* line_loss, float* loss_out, void* dsim,
                                       void* dcross, int64_t lines, int64_t Sp, int64_t L, int64_t own0, int dtype, void* stream) {
  PERO_REQUIRE(sim && count && line_loss && loss_out && lines > 0 && lines < (1ll << 31) && Sp > 0 && Sp <= 4096, "pero_ntxent_cols_ragged: bad arguments (Sp <= 4096)");
  PERO_REQUIRE(cross ? (L > 0 && own0 >= 0 && own0 + lines <= L) : (dcross == nullptr), "pero_ntxent_cols_ragged: cross needs 0 <= own0, own0 + lines <= L; dcross needs cross");
  hipStream_t st = (hipStream_t)stream;
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t);
    hipLaunchKernelGGL((ntxent_cols_ragged_k<T>), dim3((unsigned)lines), dim3(256), (size_t)(3 * Sp * sizeof(float)), st, sim, count, cross,
                       line_loss, (T*)dsim, (T*)dcross, (int)Sp, (int)(cross ? L : 0), (int)lines, (int)own0); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_ntxent_cols_ragged");
  return pero_sum_scale(line_loss, loss_out, lines, 1.0f / (float)lines, stream);
}
extern "C" int pero_line_mean_ragged(const void* x, const int* count, float* out, int64_t lines, int64_t Sp, int64_t d, int dtype, void* stream) {
  PERO_REQUIRE(x && count && out && lines > 0 && Sp > 0 && d > 0 && d % 8 == 0 && lines < 65536, "pero_line_mean_ragged: bad arguments (d %% 8 == 0)");
  PERO_REQUIRE(v8_ok(d, dtype, {x}) && aligned16(out), "pero_line_mean_ragged: 16-byte aligned rows");
  dim3 grid((unsigned)((d / 8 + 255) / 256), (unsigned)lines), block(256);
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t);
    hipLaunchKernelGGL((line_mean_ragged_k<T>), grid, block, 0, (hipStream_t)stream, (const T*)x, count, out, (int)Sp, (int)d); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_line_mean_ragged");
  return PERO_OK;
}
extern "C" int pero_add_line_rows_ragged(void* dst, const float* src, const int* count, int64_t lines, int64_t Sp, int64_t d, int dtype, void* stream) {
  PERO_REQUIRE(dst && src && count && lines > 0 && Sp > 0 && d > 0 && d % 8 == 0 && lines < 65536, "pero_add_line_rows_ragged: bad arguments (d %% 8 == 0)");
  PERO_REQUIRE(v8_ok(d, dtype, {dst}) && aligned16(src), "pero_add_line_rows_ragged: 16-byte aligned rows");
  dim3 grid((unsigned)((d / 8 + 255) / 256), (unsigned)lines), block(256);
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t);
    hipLaunchKernelGGL((add_line_rows_ragged_k<T>), grid, block, 0, (hipStream_t)stream, (T*)dst, src, count, (int)Sp, (int)d); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_add_line_rows_ragged");
  return PERO_OK;
}
