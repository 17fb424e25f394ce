// The tokenizer's VGG front end (models/autoencoders.py VGGEncoder): 3x3 convolution as an implicit GEMM, image
// ingestion and max pooling, all on activations kept NHWC with a one-pixel zero halo: (N, H + 2, W + 2, C), read as R = N (H + 2)(W + 2)
// rows of C values.  Output row r of the convolution is  sum over the nine taps of  Xp[r + (ky - 1)(W + 2) + (kx - 1)] . Wt[:, ky, kx, :]^T
// - a R x Cout x 9 Cin product whose A-row base moves by a constant per tap; the im2col matrix exists nowhere.  Halo rows of the output
// are written as zeros, so the next layer finds its padding in place.  Loads are guarded (a row index is clamped into [0, R - 1]; such a row
// only ever feeds a halo row or a row past R, whose results are not stored), so no access leaves the caller's buffers and no slack is needed.
// No atomics; every output element is one fixed-order sum: a second run gives the same bits.
#include "dispatch.hpp"

// activation of pero_conv3x3's epilogue
__device__ __forceinline__ float conv_act(float v, int act, float slope) {
  if (act == PERO_CONV_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == PERO_CONV_ACT_LEAKY_RELU) return v > 0.f ? v : v * slope;
  return v;
}

__device__ __forceinline__ bool halo_interior(long long r, int Hp, int Wp) {
  const int xx = (int)(r % Wp), yy = (int)((r / Wp) % Hp);
  return xx >= 1 && xx <= Wp - 2 && yy >= 1 && yy <= Hp - 2;
}

// --------------------------------------------------------------------------------------------
// Direct form: one thread per (row, output channel), channel fastest; exact f32 FMA.  Each tap's Cin products are summed on their own, the
// nine partial sums are then added in tap order and the bias last.  For the channel counts the tile kernel does not take (Cin not a
// multiple of 8 in bf16, of 4 in f32, e.g. an unpadded first layer); it has no speed target.  An interior row's nine neighbours all lie
// inside its own padded image, so these loads need no guard.
// --------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void conv3x3_direct_k(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ y,
                                                        long long R, int Hp, int Wp, int Cin, int Cout, int act, float slope) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long r = gid / Cout;
  const int co = (int)(gid % Cout);
  if (r >= R) return;
  float out = 0.f;
  if (halo_interior(r, Hp, Wp)) {
    float total = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
      const T* xr = x + (r + (long long)(tap / 3 - 1) * Wp + (tap % 3 - 1)) * Cin;
      const T* wr = w + ((long long)co * 9 + tap) * Cin;
      float s = 0.f;
      for (int c = 0; c < Cin; c++) s = fmaf(Elem<T>::ld(xr + c), Elem<T>::ld(wr + c), s);
      total += s;
    }
    out = conv_act(total + (bias ? bias[co] : 0.f), act, slope);
  }
  Elem<T>::st(y + r * Cout + co, out);
}

// --------------------------------------------------------------------------------------------
// Implicit GEMM on the matrix pipe: v_mfma_f32_32x32x16_bf16 (bf16) or v_mfma_f32_32x32x2_f32 (f32: exact f32 products and sums).
// Workgroup = 4 waves = a tile of BM = WR * TM * 32 rows x BN = (4 / WR) * TN * 32 output channels; a wave owns TM x TN accumulators of
// 32 x 32.  K = 9 Cin is walked in 16-byte groups of EPG channels (8 bf16 / 4 f32; Cin % EPG == 0), group kg = (tap, channel group) in the
// order of the packed weight's row, so that row is read contiguously and small channel counts waste no MFMA; a chunk is 32 k-values.  A
// chunk of A (BM rows, each moved by its group's tap constant) and of the weight (BN rows) goes global -> registers -> LDS, the next chunk's
// global loads are in flight under the current chunk's MFMAs.  The weight is the MFMA's A operand and the activation its B operand, so a
// lane's 16 results are 4 x 4 consecutive output channels of ONE row.  f32: a lane's 16-byte LDS read holds k = 8 j + 4 h + 0..3 for both
// operands and feeds four MFMAs (the k order inside a chunk is permuted the same way on both sides), and the accumulator is folded into a
// second one after every max(1, Cin / 32) chunks - one tap at the production widths - so that no chain of additions is longer than a tap.
// --------------------------------------------------------------------------------------------
#define CONV_KC 32

template <typename T> struct ConvElem;
template <> struct ConvElem<bf16raw> { static constexpr int EPG = 8, PITCH = CONV_KC + 8; };    // 80-byte LDS rows
template <> struct ConvElem<float> { static constexpr int EPG = 4, PITCH = CONV_KC + 4; };      // 144-byte LDS rows

template <typename T, int WR, int TM, int TN>
__global__ __launch_bounds__(256) void conv3x3_mfma_k(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias,
                                                      T* __restrict__ y, long long R, int Hp, int Wp, int Cin, int Cout, int n_col_tiles,
                                                      int act, float slope) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int EPG = ConvElem<T>::EPG, PITCH = ConvElem<T>::PITCH, GPC = CONV_KC / EPG, RP = 256 / GPC;
  constexpr int WC = 4 / WR, BM = WR * TM * 32, BN = WC * TN * 32;
  constexpr int LA = BM / RP, LB = BN / RP;   // 16-byte loads per thread and chunk
  __shared__ __attribute__((aligned(16))) T sA[BM * PITCH];
  __shared__ __attribute__((aligned(16))) T sB[BN * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const int ct = blockIdx.x % n_col_tiles;
  const long long r0 = (long long)(blockIdx.x / n_col_tiles) * BM;
  const int n0 = ct * BN;
  const int g = tid % GPC, li = tid / GPC;       // this thread's 16-byte group of a chunk, and its row within RP
  const int cgroups = Cin / EPG, G = 9 * cgroups, KT = (G + GPC - 1) / GPC;
  const int fold = Cin / CONV_KC > 1 ? Cin / CONV_KC : 1;

  f16v acc[TM][TN], sum[F32 ? TM : 1][F32 ? TN : 1];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        acc[i][j][e] = 0.f;
        if constexpr (F32) sum[i][j][e] = 0.f;
      }

  uint4 ra[LA], rb[LB];
  auto fetch = [&](int kt) {
    const int kg = kt * GPC + g;
    const bool k_ok = kg < G;
    const int tap = kg / cgroups, c = (kg - tap * cgroups) * EPG;
    const long long off = (long long)(tap / 3 - 1) * Wp + (tap % 3 - 1);
#pragma unroll
    for (int u = 0; u < LA; u++) {
      long long rr = r0 + li + RP * u + off;
      rr = rr < 0 ? 0 : (rr > R - 1 ? R - 1 : rr);
      ra[u] = k_ok ? *(const uint4*)(x + rr * Cin + c) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < LB; u++) {
      const int co = n0 + li + RP * u;
      rb[u] = (k_ok && co < Cout) ? *(const uint4*)(w + (long long)co * 9 * Cin + (long long)kg * EPG) : make_uint4(0u, 0u, 0u, 0u);
    }
  };

  fetch(0);
  for (int kt = 0; kt < KT; kt++) {
#pragma unroll
    for (int u = 0; u < LA; u++) *(uint4*)(sA + (li + RP * u) * PITCH + EPG * g) = ra[u];
#pragma unroll
    for (int u = 0; u < LB; u++) *(uint4*)(sB + (li + RP * u) * PITCH + EPG * g) = rb[u];
    __syncthreads();
    if (kt + 1 < KT) fetch(kt + 1);
    if constexpr (F32) {
#pragma unroll
      for (int ks = 0; ks < CONV_KC / 8; ks++) {
        const int k = ks * 8 + 4 * (lane >> 5);
        f4v fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; i++) fa[i] = *(const f4v*)(sA + ((wr * TM + i) * 32 + (lane & 31)) * PITCH + k);
#pragma unroll
        for (int j = 0; j < TN; j++) fb[j] = *(const f4v*)(sB + ((wc * TN + j) * 32 + (lane & 31)) * PITCH + k);
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
          for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[j][q], fa[i][q], acc[i][j], 0, 0, 0);
      }
      if ((kt + 1) % fold == 0 || kt + 1 == KT) {
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
          for (int j = 0; j < TN; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) { sum[i][j][e] += acc[i][j][e]; acc[i][j][e] = 0.f; }
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < CONV_KC / 16; ks++) {
        const int k = ks * 16 + 8 * (lane >> 5);
        bf8v fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; i++) fa[i] = *(const bf8v*)(sA + ((wr * TM + i) * 32 + (lane & 31)) * PITCH + k);
#pragma unroll
        for (int j = 0; j < TN; j++) fb[j] = *(const bf8v*)(sB + ((wc * TN + j) * 32 + (lane & 31)) * PITCH + k);
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
          for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // D[channel][row]: the lane's column is its row of the tile, register 4 q + e is channel 8 q + 4 (lane >> 5) + e of the 32
  const bool vec = (Cout & 3) == 0;
#pragma unroll
  for (int i = 0; i < TM; i++) {
    const long long r = r0 + (wr * TM + i) * 32 + (lane & 31);
    if (r >= R) continue;
    const bool inside = halo_interior(r, Hp, Wp);
    T* yr = y + r * Cout;
#pragma unroll
    for (int j = 0; j < TN; j++) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int co = n0 + (wc * TN + j) * 32 + 8 * q + 4 * (lane >> 5);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const float a = F32 ? sum[F32 ? i : 0][F32 ? j : 0][4 * q + e] : acc[i][j][4 * q + e];
          v[e] = (inside && co + e < Cout) ? conv_act(a + (bias ? bias[co + e] : 0.f), act, slope) : 0.f;
        }
        if (vec) {
          if (co < Cout) {
            if constexpr (F32) *(f4v*)(yr + co) = (f4v){v[0], v[1], v[2], v[3]};
            else *(uint2*)(yr + co) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++)
            if (co + e < Cout) Elem<T>::st(yr + co + e, v[e]);
        }
      }
    }
  }
}

// --------------------------------------------------------------------------------------------
// Image ingestion: one thread per pixel of the halo layout; every element of dst is written (halo pixels and the channels C .. Cp - 1 that
// pad a pixel to Cp values: zeros).  VEC: Cp values are 16 bytes (8 bf16 / 4 f32), one store per pixel.
// SRC 0: uint8 (N, H, W, C), value / 255 - looked up in a table of the 256 quotients, each the f64 quotient rounded once to f32 (what
//        `batch / 255.` followed by `.float()` gives on the host).  SRC 1: f32 (N, C, H, W), copied as it is.
// --------------------------------------------------------------------------------------------
template <typename T, int SRC, bool VEC>
__global__ __launch_bounds__(256) void image_to_halo_k(const void* __restrict__ src, T* __restrict__ dst, long long R, int H, int W, int C, int Cp) {
  __shared__ float lut[256];
  if (SRC == 0) {
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
    __syncthreads();
  }
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const int Wp = W + 2, Hp = H + 2;
  const int xx = (int)(r % Wp), yy = (int)((r / Wp) % Hp);
  const long long n = r / ((long long)Wp * Hp);
  const bool inside = xx >= 1 && xx <= W && yy >= 1 && yy <= H;
  T* o = dst + r * Cp;
  auto value = [&](int c) -> float {
    if (!inside || c >= C) return 0.f;
    if (SRC == 0) return lut[((const unsigned char*)src)[((n * H + (yy - 1)) * W + (xx - 1)) * C + c]];
    return ((const float*)src)[((n * C + c) * H + (yy - 1)) * W + (xx - 1)];
  };
  if (VEC) {
    constexpr int E = 16 / sizeof(T);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < E; c++) v[c] = value(c);
    if constexpr (sizeof(T) == 4) *(f4v*)o = (f4v){v[0], v[1], v[2], v[3]};
    else store8<T>(o, v);
  } else {
    for (int c = 0; c < Cp; c++) Elem<T>::st(o + c, value(c));
  }
}

// --------------------------------------------------------------------------------------------
// Max pooling, kernel = stride = (ph, pw), of the interior of a halo-layout activation, then y = max * a[c] + b[c] where a is given.
// One thread per (output pixel, group of 8 channels), group fastest: 16-byte accesses when C % 8 == 0 (V8), element by element otherwise.
// TOK 0: output in halo layout (N, H / ph + 2, W / pw + 2, C), halo pixels zeros.   TOK 1: token rows (N * W / pw, (H / ph) * C):
// row n * Wo + xo holds the column's Ho pixels top to bottom, C channels each.
// --------------------------------------------------------------------------------------------
template <typename T, bool V8, int TOK>
__global__ __launch_bounds__(256) void maxpool_k(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ a, const float* __restrict__ b,
                                                 long long total, int H, int W, int C, int ph, int pw) {
  const int groups = (C + 7) / 8, Ho = H / ph, Wo = W / pw;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int col = (int)(gid % groups) * 8;
  const long long p = gid / groups;
  long long n;
  int yo, xo;          // output pixel, interior coordinates
  bool inside = true;
  T* o;
  if (TOK) {
    yo = (int)(p % Ho);
    xo = (int)((p / Ho) % Wo);
    n = p / ((long long)Ho * Wo);
    o = y + ((n * Wo + xo) * Ho + yo) * (long long)C;
  } else {
    const int xx = (int)(p % (Wo + 2)), yy = (int)((p / (Wo + 2)) % (Ho + 2));
    n = p / ((long long)(Wo + 2) * (Ho + 2));
    inside = xx >= 1 && xx <= Wo && yy >= 1 && yy <= Ho;
    xo = xx - 1; yo = yy - 1;
    o = y + p * C;
  }
  float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (inside) {
    for (int dy = 0; dy < ph; dy++)
      for (int dx = 0; dx < pw; dx++) {
        const T* src = x + ((n * (H + 2) + (yo * ph + dy + 1)) * (W + 2) + (xo * pw + dx + 1)) * (long long)C;
        float v[8];
        if (V8) load8<T>(src + col, v);
        else {
#pragma unroll
          for (int e = 0; e < 8; e++) v[e] = col + e < C ? Elem<T>::ld(src + col + e) : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; e++) m[e] = (dy == 0 && dx == 0) ? v[e] : fmaxf(m[e], v[e]);
      }
    if (a) {
#pragma unroll
      for (int e = 0; e < 8; e++)
        if (col + e < C) m[e] = m[e] * a[col + e] + b[col + e];
    }
  }
  if (V8) store8<T>(o + col, m);
  else {
#pragma unroll
    for (int e = 0; e < 8; e++)
      if (col + e < C) Elem<T>::st(o + col + e, m[e]);
  }
}

// host side ------------------------------------------------------------------------------------
static inline bool conv_dims_ok(int64_t N, int64_t H, int64_t W, int64_t C) {
  return N > 0 && H > 0 && W > 0 && C > 0 && H < (1ll << 30) && W < (1ll << 30) && C < (1ll << 30) && N < (1ll << 40) &&
         (double)N * (double)(H + 2) * (double)(W + 2) * (double)C < 9.0e18;
}

template <typename T>
static int conv3x3_tiles(const void* x, const void* w, const float* bias, void* y, long long R, int Hp, int Wp, int Cin, int Cout, int act, float slope,
                         hipStream_t st) {
  if (Cout <= 64) {
    const long long blocks = (R + 127) / 128;
    PERO_REQUIRE(blocks < (1ll << 31), "pero_conv3x3: too many row tiles");
    hipLaunchKernelGGL((conv3x3_mfma_k<T, 4, 1, 2>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, (const T*)w, bias, (T*)y, R, Hp, Wp, Cin, Cout, 1,
                       act, slope);
  } else {
    const long long nct = (Cout + 127) / 128, blocks = ((R + 127) / 128) * nct;
    PERO_REQUIRE(blocks < (1ll << 31), "pero_conv3x3: too many tiles");
    hipLaunchKernelGGL((conv3x3_mfma_k<T, 2, 2, 2>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, (const T*)w, bias, (T*)y, R, Hp, Wp, Cin, Cout,
                       (int)nct, act, slope);
  }
  return PERO_OK;
}

extern "C" int pero_conv3x3(const void* x, const void* w, const float* bias, void* y, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                            int act, float slope, int dtype, void* stream) {
  PERO_REQUIRE(x && w && y, "pero_conv3x3: null pointer");
  PERO_REQUIRE(dtype == PERO_F32 || dtype == PERO_BF16, "pero_conv3x3: bad dtype %d", dtype);
  PERO_REQUIRE(conv_dims_ok(N, H, W, Cin) && conv_dims_ok(N, H, W, Cout), "pero_conv3x3: bad shape N %lld H %lld W %lld Cin %lld Cout %lld",
               (long long)N, (long long)H, (long long)W, (long long)Cin, (long long)Cout);
  PERO_REQUIRE(act == PERO_CONV_ACT_NONE || act == PERO_CONV_ACT_RELU || act == PERO_CONV_ACT_LEAKY_RELU, "pero_conv3x3: bad activation %d", act);
  PERO_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y) && (((uintptr_t)bias) & 3) == 0, "pero_conv3x3: x, w, y must be 16-byte aligned (bias: 4)");
  PERO_REQUIRE(x != y, "pero_conv3x3: the output may not be the input");
  const long long R = (long long)N * (H + 2) * (W + 2);
  const int Hp = (int)H + 2, Wp = (int)W + 2;
  hipStream_t st = (hipStream_t)stream;
  if (Cin % (dtype == PERO_BF16 ? 8 : 4) == 0) {
    int rc = PERO_OK;
    with_elem(dtype, [&](auto t) { rc = conv3x3_tiles<decltype(t)>(x, w, bias, y, R, Hp, Wp, (int)Cin, (int)Cout, act, slope, st); });
    if (rc != PERO_OK) return rc;
  } else {
    const double threads = (double)R * (double)Cout;
    PERO_REQUIRE(threads / 256.0 < 2147483647.0, "pero_conv3x3: too many outputs for one launch");
    const unsigned blocks = (unsigned)((R * Cout + 255) / 256);
    with_elem(dtype, [&](auto t) { using T = decltype(t);
      hipLaunchKernelGGL((conv3x3_direct_k<T>), dim3(blocks), dim3(256), 0, st, (const T*)x, (const T*)w, bias, (T*)y, R, Hp, Wp, (int)Cin, (int)Cout, act, slope); });
  }
  PERO_CHECK_LAUNCH("pero_conv3x3");
  return PERO_OK;
}

extern "C" int pero_image_to_halo(const void* src, void* dst, int64_t N, int64_t H, int64_t W, int64_t C, int64_t C_pad, int src_kind, int dtype,
                                  void* stream) {
  PERO_REQUIRE(src && dst, "pero_image_to_halo: null pointer");
  PERO_REQUIRE(dtype == PERO_F32 || dtype == PERO_BF16, "pero_image_to_halo: bad dtype %d", dtype);
  PERO_REQUIRE(src_kind == PERO_IMAGE_U8_NHWC || src_kind == PERO_IMAGE_F32_NCHW, "pero_image_to_halo: bad source kind %d", src_kind);
  PERO_REQUIRE(conv_dims_ok(N, H, W, C) && C_pad >= C && conv_dims_ok(N, H, W, C_pad), "pero_image_to_halo: bad shape N %lld H %lld W %lld C %lld C_pad %lld",
               (long long)N, (long long)H, (long long)W, (long long)C, (long long)C_pad);
  PERO_REQUIRE(src_kind == PERO_IMAGE_U8_NHWC || (((uintptr_t)src) & 3) == 0, "pero_image_to_halo: misaligned f32 source");
  PERO_REQUIRE((((uintptr_t)dst) & (dtype == PERO_F32 ? 3 : 1)) == 0, "pero_image_to_halo: misaligned destination");
  const long long R = (long long)N * (H + 2) * (W + 2);
  PERO_REQUIRE((R + 255) / 256 < (1ll << 31), "pero_image_to_halo: too many pixels for one launch");
  const dim3 grid((unsigned)((R + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = C_pad * (dtype == PERO_F32 ? 4 : 2) == 16 && aligned16(dst);
  with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(src_kind == PERO_IMAGE_F32_NCHW, [&](auto S) { with_flag(vec, [&](auto V) {
    hipLaunchKernelGGL((image_to_halo_k<T, decltype(S)::value, decltype(V)::value>), grid, block, 0, st, src, (T*)dst, R, (int)H, (int)W, (int)C, (int)C_pad); }); }); });
  PERO_CHECK_LAUNCH("pero_image_to_halo");
  return PERO_OK;
}

extern "C" int pero_maxpool_nhwc(const void* x, void* y, const float* a, const float* b, int64_t N, int64_t H, int64_t W, int64_t C, int ph, int pw,
                                 int token_rows, int dtype, void* stream) {
  PERO_REQUIRE(x && y, "pero_maxpool_nhwc: null pointer");
  PERO_REQUIRE((a == nullptr) == (b == nullptr), "pero_maxpool_nhwc: the affine needs both a and b");
  PERO_REQUIRE(dtype == PERO_F32 || dtype == PERO_BF16, "pero_maxpool_nhwc: bad dtype %d", dtype);
  PERO_REQUIRE(conv_dims_ok(N, H, W, C), "pero_maxpool_nhwc: bad shape N %lld H %lld W %lld C %lld", (long long)N, (long long)H, (long long)W, (long long)C);
  PERO_REQUIRE((ph == 1 || ph == 2) && (pw == 1 || pw == 2), "pero_maxpool_nhwc: pool (%d, %d) is not one of (1|2, 1|2)", ph, pw);
  PERO_REQUIRE(H % ph == 0 && W % pw == 0, "pero_maxpool_nhwc: H %lld, W %lld not divisible by the pool (%d, %d)", (long long)H, (long long)W, ph, pw);
  PERO_REQUIRE(x != y, "pero_maxpool_nhwc: the output may not be the input");
  const int esz = dtype == PERO_F32 ? 4 : 2;
  PERO_REQUIRE((((uintptr_t)x) & (esz - 1)) == 0 && (((uintptr_t)y) & (esz - 1)) == 0 && (((uintptr_t)a) & 3) == 0 && (((uintptr_t)b) & 3) == 0,
               "pero_maxpool_nhwc: misaligned pointer");
  const long long Ho = H / ph, Wo = W / pw, groups = (C + 7) / 8;
  const long long pixels = token_rows ? (long long)N * Ho * Wo : (long long)N * (Ho + 2) * (Wo + 2);
  const long long total = pixels * groups;
  PERO_REQUIRE((total + 255) / 256 < (1ll << 31), "pero_maxpool_nhwc: too many outputs for one launch");
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const bool v8 = v8_ok(C, dtype, {x, y});
  with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(v8, [&](auto V) { with_flag(token_rows != 0, [&](auto K) {
    hipLaunchKernelGGL((maxpool_k<T, decltype(V)::value, decltype(K)::value>), grid, block, 0, st, (const T*)x, (T*)y, a, b, total, (int)H, (int)W, (int)C, ph, pw); }); }); });
  PERO_CHECK_LAUNCH("pero_maxpool_nhwc");
  return PERO_OK;
}
