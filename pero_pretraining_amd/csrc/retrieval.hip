// Fused similarity top-k (evaluation of the joint-embedding pre-training: does a position of one view find its twin in the other?).
//
//   score[m][n] = (q_m . key_n) * q_scale[m] * key_scale[n];   idx[m][0..k), val[m][0..k) = the k best keys of query m,
//   higher score first, equal f32 scores: lower key index first (a strict order: the result does not depend on how the keys are visited).
//
// The (M, N) score matrix is never stored.  As in vq.hip the KEYS sit on the MFMA row index and the QUERIES on the lane index, so that a
// query's running list (KC (score, index) pairs, KC = 4 or 16 >= k) lives in one lane's registers; lists meet other lanes only at the
// end: the two lane halves by one shuffle, the four waves through LDS.  A workgroup owns 64 queries and walks the key tiles of its key
// split, 128 keys at a time, 128 bytes of depth per stage (32 f32 / 64 bf16: the LDS image is the same bytes for both, only the MFMA that
// eats a 16-byte fragment differs).  Tiles are fetched into registers one stage ahead (zero-filled past M, N and D: ragged edges are
// predication, there is no second kernel) and stored into a two-stage LDS ring with the 16-byte chunk index XORed with (row & 7).
#include "dispatch.hpp"

#define RT_BQ 64                       // queries per workgroup
#define RT_BN 128                      // keys per tile (32 per wave)
#define RT_ROWB 128                    // bytes of depth per stage and row
#define RT_KBYTES (RT_BN * RT_ROWB)    // 16 KiB
#define RT_QBYTES (RT_BQ * RT_ROWB)    // 8 KiB
#define RT_STAGE (RT_KBYTES + RT_QBYTES)
#define RT_EMPTY 0x7fffffff            // index of an unused list slot: sorts behind every key of score -inf
#define RT_MAX_SPLITS 128

// the strict order of the header: (s, n) goes in front of (t, o)
__device__ __forceinline__ bool rt_better(float s, int n, float t, int o) { return s > t || (s == t && n < o); }

template <int KC> struct RtList {
  float v[KC];
  int i[KC];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int e = 0; e < KC; e++) { v[e] = -INFINITY; i[e] = RT_EMPTY; }
  }
  // static indexing only: the candidate replaces the last entry, then bubbles up through a fixed compare-exchange chain
  __device__ __forceinline__ void insert(float s, int n) {
    if (rt_better(s, n, v[KC - 1], i[KC - 1])) {
      v[KC - 1] = s;
      i[KC - 1] = n;
#pragma unroll
      for (int e = KC - 1; e > 0; e--) {
        const bool up = rt_better(v[e], i[e], v[e - 1], i[e - 1]);
        const float hv = up ? v[e] : v[e - 1], lv = up ? v[e - 1] : v[e];
        const int hi = up ? i[e] : i[e - 1], li = up ? i[e - 1] : i[e];
        v[e - 1] = hv; v[e] = lv;
        i[e - 1] = hi; i[e] = li;
      }
    }
  }
};

// ---- the two operand loaders: one 128-byte stage of 32 keys (this wave's) x 64 queries into the two accumulators -----------------
__device__ __forceinline__ uint4 rt_frag(const unsigned char* img, int row, int j, int h5) {
  return *(const uint4*)(img + row * RT_ROWB + (((2 * j + h5) ^ (row & 7)) << 4));
}
template <typename T> struct RtOperand;
// f32: MFMA step e of fragment j multiplies depth 8j + e on lanes 0-31 and 8j + 4 + e on lanes 32-63 (vq.hip), 4 steps per 16-byte read
template <> struct RtOperand<float> {
  static __device__ __forceinline__ void mma(const unsigned char* kimg, const unsigned char* qimg, int krow, int r, int h5, f16v& acc0, f16v& acc1) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const f4v kf = __builtin_bit_cast(f4v, rt_frag(kimg, krow, j, h5));
      const f4v q0 = __builtin_bit_cast(f4v, rt_frag(qimg, r, j, h5));
      const f4v q1 = __builtin_bit_cast(f4v, rt_frag(qimg, 32 + r, j, h5));
#pragma unroll
      for (int e = 0; e < 4; e++) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], q0[e], acc0, 0, 0, 0);  // D[key][query]
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], q1[e], acc1, 0, 0, 0);
      }
    }
  }
};
// bf16: lane (r, h) holds depth 16j + 8h + 0..7 of its row: one 16-byte read is one v_mfma_f32_32x32x16_bf16 operand
template <> struct RtOperand<bf16raw> {
  static __device__ __forceinline__ void mma(const unsigned char* kimg, const unsigned char* qimg, int krow, int r, int h5, f16v& acc0, f16v& acc1) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bf8v kf = __builtin_bit_cast(bf8v, rt_frag(kimg, krow, j, h5));
      const bf8v q0 = __builtin_bit_cast(bf8v, rt_frag(qimg, r, j, h5));
      const bf8v q1 = __builtin_bit_cast(bf8v, rt_frag(qimg, 32 + r, j, h5));
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, q0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, q1, acc1, 0, 0, 0);
    }
  }
};

// one stage = (128 keys + 64 queries) x 8 chunks of 16 bytes = 6 chunks per thread; rows past the matrix and chunks past D read as zero.
// Named members, no array: the six values stay in registers across the loop's back edge.
struct RtRegs { uint4 k0, k1, k2, k3, q0, q1; };
__device__ __forceinline__ uint4 rt_chunk(const unsigned char* base, long long ld, long long row, long long rows, long long off, bool in_d) {
  // branch-free: an address inside the matrix is loaded either way (the last row, the row's first chunk) and the value masked.  A select
  // between the load and a zero constant compiles to a select of POINTERS, with the constant in private memory.
  const bool in = in_d && row < rows;
  const uint4 v = *(const uint4*)(base + (row < rows ? row : rows - 1) * ld + (in_d ? off : 0));
  const unsigned keep = in ? 0xffffffffu : 0u;
  return (uint4){v.x & keep, v.y & keep, v.z & keep, v.w & keep};
}
__device__ __forceinline__ void rt_fetch(RtRegs& g, const unsigned char* keys, long long ldk, long long n0, long long N, const unsigned char* q,
                                         long long ldq, long long m0, long long M, long long b0, long long rowbytes, int tid) {
  const long long off = b0 + (tid & 7) * 16;
  const bool in_d = off < rowbytes;
  const int row = tid >> 3;
  g.k0 = rt_chunk(keys, ldk, n0 + row, N, off, in_d);
  g.k1 = rt_chunk(keys, ldk, n0 + row + 32, N, off, in_d);
  g.k2 = rt_chunk(keys, ldk, n0 + row + 64, N, off, in_d);
  g.k3 = rt_chunk(keys, ldk, n0 + row + 96, N, off, in_d);
  g.q0 = rt_chunk(q, ldq, m0 + row, M, off, in_d);
  g.q1 = rt_chunk(q, ldq, m0 + row + 32, M, off, in_d);
}
// rows 0-127 of a stage: keys, 128-191: queries.  Rows 32 apart share (row & 7): one swizzled offset, six immediates.
__device__ __forceinline__ void rt_stash(const RtRegs& g, unsigned char* stage, int tid) {
  const int row = tid >> 3;
  unsigned char* p = stage + row * RT_ROWB + (((tid & 7) ^ (row & 7)) << 4);
  *(uint4*)(p) = g.k0;
  *(uint4*)(p + 32 * RT_ROWB) = g.k1;
  *(uint4*)(p + 64 * RT_ROWB) = g.k2;
  *(uint4*)(p + 96 * RT_ROWB) = g.k3;
  *(uint4*)(p + 128 * RT_ROWB) = g.q0;
  *(uint4*)(p + 160 * RT_ROWB) = g.q1;
}

// grid (query tiles, key splits).  splits == 1: idx / val are the result; else the split's lists go to pv / pi [split][M][k] (unused
// slots: -inf / RT_EMPTY) for sim_topk_merge_k.
template <typename T, int KC>
__global__ __launch_bounds__(256) void sim_topk_k(const unsigned char* q, const unsigned char* keys, long long ldq, long long ldk, const float* q_scale,
                                                  const float* key_scale, const unsigned char* key_valid, const int* skip, int* idx, float* val,
                                                  float* pv, int* pi, long long M, long long N, long long rowbytes, int k) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * RT_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h5 = lane >> 5, r = lane & 31;
  const long long m0 = (long long)blockIdx.x * RT_BQ;
  const int splits = gridDim.y, split = blockIdx.y;
  const long long ntiles = (N + RT_BN - 1) / RT_BN;
  const long long t0 = ntiles * split / splits, t1 = ntiles * (split + 1) / splits;   // this split's key tiles
  const int nks = (int)((rowbytes + RT_ROWB - 1) / RT_ROWB);
  const long long nstage = (t1 - t0) * nks;

  const long long mq0 = m0 + r, mq1 = m0 + 32 + r;
  const float qs0 = (q_scale && mq0 < M) ? q_scale[mq0] : 1.f, qs1 = (q_scale && mq1 < M) ? q_scale[mq1] : 1.f;
  const int sk0 = (skip && mq0 < M) ? skip[mq0] : -1, sk1 = (skip && mq1 < M) ? skip[mq1] : -1;
  RtList<KC> l0, l1;
  l0.init();
  l1.init();

  RtRegs regs;
  if (nstage > 0) {
    rt_fetch(regs, keys, ldk, t0 * RT_BN, N, q, ldq, m0, M, 0, rowbytes, tid);
    rt_stash(regs, smem, tid);
  }
  f16v acc0 = {0}, acc1 = {0};
  long long tile = t0;
  int kb = 0;
  for (long long s = 0; s < nstage; s++) {
    __syncthreads();   // stage s is complete, and every wave is done reading the other buffer (stage s - 1)
    const unsigned char* kimg = smem + (s & 1) * RT_STAGE;
    const bool more = s + 1 < nstage;
    if (more) {
      const bool wrap = kb + 1 == nks;
      rt_fetch(regs, keys, ldk, (wrap ? tile + 1 : tile) * RT_BN, N, q, ldq, m0, M, wrap ? 0 : (long long)(kb + 1) * RT_ROWB, rowbytes, tid);
    }
    RtOperand<T>::mma(kimg, kimg + RT_KBYTES, wave * 32 + r, r, h5, acc0, acc1);
    if (more) rt_stash(regs, smem + ((s + 1) & 1) * RT_STAGE, tid);
    if (++kb == nks) {   // a 128-key tile is complete: fold it into the lists, restart the sums
      const long long c0 = tile * RT_BN + wave * 32;
#pragma unroll
      for (int rr = 0; rr < 16; rr++) {
        const long long n = c0 + (rr & 3) + 8 * (rr >> 2) + 4 * h5;   // a lane visits its keys in increasing order
        if (n < N && (!key_valid || key_valid[n])) {
          const float ks = key_scale ? key_scale[n] : 1.f;
          const float s0 = acc0[rr] * qs0 * ks, s1 = acc1[rr] * qs1 * ks;
          if (s0 == s0 && (int)n != sk0) l0.insert(s0, (int)n);
          if (s1 == s1 && (int)n != sk1) l1.insert(s1, (int)n);
        }
      }
      acc0 = (f16v){0};
      acc1 = (f16v){0};
      kb = 0;
      tile++;
    }
  }

  // the two lane halves hold interleaved keys of the same queries: each takes the other's list
  {
    float ov[KC];
    int oi[KC];
#pragma unroll
    for (int e = 0; e < KC; e++) { ov[e] = __shfl_xor(l0.v[e], 32, 64); oi[e] = __shfl_xor(l0.i[e], 32, 64); }
#pragma unroll
    for (int e = 0; e < KC; e++) l0.insert(ov[e], oi[e]);
#pragma unroll
    for (int e = 0; e < KC; e++) { ov[e] = __shfl_xor(l1.v[e], 32, 64); oi[e] = __shfl_xor(l1.i[e], 32, 64); }
#pragma unroll
    for (int e = 0; e < KC; e++) l1.insert(ov[e], oi[e]);
  }
  // the four waves: [wave][entry][query] images over the staging buffers (4 * KC * 64 * 8 bytes <= 32 KiB)
  __syncthreads();
  float* mv = (float*)smem;
  int* mi = (int*)(smem + 4 * KC * RT_BQ * 4);
  if (lane < 32) {
#pragma unroll
    for (int e = 0; e < KC; e++) {
      mv[(wave * KC + e) * RT_BQ + r] = l0.v[e];       mi[(wave * KC + e) * RT_BQ + r] = l0.i[e];
      mv[(wave * KC + e) * RT_BQ + 32 + r] = l1.v[e];  mi[(wave * KC + e) * RT_BQ + 32 + r] = l1.i[e];
    }
  }
  __syncthreads();
  if (tid < RT_BQ && m0 + tid < M) {
    RtList<KC> l;
#pragma unroll
    for (int e = 0; e < KC; e++) { l.v[e] = mv[e * RT_BQ + tid]; l.i[e] = mi[e * RT_BQ + tid]; }
#pragma unroll 1
    for (int e = KC; e < 4 * KC; e++) l.insert(mv[e * RT_BQ + tid], mi[e * RT_BQ + tid]);
    const long long m = m0 + tid;
    if (splits == 1) {
#pragma unroll
      for (int e = 0; e < KC; e++)
        if (e < k) { idx[m * k + e] = l.i[e] == RT_EMPTY ? -1 : l.i[e]; val[m * k + e] = l.v[e]; }
    } else {
      const long long o = ((long long)split * M + m) * k;
#pragma unroll
      for (int e = 0; e < KC; e++)
        if (e < k) { pi[o + e] = l.i[e]; pv[o + e] = l.v[e]; }
    }
  }
}

// One wave per query: the splits' lists under the same strict order.  Lane l takes candidates l, l + 64, ... of the splits * k, then the 64
// lists meet in six shuffle rounds (after a round both partners hold the best KC of their two disjoint sets); entry e is stored by lane e.
template <int KC>
__global__ __launch_bounds__(256) void sim_topk_merge_k(const float* pv, const int* pi, int* idx, float* val, long long M, int k, int splits) {
  const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;   // the whole wave
  RtList<KC> l;
  l.init();
  const int total = splits * k;
  for (int c = lane; c < total; c += 64) {
    const int s = c / k;
    const long long o = ((long long)s * M + m) * k + (c - s * k);
    l.insert(pv[o], pi[o]);
  }
#pragma unroll 1
  for (int off = 32; off > 0; off >>= 1) {
    float ov[KC];
    int oi[KC];
#pragma unroll
    for (int e = 0; e < KC; e++) { ov[e] = __shfl_xor(l.v[e], off, 64); oi[e] = __shfl_xor(l.i[e], off, 64); }
#pragma unroll
    for (int e = 0; e < KC; e++) l.insert(ov[e], oi[e]);
  }
#pragma unroll
  for (int e = 0; e < KC; e++)
    if (lane == e && e < k) { idx[m * k + e] = l.i[e] == RT_EMPTY ? -1 : l.i[e]; val[m * k + e] = l.v[e]; }
}

// hist[0] += queries with a target, hist[1 + r] += target at rank r, hist[k + 1] += target not listed; per-workgroup counts in LDS, then
// one integer atomic per non-zero counter
__global__ __launch_bounds__(256) void retrieval_hist_k(const int* idx, const int* target, unsigned long long* hist, long long M, int k) {
  __shared__ unsigned int cnt[PERO_SIM_TOPK_MAX + 2];
  if (threadIdx.x < PERO_SIM_TOPK_MAX + 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m < M) {
    const int t = target[m];
    if (t >= 0) {
      int rank = k;
      for (int e = k - 1; e >= 0; e--)
        if (idx[m * k + e] == t) rank = e;
      atomicAdd(&cnt[0], 1u);
      atomicAdd(&cnt[1 + rank], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < k + 2 && cnt[threadIdx.x]) atomicAdd(hist + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

// inv[r] = 1 / max(|x_r|_2, 1e-12): the cosine's scales without a normalised copy of the rows.  One wave per row, 8 elements per lane
// and step (D % 8 == 0, 16-byte aligned rows), f32 sums.
template <typename T> __global__ __launch_bounds__(256) void inv_rownorm_k(const T* x, long long ld, float* inv, long long rows, int d) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float s = 0.f;
  for (int c = (threadIdx.x & 63) * 8; c < d; c += 512) {
    float v[8];
    load8<T>(x + row * ld + c, v);
#pragma unroll
    for (int e = 0; e < 8; e++) s += v[e] * v[e];
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) inv[row] = 1.0f / fmaxf(sqrtf(s), 1e-12f);
}

// Key splits chosen for key_splits = 0: enough workgroups for two per CU of a 256-CU device (512) where the query tiles alone do not give
// them, at most one split per 128-key tile and at most RT_MAX_SPLITS.  A function of (M, N) alone: no device query.
extern "C" int pero_sim_topk_key_splits(int64_t M, int64_t N) {
  if (M < 1 || N < 1) return 1;
  const int64_t qt = (M + RT_BQ - 1) / RT_BQ, kt = (N + RT_BN - 1) / RT_BN;
  int64_t s = (512 + qt - 1) / qt;
  if (s > kt) s = kt;
  if (s > RT_MAX_SPLITS) s = RT_MAX_SPLITS;
  return (int)(s < 1 ? 1 : s);
}

template <typename T, int KC>
static void rt_launch(const void* q, const void* keys, int64_t ldq, int64_t ldk, const float* q_scale, const float* key_scale, const unsigned char* key_valid,
                      const int* skip, int* idx, float* val, void* work, int64_t M, int64_t N, int64_t D, int k, int splits, hipStream_t st) {
  float* pv = (float*)work;
  int* pi = (int*)work + (size_t)splits * M * k;
  hipLaunchKernelGGL((sim_topk_k<T, KC>), dim3((unsigned)((M + RT_BQ - 1) / RT_BQ), (unsigned)splits), dim3(256), 0, st, (const unsigned char*)q,
                     (const unsigned char*)keys, (long long)(ldq * sizeof(T)), (long long)(ldk * sizeof(T)), q_scale, key_scale, key_valid, skip, idx, val, pv,
                     pi, (long long)M, (long long)N, (long long)(D * sizeof(T)), k);
  if (splits > 1)
    hipLaunchKernelGGL((sim_topk_merge_k<KC>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, pv, pi, idx, val, (long long)M, k, splits);
}

extern "C" int pero_sim_topk(const void* q, int64_t ldq, const void* keys, int64_t ldk, const float* q_scale, const float* key_scale,
                             const unsigned char* key_valid, const int32_t* skip, int32_t* idx, float* val, void* work, int64_t M, int64_t N, int64_t D,
                             int32_t k, int32_t key_splits, int dtype, void* stream) {
  PERO_REQUIRE(q && keys && idx && val, "pero_sim_topk: null pointer");
  PERO_REQUIRE(dtype == PERO_F32 || dtype == PERO_BF16, "pero_sim_topk: dtype must be PERO_F32 or PERO_BF16");
  PERO_REQUIRE(k >= 1 && k <= PERO_SIM_TOPK_MAX, "pero_sim_topk: k = %d outside [1, %d]", (int)k, PERO_SIM_TOPK_MAX);
  PERO_REQUIRE(M >= 1 && N >= 1 && D >= 8 && M < 2147483647LL && N < 2147483647LL && D < 2147483647LL, "pero_sim_topk: bad sizes");
  PERO_REQUIRE(D % 8 == 0, "pero_sim_topk: D = %lld is not a multiple of 8", (long long)D);
  const int64_t es = dtype == PERO_F32 ? 4 : 2;
  PERO_REQUIRE(ldq >= D && ldk >= D && (ldq * es) % 16 == 0 && (ldk * es) % 16 == 0 && aligned16(q) && aligned16(keys),
               "pero_sim_topk: rows of q and keys must be 16-byte aligned (base pointer and pitch), pitch >= D");
  PERO_REQUIRE(key_splits >= 0 && key_splits <= RT_MAX_SPLITS, "pero_sim_topk: key_splits = %d outside [0, %d]", (int)key_splits, RT_MAX_SPLITS);
  const int splits = key_splits == 0 ? pero_sim_topk_key_splits(M, N) : (int)key_splits;
  PERO_REQUIRE(splits == 1 || work, "pero_sim_topk: %d key splits need the work buffer", splits);
  hipStream_t st = (hipStream_t)stream;
  with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(k <= 4, [&](auto small) {
    rt_launch<T, decltype(small)::value ? 4 : 16>(q, keys, ldq, ldk, q_scale, key_scale, key_valid, skip, idx, val, work, M, N, D, k, splits, st); }); });
  PERO_CHECK_LAUNCH("pero_sim_topk");
  return PERO_OK;
}

extern "C" int pero_retrieval_hist(const int32_t* idx, const int32_t* target, uint64_t* hist, int64_t M, int32_t k, void* stream) {
  PERO_REQUIRE(idx && target && hist, "pero_retrieval_hist: null pointer");
  PERO_REQUIRE(k >= 1 && k <= PERO_SIM_TOPK_MAX, "pero_retrieval_hist: k = %d outside [1, %d]", (int)k, PERO_SIM_TOPK_MAX);
  PERO_REQUIRE(M >= 0 && M < 2147483647LL, "pero_retrieval_hist: bad M");
  if (M == 0) return PERO_OK;
  hipLaunchKernelGGL(retrieval_hist_k, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx, target, (unsigned long long*)hist,
                     (long long)M, (int)k);
  PERO_CHECK_LAUNCH("pero_retrieval_hist");
  return PERO_OK;
}

extern "C" int pero_inv_rownorm(const void* x, int64_t ld, float* inv, int64_t rows, int64_t D, int dtype, void* stream) {
  PERO_REQUIRE(x && inv, "pero_inv_rownorm: null pointer");
  PERO_REQUIRE(dtype == PERO_F32 || dtype == PERO_BF16, "pero_inv_rownorm: dtype must be PERO_F32 or PERO_BF16");
  PERO_REQUIRE(rows >= 1 && D >= 8 && D % 8 == 0 && D < 2147483647LL, "pero_inv_rownorm: rows >= 1 and D %% 8 == 0 required");
  const int64_t es = dtype == PERO_F32 ? 4 : 2;
  PERO_REQUIRE(ld >= D && (ld * es) % 16 == 0 && aligned16(x), "pero_inv_rownorm: rows must be 16-byte aligned (base pointer and pitch), pitch >= D");
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  with_elem(dtype, [&](auto t) { using T = decltype(t);
    hipLaunchKernelGGL((inv_rownorm_k<T>), grid, block, 0, (hipStream_t)stream, (const T*)x, (long long)ld, inv, (long long)rows, (int)D); });
  PERO_CHECK_LAUNCH("pero_inv_rownorm");
  return PERO_OK;
}
