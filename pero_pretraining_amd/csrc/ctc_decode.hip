// Evaluation of a recogniser on the device: CTC prefix beam search and batched edit distance.  Contract: include/pero_hip.h; derivation,
// trie and tie rule: DESIGN.md "CTC decoding".
//
//   pero_ctc_beam      ctc_beam_top_k  one wave per logit row t < T: row_lse (ctc_wave_row_lse, the function of ctc_row_lse_k) and the
//                                      K = min(W + 1, C - 1) best non-blank classes of the row with their log-probabilities (all rows in
//                                      parallel)
//                      ctc_beam_k      one workgroup per line, frame by frame: the <= W (K + 1) candidates of the frame are scored by the
//                                      threads, ranked by counting, the kept ones find or create their prefix node; five barriers per frame
//   pero_edit_distance edit_distance_k one workgroup per pair: the anti-diagonals of the unit-cost table out of LDS, one barrier each
//
// Why K = W + 1 classes are enough: the extensions of one beam entry j score logp(c) + tot_j, except c = last_j, which scores logp(c) + pb_j
// <= logp(c) + tot_j.  A class outside the row's best W + 1 is beaten, for the same j, by at least W extensions (or by the stay candidates
// they merged into, whose totals are no smaller), so it is never among the frame's best W.
#include "ctc_common.hpp"

#define BEAM_MAX_W 32
#define BEAM_MAX_K (BEAM_MAX_W + 1)
#define BEAM_MAX_Q (BEAM_MAX_W * (BEAM_MAX_K + 1))                      // stay + extension candidates of one frame
#define BEAM_QPT ((BEAM_MAX_Q + CTC_THREADS - 1) / CTC_THREADS)         // candidates of one thread
#define EDIT_THREADS 256
#define EDIT_MAX_L 512

// A candidate's sort key: the larger key ranks first.  High word: the total's bits made monotone (a float order is an unsigned order after
// flipping the sign bit of a non-negative value and every bit of a negative one; -0 counts as +0); low word: ~q, so that equal totals rank by
// candidate index and no two keys are equal.  0 = no candidate (a total of -inf, or a string merged into another candidate).
static __device__ __forceinline__ unsigned long long beam_key(float total, int q) {
  if (total == CTC_NEG_INF) return 0;
  const unsigned u = __float_as_uint(total + 0.f);
  return ((unsigned long long)(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u)) << 32) | (unsigned)~q;
}

// Number of hash slots of a line: the smallest power of two >= 2 S W, so that the S W nodes a line can create fill at most half of it.
static inline int64_t beam_hash_slots(int64_t S, int64_t W) {
  int64_t h = 1;
  while (h < 2 * S * W) h <<= 1;
  return h;
}

template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_beam_top_k(const T* __restrict__ logits, const int64_t* __restrict__ input_lengths,
                                                               float* __restrict__ row_lse, float* __restrict__ top_logp,
                                                               int32_t* __restrict__ top_class, long long rows, int S, int C, int blank, int K) {
  const long long row = (long long)blockIdx.x * (CTC_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  if ((int)(row % S) >= ctc_clamp_len(input_lengths[row / S], S)) return;   // a row behind the line's frames is never read
  const int lane = threadIdx.x & 63;
  const T* x = logits + row * C;
  const float lse = ctc_wave_row_lse(x, C, lane);
  if (lane == 0) row_lse[row] = lse;
  // K rounds of "the best non-blank class behind the previous winner" in the order (logit descending, class ascending)
  float px = __builtin_huge_valf();
  int pc = -1;
  for (int r = 0; r < K; r++) {
    float best = CTC_NEG_INF;
    int at = C;   // no candidate yet
    for (int c = lane; c < C; c += 64) {
      if (c == blank) continue;
      const float v = Elem<T>::ld(x + c);
      const bool behind = v < px || (v == px && c > pc);
      if (behind && (at == C || v > best)) { best = v; at = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oa = __shfl_xor(at, o, 64);
      if (oa < C && (at == C || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    if (lane == 0) {   // at == C only for a row with NaNs: a valid class with probability 0, so that nothing downstream indexes out of range
      top_class[row * K + r] = at < C ? at : (blank == 0 ? 1 : 0);
      top_logp[row * K + r] = at < C ? ctc_logp(best, lse) : CTC_NEG_INF;
    }
    px = best;
    pc = at;
  }
}

// The line's hash of prefix nodes, open addressing with linear probing: a slot is 0 (free) or ((parent * CTC_MAX_C + label + 1) << 32) | node.
// Every access is an atomic at device scope, so no read is served from a stale line of the CU's vector cache.
static __device__ __forceinline__ unsigned beam_hash_of(unsigned key) {
  unsigned h = key * 2654435761u;
  return h ^ (h >> 15);
}
static __device__ __forceinline__ int beam_hash_find(unsigned long long* hs, int H, unsigned key) {
  for (unsigned s = beam_hash_of(key) & (H - 1);; s = (s + 1) & (H - 1)) {
    const unsigned long long v = __hip_atomic_load(hs + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == 0) return 0;
    if ((unsigned)(v >> 32) == key + 1) return (int)(unsigned)v;
  }
}
static __device__ __forceinline__ void beam_hash_insert(unsigned long long* hs, int H, unsigned key, int node) {
  const unsigned long long mine = ((unsigned long long)(key + 1) << 32) | (unsigned)node;
  for (unsigned s = beam_hash_of(key) & (H - 1);; s = (s + 1) & (H - 1)) {
    unsigned long long expected = 0;
    if (__hip_atomic_compare_exchange_strong(hs + s, &expected, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
}

// One beam entry: the prefix's node, its parent node and last label (-1 for the empty prefix), its length, pb and pnb.  Two copies in ping-pong.
struct BeamLds {
  int node[2][BEAM_MAX_W], parent[2][BEAM_MAX_W], last[2][BEAM_MAX_W], len[2][BEAM_MAX_W];
  float pb[2][BEAM_MAX_W], pnb[2][BEAM_MAX_W];
  float tot[BEAM_MAX_W], lpe[BEAM_MAX_W], stay_pb[BEAM_MAX_W], stay_pnb[BEAM_MAX_W];
  int pslot[BEAM_MAX_W];   // the beam slot of the entry's parent prefix, -1 if that prefix is not in the beam
  alignas(16) unsigned long long key[BEAM_MAX_Q];   // the candidates' sort keys (beam_key), read two at a time by the ranking loop
  int top_class[BEAM_MAX_K];             // the frame's best classes and their log-probabilities
  float top_logp[BEAM_MAX_K];
  int count[2], nodes;
};

template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_beam_k(const T* __restrict__ logits, const int64_t* __restrict__ input_lengths,
                                                           const float* __restrict__ row_lse, const float* __restrict__ top_logp,
                                                           const int32_t* __restrict__ top_class, unsigned long long* __restrict__ hash,
                                                           int64_t* __restrict__ out, int64_t* __restrict__ out_lengths, float* __restrict__ out_scores,
                                                           int64_t* __restrict__ out_count, int32_t* __restrict__ node_parent,
                                                           int32_t* __restrict__ node_label, int32_t* __restrict__ node_count,
                                                           int32_t* __restrict__ beam_node, float* __restrict__ beam_score, int S, int C, int blank,
                                                           int W, int K, int H) {
  __shared__ BeamLds b;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int Tn = ctc_clamp_len(input_lengths[n], S);
  const T* x = logits + (long long)n * S * C;
  const float* lse = row_lse + (long long)n * S;
  const float* tv = top_logp + (long long)n * S * K;
  const int32_t* tc = top_class + (long long)n * S * K;
  unsigned long long* hs = hash + (long long)n * H;
  int32_t* np = node_parent + (long long)n * (S * W + 1);
  int32_t* nl = node_label + (long long)n * (S * W + 1);
  int32_t* bn = beam_node + (long long)n * S * W;
  float* bs = beam_score + (long long)n * S * W * 2;

  for (int i = tid; i < H; i += CTC_THREADS) hs[i] = 0;
  if (tid == 0) {   // before frame 0: the empty prefix, pb = 0, pnb = -inf
    b.node[0][0] = 0; b.parent[0][0] = -1; b.last[0][0] = -1; b.len[0][0] = 0;
    b.pb[0][0] = 0.f; b.pnb[0][0] = CTC_NEG_INF;
    b.count[0] = 1;
    b.nodes = 1;
    np[0] = -1;
    nl[0] = -1;
  }
  __threadfence();   // the cleared slots are in memory before the first atomic reads one
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < Tn; t++) {
    const int nxt = cur ^ 1;
    const int B = b.count[cur];
    const float le = lse[t];
    const float lpb = ctc_logp(Elem<T>::ld(x + (long long)t * C + blank), le);
    if (tid < B) {
      const int last = b.last[cur][tid], pn = b.parent[cur][tid];
      b.tot[tid] = ctc_lse3(b.pb[cur][tid], b.pnb[cur][tid], CTC_NEG_INF);
      b.lpe[tid] = last >= 0 ? ctc_logp(Elem<T>::ld(x + (long long)t * C + last), le) : CTC_NEG_INF;
      int ps = -1;
      if (pn >= 0)
        for (int j = 0; j < B; j++)
          if (b.node[cur][j] == pn) ps = j;
      b.pslot[tid] = ps;
    }
    if (tid >= 64 && tid < 64 + K) {   // the second wave, beside the first wave's work above
      b.top_class[tid - 64] = tc[t * K + tid - 64];
      b.top_logp[tid - 64] = tv[t * K + tid - 64];
    }
    if (tid == 0) b.count[nxt] = 0;
    __syncthreads();

    // candidate q: q < B the stay of entry q (with the extension of its parent that spells the same string merged in);
    // q = B + j K + r the extension of entry j by the row's r-th best class, unless that string is a beam entry (merged above: struck out below)
    const int Q = B * (K + 1), Q2 = (Q + 1) & ~1;
    float sc[BEAM_QPT];
#pragma unroll
    for (int k = 0; k < BEAM_QPT; k++) {
      const int q = tid + k * CTC_THREADS;
      float v = CTC_NEG_INF;
      if (q < B) {
        const float lpe = b.lpe[q];
        const int ps = b.pslot[q];
        const float a0 = b.pnb[cur][q] + lpe;
        float a1 = CTC_NEG_INF, a2 = CTC_NEG_INF;
        if (ps >= 0) {
          a1 = b.pb[cur][ps] + lpe;
          if (b.last[cur][ps] != b.last[cur][q]) a2 = b.pnb[cur][ps] + lpe;
        }
        const float pb = b.tot[q] + lpb, pnb = ctc_lse3(a0, a1, a2);
        b.stay_pb[q] = pb;
        b.stay_pnb[q] = pnb;
        v = ctc_lse3(pb, pnb, CTC_NEG_INF);
      } else if (q < Q) {
        const int j = (q - B) / K, c = b.top_class[(q - B) % K];
        v = b.top_logp[(q - B) % K] + (c == b.last[cur][j] ? b.pb[cur][j] : b.tot[j]);
      }
      sc[k] = v;
      if (q < Q2) b.key[q] = beam_key(v, q);
    }
    __syncthreads();
    if (tid < B && b.pslot[tid] >= 0) {   // the extension of the parent's slot that spells this entry's string is part of this entry's stay
      const int base = B + b.pslot[tid] * K, last = b.last[cur][tid];
      for (int r = 0; r < K; r++)
        if (b.top_class[r] == last) b.key[base + r] = 0;
    }
    __syncthreads();

    // rank = the number of larger keys: the order (total descending, candidate index ascending); the first W candidates are kept
    unsigned long long mine[BEAM_QPT];
    int rk[BEAM_QPT];
#pragma unroll
    for (int k = 0; k < BEAM_QPT; k++) {
      const int q = tid + k * CTC_THREADS;
      mine[k] = q < Q ? b.key[q] : 0;
      rk[k] = 0;
    }
    const int wave_first = __builtin_amdgcn_readfirstlane(tid & ~63);   // a wave skips the candidate rows in which it holds none
    for (int q2 = 0; q2 < Q2; q2 += 2) {
      const unsigned long long k0 = b.key[q2], k1 = b.key[q2 + 1];
#pragma unroll
      for (int k = 0; k < BEAM_QPT; k++)
        if (wave_first + k * CTC_THREADS < Q) rk[k] += (k0 > mine[k]) + (k1 > mine[k]);
    }
#pragma unroll
    for (int k = 0; k < BEAM_QPT; k++) {
      const int q = tid + k * CTC_THREADS, slot = rk[k];
      if (mine[k] != 0 && slot < W) {
        if (q < B) {
          b.node[nxt][slot] = b.node[cur][q]; b.parent[nxt][slot] = b.parent[cur][q]; b.last[nxt][slot] = b.last[cur][q];
          b.len[nxt][slot] = b.len[cur][q];
          b.pb[nxt][slot] = b.stay_pb[q]; b.pnb[nxt][slot] = b.stay_pnb[q];
        } else {
          const int j = (q - B) / K;
          b.node[nxt][slot] = -1;   // found or created below
          b.parent[nxt][slot] = b.node[cur][j]; b.last[nxt][slot] = b.top_class[(q - B) % K];
          b.len[nxt][slot] = b.len[cur][j] + 1;
          b.pb[nxt][slot] = CTC_NEG_INF; b.pnb[nxt][slot] = sc[k];
        }
        atomicMax(&b.count[nxt], slot + 1);
      }
    }
    __syncthreads();

    // the first wave: find or create the node of every kept extension (W <= 32 lanes), then the frame's trace
    if (tid < 64) {
      const int B2 = b.count[nxt], base = b.nodes;
      const bool ext = tid < B2 && b.node[nxt][tid] < 0;
      unsigned key = 0;
      int id = 0;
      if (ext) {
        key = (unsigned)b.parent[nxt][tid] * CTC_MAX_C + (unsigned)b.last[nxt][tid];
        id = beam_hash_find(hs, H, key);
      }
      const bool fresh = ext && id == 0;
      const unsigned long long m = __ballot(fresh);   // every lookup of the frame is done before the first insertion
      if (fresh) {
        id = base + __popcll(m & ((1ull << tid) - 1));   // new nodes are numbered in rank order
        np[id] = b.parent[nxt][tid];
        nl[id] = b.last[nxt][tid];
        beam_hash_insert(hs, H, key, id);
      }
      if (ext) b.node[nxt][tid] = id;
      if (tid == 0) b.nodes = base + __popcll(m);
      if (tid < W) {
        const bool live = tid < B2;
        bn[t * W + tid] = live ? (ext ? id : b.node[nxt][tid]) : -1;
        bs[(t * W + tid) * 2] = live ? b.pb[nxt][tid] : CTC_NEG_INF;
        bs[(t * W + tid) * 2 + 1] = live ? b.pnb[nxt][tid] : CTC_NEG_INF;
      }
    }
    __syncthreads();
    cur = nxt;
  }

  // the hypotheses, best first: the beam is in rank order.  One thread per hypothesis walks its prefix back to the root.
  const int B = b.count[cur];
  if (tid == 0) {
    out_count[n] = B;
    node_count[n] = b.nodes;
  }
  __threadfence();   // the node table written above is read back below
  __syncthreads();
  if (tid < W) {
    const bool live = tid < B;
    const int len = live ? b.len[cur][tid] : 0;
    out_scores[(long long)n * W + tid] = live ? ctc_lse3(b.pb[cur][tid], b.pnb[cur][tid], CTC_NEG_INF) : CTC_NEG_INF;
    out_lengths[(long long)n * W + tid] = len;
    int64_t* o = out + ((long long)n * W + tid) * S;
    int node = live ? b.node[cur][tid] : 0;
    for (int p = len - 1; p >= 0; p--) {
      o[p] = __hip_atomic_load(nl + node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      node = __hip_atomic_load(np + node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  for (int k = 0; k < W; k++) {
    int64_t* o = out + ((long long)n * W + k) * S;
    for (int p = (k < B ? b.len[cur][k] : 0) + tid; p < S; p += CTC_THREADS) o[p] = -1;
  }
}

// Table entry (i, j) = distance of a[0, i) and b[0, j).  Anti-diagonal d = i + j, indexed by i, three of them in rotation.
__global__ __launch_bounds__(EDIT_THREADS) void edit_distance_k(const int64_t* __restrict__ a, const int64_t* __restrict__ bq,
                                                                const int64_t* __restrict__ a_len, const int64_t* __restrict__ b_len,
                                                                int64_t* __restrict__ dist, unsigned long long* __restrict__ totals, int La, int Lb) {
  __shared__ int64_t sa[EDIT_MAX_L], sb[EDIT_MAX_L];
  __shared__ int diag[3][EDIT_MAX_L + 1];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int la = ctc_clamp_len(a_len[n], La), lb = ctc_clamp_len(b_len[n], Lb);
  for (int i = tid; i < la; i += EDIT_THREADS) sa[i] = a[(long long)n * La + i];
  for (int j = tid; j < lb; j += EDIT_THREADS) sb[j] = bq[(long long)n * Lb + j];
  __syncthreads();
  for (int d = 0; d <= la + lb; d++) {
    int* cur = diag[d % 3];
    const int* p1 = diag[(d + 2) % 3];   // diagonal d - 1: (i - 1, j) at i - 1, (i, j - 1) at i
    const int* p2 = diag[(d + 1) % 3];   // diagonal d - 2: (i - 1, j - 1) at i - 1
    const int lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    for (int i = lo + tid; i <= hi; i += EDIT_THREADS) {
      const int j = d - i;
      int v;
      if (i == 0) v = j;
      else if (j == 0) v = i;
      else v = min(min(p1[i - 1], p1[i]) + 1, p2[i - 1] + (sa[i - 1] != sb[j - 1] ? 1 : 0));
      cur[i] = v;
    }
    __syncthreads();   // diagonal d is complete; its readers of d - 2 are done before d + 1 overwrites that buffer
  }
  if (tid == 0) {
    const int v = diag[(la + lb) % 3][la];
    dist[n] = v;
    if (totals) {
      atomicAdd(totals, (unsigned long long)v);
      atomicAdd(totals + 1, (unsigned long long)lb);
    }
  }
}

// ---------------------------------------------------------------------------------------------- host side
#define BEAM_LAUNCH_TOP(T, ...)                                                                                                          \
  hipLaunchKernelGGL((ctc_beam_top_k<T>), dim3((unsigned)((rows + 3) / 4)), dim3(CTC_THREADS), 0, st, (const T*)logits, input_lengths, row_lse, \
                     top_logp, top_class, (long long)rows, (int)S, (int)C, (int)blank, (int)K)
#define BEAM_LAUNCH(T, ...)                                                                                                                  \
  hipLaunchKernelGGL((ctc_beam_k<T>), dim3((unsigned)N), dim3(CTC_THREADS), 0, st, (const T*)logits, input_lengths, (const float*)row_lse,        \
                     (const float*)top_logp, (const int32_t*)top_class, (unsigned long long*)hash, out, out_lengths, out_scores, out_count,      \
                     node_parent, node_label, node_count, beam_node, beam_score, (int)S, (int)C, (int)blank, (int)W, (int)K, (int)H)

extern "C" int pero_ctc_beam(const void* logits, const int64_t* input_lengths, int64_t* out, int64_t* out_lengths, float* out_scores,
                             int64_t* out_count, int32_t* node_parent, int32_t* node_label, int32_t* node_count, int32_t* beam_node,
                             float* beam_score, float* row_lse, float* top_logp, int32_t* top_class, uint64_t* hash, int64_t N, int64_t S, int64_t C,
                             int64_t blank, int64_t W, int dtype, void* stream) {
  const int rc = ctc_check("pero_ctc_beam", N, S, C, 0, blank, dtype);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE(W > 0, "pero_ctc_beam: bad sizes (W %lld)", (long long)W);
  if (W > BEAM_MAX_W) {
    pero_set_error("pero_ctc_beam: supported up to W = %d (got W %lld)", BEAM_MAX_W, (long long)W);
    return PERO_E_UNSUPPORTED;
  }
  PERO_REQUIRE(logits && input_lengths && out && out_lengths && out_scores && out_count && node_parent && node_label && node_count && beam_node &&
                   beam_score && row_lse && top_logp && top_class && hash,
               "pero_ctc_beam: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = N * S, K = W + 1 < C - 1 ? W + 1 : C - 1, H = beam_hash_slots(S, W);
  DISPATCH_T(dtype, BEAM_LAUNCH_TOP, 0);
  PERO_CHECK_LAUNCH("pero_ctc_beam (row lse, best classes)");
  DISPATCH_T(dtype, BEAM_LAUNCH, 0);
  PERO_CHECK_LAUNCH("pero_ctc_beam (search)");
  return PERO_OK;
}

extern "C" int pero_edit_distance(const int64_t* a, const int64_t* a_len, const int64_t* b, const int64_t* b_len, int64_t* dist, int64_t* totals,
                                  int64_t N, int64_t La, int64_t Lb, void* stream) {
  PERO_REQUIRE(N > 0 && N < (1LL << 31) && La >= 0 && Lb >= 0, "pero_edit_distance: bad sizes (N %lld, La %lld, Lb %lld)", (long long)N, (long long)La,
               (long long)Lb);
  if (La > EDIT_MAX_L || Lb > EDIT_MAX_L) {
    pero_set_error("pero_edit_distance: supported up to La, Lb = %d (got La %lld, Lb %lld)", EDIT_MAX_L, (long long)La, (long long)Lb);
    return PERO_E_UNSUPPORTED;
  }
  PERO_REQUIRE((a || La == 0) && (b || Lb == 0) && a_len && b_len && dist, "pero_edit_distance: null pointer");
  hipLaunchKernelGGL(edit_distance_k, dim3((unsigned)N), dim3(EDIT_THREADS), 0, (hipStream_t)stream, a, b, a_len, b_len, dist,
                     (unsigned long long*)totals, (int)La, (int)Lb);
  PERO_CHECK_LAUNCH("pero_edit_distance");
  return PERO_OK;
}
