// Decoding of a recogniser's output on the device: CTC prefix beam search, with or without an n-gram language model.  Contract: include/pero_hip.h; derivation,
// trie and tie rule: DESIGN.md "CTC decoding".
//
//   pero_ctc_beam      ctc_beam_top_k  one wave per logit row t < T: row_lse (ctc_wave_row_lse, the function of ctc_row_lse_k) and the
//                                      K = min(W + 1, C - 1) best non-blank classes of the row with their log-probabilities (all rows in
//                                      parallel)
//                      ctc_beam_k      one workgroup per line, frame by frame: the <= W (K + 1) candidates of the frame are scored by the
//                                      threads, ranked by counting, the kept ones find or create their prefix node; five barriers per frame
//   pero_ctc_beam_lm   the same two kernels; ctc_beam_k<T, true> adds the n-gram term of every new string (one walk of the LM automaton per
//                                      extension candidate, issued ahead of the frame's first barrier) and takes K from the caller
//
// Why K = W + 1 classes are enough: the extensions of one beam entry j score logp(c) + tot_j, except c = last_j, which scores logp(c) + pb_j
// <= logp(c) + tot_j.  A class outside the row's best W + 1 is beaten, for the same j, by at least W extensions (or by the stay candidates
// they merged into, whose totals are no smaller), so it is never among the frame's best W.  With a language model the score of p + c depends
// on p and the argument is gone: K is the caller's (a pruning of the NEW strings), bounded by W (K + 1) <= BEAM_MAX_Q.
#include "ctc_common.hpp"

#define BEAM_MAX_W 32
#define BEAM_MAX_K (BEAM_MAX_W + 1)
#define BEAM_MAX_Q (BEAM_MAX_W * (BEAM_MAX_K + 1))                      // stay + extension candidates of one frame
#define BEAM_LM_MAX_K (BEAM_MAX_Q - 1)                                  // W = 1: the largest K with W (K + 1) <= BEAM_MAX_Q
#define BEAM_LM_MAX_HOPS PERO_CTC_LM_MAX_ORDER                          // back-off steps of one look-up
#define BEAM_QPT ((BEAM_MAX_Q + CTC_THREADS - 1) / CTC_THREADS)         // candidates of one thread

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

// The language model of pero_ctc_beam_lm (include/pero_hip.h): the automaton's arrays, the fusion weights and the LM part of the trace.  All null /
// zero for pero_ctc_beam, whose kernel never reads it.
struct BeamLm {
  const int32_t* backoff_state;
  const float* backoff_weight;
  const float* final;
  const int32_t* arc_begin;
  const int32_t* arc_label;
  const float* arc_logp;
  const int32_t* arc_next;
  float* out_lm;
  int32_t* node_state;
  float* node_weight;
  int M, A, start, use_final;
  float alpha, beta;
};

// lm(s, c) and the next state: the header's walk, f32 additions in its order.  false: c has no arc in state 0 (a forbidden class), or the tables
// are malformed (an index outside its array, a back-off chain longer than BEAM_LM_MAX_HOPS): nothing out of range is ever read.
static __device__ __forceinline__ bool beam_lm_lookup(const BeamLm& lm, int s, int c, float& logp, int& next) {
  float acc = 0.f;
  for (int hop = 0; hop <= BEAM_LM_MAX_HOPS; hop++) {
    if ((unsigned)s >= (unsigned)lm.M) return false;
    const int first = lm.arc_begin[s], end = lm.arc_begin[s + 1];
    if (first < 0 || end > lm.A || first > end) return false;
    int lo = first, hi = end;   // the first arc of s whose label is >= c
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (lm.arc_label[mid] < c) lo = mid + 1;
      else hi = mid;
    }
    if (lo < end && lm.arc_label[lo] == c) {
      logp = __fadd_rn(acc, lm.arc_logp[lo]);
      next = lm.arc_next[lo];
      return (unsigned)next < (unsigned)lm.M;
    }
    if (s == 0) return false;
    acc = __fadd_rn(acc, lm.backoff_weight[s]);
    s = lm.backoff_state[s];
  }
  return false;
}

// One beam entry: the prefix's node, its parent node and last label (-1 for the empty prefix), its length, pb and pnb; with a language model its LM
// state, the weight w its last label added and the sum of the w from the root.  Two copies in ping-pong.  MAXK: the frame's classes.
template <int MAXK>
struct BeamLds {
  int node[2][BEAM_MAX_W], parent[2][BEAM_MAX_W], last[2][BEAM_MAX_W], len[2][BEAM_MAX_W];
  float pb[2][BEAM_MAX_W], pnb[2][BEAM_MAX_W];
  int lm_state[2][BEAM_MAX_W];
  float lm_w[2][BEAM_MAX_W], lm_total[2][BEAM_MAX_W];
  float tot[BEAM_MAX_W], lpe[BEAM_MAX_W], stay_pb[BEAM_MAX_W], stay_pnb[BEAM_MAX_W];
  int pslot[BEAM_MAX_W];   // the beam slot of the entry's parent prefix, -1 if that prefix is not in the beam
  alignas(16) unsigned long long key[BEAM_MAX_Q];   // the candidates' sort keys (beam_key), read two at a time by the ranking loop
  int top_class[MAXK];                   // the frame's best classes and their log-probabilities
  float top_logp[MAXK];
  int count[2], nodes;
};

template <typename T, bool LM>
__global__ __launch_bounds__(CTC_THREADS) void ctc_beam_k(const T* __restrict__ logits, const int64_t* __restrict__ input_lengths,
                                                           const float* __restrict__ row_lse, const float* __restrict__ top_logp,
                                                           const int32_t* __restrict__ top_class, unsigned long long* __restrict__ hash,
                                                           int64_t* __restrict__ out, int64_t* __restrict__ out_lengths, float* __restrict__ out_scores,
                                                           int64_t* __restrict__ out_count, int32_t* __restrict__ node_parent,
                                                           int32_t* __restrict__ node_label, int32_t* __restrict__ node_count,
                                                           int32_t* __restrict__ beam_node, float* __restrict__ beam_score, int S, int C, int blank,
                                                           int W, int K, int H, BeamLm lm) {
  __shared__ BeamLds<LM ? BEAM_LM_MAX_K : BEAM_MAX_K> b;
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
  int32_t* ns = LM ? lm.node_state + (long long)n * (S * W + 1) : nullptr;
  float* nw = LM ? lm.node_weight + (long long)n * (S * W + 1) : nullptr;

  for (int i = tid; i < H; i += CTC_THREADS) hs[i] = 0;
  if (tid == 0) {   // before frame 0: the empty prefix, pb = 0, pnb = -inf
    b.node[0][0] = 0; b.parent[0][0] = -1; b.last[0][0] = -1; b.len[0][0] = 0;
    b.pb[0][0] = 0.f; b.pnb[0][0] = CTC_NEG_INF;
    b.count[0] = 1;
    b.nodes = 1;
    np[0] = -1;
    nl[0] = -1;
    if (LM) {
      b.lm_state[0][0] = lm.start; b.lm_w[0][0] = 0.f; b.lm_total[0][0] = 0.f;
      ns[0] = lm.start;
      nw[0] = 0.f;
    }
  }
  __threadfence();   // the cleared slots are in memory before the first atomic reads one
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < Tn; t++) {
    const int nxt = cur ^ 1;
    const int B = b.count[cur];
    const float le = lse[t];
    const float lpb = ctc_logp(Elem<T>::ld(x + (long long)t * C + blank), le);
    // the LM term of the thread's extension candidates: w = alpha lm(state of p, c) + beta, and the state of p + c.  Chains of dependent loads,
    // issued here so that they run beside the loads and the parent search below.
    float lw[BEAM_QPT];
    int ln[BEAM_QPT];
    if (LM) {
#pragma unroll
      for (int k = 0; k < BEAM_QPT; k++) {
        const int q = tid + k * CTC_THREADS;
        lw[k] = CTC_NEG_INF;   // no candidate
        ln[k] = 0;
        if (q >= B && q < B * (K + 1)) {
          float l;
          if (beam_lm_lookup(lm, b.lm_state[cur][(q - B) / K], tc[t * K + (q - B) % K], l, ln[k])) lw[k] = __fadd_rn(__fmul_rn(lm.alpha, l), lm.beta);
        }
      }
    }
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
    if (tid >= 64)   // the other waves, beside the first wave's work above (K <= BEAM_MAX_K: the second wave alone, one round)
      for (int r = tid - 64; r < K; r += CTC_THREADS - 64) {
        b.top_class[r] = tc[t * K + r];
        b.top_logp[r] = tv[t * K + r];
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
        if (ps >= 0) {   // the parent's extension carries the w of this entry's last label, as when the string was created
          const float lpw = LM ? lpe + b.lm_w[cur][q] : lpe;
          a1 = b.pb[cur][ps] + lpw;
          if (b.last[cur][ps] != b.last[cur][q]) a2 = b.pnb[cur][ps] + lpw;
        }
        const float pb = b.tot[q] + lpb, pnb = ctc_lse3(a0, a1, a2);
        b.stay_pb[q] = pb;
        b.stay_pnb[q] = pnb;
        v = ctc_lse3(pb, pnb, CTC_NEG_INF);
      } else if (q < Q) {
        const int j = (q - B) / K, c = b.top_class[(q - B) % K];
        float lpw = b.top_logp[(q - B) % K];
        if (LM) lpw = lw[k] == CTC_NEG_INF ? CTC_NEG_INF : lpw + lw[k];
        v = lpw + (c == b.last[cur][j] ? b.pb[cur][j] : b.tot[j]);
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
          if (LM) { b.lm_state[nxt][slot] = b.lm_state[cur][q]; b.lm_w[nxt][slot] = b.lm_w[cur][q]; b.lm_total[nxt][slot] = b.lm_total[cur][q]; }
        } else {
          const int j = (q - B) / K;
          b.node[nxt][slot] = -1;   // found or created below
          b.parent[nxt][slot] = b.node[cur][j]; b.last[nxt][slot] = b.top_class[(q - B) % K];
          b.len[nxt][slot] = b.len[cur][j] + 1;
          b.pb[nxt][slot] = CTC_NEG_INF; b.pnb[nxt][slot] = sc[k];
          if (LM) { b.lm_state[nxt][slot] = ln[k]; b.lm_w[nxt][slot] = lw[k]; b.lm_total[nxt][slot] = b.lm_total[cur][j]; }   // the parent's sum: + w below
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
        if (LM) {
          ns[id] = b.lm_state[nxt][tid];
          nw[id] = b.lm_w[nxt][tid];
        }
        beam_hash_insert(hs, H, key, id);
      } else if (LM && ext) {   // a prefix that comes back takes state and weight from its node (written in an earlier frame, behind a barrier)
        b.lm_state[nxt][tid] = __hip_atomic_load(ns + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.lm_w[nxt][tid] = __hip_atomic_load(nw + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (LM && ext) b.lm_total[nxt][tid] = __fadd_rn(b.lm_total[nxt][tid], b.lm_w[nxt][tid]);
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

  // the hypotheses, best first: the beam is in rank order; with the LM's final term the totals are ranked once more (ties by the beam's order).
  // One thread per hypothesis walks its prefix back to the root.
  const int B = b.count[cur];
  if (tid == 0) {
    out_count[n] = B;
    node_count[n] = b.nodes;
  }
  if (tid < W) {
    float total = tid < B ? ctc_lse3(b.pb[cur][tid], b.pnb[cur][tid], CTC_NEG_INF) : CTC_NEG_INF;
    if (LM && lm.use_final && tid < B) total = __fadd_rn(total, __fmul_rn(lm.alpha, lm.final[b.lm_state[cur][tid]]));
    b.tot[tid] = total;
    b.key[tid] = tid < B ? beam_key(total, tid) : 0;
    b.pslot[tid] = tid;
  }
  __threadfence();   // the node table written above is read back below
  __syncthreads();
  if (LM && lm.use_final && tid < B) {
    int rank = 0;
    for (int j = 0; j < B; j++) rank += b.key[j] > b.key[tid];
    b.pslot[rank] = tid;   // a total of -inf (key 0) cannot be in the beam: the ranks are a permutation
  }
  if (LM) __syncthreads();
  if (tid < W) {
    const bool live = tid < B;
    const int e = b.pslot[tid];   // the beam entry of hypothesis tid
    const int len = live ? b.len[cur][e] : 0;
    out_scores[(long long)n * W + tid] = live ? b.tot[e] : CTC_NEG_INF;
    if (LM) {
      float part = live ? b.lm_total[cur][e] : 0.f;
      if (lm.use_final && live) part = __fadd_rn(part, __fmul_rn(lm.alpha, lm.final[b.lm_state[cur][e]]));
      lm.out_lm[(long long)n * W + tid] = part;
    }
    out_lengths[(long long)n * W + tid] = len;
    int64_t* o = out + ((long long)n * W + tid) * S;
    int node = live ? b.node[cur][e] : 0;
    for (int p = len - 1; p >= 0; p--) {
      o[p] = __hip_atomic_load(nl + node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      node = __hip_atomic_load(np + node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  for (int k = 0; k < W; k++) {
    int64_t* o = out + ((long long)n * W + k) * S;
    for (int p = (k < B ? b.len[cur][b.pslot[k]] : 0) + tid; p < S; p += CTC_THREADS) o[p] = -1;
  }
}

// ---------------------------------------------------------------------------------------------- host side
// Both entry points: the checks they share, then the two launches.  with_lm: ctc_beam_k<T, true> with the caller's K.
static int beam_run(const char* name, const void* logits, const int64_t* input_lengths, int64_t* out, int64_t* out_lengths, float* out_scores,
                    int64_t* out_count, int32_t* node_parent, int32_t* node_label, int32_t* node_count, int32_t* beam_node, float* beam_score,
                    float* row_lse, float* top_logp, int32_t* top_class, uint64_t* hash, int64_t N, int64_t S, int64_t C, int64_t blank, int64_t W,
                    int64_t K, bool with_lm, const BeamLm& lm, int dtype, void* stream) {
  const int rc = ctc_check(name, N, S, C, 0, blank, dtype);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE(W > 0, "%s: bad sizes (W %lld)", name, (long long)W);
  if (W > BEAM_MAX_W) {
    pero_set_error("%s: supported up to W = %d (got W %lld)", name, BEAM_MAX_W, (long long)W);
    return PERO_E_UNSUPPORTED;
  }
  PERO_REQUIRE(logits && input_lengths && out && out_lengths && out_scores && out_count && node_parent && node_label && node_count && beam_node &&
                   beam_score && row_lse && top_logp && top_class && hash,
               "%s: null pointer", name);
  K = K < 1 ? 1 : (K > C - 1 ? C - 1 : K);
  if (W * (K + 1) > BEAM_MAX_Q) {
    pero_set_error("%s: supported up to W (K + 1) = %d (got W %lld, K %lld)", name, BEAM_MAX_Q, (long long)W, (long long)K);
    return PERO_E_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = N * S, H = beam_hash_slots(S, W);
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t);
    hipLaunchKernelGGL((ctc_beam_top_k<T>), dim3((unsigned)((rows + 3) / 4)), dim3(CTC_THREADS), 0, st, (const T*)logits, input_lengths, row_lse,
                       top_logp, top_class, (long long)rows, (int)S, (int)C, (int)blank, (int)K); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_ctc_beam (row lse, best classes)");
  PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(with_lm, [&](auto LM) {
    hipLaunchKernelGGL((ctc_beam_k<T, decltype(LM)::value>), dim3((unsigned)N), dim3(CTC_THREADS), 0, st, (const T*)logits, input_lengths, (const float*)row_lse,
                       (const float*)top_logp, (const int32_t*)top_class, (unsigned long long*)hash, out, out_lengths, out_scores, out_count,
                       node_parent, node_label, node_count, beam_node, beam_score, (int)S, (int)C, (int)blank, (int)W, (int)K, (int)H, lm); }); }), "bad dtype");
  PERO_CHECK_LAUNCH("pero_ctc_beam (search)");
  return PERO_OK;
}

extern "C" int pero_ctc_beam(const void* logits, const int64_t* input_lengths, int64_t* out, int64_t* out_lengths, float* out_scores,
                             int64_t* out_count, int32_t* node_parent, int32_t* node_label, int32_t* node_count, int32_t* beam_node,
                             float* beam_score, float* row_lse, float* top_logp, int32_t* top_class, uint64_t* hash, int64_t N, int64_t S, int64_t C,
                             int64_t blank, int64_t W, int dtype, void* stream) {
  return beam_run("pero_ctc_beam", logits, input_lengths, out, out_lengths, out_scores, out_count, node_parent, node_label, node_count, beam_node,
                  beam_score, row_lse, top_logp, top_class, hash, N, S, C, blank, W, W + 1, false, BeamLm{}, dtype, stream);
}

extern "C" int pero_ctc_beam_lm(const void* logits, const int64_t* input_lengths, const int32_t* lm_backoff_state, const float* lm_backoff_weight,
                                const float* lm_final, const int32_t* lm_arc_begin, const int32_t* lm_arc_label, const float* lm_arc_logp,
                                const int32_t* lm_arc_next, int64_t* out, int64_t* out_lengths, float* out_scores, float* out_lm, int64_t* out_count,
                                int32_t* node_parent, int32_t* node_label, int32_t* node_lm_state, float* node_lm_weight, int32_t* node_count,
                                int32_t* beam_node, float* beam_score, float* row_lse, float* top_logp, int32_t* top_class, uint64_t* hash, int64_t N,
                                int64_t S, int64_t C, int64_t blank, int64_t W, int64_t K, int64_t M, int64_t A, int64_t start, float lm_weight,
                                float length_bonus, int use_final, int dtype, void* stream) {
  PERO_REQUIRE(M >= 1 && M < (1LL << 31) && A >= 0 && A < (1LL << 31) && start >= 0 && start < M,
               "pero_ctc_beam_lm: bad language model sizes (M %lld, A %lld, start %lld)", (long long)M, (long long)A, (long long)start);
  PERO_REQUIRE(std::isfinite(lm_weight) && std::isfinite(length_bonus), "pero_ctc_beam_lm: lm_weight and length_bonus must be finite");
  PERO_REQUIRE(lm_backoff_state && lm_backoff_weight && lm_final && lm_arc_begin && (A == 0 || (lm_arc_label && lm_arc_logp && lm_arc_next)) && out_lm &&
                   node_lm_state && node_lm_weight,
               "pero_ctc_beam_lm: null pointer");
  const BeamLm lm = {lm_backoff_state, lm_backoff_weight, lm_final, lm_arc_begin, lm_arc_label, lm_arc_logp, lm_arc_next, out_lm, node_lm_state,
                     node_lm_weight, (int)M, (int)A, (int)start, use_final != 0, lm_weight, length_bonus};
  return beam_run("pero_ctc_beam_lm", logits, input_lengths, out, out_lengths, out_scores, out_count, node_parent, node_label, node_count, beam_node,
                  beam_score, row_lse, top_logp, top_class, hash, N, S, C, blank, W, K, true, lm, dtype, stream);
}
