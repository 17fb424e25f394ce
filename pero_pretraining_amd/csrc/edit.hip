// Edit distance and edit operations on the device: the Levenshtein table of every pair of a batch, and - for pero_edit_ops - its backtrace:
// the script of hits, substitutions, insertions and deletions, their counts, a confusion matrix, and the same over words.  Contract:
// include/pero_hip.h; kernel shapes, LDS budgets and measurements: DESIGN.md sections 12 and 16.
//
//   both kernels       edit_sweep<DIRS>   the table by anti-diagonals out of LDS, three of them in rotation, one barrier each
//   pero_edit_distance edit_distance_k    one workgroup per pair, static LDS at the limits: the sweep, and the corner of the table
//   pero_edit_ops      edit_ops_k<WORDS>  one workgroup per pair.  The sweep with DIRS: every cell's 2-bit operation is written as the cell
//                                         is computed, packed 16 to a word, row-wise by i, in LDS - the directions never reach HBM.  One lane
//                                         walks back from (la, lb) and leaves the reversed script in LDS; all threads copy it out forwards
//                                         and add the confusion counts.  WORDS: the rows are split at the separators first (two ballots per
//                                         row), every word gets the slot of the first word with the same content (a hash finds candidates,
//                                         the labels decide), and the table runs over those slots.
//
// The dynamic LDS of edit_ops_k is sized from the call's La, Lb (edit_lds): about 4 KB at 70 labels, 86 KB at 512 x 512, so short lines keep
// many workgroups on a CU.  A cell's operation IS the script code (0 hit, 1 substitution, 2 insertion, 3 deletion); every code moves i or j
// towards 0 and the walk is a loop over at most la + lb steps, so it ends and stays inside its arrays whatever the LDS holds.
#include "ctc_common.hpp"

#define EDIT_THREADS 256   // one workgroup per pair
#define EDIT_MAX_L 512

static_assert(EDIT_MAX_L <= 2 * EDIT_THREADS, "edit_split: two positions per thread");
static_assert(EDIT_MAX_L < (1 << 10), "a step packs i and j into 10 bits each");

// Table entry (i, j) = distance of a[0, i) and b[0, j); anti-diagonal d = i + j, indexed by i.  All EDIT_THREADS threads call it, after a
// barrier behind the writes of ea and eb.  diag: three diagonals of W >= la + 1 ints in rotation; on return (behind a barrier) the distance is
// diag[((la + lb) % 3) * W + la].  DIRS: cell (i, j), i, j >= 1, leaves its operation in dir (layout: edit_lds), tie rule of the header:
// diagonal, then deletion, then insertion.
template <bool DIRS>
static __device__ __forceinline__ void edit_sweep(const int64_t* ea, const int64_t* eb, int la, int lb, int* diag, int W, unsigned* dir, int stride) {
  const int tid = threadIdx.x;
  for (int d = 0; d <= la + lb; d++) {
    int* cur = diag + (d % 3) * W;
    const int* p1 = diag + ((d + 2) % 3) * W;   // diagonal d - 1: (i - 1, j) at i - 1, (i, j - 1) at i
    const int* p2 = diag + ((d + 1) % 3) * W;   // diagonal d - 2: (i - 1, j - 1) at i - 1
    const int lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    for (int i = lo + tid; i <= hi; i += EDIT_THREADS) {
      int v;
      if (i == 0 || i == d) v = d;   // the boundary cells (0, j) and (i, 0): the other index
      else {
        const int j = d - i;
        const int ne = ea[i - 1] != eb[j - 1] ? 1 : 0;
        const int dg = p2[i - 1] + ne, left = p1[i] + 1, up = p1[i - 1] + 1;
        v = min(min(up, left), dg);
        if (DIRS) {
          const unsigned code = dg == v ? (unsigned)ne : (left == v ? 3u : 2u);
          // a row has one cell per diagonal, so this word has one writer now; its first cell starts the word, the barrier orders the others
          unsigned* word = dir + (i - 1) * stride + ((j - 1) >> 4);
          const int sh = ((j - 1) & 15) * 2;
          *word = sh == 0 ? code : (*word | (code << sh));
        }
      }
      cur[i] = v;
    }
    __syncthreads();   // diagonal d is complete; its readers of d - 2 are done before d + 1 overwrites that buffer
  }
}

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
  edit_sweep<false>(sa, sb, la, lb, &diag[0][0], EDIT_MAX_L + 1, nullptr, 0);
  if (tid == 0) {
    const int v = diag[(la + lb) % 3][la];
    dist[n] = v;
    if (totals) {
      atomicAdd(totals, (unsigned long long)v);
      atomicAdd(totals + 1, (unsigned long long)lb);
    }
  }
}

// Byte offsets into the dynamic LDS, the same function on both sides of the launch.  rows, cols: the widest table of the call (labels, or
// words: a row of L labels holds at most (L + 1) / 2 words).  stride: words of one row of directions, odd, so that the cells of a diagonal
// (one per row) fall into different banks.
struct EditLds {
  int rows, cols, stride;
  unsigned ea, eb, ra, rb, hash, diag, dir, steps, wbeg, wend, bytes;
};
static __host__ __device__ inline EditLds edit_lds(int La, int Lb, bool words) {
  EditLds l;
  l.rows = words ? (La + 1) / 2 : La;
  l.cols = words ? (Lb + 1) / 2 : Lb;
  l.stride = ((l.cols + 15) / 16) | 1;
  const unsigned list = (unsigned)(l.rows + l.cols);
  unsigned o = 0;
  l.ea = o, o += 8u * l.rows;                  // int64: the table's elements (labels, or word slots)
  l.eb = o, o += 8u * l.cols;
  l.ra = o, o += words ? 8u * La : 0;          // int64: the rows as given
  l.rb = o, o += words ? 8u * Lb : 0;
  l.hash = o, o += words ? 8u * list : 0;      // uint64 per word slot: b's words in [0, cols), a's in [cols, cols + rows)
  l.diag = o, o += 4u * 3 * (l.rows + 1);
  l.dir = o, o += 4u * l.rows * l.stride;      // cell (i, j), i, j >= 1: bits 2 ((j - 1) % 16) of word (i - 1) stride + (j - 1) / 16
  l.steps = o, o += 4u * list;                 // the walk, last step first: code | i << 2 | j << 12
  l.wbeg = o, o += words ? 4u * list : 0;      // [begin, end) of every word slot in its row
  l.wend = o, o += words ? 4u * list : 0;
  l.bytes = o;
  return l;
}

// The words of one row: maximal runs of labels that are no separator.  wbeg, wend [w] of the row's words in order; returns their number.
// All threads call it; `chunk` is 8 ints of LDS.  Position p = tid + 256 k; a word's number is the count of word beginnings in front of it.
static __device__ __forceinline__ bool edit_in_word(int64_t c, const uint8_t* __restrict__ is_sep, int C) { return !(c >= 0 && c < C && is_sep[c]); }
static __device__ int edit_split(const int64_t* r, int len, const uint8_t* __restrict__ is_sep, int C, int* wbeg, int* wend, int* chunk) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bool beg[2], end[2];
  int rank[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int p = tid + k * EDIT_THREADS;
    const bool w = p < len && edit_in_word(r[p], is_sep, C);
    beg[k] = w && !(p > 0 && edit_in_word(r[p - 1], is_sep, C));
    end[k] = w && !(p + 1 < len && edit_in_word(r[p + 1], is_sep, C));
    const unsigned long long m = __ballot(beg[k]);
    rank[k] = __popcll(m & ((1ull << lane) - 1));
    if (lane == 0) chunk[k * 4 + wave] = __popcll(m);
  }
  __syncthreads();
  int total = 0, base[2] = {0, 0};
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const int v = chunk[c];
    if (c < wave) base[0] += v;
    if (c < 4 + wave) base[1] += v;
    total += v;
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int p = tid + k * EDIT_THREADS, w = base[k] + rank[k];   // beginnings in front of p
    if (beg[k]) wbeg[w] = p;
    if (end[k]) wend[w + (beg[k] ? 1 : 0) - 1] = p + 1;
  }
  __syncthreads();   // the spans are complete; chunk is free again
  return total;
}

template <bool WORDS>
__global__ __launch_bounds__(EDIT_THREADS) void edit_ops_k(const int64_t* __restrict__ a, const int64_t* __restrict__ bq,
                                                           const int64_t* __restrict__ a_len, const int64_t* __restrict__ b_len,
                                                           const uint8_t* __restrict__ is_sep, int64_t* __restrict__ counts,
                                                           int8_t* __restrict__ script, int32_t* __restrict__ script_len,
                                                           int32_t* __restrict__ a_spans, int32_t* __restrict__ b_spans,
                                                           unsigned long long* __restrict__ totals, unsigned long long* __restrict__ confusion,
                                                           int La, int Lb, int C) {
  extern __shared__ __align__(16) unsigned char edit_smem[];
  __shared__ int chunk[8];
  __shared__ int walk_len;
  __shared__ unsigned long long walk_counts;
  const EditLds l = edit_lds(La, Lb, WORDS);
  int64_t* ea = (int64_t*)(edit_smem + l.ea);
  int64_t* eb = (int64_t*)(edit_smem + l.eb);
  int* diag = (int*)(edit_smem + l.diag);
  unsigned* dir = (unsigned*)(edit_smem + l.dir);
  int* steps = (int*)(edit_smem + l.steps);
  const int n = blockIdx.x, tid = threadIdx.x, stride = l.stride;
  int la = ctc_clamp_len(a_len[n], La), lb = ctc_clamp_len(b_len[n], Lb);

  if (!WORDS) {
    for (int i = tid; i < la; i += EDIT_THREADS) ea[i] = a[(long long)n * La + i];
    for (int j = tid; j < lb; j += EDIT_THREADS) eb[j] = bq[(long long)n * Lb + j];
  } else {
    int64_t* ra = (int64_t*)(edit_smem + l.ra);
    int64_t* rb = (int64_t*)(edit_smem + l.rb);
    unsigned long long* hash = (unsigned long long*)(edit_smem + l.hash);
    int* wbeg = (int*)(edit_smem + l.wbeg);
    int* wend = (int*)(edit_smem + l.wend);
    const int rows = l.rows, cols = l.cols;
    for (int i = tid; i < la; i += EDIT_THREADS) ra[i] = a[(long long)n * La + i];
    for (int j = tid; j < lb; j += EDIT_THREADS) rb[j] = bq[(long long)n * Lb + j];
    __syncthreads();
    const int nb = edit_split(rb, lb, is_sep, C, wbeg, wend, chunk);
    const int na = edit_split(ra, la, is_sep, C, wbeg + cols, wend + cols, chunk);
    if (a_spans)
      for (int w = tid; w < rows; w += EDIT_THREADS) {
        a_spans[((long long)n * rows + w) * 2] = w < na ? wbeg[cols + w] : -1;
        a_spans[((long long)n * rows + w) * 2 + 1] = w < na ? wend[cols + w] : -1;
      }
    if (b_spans)
      for (int w = tid; w < cols; w += EDIT_THREADS) {
        b_spans[((long long)n * cols + w) * 2] = w < nb ? wbeg[w] : -1;
        b_spans[((long long)n * cols + w) * 2 + 1] = w < nb ? wend[w] : -1;
      }
    // the word list: b's words, then a's.  Slot q of it holds a word iff `live`.
    for (int q = tid; q < cols + rows; q += EDIT_THREADS) {
      const bool live = q < cols ? q < nb : q - cols < na;
      unsigned long long h = 0xcbf29ce484222325ull;
      if (live) {
        const int64_t* src = q < cols ? rb : ra;
        for (int p = wbeg[q]; p < wend[q]; p++) h = (h ^ (unsigned long long)src[p]) * 0x100000001b3ull;
      }
      hash[q] = h;
    }
    __syncthreads();
    // every word's element = the slot of the first word of the list with the same length and labels (the hash only skips unequal words)
    for (int q = tid; q < cols + rows; q += EDIT_THREADS) {
      const bool live = q < cols ? q < nb : q - cols < na;
      if (!live) continue;
      const int64_t* src = (q < cols ? rb : ra) + wbeg[q];
      const int len = wend[q] - wbeg[q], before = q < cols ? q : nb + (q - cols);
      const unsigned long long h = hash[q];
      int id = q;
      for (int t = 0; t < before; t++) {
        const int q2 = t < nb ? t : cols + (t - nb);
        if (hash[q2] != h || wend[q2] - wbeg[q2] != len) continue;
        const int64_t* other = (q2 < cols ? rb : ra) + wbeg[q2];
        bool same = true;
        for (int p = 0; p < len && same; p++) same = src[p] == other[p];
        if (same) {
          id = q2;
          break;
        }
      }
      if (q < cols) eb[q] = id;
      else ea[q - cols] = id;
    }
    la = na, lb = nb;
  }
  __syncthreads();

  edit_sweep<true>(ea, eb, la, lb, diag, l.rows + 1, dir, stride);

  if (tid == 0) {
    int i = la, j = lb, k = 0;
    unsigned long long cnt = 0;   // four 16-bit counters, code c in bits [16 c, 16 c + 16): each is at most la + lb <= 1024
    for (int s = 0; s < la + lb && (i > 0 || j > 0); s++) {
      int code;
      if (i > 0 && j > 0) code = (dir[(i - 1) * stride + ((j - 1) >> 4)] >> (((j - 1) & 15) * 2)) & 3;
      else code = j > 0 ? 3 : 2;
      steps[k++] = code | (i << 2) | (j << 12);
      cnt += 1ull << (16 * code);
      if (code != 3) i--;
      if (code != 2) j--;
    }
    walk_len = k;
    walk_counts = cnt;
  }
  __syncthreads();
  const int len = walk_len;
  if (tid == 0) {
    const unsigned long long cnt = walk_counts;
    const unsigned long long hit = cnt & 0xffff, sub = (cnt >> 16) & 0xffff, ins = (cnt >> 32) & 0xffff, del = (cnt >> 48) & 0xffff;
    counts[(long long)n * 4] = (int64_t)sub;
    counts[(long long)n * 4 + 1] = (int64_t)ins;
    counts[(long long)n * 4 + 2] = (int64_t)del;
    counts[(long long)n * 4 + 3] = (int64_t)hit;
    if (script_len) script_len[n] = len;
    if (totals) {
      if (sub) atomicAdd(totals, sub);
      if (ins) atomicAdd(totals + 1, ins);
      if (del) atomicAdd(totals + 2, del);
      if (hit) atomicAdd(totals + 3, hit);
      atomicAdd(totals + 4, 1ull);
      if (sub + ins + del) atomicAdd(totals + 5, 1ull);
    }
  }
  if (script) {
    const int width = La + Lb;
    for (int k = tid; k < width; k += EDIT_THREADS) script[(long long)n * width + k] = k < len ? (int8_t)(steps[len - 1 - k] & 3) : (int8_t)-1;
  }
  if (!WORDS && confusion) {
    const long long ld = (long long)C + 1;
    for (int k = tid; k < len; k += EDIT_THREADS) {
      const int s = steps[k], code = s & 3, i = (s >> 2) & 1023, j = (s >> 12) & 1023;
      const int64_t h = code != 3 ? ea[i - 1] : (int64_t)C, r = code != 2 ? eb[j - 1] : (int64_t)C;   // the gap is row / column C
      const bool h_ok = code == 3 || (h >= 0 && h < C), r_ok = code == 2 || (r >= 0 && r < C);
      if (h_ok && r_ok) atomicAdd(confusion + r * ld + h, 1ull);
    }
  }
}

// ---------------------------------------------------------------------------------------------- host side
#define EDIT_OPS_LAUNCH(WORDS)                                                                                                                \
  do {                                                                                                                                        \
    PERO_LDS_ATTR((edit_ops_k<WORDS>), edit_lds(EDIT_MAX_L, EDIT_MAX_L, WORDS).bytes);                                                        \
    hipLaunchKernelGGL((edit_ops_k<WORDS>), dim3((unsigned)N), dim3(EDIT_THREADS), edit_lds((int)La, (int)Lb, WORDS).bytes, (hipStream_t)stream, \
                       a, b, a_len, b_len, is_sep, counts, script, script_len, a_spans, b_spans, (unsigned long long*)totals,                  \
                       (unsigned long long*)confusion, (int)La, (int)Lb, (int)C);                                                              \
  } while (0)

// The refusals both entry points share: sizes, the limit, and the rows (a row of width 0 may be null).
static int edit_check(const char* name, int64_t N, int64_t La, int64_t Lb, const int64_t* a, const int64_t* a_len, const int64_t* b,
                      const int64_t* b_len) {
  PERO_REQUIRE(N > 0 && N < (1LL << 31) && La >= 0 && Lb >= 0, "%s: bad sizes (N %lld, La %lld, Lb %lld)", name, (long long)N, (long long)La,
               (long long)Lb);
  if (La > EDIT_MAX_L || Lb > EDIT_MAX_L) {
    pero_set_error("%s: supported up to La, Lb = %d (got La %lld, Lb %lld)", name, EDIT_MAX_L, (long long)La, (long long)Lb);
    return PERO_E_UNSUPPORTED;
  }
  PERO_REQUIRE((a || La == 0) && (b || Lb == 0) && a_len && b_len, "%s: null pointer", name);
  return PERO_OK;
}

extern "C" int pero_edit_distance(const int64_t* a, const int64_t* a_len, const int64_t* b, const int64_t* b_len, int64_t* dist, int64_t* totals,
                                  int64_t N, int64_t La, int64_t Lb, void* stream) {
  const int rc = edit_check("pero_edit_distance", N, La, Lb, a, a_len, b, b_len);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE(dist, "pero_edit_distance: null pointer");
  hipLaunchKernelGGL(edit_distance_k, dim3((unsigned)N), dim3(EDIT_THREADS), 0, (hipStream_t)stream, a, b, a_len, b_len, dist,
                     (unsigned long long*)totals, (int)La, (int)Lb);
  PERO_CHECK_LAUNCH("pero_edit_distance");
  return PERO_OK;
}

extern "C" int pero_edit_ops(const int64_t* a, const int64_t* a_len, const int64_t* b, const int64_t* b_len, const uint8_t* is_sep, int64_t* counts,
                             int8_t* script, int32_t* script_len, int32_t* a_spans, int32_t* b_spans, int64_t* totals, int64_t* confusion, int64_t N,
                             int64_t La, int64_t Lb, int64_t C, void* stream) {
  PERO_REQUIRE(!(confusion || is_sep) || (C >= 1 && C < (1LL << 31) - 1), "pero_edit_ops: bad sizes (C %lld with a confusion matrix or separators)",
               (long long)C);
  const int rc = edit_check("pero_edit_ops", N, La, Lb, a, a_len, b, b_len);
  if (rc != PERO_OK) return rc;
  PERO_REQUIRE(counts, "pero_edit_ops: null pointer");
  PERO_REQUIRE(script_len ? (script || La + Lb == 0) : !script, "pero_edit_ops: null pointer (script and script_len are given together)");
  PERO_REQUIRE(!(confusion && is_sep), "pero_edit_ops: the confusion matrix is symbol level only (is_sep must be null with it)");
  PERO_REQUIRE(is_sep || !(a_spans || b_spans), "pero_edit_ops: a_spans and b_spans are word level only (is_sep is null)");
  if (!(confusion || is_sep)) C = 0;   // not used
  if (is_sep) EDIT_OPS_LAUNCH(true);
  else EDIT_OPS_LAUNCH(false);
  PERO_CHECK_LAUNCH("pero_edit_ops");
  return PERO_OK;
}
