"""f64 reference of pero_sim_topk / pero_retrieval_hist (include/pero_hip.h "Retrieval") for tests/test_gpu_retrieval.py, in the style of
tests/datapath_ref.py: scores in f64 from the very input values (for bf16 cases the bf16-rounded ones), the header's strict order
(higher score first, equal scores: lower key index first), a derived per-score rounding bound of the f32 evaluation, and the rank
positions at which that bound leaves no doubt ("sure")."""
import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24            # unit roundoff of f32
NEAR_TIE_CAP = 0.02       # the project's cap (tests/datapath_ref.py), here per rank position: of M * min(k, N)

# (M, N, D, k).  The kernel's tiles: 64 queries per workgroup, 128 keys per tile (32 per wave), 128 bytes of depth per stage = 32 f32 /
# 64 bf16 elements; lists of 4 (k <= 4) or 16 entries.
SHAPES = [(1, 1, 8, 1), (5, 3, 8, 16), (65, 33, 8, 4), (70, 200, 40, 16), (64, 128, 32, 10), (128, 256, 64, 16), (130, 300, 72, 16),
          (33, 1100, 16, 16),
          (63, 129, 24, 5),     # one query short of a query tile, one key past a key tile, D below the f32 stage; the first k on 16-entry lists
          (66, 127, 56, 4),     # one key short of a key tile, D below the bf16 stage; the last k on 4-entry lists
          (64, 257, 136, 10)]   # exactly one query tile; D one 16-byte chunk past 2 bf16 / 4 f32 stages (two chunks for f32)

# Bit-for-bit duplicate keys (n, n + delta): the two copies fall into every pair of places the kernel keeps keys apart.  Inside a 128-key
# tile key t sits in wave t / 32, lane half (t >> 2) & 1, accumulator register (t & 3) + 4 * ((t % 32) >> 3).
PLANTS = [(20, 1),      # other accumulator register of one lane (registers 8 and 9 of lane half 1, wave 0)
          (1, 4),       # other lane half, lower index in half 0 (key 1) and higher in half 1 (key 5)
          (12, 4),      # other lane half, the other order: key 12 in half 1, key 16 in half 0
          (3, 32),      # other wave: wave 0 and wave 1 of one tile
          (100, 64),    # next key tile AND the other order of waves: key 100 in wave 3 of tile 0, key 164 in wave 1 of tile 1
          (8, 128),     # next key tile, same wave, lane half and register.  Tiles 0 | 1 is also a split boundary for 2, 3 and 7 splits of N = 300
                        # (3 tiles: 0 | 1 2, 0 | 1 | 2, and 7 splits of which four are empty)
          (380, 8),     # other key split of N = 1100 (9 tiles) with 3 splits (tiles 0-2 | 3-5 | 6-8: key 380 in tile 2, 388 in tile 3) and with 7
          (500, 24)]    # other key split of N = 1100 with 2 splits (tiles 0-3 | 4-8: key 500 in tile 3, 524 in tile 4)


def to_dtype(a, dtype):
    """f32 array holding the values of `a` rounded to `dtype` (torch.float32: unchanged)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dtype).float().numpy()


def inv_norm_f32(x):
    """f32 1 / max(|x_r|, 1e-12): scales handed to the kernel as INPUTS (the reference takes these f32 values as they are)."""
    n = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    return (1.0 / np.maximum(n, 1e-12)).astype(F32)


def case(M, N, D, dtype=torch.float32):
    """q (M, D), keys (N, D) as f32 arrays of `dtype`-representable values, and the plants: (query row, lower key, higher key) with
    keys[higher] a copy of keys[lower] and q[row] equal to both, for every pair of PLANTS that N (and M) has room for."""
    rng = np.random.default_rng(100000 * M + 100 * N + D)
    q = to_dtype(rng.standard_normal((M, D)), dtype)
    keys = to_dtype(rng.standard_normal((N, D)), dtype)
    plants = []
    for n, delta in PLANTS:
        if n + delta < N and len(plants) < M:
            keys[n + delta] = keys[n]
            row = (7 * len(plants) + 3) % M
            assert row not in [p[0] for p in plants]
            q[row] = keys[n]
            plants.append((row, n, n + delta))
    return q, keys, plants


def scores64(q, keys, q_scale=None, key_scale=None):
    s = q.astype(np.float64) @ keys.astype(np.float64).T
    if q_scale is not None:
        s = s * np.asarray(q_scale, dtype=np.float64)[:, None]
    if key_scale is not None:
        s = s * np.asarray(key_scale, dtype=np.float64)[None, :]
    return s


def rounding_bound(q, keys, q_scale=None, key_scale=None, scales="given"):
    """(M, N) bound on |f32 evaluation - f64 score| of score = ((q . key) q_scale) key_scale, in units u = 2^-24 of
    A = |q|_2 |key|_2 |q_scale| |key_scale| (>= sum_i |q_i key_i| |q_scale key_scale| by Cauchy-Schwarz; A is about 1 for a cosine):
      the dot     a D-term f32 accumulation.  The f32 MFMA is a chain of D fused multiply-adds, one rounding (u) each; the bf16 MFMA's
                  products are exact in f32 and its adders are not documented to round to nearest, so every addition is given a
                  truncation's 2u: (2 D + 2) u A, the 2 covering the second-order terms;
      the scales  two f32 multiplications, u each relative to a value of at most A (1 + small): 2 u A.  With both scales null there is
                  none, and the bound is only the larger for it;
      scales="computed" (retrieve(normalize=True): the scales are themselves f32 results, compared against exact norms): D squares added
                  in f32, (D + 1) u relative, halved by the square root; the root and the division round once each: (D + 1) / 2 + 2 per
                  scale, (D + 5) u A for both.
    In all (2 D + 4) u A for given scales, (3 D + 9) u A for computed ones, plus the smallest normal number."""
    D = q.shape[1]
    nq = np.sqrt((q.astype(np.float64) ** 2).sum(1))
    nk = np.sqrt((keys.astype(np.float64) ** 2).sum(1))
    if q_scale is not None:
        nq = nq * np.abs(np.asarray(q_scale, dtype=np.float64))
    if key_scale is not None:
        nk = nk * np.abs(np.asarray(key_scale, dtype=np.float64))
    units = (2 * D + 4) + ((D + 5) if scales == "computed" else 0)
    return units * U * nq[:, None] * nk[None, :] + 2.0 ** -126


def rank(scores, k, key_valid=None, skip=None):
    """The header's lists from an (M, N) score matrix: idx (M, k) int32 / val (M, k) of the matrix's dtype, -1 / -inf behind the last
    qualifying key; nq (M): how many keys qualify; order (M, N): all keys, the qualifying ones first in the strict order."""
    M, N = scores.shape
    out = np.zeros((M, N), dtype=bool) | np.isnan(scores)
    if key_valid is not None:
        out |= (np.asarray(key_valid) == 0)[None, :]
    if skip is not None:
        out |= np.arange(N)[None, :] == np.asarray(skip)[:, None]
    s = np.where(out, -np.inf, scores)
    # a stable sort on the negated score keeps equal scores in index order; keys that are out go behind every real -inf
    order = np.lexsort((np.broadcast_to(np.arange(N), (M, N)), -s, out), axis=1)
    nq = (~out).sum(1)
    kk = min(k, N)
    idx = np.full((M, k), -1, dtype=np.int32)
    val = np.full((M, k), -np.inf, dtype=scores.dtype)
    top = order[:, :kk]
    live = np.arange(kk)[None, :] < nq[:, None]
    idx[:, :kk] = np.where(live, top, -1)
    val[:, :kk] = np.where(live, np.take_along_axis(s, top, 1), -np.inf)
    return idx, val, nq, order


def key_classes(keys, key_scale=None):
    """class id per key: equal ids = bit-for-bit equal rows (and scales), whose f32 scores are the same bits for every query."""
    rows = np.ascontiguousarray(keys, dtype=F32).view(np.uint32)
    if key_scale is not None:
        rows = np.concatenate([rows, np.asarray(key_scale, dtype=F32).view(np.uint32)[:, None]], axis=1)
    return np.unique(rows, axis=0, return_inverse=True)[1].reshape(-1)


def sure_positions(scores, bound, order, nq, k, classes):
    """(M, min(k, N)) bool: rank position (m, r), r < nq[m], is SURE when the f64 gaps to its neighbours in the ranking - rank r - 1 and
    rank r + 1, which at r = k - 1 is the first key left out - both exceed the sum of the two scores' bounds.  A neighbour that is a
    bit-for-bit copy of the key (same class) does not make a position unsure: the two f32 scores are the same bits and the header's tie
    rule, lower index first, decides - which is what the planted copies are there to test."""
    M, N = scores.shape
    kk = min(k, N)
    w = min(kk + 1, N)
    top = order[:, :w]
    s = np.take_along_axis(scores, top, 1)
    b = np.take_along_axis(bound, top, 1)
    c = classes[top]
    live = np.arange(w)[None, :] < nq[:, None]
    # sep[:, j]: positions j and j + 1 are kept apart (or j + 1 does not exist)
    with np.errstate(invalid="ignore"):
        apart = (s[:, :-1] - s[:, 1:] > b[:, :-1] + b[:, 1:]) | (c[:, :-1] == c[:, 1:])
    sep = apart | ~live[:, 1:]
    sep = np.concatenate([sep, np.ones((M, kk + 1 - sep.shape[1]), dtype=bool)], axis=1)[:, :kk]     # no lower neighbour at all: N <= k
    up = np.concatenate([np.ones((M, 1), dtype=bool), sep[:, :kk - 1]], axis=1)
    return up & sep & live[:, :kk]


def reference(q, keys, k, q_scale=None, key_scale=None, key_valid=None, skip=None, scales="given"):
    """Everything the parity test needs, computed once per case."""
    s = scores64(q, keys, q_scale, key_scale)
    b = rounding_bound(q, keys, q_scale, key_scale, scales)
    idx, val, nq, order = rank(s, k, key_valid, skip)
    sure = sure_positions(s, b, order, nq, k, key_classes(keys, key_scale))
    return {"scores": s, "bound": b, "idx": idx, "val": val, "nq": nq, "order": order, "sure": sure}


def hist_loop(idx, target, k):
    """pero_retrieval_hist as a plain loop."""
    h = [0] * (k + 2)
    for row, t in zip(np.asarray(idx).tolist(), np.asarray(target).tolist()):
        if t < 0:
            continue
        h[0] += 1
        h[1 + (row.index(t) if t in row else k)] += 1
    return h


def alignment_targets_loop(im1, im2, sm1, sm2):
    """alignment_targets as a plain loop over the masks: the j-th position of view 1 with both masks 1 pairs with the j-th such position
    of view 2; a line whose views select different numbers has no pairs."""
    im1, im2, sm1, sm2 = (np.asarray(m) for m in (im1, im2, sm1, sm2))
    lines, S = im1.shape
    out = np.full((lines, S), -1, dtype=np.int32)
    for l in range(lines):
        p1 = [p for p in range(S) if im1[l, p] == 1 and sm1[l, p] == 1]
        p2 = [p for p in range(S) if im2[l, p] == 1 and sm2[l, p] == 1]
        if len(p1) == len(p2):
            for a, b in zip(p1, p2):
                out[l, a] = l * S + b
    return out
