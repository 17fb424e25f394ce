"""pero_edit_ops restated in plain Python (include/pero_hip.h "Edit operations"): the table, the walk back with its tie rule, the split
into words, counts, confusion counts and totals.  Integers only; it does not import the library.  Also here: the cases the CPU and GPU
tests share, and the padding helper."""
import itertools
import random

import torch

HIT, SUB, INS, DEL = 0, 1, 2, 3


def table(a, b):
    """D[i][j] = distance of a[:i] and b[:j]."""
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return D


def walk(a, b):
    """The script in forward order, as (code, i, j) with i, j the 1-based elements the step involves (0: none)."""
    D = table(a, b)
    i, j, steps = len(a), len(b), []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1][j - 1] + (a[i - 1] != b[j - 1]) == D[i][j]:
            steps.append((HIT if a[i - 1] == b[j - 1] else SUB, i, j))
            i, j = i - 1, j - 1
        elif j > 0 and D[i][j - 1] + 1 == D[i][j]:
            steps.append((DEL, 0, j))
            j -= 1
        else:
            steps.append((INS, i, 0))
            i -= 1
    return steps[::-1]


def script(a, b):
    return [s[0] for s in walk(a, b)]


def counts(codes):
    """(substitutions, insertions, deletions, hits)."""
    return [codes.count(SUB), codes.count(INS), codes.count(DEL), codes.count(HIT)]


def replay(a, b, codes):
    """Apply a script to a, taking from b what a substitution or a deletion puts there: the string it builds.  Raises if a hit meets unequal
    elements, a substitution equal ones, or the script does not use up both strings."""
    i, j, out = 0, 0, []
    for c in codes:
        if c in (HIT, SUB):
            if (a[i] == b[j]) != (c == HIT):
                raise ValueError(f"code {c} at ({i}, {j}): {a[i]} against {b[j]}")
            out.append(a[i] if c == HIT else b[j])
            i, j = i + 1, j + 1
        elif c == INS:
            i += 1          # a's element is dropped
        elif c == DEL:
            out.append(b[j])
            j += 1
        else:
            raise ValueError(f"code {c}")
    if i != len(a) or j != len(b):
        raise ValueError("the script does not cover both strings")
    return out


def words(row, is_sep, C):
    """[(begin, end)] of the words of a row: maximal runs of labels c with not (0 <= c < C and is_sep[c])."""
    spans, begin = [], None
    for p, c in enumerate(list(row) + [None]):
        inside = c is not None and not (0 <= c < C and is_sep[c])
        if inside and begin is None:
            begin = p
        if not inside and begin is not None:
            spans.append((begin, p))
            begin = None
    return spans


def sep_table(separators, C):
    return [1 if c in set(separators) else 0 for c in range(C)]


def expected(a, a_len, b, b_len, C=None, separators=None, confusion=False):
    """The outputs of pero_edit_ops for padded int64 matrices a (N, La), b (N, Lb) and lengths (clamped here as the library does):
    dict of counts (N, 4) int64, script (N, La + Lb) int8, script_len (N) int32, totals (6) int64 of one call, and with separators a_spans,
    b_spans, with confusion=True the (C + 1, C + 1) int64 matrix of one call."""
    N, La, Lb = a.shape[0], a.shape[1], b.shape[1]
    out = {"counts": torch.zeros((N, 4), dtype=torch.int64), "script": torch.full((N, La + Lb), -1, dtype=torch.int8),
           "script_len": torch.zeros(N, dtype=torch.int32), "totals": torch.zeros(6, dtype=torch.int64)}
    if separators is not None:
        is_sep = sep_table(separators, C)
        out["a_spans"] = torch.full((N, (La + 1) // 2, 2), -1, dtype=torch.int32)
        out["b_spans"] = torch.full((N, (Lb + 1) // 2, 2), -1, dtype=torch.int32)
    if confusion:
        out["confusion"] = torch.zeros((C + 1, C + 1), dtype=torch.int64)
    for n in range(N):
        x = a[n, :min(max(int(a_len[n]), 0), La)].tolist()
        y = b[n, :min(max(int(b_len[n]), 0), Lb)].tolist()
        if separators is not None:
            wa, wb = words(x, is_sep, C), words(y, is_sep, C)
            for k, s in enumerate(wa):
                out["a_spans"][n, k] = torch.tensor(s, dtype=torch.int32)
            for k, s in enumerate(wb):
                out["b_spans"][n, k] = torch.tensor(s, dtype=torch.int32)
            x, y = [tuple(x[s:e]) for s, e in wa], [tuple(y[s:e]) for s, e in wb]
        steps = walk(x, y)
        codes = [s[0] for s in steps]
        c = counts(codes)
        out["counts"][n] = torch.tensor(c)
        out["script"][n, :len(codes)] = torch.tensor(codes, dtype=torch.int8)
        out["script_len"][n] = len(codes)
        out["totals"] += torch.tensor(c + [1, 1 if c[0] + c[1] + c[2] else 0])
        if confusion:
            for code, i, j in steps:
                h = x[i - 1] if i else C
                r = y[j - 1] if j else C
                if (i == 0 or 0 <= h < C) and (j == 0 or 0 <= r < C):
                    out["confusion"][r, h] += 1
    return out


def pad(rows, width, fill=1):
    """(N, width) int64 matrix of the rows, filled behind each row with `fill` (a label that may occur in the rows), and their lengths."""
    m = torch.full((len(rows), width), fill, dtype=torch.int64)
    for n, r in enumerate(rows):
        m[n, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return m, torch.tensor([len(r) for r in rows], dtype=torch.int64)


def random_pairs(count, max_len, symbols, seed):
    rng = random.Random(seed)
    return [([rng.randrange(symbols) for _ in range(rng.randint(0, max_len))], [rng.randrange(symbols) for _ in range(rng.randint(0, max_len))])
            for _ in range(count)]


def noisy_copy(row, symbols, rng, rate=0.15):
    """A copy of the row with some labels changed, dropped or doubled: pairs that share long stretches, like a recogniser's output."""
    out = []
    for c in row:
        u = rng.random()
        if u < rate / 3:
            continue
        out.append(rng.randrange(symbols) if u < 2 * rate / 3 else c)
        if u > 1 - rate / 3:
            out.append(rng.randrange(symbols))
    return out


def all_scripts_minimum(a, b):
    """The length of the cheapest script by brute force: every way to interleave keep / substitute / insert / delete."""
    best = [len(a) + len(b)]

    def go(i, j, cost):
        if cost >= best[0] and not (i == len(a) and j == len(b)):
            return
        if i == len(a) and j == len(b):
            best[0] = min(best[0], cost)
            return
        if i < len(a) and j < len(b):
            go(i + 1, j + 1, cost + (a[i] != b[j]))
        if i < len(a):
            go(i + 1, j, cost + 1)
        if j < len(b):
            go(i, j + 1, cost + 1)
    go(0, 0, 0)
    return best[0]


def small_strings(max_len=4, symbols=2):
    return [list(s) for n in range(max_len + 1) for s in itertools.product(range(symbols), repeat=n)]


# word-level cases, C = 8, separators {0, 7}: (hypothesis, reference)
WORD_C, WORD_SEPS = 8, (0, 7)
WORD_CASES = [
    ([0, 1, 2, 0, 3, 0], [1, 2, 0, 3]),                      # separators at both ends
    ([1, 2, 0, 0, 7, 0, 3, 4], [1, 2, 0, 3, 4]),             # runs of separators, two separator classes
    ([0, 7, 0, 0], [1, 2, 0, 3]),                            # a line of separators only: no words
    ([0, 0], [7]),                                           # both sides without words
    ([1, 2, 0, 3], [1, 2, 3, 0, 3]),                         # words that differ only in length: 1 2 against 1 2 3
    ([1, 2, 3, 0, 4], [1, 2, 4, 0, 4]),                      # words equal except for their last label
    ([1, -1, 2, 0, 3, 11, 0, 5], [1, -1, 2, 0, 3, 12, 0, 5]),   # labels outside [0, C) inside words: they belong to the word and are compared
    ([], [1, 0, 2]),
    ([1, 0, 2], []),
    ([3, 0, 3, 0, 3, 0, 4], [3, 0, 4, 0, 3]),                # repeated words
]
