"""Plain torch f64 restatement of the three CTC entry points of include/pero_hip.h (pero_ctc_fwd, pero_ctc_bwd, pero_ctc_greedy),
written from the header's formulas (not a test module; it never imports the library).  Like parity_ref.py, every result comes
with `mag`, and the comparisons go through parity_ref.assert_within.

Error budget, in parity_ref's units (u = 2^-24; EXPF, LOGF units per call; exp_arg_units for the argument of an expf).

Row log-sum-exp, lse = mx + log sum_c exp(x_c - mx).  Its ABSOLUTE error in units, `row_units`:
  * the arguments x_c - mx are rounded: a relative error sum_c p_c |d_c| u of the sum, d_c = x_c - mx = log p_c + log Z with Z >= 1,
    so |d_c| <= -log p_c and the weighted sum is at most the row's entropy <= ln C                      -> ln C
  * expf                                                                                                -> EXPF
  * C terms added in any order                                                                          -> C - 1
  * logf of a value in [0, ln C]: LOGF units relative to at most ln C                                   -> LOGF ln C
  * the rounding of mx + log(..), of magnitude |lse|                                                    -> |lse|
  row_units = ceil(ln C + EXPF + (C - 1) + LOGF ln C + max |lse|).

One step of the recursion, new = m + log(sum_i exp(a_i - m)) + (x - lse), m = max of the (up to three) finite a_i.  An absolute
error of a log-alpha passes through this map with factor <= 1 (the derivatives of log-sum-exp are weights that sum to 1), so the
steps' own errors ADD.  With A = max |finite log-alpha| of the line (every log-alpha and every emission that reaches one is <= 0
and no larger in magnitude than A):
  absolute, not scaled (units of u):   the rounded arguments a_i - m, weight e^d |d| <= 1/e each        -> 1
                                       expf                                                             -> EXPF
                                       the three-term sum                                               -> 2
                                       logf of a value in [0, ln 3]                                     -> ceil(LOGF ln 3) = 3
                                       the error of lse inside the emission                             -> row_units
  scaled by the magnitude (units of u (A + 1)):
                                       m + log(..), magnitude <= A + ln 3 <= 2 (A + 1)                  -> 2
                                       x - lse, magnitude |emission| <= A                               -> 1
                                       the sum with the emission, magnitude <= A                        -> 1
  per-step units K = 4 + ceil((1 + EXPF + 2 + 3 + row_units) / (A + 1)).
nll = -logaddexp of two entries of the last row is one more step of that shape, so

    |nll - ref| <= (T + 1) K u (A + 1).

(For scale: C = 37, logits 4 randn, T = 24: row_units ~ 65, A ~ 200, K = 5, bound ~ 1.7e-3 on nll ~ 200; torch's own f32
ctc_loss is 3e-6 .. 4e-5 from f64 there.)  beta obeys the same recursion backwards, with B = max |finite log-beta|; M = max(A, B)
and K is evaluated at M.

A gradient entry is g (p_c - sum_{s in class c} w_s), p_c = exp(x_c - lse), w_s = exp(((alpha_t(s) + beta_t(s)) + nll) - (x_c - lse)).
The RELATIVE error of an expf is the ABSOLUTE error of its argument:
  * alpha_t(s): t + 1 steps, beta_t(s): T - t steps, nll: T + 1 steps                                   -> 2 (T + 1) K (M + 1)
  * the roundings of forming the argument: alpha + beta (magnitude <= 2 M), + nll (<= M), x - lse (<= M), the difference (<= M)
                                                                                                        -> exp_arg_units(2 M, M, M, M)
  * p_c: the rounding of x_c - lse (at most the row's range R)                                          -> exp_arg_units(R)
  * lse's own error, expf, the product with g                                                           -> row_units + EXPF + 1
`grad_units` is their sum; the terms are p_c and the w_s of the class (at most L + 1 of them: n_terms = L + 2), the magnitude
|g| (p_c + sum w_s).  bf16 logits are rounded once on the host; the reference is evaluated on the rounded values, and a bf16
gradient gets parity_ref's one output rounding."""
import math

import torch

from parity_ref import EXPF, LOGF, exp_arg_units, f64

NEG_INF = -math.inf


def extended(targets_n, L, blank):
    ext = torch.full((2 * L + 1,), blank, dtype=torch.int64)
    ext[1::2] = targets_n[:L]
    return ext


def _lse3(a, b, c):
    return torch.logsumexp(torch.stack((a, b, c)), dim=0)   # -inf where all three are -inf


def _shift(v, k):
    """v moved k entries to the right (k > 0) or left (k < 0), -inf shifted in."""
    out = torch.full_like(v, NEG_INF)
    if k > 0:
        out[k:] = v[:-k] if k < v.numel() else v[:0]
    else:
        out[:k] = v[-k:] if -k < v.numel() else v[:0]
    return out


def _max_finite(v):
    f = v[torch.isfinite(v)]
    return float(f.abs().max()) if f.numel() else 0.0


def ctc(logits, targets, input_lengths, target_lengths, blank, g=None, zero_infinity=False):
    """logits (N, S, C), targets (N, Lmax), lengths (N), g (N) or None (= 1).
    res: nll (N), row_lse (N, S), grad (N, S, C) (NaN in the rows the header leaves unspecified), alpha / beta: per-line (T, L') lists.
    mag: nll (N) = M + 1, nll_terms (N) = (T + 1) K, grad (N, S, C), grad_terms, grad_units (N), row_units (absolute, of the rows t < T)."""
    x = f64(logits)
    N, S, C = x.shape
    targets, il, tl = (torch.as_tensor(t).cpu().long() for t in (targets, input_lengths, target_lengths))
    gs = torch.ones(N, dtype=torch.float64) if g is None else f64(g)
    lse = torch.logsumexp(x, dim=-1)
    nll = torch.zeros(N, dtype=torch.float64)
    grad, gmag = torch.zeros_like(x), torch.zeros_like(x)
    mag_nll, nll_terms, grad_units, alphas, betas, all_row_units = torch.zeros(N, dtype=torch.float64), [], [], [], [], [0]
    for n in range(N):
        T, L = int(il[n]), int(tl[n])
        Lp = 2 * L + 1
        ext = extended(targets[n], L, blank)
        if T == 0:
            nll[n] = 0.0 if L == 0 else math.inf
            mag_nll[n] = 1.0
            nll_terms.append(1)
            grad_units.append(0)
            alphas.append(torch.zeros(0, Lp))
            betas.append(torch.zeros(0, Lp))
            continue
        lp = x[n, :T] - lse[n, :T, None]
        e = lp[:, ext]                                                        # (T, L')
        skip = torch.zeros(Lp, dtype=torch.bool)                              # s - 2 -> s is a transition
        skip[2:] = ext[2:] != ext[:-2]
        alpha = torch.full((T, Lp), NEG_INF, dtype=torch.float64)
        alpha[0, :2] = e[0, :2]
        for t in range(1, T):
            p = alpha[t - 1]
            alpha[t] = e[t] + _lse3(p, _shift(p, 1), torch.where(skip, _shift(p, 2), torch.full_like(p, NEG_INF)))
        nll[n] = -torch.logsumexp(alpha[T - 1, max(Lp - 2, 0):], dim=0)
        skipf = torch.zeros(Lp, dtype=torch.bool)                             # s -> s + 2 is a transition
        skipf[:-2] = skip[2:]
        beta = torch.full((T, Lp), NEG_INF, dtype=torch.float64)
        beta[T - 1, max(Lp - 2, 0):] = e[T - 1, max(Lp - 2, 0):]
        for t in range(T - 2, -1, -1):
            q = beta[t + 1]
            beta[t] = e[t] + _lse3(q, _shift(q, -1), torch.where(skipf, _shift(q, -2), torch.full_like(q, NEG_INF)))
        alphas.append(alpha)
        betas.append(beta)
        # ---- budget
        A, B = _max_finite(alpha), _max_finite(beta)
        M = max(A, B)
        row_units = math.ceil(math.log(C) + EXPF + (C - 1) + LOGF * math.log(C) + float(lse[n, :T].abs().max()))
        K = 4 + math.ceil((1 + EXPF + 2 + 3 + row_units) / (M + 1))
        all_row_units.append(row_units)
        mag_nll[n] = M + 1
        nll_terms.append((T + 1) * K)
        R = float((x[n, :T].max(-1).values - x[n, :T].min(-1).values).max())
        grad_units.append(2 * (T + 1) * K * math.ceil(M + 1) + exp_arg_units(2 * M, M, M, M) + exp_arg_units(R) + row_units + EXPF + 1)
        # ---- gradient
        p = torch.exp(lp)
        if math.isinf(float(nll[n])):
            if not zero_infinity:
                grad[n, :T] = math.nan
            continue
        w = torch.exp(alpha + beta + nll[n] - e)                              # (T, L'), exp(-inf) = 0
        occ = torch.zeros(T, C, dtype=torch.float64).index_add_(1, ext, w)
        grad[n, :T] = gs[n] * (p - occ)
        gmag[n, :T] = gs[n].abs() * (p + occ)
    res = {"nll": nll, "row_lse": lse, "grad": grad, "alpha": alphas, "beta": betas}
    mag = {"nll": mag_nll, "nll_terms": torch.tensor(nll_terms, dtype=torch.float64), "grad": gmag, "grad_terms": int(tl.max()) + 2 if N else 2,
           "grad_units": grad_units, "row_units": max(all_row_units)}
    return res, mag


def reduce(nll, target_lengths, reduction, zero_infinity=False, mag_nll=None):
    """torch.nn.CTCLoss's reductions of the (N) vector; with mag_nll also the magnitude of the reduced value."""
    nll = f64(nll)
    tl = f64(target_lengths).clamp_min(1.0)
    inf = torch.isinf(nll)
    if zero_infinity:
        nll = torch.where(inf, torch.zeros_like(nll), nll)
    m = None if mag_nll is None else torch.where(inf, torch.zeros_like(nll), f64(mag_nll))
    if reduction == "none":
        return (nll, m) if m is not None else nll
    if reduction == "sum":
        return (nll.sum(), m.sum()) if m is not None else nll.sum()
    if reduction == "mean":
        return ((nll / tl).mean(), (m / tl).mean()) if m is not None else (nll / tl).mean()
    raise ValueError(reduction)


def greedy(logits, input_lengths, blank):
    """Per row the first maximal class; per line over t < T repeats collapsed, then blanks dropped.  out (N, S) int64 padded with -1, lengths (N)."""
    x = f64(logits)
    N, S, C = x.shape
    il = torch.as_tensor(input_lengths).cpu().long().clamp(0, S)
    top = x.max(-1, keepdim=True).values
    am = torch.where(x == top, torch.arange(C).expand(N, S, C), torch.full((N, S, C), C)).min(-1).values   # the first maximum
    prev = torch.cat((torch.full((N, 1), -1, dtype=torch.int64), am[:, :-1]), dim=1)
    keep = (am != prev) & (am != blank) & (torch.arange(S)[None, :] < il[:, None])
    out = torch.full((N, S), -1, dtype=torch.int64)
    lengths = keep.sum(1)
    for n in range(N):
        out[n, :int(lengths[n])] = am[n][keep[n]]
    return out, lengths


def levenshtein(a, b):
    """The textbook full-table edit distance (the package's helper keeps one row)."""
    d = [[max(i, j) if 0 in (i, j) else 0 for j in range(len(b) + 1)] for i in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return d[len(a)][len(b)]


# ---------------------------------------------------------------------------------------------- the shared case list
SENTINEL = 1 << 40   # padding entries of `targets`: far outside every class range; reading one would change a result


def _labels(gen, count, C, blank):
    """`count` random non-blank classes"""
    pool = torch.tensor([c for c in range(C) if c != blank])
    return pool[torch.randint(len(pool), (count,), generator=gen)]


def mixed_case(C, blank, scale, seed=0):
    """N = 6 lines at S = 24, Lmax = 26 > max L: L = 0 | L = 1 | L = 5 with 9 frames | 12 equal labels (needs 23 frames) | L = T = 24 all
    distinct (one path; two equal labels where C - 1 < 24) | 13 equal labels (needs 25 frames: infeasible)."""
    gen = torch.Generator().manual_seed(seed + 1000 * C + blank)
    N, S, Lmax = 6, 24, 26
    logits = scale * torch.randn(N, S, C, generator=gen)
    one = int(_labels(gen, 1, C, blank)[0])
    distinct = torch.tensor([c for c in range(C) if c != blank])[torch.randperm(C - 1, generator=gen)][:24] if C - 1 >= 24 else torch.full((2,), one)
    lines = [torch.zeros(0, dtype=torch.int64), _labels(gen, 1, C, blank), _labels(gen, 5, C, blank), torch.full((12,), one), distinct,
             torch.full((13,), one)]
    targets = torch.full((N, Lmax), SENTINEL, dtype=torch.int64)
    for n, l in enumerate(lines):
        targets[n, :len(l)] = l
    return {"logits": logits, "targets": targets, "input_lengths": torch.tensor([24, 24, 9, 24, 24, 24]),
            "target_lengths": torch.tensor([len(l) for l in lines]), "blank": blank, "infeasible": [5]}


def long_case(S, lengths, input_lengths, C=37, blank=0, scale=4.0, seed=0):
    gen = torch.Generator().manual_seed(seed + S)
    N, Lmax = len(lengths), max(lengths) + 1
    logits = scale * torch.randn(N, S, C, generator=gen)
    targets = torch.full((N, Lmax), SENTINEL, dtype=torch.int64)
    for n, L in enumerate(lengths):
        targets[n, :L] = _labels(gen, L, C, blank)
    return {"logits": logits, "targets": targets, "input_lengths": torch.tensor(input_lengths), "target_lengths": torch.tensor(lengths),
            "blank": blank, "infeasible": []}


def _case_table():
    table = {}
    for C in (2, 37, 130):
        for blank in (0, C - 1):
            for scale in (4.0, 30.0):
                table[f"mixed-C{C}-blank{blank}-x{int(scale)}"] = (mixed_case, (C, blank, scale))
    table["wave-S72-L31-32-33"] = (long_case, (72, [31, 32, 33], [72, 72, 70]))       # L' = 63, 65, 67 straddle a wave
    table["block-S264-L130"] = (long_case, (264, [130, 100], [264, 250]))             # L' = 261 > 256 threads
    return table


CASES = _case_table()


def case(name):
    fn, args = CASES[name]
    return fn(*args)


def greedy_case():
    """N = 4, S = 12, C = 7: planted ties (the first maximum wins), a repeat across a blank, a line of 7 frames, an empty line (input_length 0).
    Every planted value is exact in bf16."""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(4, 12, 7, generator=gen)
    x[0, 0, [2, 5]] = 9.0            # tie: 2
    x[0, 1, [2, 6]] = 9.0            # tie: 2 again -> collapsed
    x[0, 2, 0] = 9.0                 # class 0
    x[0, 3, [2, 3, 4]] = 9.0         # 2 after another class -> emitted again
    x[0, 4, :] = 1.0                 # every class ties: class 0
    x[1, :, 3] = 20.0                # one label the whole line
    return x, torch.tensor([12, 12, 7, 0]), 0
