"""Restatements of pero_ctc_align (include/pero_hip.h), written from the header's formulas (not a test module; it never imports the
library):

  align_f32    the recursion, tie rule, walk back, spans and path_logit in numpy float32.  The recursion holds f32 additions and
               comparisons only and the library is built without fused multiply-adds, so the kernel must give the SAME BITS: states,
               spans and path_logit are compared as integers, with no margin.
  align_f64    the f64 values of path_logit, score and label_logp along a GIVEN path (the kernel's own), their error budgets, and the
               f64 optimum of the line.
  brute_force  every state path of a tiny line, one by one; the best by (value, state sequence read from the last frame backwards).

Error budgets, ABSOLUTE, in parity_ref's unit u = 2^-24 (EXPF, LOGF: units of one call), to first order like parity_ref's own.  They go
through parity_ref.assert_within with mag = 1 and n_terms = the units.  Nothing here is fitted to the kernel.

path_logit = ((x_0 + x_1) + x_2) + .. along the path: T f32 additions, each rounding its result, a partial sum:
    path_units = T max_t |x_0 + .. + x_t|.
The same bound holds between the f32 and the f64 value of ANY path, so the f64 value of the f32-best path is within
2 path_units (the larger of the two paths') of the f64 optimum: both f32 values are within their bound of the f64 ones, and the
f32-best path's f32 value is no smaller than the f64-best path's.

Row log-sum-exp, after ctc_ref.py: row_units = ceil(ln C + EXPF + (C - 1) + LOGF ln C + max_t |lse_t|) per row t < T.

score = path_logit - (((lse_0 + lse_1) + ..) + lse_{T-1}):
    path_units                                   the path's own additions
  + T row_units                                  the error of every lse_t
  + T max_t |lse_0 + .. + lse_t|                 the T roundings of the lse sum
  + |path_logit| + |sum lse|                     the final difference, rounded once (its magnitude is at most the sum of the two)
label_logp_k = sum_{t in span k} (x_t(l_k) - lse_t), n_k frames:
    n_k row_units                                the error of every lse_t
  + sum_t |x_t(l_k) - lse_t|                     every difference is rounded once
  + n_k max |partial sum|                        the n_k additions
bf16 logits are rounded once on the host; every function here sees the rounded values."""
import math

import numpy as np
import torch

from parity_ref import EXPF, LOGF

NEG_INF = -math.inf


def clamp(v, hi):
    return min(max(int(v), 0), hi)


def state_classes(targets_n, L, C, blank):
    """class of every extended state (even: blank); -1 for a label outside [0, C): such a state emits -inf"""
    cls = np.full(2 * L + 1, blank, dtype=np.int64)
    for k in range(L):
        l = int(targets_n[k])
        cls[2 * k + 1] = l if 0 <= l < C else -1
    return cls


def _emissions(x, cls, T, dtype):
    """(T, L') emissions in `dtype`; x (S, C)"""
    x = np.asarray(x, dtype=dtype)
    e = np.full((T, len(cls)), NEG_INF, dtype=dtype)
    ok = cls >= 0
    e[:, ok] = x[:T][:, cls[ok]]
    return e


def _viterbi(e, cls):
    """the header's recursion in e's dtype: (v_{T-1}, back (T, L')).  Equal values -> the smallest step; all -inf -> 0."""
    T, Lp = e.shape
    dtype = e.dtype
    skip = np.zeros(Lp, dtype=bool)
    skip[2:] = cls[2:] != cls[:-2]
    v = np.full(Lp, NEG_INF, dtype=dtype)
    v[:2] = e[0, :2]
    back = np.zeros((T, Lp), dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            a1 = np.full(Lp, NEG_INF, dtype=dtype)
            a2 = np.full(Lp, NEG_INF, dtype=dtype)
            a1[1:] = v[:-1]
            a2[2:] = v[:-2]
            a2[~skip] = NEG_INF
            best, step = v.copy(), np.zeros(Lp, dtype=np.int8)
            m = a1 > best
            best[m], step[m] = a1[m], 1
            m = a2 > best
            best[m], step[m] = a2[m], 2
            v = e[t] + best          # one addition per state, in e's dtype
            back[t] = step
    assert v.dtype == dtype
    return v, back


def _end_state(v):
    Lp = len(v)
    return Lp - 1 if Lp == 1 or v[Lp - 1] >= v[Lp - 2] else Lp - 2


def spans_of(states, T, Lmax):
    """[first frame, last frame + 1) of every label's state 2 k + 1; -1 where the path has none"""
    spans = np.full((Lmax, 2), -1, dtype=np.int32)
    for t in range(T):
        s = int(states[t])
        if s & 1:
            if spans[s >> 1, 0] < 0:
                spans[s >> 1, 0] = t
            spans[s >> 1, 1] = t + 1
    return spans


def _align(x, targets_n, T, L, blank, dtype):
    """one line in `dtype`: (feasible, states (T), value)"""
    C = x.shape[1]
    if T == 0:
        return L == 0, np.zeros(0, dtype=np.int32), dtype(0.0)
    cls = state_classes(targets_n, L, C, blank)
    v, back = _viterbi(_emissions(x, cls, T, dtype), cls)
    s = _end_state(v)
    value = v[s]
    if not np.isfinite(value):
        return False, np.zeros(0, dtype=np.int32), dtype(NEG_INF)
    states = np.zeros(T, dtype=np.int32)
    states[T - 1] = s
    for t in range(T - 1, 0, -1):
        s -= int(back[t, s])
        states[t - 1] = s
    return True, states, value


def align_f32(logits, targets, input_lengths, target_lengths, blank):
    """logits (N, S, C) holding f32 values; targets (N, Lmax); lengths (N).  The outputs the kernel must reproduce bit for bit:
    states (N, S) int32, spans (N, Lmax, 2) int32, path_logit (N) float32, and feasible (N) bool."""
    x = np.asarray(torch.as_tensor(logits).float().numpy(), dtype=np.float32)
    targets = np.asarray(torch.as_tensor(targets).numpy())
    N, S, C = x.shape
    Lmax = targets.shape[1]
    states = np.full((N, S), -1, dtype=np.int32)
    spans = np.full((N, Lmax, 2), -1, dtype=np.int32)
    path_logit = np.full(N, NEG_INF, dtype=np.float32)
    feasible = np.zeros(N, dtype=bool)
    for n in range(N):
        T, L = clamp(input_lengths[n], S), clamp(target_lengths[n], Lmax)
        ok, st, value = _align(x[n], targets[n], T, L, blank, np.float32)
        feasible[n] = ok
        if ok:
            states[n, :T] = st
            spans[n] = spans_of(st, T, Lmax)
            path_logit[n] = value
    return {"states": states, "spans": spans, "path_logit": path_logit, "feasible": feasible}


def _lse64(rows):
    """log sum exp of every row in f64; -inf for a row of -inf"""
    m = rows.max(axis=1)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), safe + np.log(np.exp(rows - safe[:, None]).sum(axis=1)), NEG_INF)


def _max_abs_partial(terms):
    return float(np.abs(np.cumsum(terms)).max()) if len(terms) else 0.0


def align_f64(logits, targets, input_lengths, target_lengths, blank, states, feasible):
    """The f64 values along the GIVEN paths (states (N, S), feasible (N): the kernel's, or align_f32's) and their budgets in units
    (the docstring): path_logit, score, label_logp (N, Lmax) with path_units, score_units, label_units; optimum (N): the f64 best
    path value of the line (-inf: infeasible).  Infeasible lines: -inf, -inf, 0 and zero units."""
    x = np.asarray(torch.as_tensor(logits).double().numpy(), dtype=np.float64)
    targets = np.asarray(torch.as_tensor(targets).numpy())
    states = np.asarray(states)
    N, S, C = x.shape
    Lmax = targets.shape[1]
    out = {"path_logit": np.full(N, NEG_INF), "score": np.full(N, NEG_INF), "label_logp": np.zeros((N, Lmax)), "optimum": np.full(N, NEG_INF),
           "path_units": np.zeros(N), "score_units": np.zeros(N), "label_units": np.zeros((N, Lmax))}
    for n in range(N):
        T, L = clamp(input_lengths[n], S), clamp(target_lengths[n], Lmax)
        out["optimum"][n] = float(_align(x[n], targets[n], T, L, blank, np.float64)[2])
        if not feasible[n]:
            continue
        if T == 0:
            out["path_logit"][n] = out["score"][n] = 0.0
            continue
        cls = state_classes(targets[n], L, C, blank)
        st = states[n, :T].astype(np.int64)
        assert st.min() >= 0 and st.max() < 2 * L + 1 and (cls[st] >= 0).all()
        xs = x[n, np.arange(T), cls[st]]                                   # the path's logits
        lse = _lse64(x[n, :T])
        row_units = math.ceil(math.log(C) + EXPF + (C - 1) + LOGF * math.log(C) + float(np.abs(lse).max()))
        out["path_logit"][n] = xs.sum()
        out["path_units"][n] = T * _max_abs_partial(xs)
        out["score"][n] = xs.sum() - lse.sum()
        out["score_units"][n] = out["path_units"][n] + T * row_units + T * _max_abs_partial(lse) + abs(xs.sum()) + abs(lse.sum())
        for k in range(L):
            frames = np.nonzero(st == 2 * k + 1)[0]
            terms = xs[frames] - lse[frames]
            out["label_logp"][n, k] = terms.sum()
            out["label_units"][n, k] = len(frames) * row_units + np.abs(terms).sum() + len(frames) * _max_abs_partial(terms)
    return {k: torch.from_numpy(np.ceil(v) if k.endswith("units") else v) for k, v in out.items()}


def brute_force(x, targets_n, T, L, blank):
    """Every state path of one tiny line (x (S, C)): (value, states) of the best, by the value (a python float sum in frame order: exact
    on small integers) and then by the state sequence read from the last frame back to the first, the LARGER winning; (-inf, None) if no
    path has a finite value."""
    x = np.asarray(x, dtype=np.float64)
    C = x.shape[1]
    if T == 0:
        return (0.0, []) if L == 0 else (NEG_INF, None)
    cls = state_classes(targets_n, L, C, blank)
    Lp = len(cls)
    best = (NEG_INF, None)

    def emit(t, s):
        return float(x[t, cls[s]]) if cls[s] >= 0 else NEG_INF

    def walk(path, value):
        nonlocal best
        t, s = len(path), path[-1]
        if t == T:
            if s >= Lp - 2 and value > NEG_INF:
                key = (value, tuple(reversed(path)))
                if best[1] is None or key > (best[0], tuple(reversed(best[1]))):
                    best = (value, list(path))
            return
        for step in (0, 1, 2):
            s2 = s + step
            if s2 >= Lp or (step == 2 and cls[s2] == cls[s]):
                continue
            walk(path + [s2], value + emit(t, s2))

    for s0 in range(min(2, Lp)):
        walk([s0], emit(0, s0))
    return best
