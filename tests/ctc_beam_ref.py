"""f64 restatement of pero_ctc_beam (include/pero_hip.h), written from the header's recursion with a DICTIONARY OF STRINGS
(Python tuples): no trie, no nodes, no hash, so it shares no data structure with csrc/ctc_decode.hip.  Not a test module; it never
imports the library.  Also here: pero_edit_distance's cases, and the REPLAY CHECKER that judges a trace of the kernel.

`search` is the independent reference: the whole beam search in f64.  Its ranking can differ from a correct f32 kernel's wherever
two totals are closer than the two error bounds, so it reports, per line, the smallest DECISION MARGIN: over all frames the gap
between the totals of rank W and rank W + 1 (the one pruning decision of a frame; +inf where nothing is pruned), and the gaps between
neighbours of the final ranking.  A line whose margin is >= 2 x its bound has one right answer, strings and order, and only such
lines are compared string by string (`exact_case`).  `search` also counts RE-ENTRY MERGES: frames at which the extension (p, c) of
a beam entry p is merged into a beam entry p + c that has been in the beam since before p (last) entered it - p left the beam and
was created again from its parent while p + c stayed.  An implementation that identifies strings by "same parent beam slot", or
that gives the returning p a new node, splits p + c in two there.

`replay` needs no margin.  It rebuilds the strings from the kernel's node table and replays the recursion in f64 ON THE KERNEL'S
OWN KEPT SETS: at every frame the f64 candidates of the kernel's previous beam are formed (with the dictionary: merging is by
string), and the kept slots must be distinct finite candidates, all of them if there are at most W, none worse than a dropped one
by more than 2 x the bound, in rank order up to 2 x the bound, with (pb, pnb) within the bound of the f64 values.

Error bound, in the units of parity_ref.py (u = 2^-24; EXPF, LOGF units per call), following ctc_ref.py's derivation of the alpha
recursion.  A frame computes each new pb and each new pnb as ONE log-sum-exp of at most three terms, v = m + log(sum_i exp(a_i -
m)), whose terms are old values plus an emission logp_t(c) = x - lse (pb: two terms pb + e, pnb + e, formed as (pb (+) pnb) + e; pnb
of a kept string: pnb + e, parent's pb + e and parent's pnb + e; pnb of a new string: one or two terms, formed as tot + e).  An
absolute error of the old values passes through with factor <= 1 (the weights of a log-sum-exp sum to 1), so the frames' own
errors ADD.  With A = max |finite pb', pnb'| over every candidate of the line, kept or dropped (all are <= 0, and every emission
that reaches a finite candidate is no larger in magnitude than that candidate):
  absolute (units of u):             rounded arguments a_i - m 1, expf EXPF, the three-term sum 2, logf of a value in [0, ln 3]
                                     ceil(LOGF ln 3) = 3, the error of lse inside the emission row_units (ctc_ref.py's, of the line's rows)
  scaled (units of u (A + 1)):       m + log(..) 2, x - lse 1, the sum with the emission 1
  per-frame units  K = 4 + ceil((1 + EXPF + 2 + 3 + row_units) / (A + 1)).
pb, pnb after frame t have passed t + 1 frames:        |pb - ref| <= (t + 1) K u (A + 1);
a total pb (+) pnb is one more log-sum-exp (no emission, so K covers it):  |total - ref| <= (t + 2) K u (A + 1).
Two f32 totals, each within that bound, can be ranked against their f64 order only if they are within 2 x the bound.  Nothing
here is measured on the kernel.  bf16 logits are rounded once on the host and every function below sees the rounded values."""
import math

import torch

from parity_ref import EXPF, LOGF, U32, f64

NEG_INF = -math.inf


def lse(*a):
    m = max(a)
    if m == NEG_INF:
        return NEG_INF
    return m + math.log(sum(math.exp(v - m) for v in a))


def line_logp(x_line, T):
    """(T, C) nested lists of logp in f64, the row log-sum-exps, and row_units of the line (ctc_ref.py's formula)."""
    x = f64(x_line)[:T]
    C = x.shape[-1]
    if T == 0:
        return [], [], 0
    row_lse = torch.logsumexp(x, dim=-1)
    lp = torch.where(torch.isinf(x) & (x < 0), x, x - row_lse[:, None])
    row_units = math.ceil(math.log(C) + EXPF + (C - 1) + LOGF * math.log(C) + float(row_lse.abs().max()))
    return lp.tolist(), row_lse.tolist(), row_units


def candidates(beam, lp_t, blank):
    """beam: {string: (pb, pnb)}.  Returns {string: [pb', pnb']} of one frame, contributions to the same string merged."""
    cand = {}

    def add(s, k, v):
        e = cand.setdefault(s, [NEG_INF, NEG_INF])
        e[k] = lse(e[k], v)

    for p, (pb, pnb) in beam.items():
        tot = lse(pb, pnb)
        add(p, 0, tot + lp_t[blank])
        if p:
            add(p, 1, pnb + lp_t[p[-1]])
        for c in range(len(lp_t)):
            if c != blank:
                add(p + (c,), 1, lp_t[c] + (pb if p and c == p[-1] else tot))
    return cand


def magnitude(cand):
    return max([abs(v) for e in cand.values() for v in e if v != NEG_INF] + [0.0])


def frame_units(row_units, A):
    return 4 + math.ceil((1 + EXPF + 2 + 3 + row_units) / (A + 1))


def bound_state(t, row_units, A):
    """pb, pnb after frame t"""
    return (t + 1) * frame_units(row_units, A) * U32 * (A + 1)


def bound_total(t, row_units, A):
    """a total after frame t (t = -1: before any frame, the exact 0 of the empty beam gets one step)"""
    return (t + 2) * frame_units(row_units, A) * U32 * (A + 1)


def search_line(x_line, T, blank, W):
    """One line.  {"hyps": [(string, total)] best first, "frames": [[(string, pb, pnb)] in rank order per frame], "margin", "reentries",
    "A", "row_units", "bound": bound_total of the last frame}."""
    lp, _, row_units = line_logp(x_line, T)
    beam = {(): (0.0, NEG_INF)}
    entered = {(): -1}
    frames, margin, reentries, A = [], math.inf, 0, 0.0
    for t in range(T):
        for p in beam:   # the extension (p, c) merges with the beam entry p + c
            for c in range(len(lp[t])):
                s = p + (c,)
                if c != blank and s in beam and entered[p] > entered[s]:
                    reentries += 1
        cand = candidates(beam, lp[t], blank)
        A = max(A, magnitude(cand))
        ranked = sorted(((lse(*e), s) for s, e in cand.items() if lse(*e) != NEG_INF), key=lambda v: (-v[0], v[1]))
        if len(ranked) > W:
            margin = min(margin, ranked[W - 1][0] - ranked[W][0])
        kept = ranked[:W]
        new = {s: tuple(cand[s]) for _, s in kept}
        entered = {s: (entered[s] if s in beam else t) for s in new}
        beam = new
        frames.append([(s, cand[s][0], cand[s][1]) for _, s in kept])
    hyps = sorted(((lse(*e), s) for s, e in beam.items()), key=lambda v: (-v[0], v[1]))
    for a, b in zip(hyps, hyps[1:]):
        margin = min(margin, a[0] - b[0])
    return {"hyps": [(s, v) for v, s in hyps], "frames": frames, "margin": margin, "reentries": reentries, "A": A, "row_units": row_units,
            "bound": bound_total(T - 1, row_units, A)}


def search(logits, input_lengths, blank, W):
    """logits (N, S, C); a list of search_line results."""
    S = logits.shape[1]
    return [search_line(logits[n], min(max(int(T), 0), S), blank, W) for n, T in enumerate(torch.as_tensor(input_lengths).tolist())]


# ---------------------------------------------------------------------------------------------- the replay checker
def trace_line(trace, n):
    """Line n of ops.ctc_beam's trace dict as host lists."""
    return {k: v[n].cpu().tolist() for k, v in trace.items()}


def replay(x_line, T, blank, W, tr, out=None, out_length=None, out_score=None, out_count=None):
    """Judge one line of a kernel trace (see the module docstring); raises AssertionError with the frame and the reason.
    tr: node_parent, node_label (lists), node_count, beam_node (S, W), beam_score (S, W, 2).  out (W, S), out_length (W), out_score (W),
    out_count: the line's outputs, or None to check the trace only.  Returns {"ratio": worst error / bound seen, "A", "row_units"}."""
    lp, _, row_units = line_logp(x_line, T)
    C = x_line.shape[-1]
    count = tr["node_count"]
    assert 1 <= count <= T * W + 1, f"node_count {count}"
    assert tr["node_parent"][0] == -1 and tr["node_label"][0] == -1, "node 0 is the empty prefix"
    strings = [()]
    for k in range(1, count):
        par, lab = tr["node_parent"][k], tr["node_label"][k]
        assert 0 <= par < k and 0 <= lab < C and lab != blank, f"node {k}: parent {par}, label {lab}"
        strings.append(strings[par] + (lab,))
    assert len(set(strings)) == count, "two nodes spell the same string"

    # pass 1: the f64 recursion on the kernel's kept sets, and the line's magnitude A
    beam = {(): (0.0, NEG_INF)}
    steps, A = [], 0.0
    for t in range(T):
        nodes = [k for k in tr["beam_node"][t] if k >= 0]
        assert nodes == tr["beam_node"][t][:len(nodes)] and all(k < count for k in nodes), f"frame {t}: slots {tr['beam_node'][t]}"
        kept = [strings[k] for k in nodes]
        assert len(set(kept)) == len(kept), f"frame {t}: a string is kept twice"
        cand = candidates(beam, lp[t], blank)
        A = max(A, magnitude(cand))
        finite = {s: lse(*e) for s, e in cand.items() if lse(*e) != NEG_INF}
        for s in kept:
            assert s in finite, f"frame {t}: kept string {s} is no finite candidate"
        assert len(kept) == min(W, len(finite)), f"frame {t}: {len(kept)} kept of {len(finite)} finite candidates, W = {W}"
        steps.append((kept, cand, finite))
        beam = {s: tuple(cand[s]) for s in kept}

    # pass 2: the decisions and the scores against the bounds
    ratio = 0.0

    def near(got, ref, b, what):
        nonlocal ratio
        if ref == NEG_INF or got == NEG_INF:
            assert got == ref, f"{what}: got {got}, ref {ref}"
            return
        assert not math.isnan(got), what
        ratio = max(ratio, abs(got - ref) / b)
        assert abs(got - ref) <= b, f"{what}: got {got!r}, ref {ref!r}, bound {b!r} (error / bound = {abs(got - ref) / b:.3g})"

    for t, (kept, cand, finite) in enumerate(steps):
        bt, bs = bound_total(t, row_units, A), bound_state(t, row_units, A)
        totals = [finite[s] for s in kept]
        dropped = [v for s, v in finite.items() if s not in set(kept)]
        if dropped:
            assert min(totals) >= max(dropped) - 2 * bt, f"frame {t}: kept {min(totals)!r}, dropped {max(dropped)!r}, 2 x bound {2 * bt!r}"
        for k in range(len(totals) - 1):
            assert totals[k] >= totals[k + 1] - 2 * bt, f"frame {t}: slots {k}, {k + 1} out of rank order: {totals[k]!r} < {totals[k + 1]!r}"
        for k in range(W):
            got_pb, got_pnb = tr["beam_score"][t][k]
            if k < len(kept):
                near(got_pb, cand[kept[k]][0], bs, f"frame {t} slot {k} pb")
                near(got_pnb, cand[kept[k]][1], bs, f"frame {t} slot {k} pnb")
            else:
                assert got_pb == NEG_INF and got_pnb == NEG_INF, f"frame {t}: unused slot {k} has a score"

    if out is not None:
        final = [(s, lse(*beam[s])) for s in (steps[-1][0] if T else [()])]
        assert out_count == len(final), f"out_count {out_count}, the trace holds {len(final)}"
        for k in range(W):
            if k < len(final):
                s, v = final[k]
                assert out_length[k] == len(s) and tuple(out[k][:len(s)]) == s, f"hypothesis {k}: {out[k][:out_length[k]]} is not the trace's {s}"
                assert all(v == -1 for v in out[k][len(s):]), f"hypothesis {k}: padding"
                near(out_score[k], v, bound_total(T - 1, row_units, A), f"hypothesis {k} score")
            else:
                assert out_length[k] == 0 and out_score[k] == NEG_INF and all(v == -1 for v in out[k]), f"unused hypothesis {k}"
    return {"ratio": ratio, "A": A, "row_units": row_units}


def trace_of(res, W, S):
    """A trace (and outputs) built from a search_line result: what a perfect kernel would write.  For the checker's own tests."""
    ids = {(): 0}
    parent, label = [-1], [-1]
    beam_node, beam_score = [], []
    for frame in res["frames"]:
        row, sc = [], []
        for s, pb, pnb in frame:
            if s not in ids:
                ids[s] = len(parent)
                parent.append(ids[s[:-1]])
                label.append(s[-1])
            row.append(ids[s])
            sc.append([pb, pnb])
        beam_node.append(row + [-1] * (W - len(row)))
        beam_score.append(sc + [[NEG_INF, NEG_INF]] * (W - len(sc)))
    tr = {"node_parent": parent, "node_label": label, "node_count": len(parent), "beam_node": beam_node, "beam_score": beam_score}
    hyps = res["hyps"] if res["frames"] else [((), 0.0)]
    if res["frames"]:   # the outputs follow the last frame's rank order
        hyps = [(s, lse(pb, pnb)) for s, pb, pnb in res["frames"][-1]]
    out = [list(s) + [-1] * (S - len(s)) for s, _ in hyps] + [[-1] * S] * (W - len(hyps))
    return tr, out, [len(s) for s, _ in hyps] + [0] * (W - len(hyps)), [v for _, v in hyps] + [NEG_INF] * (W - len(hyps)), len(hyps)


# ---------------------------------------------------------------------------------------------- cases
def feasible_strings(C, T, blank):
    """Every label string some alignment of T frames spells."""
    labels = [c for c in range(C) if c != blank]
    out = set()

    def grow(s, need):   # need = frames the string takes at least
        out.add(s)
        for c in labels:
            n2 = need + (2 if s and s[-1] == c else 1)
            if n2 <= T:
                grow(s + (c,), n2)

    grow((), 0)
    return sorted(out, key=lambda s: (len(s), s))


def exhaustive_case(dtype=torch.float32):
    """C = 3, T = 4, W = 32: nothing is pruned, every feasible string (15) is a hypothesis."""
    gen = torch.Generator().manual_seed(11)
    return (2 * torch.randn(1, 4, 3, generator=gen)).to(dtype).float(), torch.tensor([4]), 0, 32


REENTRY_CASES = {"C3-S10-W3-x4": (3, 10, 3, 4.0, 9), "C3-S12-W4-x6": (3, 12, 4, 6.0, 6)}   # (C, S, W, scale, seed)


def reentry_case(name, dtype=torch.float32):
    """One line whose search holds at least one re-entry merge (the seeds were found by searching on the CPU)."""
    C, S, W, scale, seed = REENTRY_CASES[name]
    gen = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(1, S, C, generator=gen)).to(dtype).float(), torch.tensor([S]), 0, W


def planted_case(C, blank, S=16, seed=0, dtype=torch.float32):
    """N = 5 lines at one S: T = 0 | T = 1 | T = S random | T = S - 3 with a planted string that repeats labels (a a b b a: a blank must
    separate the equal neighbours) under noise | T = S, logits 30 randn (wide range: many candidates underflow to tiny probabilities)."""
    gen = torch.Generator().manual_seed(seed + 1000 * C + blank)
    x = 3 * torch.randn(5, S, C, generator=gen)
    labels = [c for c in range(C) if c != blank]
    a, b = labels[0], labels[-1]
    path = [a, blank, a, a, b, blank, b, b, a, blank, blank, a, a][:S - 3]
    x[3, torch.arange(len(path)), torch.tensor(path)] += 20.0
    x[4] *= 10.0
    return x.to(dtype).float(), torch.tensor([0, 1, S, S - 3, S]), blank


def long_case(dtype=torch.float32):
    """One line of S = 264 frames (more frames than a workgroup has threads), C = 37, to run with W = 4."""
    gen = torch.Generator().manual_seed(264)
    return (3 * torch.randn(1, 264, 37, generator=gen)).to(dtype).float(), torch.tensor([264]), 0, 4


def exact_case(dtype=torch.float32, lines=24):
    """S = 12, C = 37, W = 8, logits randn: of `lines` random lines, those whose decision margin is >= 2 x their bound (deterministic
    rejection; about half pass).  Returns logits (N, 12, 37), input_lengths, blank, W and the lines' search results."""
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(lines, 12, 37, generator=gen).to(dtype).float()
    il = torch.full((lines,), 12)
    il[1::4] = 9
    res = search(x, il, 0, 8)
    keep = [n for n, r in enumerate(res) if r["margin"] >= 2 * r["bound"]]
    return x[keep], il[keep], 0, 8, [res[n] for n in keep]


SENTINEL = 7   # padding of the edit-distance cases: a value that occurs in the strings, so that reading it would change a distance


def edit_cases():
    """[(a, b)] lists of labels: empty/empty, empty/non-empty both ways, equal strings, lengths 1, 63, 64, 65 and 512 against 512, and
    pairs that need all three operations."""
    gen = torch.Generator().manual_seed(3)

    def rnd(n, hi=8):
        return torch.randint(0, hi, (n,), generator=gen).tolist()

    base = rnd(512)
    cases = [([], []), ([], rnd(5)), (rnd(4), []), (base[:40], base[:40]), (base, base)]
    cases += [(rnd(n), base) for n in (1, 63, 64, 65, 512)]
    cases += [(base, rnd(n)) for n in (1, 65)]
    cases += [([1, 2, 3, 4, 5], [1, 3, 4, 9, 5, 6]), (base[:64], base[1:65]), (base[:100], base[50:130]), ([7] * 9, [7] * 4)]
    return cases


def pad(strings, width, fill=SENTINEL):
    out = torch.full((len(strings), width), fill, dtype=torch.int64)
    for n, s in enumerate(strings):
        out[n, :len(s)] = torch.tensor(s, dtype=torch.int64)
    return out, torch.tensor([len(s) for s in strings])
