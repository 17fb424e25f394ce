"""CPU: recognition.NGramLM (estimation, the automaton, ARPA, validation) and tests/ctc_beam_lm_ref.py itself - the f64 search with the
language-model term against an exhaustive enumeration, a planted line on which the model changes the winner, the replay checker on the
reference's own trace, the margin condition of the exact case - and the host-side refusals of pero_ctc_beam_lm (no GPU is touched)."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

import ctc_beam_lm_ref as L
import ctc_beam_ref as B
from parity_ref import U32
from pero_pretraining_amd.recognition import NGramLM


@pytest.mark.parametrize("eos", [True, False])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_every_state_is_a_distribution(order, eos):
    """Per state: the probabilities of the non-blank classes by the f32 look-up and of the end symbol add to 1 within 1e-5 (f32 table
    rounding over at most 6 terms).  A model without an end symbol has final = 0 and its classes alone add to 1."""
    C, blank = 6, 2
    lm = NGramLM.fit(L.random_strings(C, blank, 50, 7, low=1, high=9), C, blank, order=order, eos=eos)
    assert lm.order == order and lm.num_classes == C and lm.blank == blank and (lm.num_states == 1) == (order == 1)
    assert (lm.start != 0) == (order > 1) and lm.backoff_state[0] == -1
    walk = L.Walk(lm, 1.0, 0.0)
    for s in range(lm.num_states):
        total = sum(math.exp(float(lm.lookup(s, c)[0])) for c in range(C) if c != blank) + (math.exp(float(lm.final[s])) if eos else 0.0)
        assert abs(total - 1.0) <= 1e-5, (s, total)
        for c in range(C):   # the reference's own walk (a linear scan) and the class's (a binary search): the same bits, the same state
            if c != blank:
                a, b = lm.lookup(s, c), walk.lookup(s, c)
                assert L.bits(a[0]) == L.bits(b[0]) and a[1] == b[1]
    if not eos:
        assert not lm.final.any()
    assert lm.lookup(0, blank) is None


ARPA = """\\data\\
ngram 1=5
ngram 2=3
ngram 3=1

\\1-grams:
-99 <s> -0.5
-1.0 </s>
-0.4 a -0.3
-0.7 b -0.2
-0.9 c

\\2-grams:
-0.25 <s> a -0.1
-0.35 a b
-0.6 b </s>

\\3-grams:
-0.15 <s> a b

\\end\\
"""


def test_score_by_hand():
    """a b c </s> from <s>, in log10:  a | <s> = -0.25 (bigram);  b | <s> a = -0.15 (trigram);  c | a b backs off TWICE: no trigram a b c,
    bow(a b) is missing = 0; no bigram b c, bow(b) = -0.2; the unigram c = -0.9.  </s> | b c: the longest suffix that is a context is (c), which
    has no bigram with </s> and no back-off weight (0): the unigram </s> = -1.0."""
    lm = NGramLM.from_arpa(ARPA, {"a": 1, "b": 2, "c": 3})
    assert lm.order == 3 and lm.num_classes == 4 and lm.blank == 0 and lm.start != 0
    ln10 = math.log(10.0)
    want = (-0.25 - 0.15 + (0.0 - 0.2 - 0.9) - 1.0) * ln10
    assert abs(lm.score([1, 2, 3]) - want) <= 1e-6
    assert abs(lm.score([1, 2, 3], eos=False) - (want + 1.0 * ln10)) <= 1e-6
    # b first: <s> has no bigram with b -> bow(<s>) + unigram b; then </s> | b is the explicit bigram
    assert abs(lm.score([2]) - (-0.5 - 0.7 - 0.6) * ln10) <= 1e-6
    assert lm.score([]) == pytest.approx((-0.5 - 1.0) * ln10, abs=1e-6)          # </s> | <s>: backed off
    # an unmapped token drops its n-grams: without c the string is forbidden
    assert NGramLM.from_arpa(ARPA, {"a": 1, "b": 2}, num_classes=4).score([1, 2, 3]) == -math.inf


@pytest.mark.parametrize("order", [1, 2, 3])
def test_arpa_round_trip(order, tmp_path):
    lm = L.fitted(6, 0, order=order, seed=3, count=50)
    back = NGramLM.from_arpa(lm.to_arpa(), {str(c): c for c in range(1, 6)}, num_classes=6, blank=0)
    assert back.order == lm.order and back.start == lm.start and back.contexts == lm.contexts
    for k, v in lm.arrays().items():
        assert v.dtype == back.arrays()[k].dtype and np.array_equal(v.view(np.int32), back.arrays()[k].view(np.int32)), k
    path = tmp_path / "lm.arpa"
    path.write_text(lm.to_arpa({chr(96 + c): c for c in range(1, 6)}))
    named = NGramLM.from_arpa(path, {chr(96 + c): c for c in range(1, 6)}, num_classes=6)
    assert all(np.array_equal(v, named.arrays()[k]) for k, v in lm.arrays().items())


def test_malformed_tables_raise():
    lm = L.fitted(5, 0, order=2, seed=1, count=40)
    a = {k: v.copy() for k, v in lm.arrays().items()}

    def build(**change):
        t = {**a, **change}
        return NGramLM(5, 0, 2, lm.start, t["backoff_state"], t["backoff_weight"], t["final"], t["arc_begin"], t["arc_label"], t["arc_logp"], t["arc_next"])

    build()
    label = a["arc_label"].copy()
    label[0] = 0
    with pytest.raises(ValueError, match="blank"):
        build(arc_label=label)
    label = a["arc_label"].copy()
    label[[0, 1]] = label[[1, 0]]
    with pytest.raises(ValueError, match="ascend"):
        build(arc_label=label)
    back = a["backoff_state"].copy()
    back[1], back[2] = 2, 1
    with pytest.raises(ValueError, match="back-off chain"):
        build(backoff_state=back)
    nxt = a["arc_next"].copy()
    nxt[3] = lm.num_states
    with pytest.raises(ValueError, match="arc_next"):
        build(arc_next=nxt)
    logp = a["arc_logp"].copy()
    logp[2] = -np.inf
    with pytest.raises(ValueError, match="finite"):
        build(arc_logp=logp)
    label = a["arc_label"].copy()
    label[-1] = 5
    with pytest.raises(ValueError, match="outside"):
        build(arc_label=label)


@pytest.mark.parametrize("alpha,beta,use_final", [(1.0, 0.0, True), (0.5, 1.5, False), (2.0, -1.0, True)])
def test_reference_search_against_exhaustive_enumeration(alpha, beta, use_final):
    """C = 3, T = 4, K = C - 1, W = the number of feasible strings (15): nothing is pruned, so every string's score is its exact CTC
    log-probability (ctc_beam_ref's unpruned search, pinned to the CTC likelihood by test_ctc_beam_ref_cpu.py) + alpha LM + beta |string| with
    LM from NGramLM.score in f64.  The search adds w in its f32 form: per label at most `order + 2` f32 roundings (the walk's additions, the
    multiplication, the addition of beta) of values no larger than alpha Lmax + |beta|, Lmax = the largest |table entry| times the order."""
    x, il, blank, _ = B.exhaustive_case()
    strings = B.feasible_strings(3, 4, blank)
    lm = L.fitted(3, 0, order=3, seed=5, count=60)
    acoustic = dict(B.search(x, il, blank, 32)[0]["hyps"])
    res = L.search(x, il, blank, len(strings), 2, lm, alpha, beta, use_final)[0]
    assert sorted(s for s, _ in res["hyps"]) == sorted(strings)
    lmax = lm.order * max(float(np.abs(lm.arc_logp).max()), float(np.abs(lm.backoff_weight).max()), float(np.abs(lm.final).max()))
    for (s, v), part in zip(res["hyps"], res["lm"]):
        want_lm = alpha * lm.score(s, eos=use_final) + beta * len(s)
        tol = (len(s) + 1) * (lm.order + 2) * U32 * (alpha * lmax + abs(beta) + 1)
        assert abs(v - (acoustic[s] + want_lm)) <= tol + 1e-12, (s, v, acoustic[s] + want_lm, tol)
        assert abs(float(part) - want_lm) <= tol, (s, float(part), want_lm)
    assert [v for _, v in res["hyps"]] == sorted((v for _, v in res["hyps"]), reverse=True)


def test_the_model_changes_the_winner_of_a_planted_line():
    x, il, blank, lm, alpha = L.winner_case()
    plain = B.search(x, il, blank, 8)[0]
    acoustic = dict(B.search(x, il, blank, 64)[0]["hyps"])          # wide enough for every string that matters
    a, b = (1, 3), (1, 2)
    assert plain["hyps"][0][0] == a
    gap, lm_gap = acoustic[a] - acoustic[b], lm.score(b) - lm.score(a)
    assert 0 < gap < alpha * lm_gap, (gap, lm_gap)          # the precondition, on the reference alone
    res = L.search(x, il, blank, 8, 3, lm, alpha, 0.0, True)[0]
    assert res["hyps"][0][0] == b
    assert abs(res["hyps"][0][1] - (acoustic[b] + alpha * lm.score(b))) <= 1e-5
    # alpha = 0 and no length bonus: the plain search, string by string and score by score (x + 0 = x)
    null = L.search(x, il, blank, 8, 3, lm, 0.0, 0.0, False)[0]
    assert dict(null["hyps"]) == dict(plain["hyps"]) and null["hyps"][0] == plain["hyps"][0]


def _good(use_final=True, K=2):
    x, il, blank, W = B.reentry_case("C3-S10-W3-x4")
    lm = L.fitted(3, 0, order=3, seed=2, count=60)
    res = L.search(x, il, blank, W, K, lm, 0.5, 1.5, use_final)[0]
    return x[0], blank, W, K, lm, res, L.trace_of(res, W, x.shape[1], lm, 0.5, 1.5)


@pytest.mark.parametrize("use_final", [True, False])
def test_replay_accepts_the_reference_trace_and_rejects_wrong_ones(use_final):
    x, blank, W, K, lm, res, (tr, out, lengths, scores, parts, count) = _good(use_final)
    args = (x, 10, blank, W, K, lm, 0.5, 1.5, use_final)
    stats = L.replay(*args, tr, out, lengths, scores, parts, count)
    assert stats["ratio"] <= 1e-6          # f64 against f64
    bad = copy.deepcopy(tr)
    bad["node_lm_state"][1] = (bad["node_lm_state"][1] + 1) % lm.num_states
    with pytest.raises(AssertionError, match="LM state"):
        L.replay(*args, bad, out, lengths, scores, parts, count)
    bad = copy.deepcopy(tr)
    bad["node_lm_weight"][2] = float(np.nextafter(np.float32(bad["node_lm_weight"][2]), np.float32(10)))          # one ulp
    with pytest.raises(AssertionError, match="LM weight"):
        L.replay(*args, bad, out, lengths, scores, parts, count)
    wrong = list(parts)
    wrong[0] = float(np.nextafter(np.float32(wrong[0]), np.float32(10)))
    with pytest.raises(AssertionError, match="out_lm"):
        L.replay(*args, tr, out, lengths, scores, wrong, count)
    shifted = [v + 1e-3 for v in scores]          # a kernel that forgot beta once
    with pytest.raises(AssertionError, match="score"):
        L.replay(*args, tr, out, lengths, shifted, parts, count)
    bad = copy.deepcopy(tr)
    bad["beam_score"][4][0][1] += 1e-3
    with pytest.raises(AssertionError, match="pnb"):
        L.replay(*args, bad, out, lengths, scores, parts, count)
    # a trace of the search WITHOUT the model is no trace of the search with it
    plain = B.search(x[None], torch.tensor([10]), blank, W)[0]
    ptr, pout, plen, psc, pcount = B.trace_of(plain, W, 10)
    ptr["node_lm_state"] = [0] * ptr["node_count"]
    ptr["node_lm_weight"] = [0.0] * ptr["node_count"]
    with pytest.raises(AssertionError):
        L.replay(*args, ptr, pout, plen, psc, [0.0] * W, pcount)


def test_pruning_by_k_spares_the_strings_of_the_beam():
    """K = 1: only the frame's best class starts new strings, but an extension that spells a beam entry still merges into it (the header's
    rule, and pero_ctc_beam's behaviour, on which the null-LM identity rests)."""
    x, il, blank, W = B.reentry_case("C3-S10-W3-x4")
    lm = L.fitted(3, 0, order=1, seed=2, count=60)
    res = L.search(x, il, blank, W, 1, lm, 0.0, 0.0, False)[0]
    walk = L.Walk(lm, 0.0, 0.0)
    lp, _, _ = B.line_logp(x[0], 10)
    raw = x[0].double().tolist()
    merged = 0
    beam = {(): (0.0, -math.inf)}
    for t, frame in enumerate(res["frames"]):
        top = L.top_classes(raw[t], blank, 1)
        for p in beam:
            for c in (1, 2):
                if p + (c,) in beam and c not in top:
                    merged += 1
                    with_it = L.candidates(beam, lp[t], top, blank, walk)[0][p + (c,)][1]
                    without = B.lse(beam[p + (c,)][1] + lp[t][c])          # the stay's own term alone
                    assert with_it > without
        beam = {s: (pb, pnb) for s, pb, pnb in frame}
    assert merged >= 1


def test_three_of_four_exact_lines_qualify():
    """The GPU test compares only lines whose margin is >= 2 x the bound; a case that skips most lines shows nothing."""
    case = L.exact_case()
    assert 4 * len(case[-2]) >= 3 * case[-1], (len(case[-2]), case[-1])
    assert any(r["hyps"][0][0] != p["hyps"][0][0] for r, p in zip(case[-2], B.search(case[0], case[1], 0, 8)))   # the model matters here


def test_host_side_refusals_of_pero_ctc_beam_lm():
    """PERO_E_INVALID / PERO_E_UNSUPPORTED before any launch: every pointer is a dummy host address that a launch would fault on."""
    from pero_pretraining_amd import _lib
    h = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def rc(N=1, S=8, C=130, blank=0, W=8, K=9, M=4, A=40, start=1, alpha=1.0, beta=0.0, null=None):
        ptrs = [p] * 25
        if null is not None:
            ptrs[null] = None
        return h.pero_ctc_beam_lm(*ptrs, N, S, C, blank, W, K, M, A, start, alpha, beta, 1, _lib.PERO_F32, None)

    assert rc(W=33) == rc(W=16, K=68) == rc(W=32, K=34) == -2 and b"1088" in h.pero_last_error()          # PERO_E_UNSUPPORTED
    for bad in (dict(M=0), dict(start=4), dict(start=-1), dict(A=-1), dict(alpha=math.inf), dict(beta=math.nan), dict(W=0), dict(blank=130),
                dict(null=2), dict(null=12), dict(null=16), dict(null=24)):
        assert rc(**bad) == -1, bad          # PERO_E_INVALID
