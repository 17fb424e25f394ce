"""CPU: tests/ctc_beam_ref.py itself - the f64 beam search against the CTC likelihood of ctc_ref.py (which test_ctc_ref_cpu.py pins to
torch), a hand-checked example, the re-entry cases, the replay checker against traces that are wrong in known ways, the margin
condition of the exact cases - and the host-side argument validation of pero_ctc_beam and pero_edit_distance (no GPU is touched)."""
import copy
import ctypes
import math

import pytest
import torch

import ctc_beam_ref as B
import ctc_ref


def test_unpruned_search_returns_every_feasible_string_with_its_ctc_likelihood():
    x, il, blank, W = B.exhaustive_case()
    res = B.search(x, il, blank, W)[0]
    strings = B.feasible_strings(3, 4, blank)
    assert len(strings) == 15 and math.isinf(res["margin"]) is False   # the final neighbours give a finite margin
    assert sorted(s for s, _ in res["hyps"]) == sorted(strings)
    for s, score in res["hyps"]:
        targets = torch.tensor([list(s) + [0] * (4 - len(s))])
        ref, _ = ctc_ref.ctc(x, targets, il, torch.tensor([len(s)]), blank)
        assert abs(score + float(ref["nll"][0])) <= 1e-14 * max(1.0, abs(score)), (s, score, float(ref["nll"][0]))
    assert [v for _, v in res["hyps"]] == sorted((v for _, v in res["hyps"]), reverse=True)


def test_beam_of_one_on_a_hand_checked_example():
    """blank 0, one label a = 1; P(blank), P(a) per frame: (.4, .6), (.5, .5), (.2, .8).
    frame 0: () has pb .4, (a) has pnb .6                                      -> (a) kept
    frame 1: (a): pb = .6 * .5 = .3, pnb = .6 * .5 = .3; (a a): pnb = .5 * pb(= 0): no candidate   -> (a), total .6
    frame 2: (a): pb = .6 * .2 = .12, pnb = .3 * .8 = .24, total .36; (a a): pnb = .8 * pb = .8 * .3 = .24   -> (a)"""
    x = torch.tensor([[[.4, .6], [.5, .5], [.2, .8]]]).log()
    res = B.search(x, torch.tensor([3]), 0, 1)[0]
    assert res["hyps"][0][0] == (1,) and len(res["hyps"]) == 1
    assert abs(res["hyps"][0][1] - math.log(.36)) < 1e-7          # the logits went through f32
    assert [len(f) for f in res["frames"]] == [1, 1, 1]
    assert abs(res["frames"][1][0][1] - math.log(.3)) < 1e-7 and abs(res["frames"][1][0][2] - math.log(.3)) < 1e-7
    assert abs(res["margin"] - (math.log(.36) - math.log(.24))) < 1e-6   # frame 0: log .6 - log .4 is the same gap; frame 2: .36 against .24
    two = B.search(x, torch.tensor([3]), 0, 2)[0]
    assert [s for s, _ in two["hyps"]] == [(1,), (1, 1)]
    # T = 0: the empty string with score 0
    assert B.search(x, torch.tensor([0]), 0, 4)[0]["hyps"] == [((), 0.0)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(B.REENTRY_CASES))
def test_reentry_cases_hold_a_reentry(name, dtype):
    x, il, blank, W = B.reentry_case(name, dtype)
    assert B.search(x, il, blank, W)[0]["reentries"] >= 1


def _good_trace(name="C3-S10-W3-x4"):
    x, il, blank, W = B.reentry_case(name)
    res = B.search(x, il, blank, W)[0]
    S = x.shape[1]
    return x[0], S, blank, W, res, B.trace_of(res, W, S)


def test_replay_accepts_the_reference_trace():
    for name in B.REENTRY_CASES:
        x, S, blank, W, res, (tr, out, lengths, scores, count) = _good_trace(name)
        stats = B.replay(x, S, blank, W, tr, out, lengths, scores, count)
        assert stats["ratio"] < 1e-6          # f64 against f64
    x, il, blank, W = B.exhaustive_case()
    res = B.search(x, il, blank, W)[0]
    B.replay(x[0], 4, blank, W, *B.trace_of(res, W, 4))
    empty = B.search(x, torch.tensor([0]), blank, 4)[0]
    B.replay(x[0], 0, blank, 4, *B.trace_of(empty, 4, 4))


def test_replay_rejects_wrong_traces():
    x, S, blank, W, res, (tr, out, lengths, scores, count) = _good_trace()
    t = next(t for t in range(S) if len(res["frames"][t]) == W and len(res["frames"][t - 1]) == W)

    # (a) a duplicated string: a second node for a string that has one (what "a new node for the returning prefix" does)
    bad = copy.deepcopy(tr)
    k = bad["beam_node"][t][1]
    bad["node_parent"].append(bad["node_parent"][k])
    bad["node_label"].append(bad["node_label"][k])
    bad["node_count"] += 1
    with pytest.raises(AssertionError, match="same string"):
        B.replay(x, S, blank, W, bad)
    bad = copy.deepcopy(tr)
    bad["beam_node"][t][2] = bad["beam_node"][t][1]
    with pytest.raises(AssertionError, match="kept twice"):
        B.replay(x, S, blank, W, bad)

    # (b) a kept candidate that is worse than a dropped one by far more than the tolerance: the last frame's worst slot is replaced by
    # the worst finite candidate of that frame
    last = S - 1
    beam = {s: (pb, pnb) for s, pb, pnb in res["frames"][last - 1]}
    lp, _, _ = B.line_logp(x, S)
    cand = B.candidates(beam, lp[last], blank)
    kept = {s for s, _, _ in res["frames"][last]}
    worst = min((s for s in cand if s not in kept and B.lse(*cand[s]) != B.NEG_INF), key=lambda s: B.lse(*cand[s]))
    assert B.lse(*cand[worst]) < min(B.lse(pb, pnb) for _, pb, pnb in res["frames"][last]) - 1e-3
    bad_res = copy.deepcopy(res)
    bad_res["frames"][last][W - 1] = (worst, cand[worst][0], cand[worst][1])
    with pytest.raises(AssertionError, match="dropped"):
        B.replay(x, S, blank, W, B.trace_of(bad_res, W, S)[0])

    # (c) wrong scores: a pb in the trace, a final score, and slots out of rank order
    bad = copy.deepcopy(tr)
    bad["beam_score"][t][0][1] += 1e-3
    with pytest.raises(AssertionError, match="pnb"):
        B.replay(x, S, blank, W, bad)
    wrong = list(scores)
    wrong[0] += 1e-3
    with pytest.raises(AssertionError, match="score"):
        B.replay(x, S, blank, W, tr, out, lengths, wrong, count)
    bad_res = copy.deepcopy(res)
    bad_res["frames"][t][0], bad_res["frames"][t][W - 1] = bad_res["frames"][t][W - 1], bad_res["frames"][t][0]
    with pytest.raises(AssertionError, match="rank order"):
        B.replay(x, S, blank, W, B.trace_of(bad_res, W, S)[0])

    # (d) outputs that disagree with the trace; fewer kept than there are candidates
    wrong_out = copy.deepcopy(out)
    wrong_out[0][0] = 2 if out[0][0] != 2 else 1
    with pytest.raises(AssertionError, match="hypothesis 0"):
        B.replay(x, S, blank, W, tr, wrong_out, lengths, scores, count)
    bad = copy.deepcopy(tr)
    bad["beam_node"][t][W - 1] = -1
    bad["beam_score"][t][W - 1] = [B.NEG_INF, B.NEG_INF]
    with pytest.raises(AssertionError, match="kept of"):
        B.replay(x, S, blank, W, bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_exact_cases_meet_the_margin_condition(dtype):
    x, il, blank, W, res = B.exact_case(dtype)
    assert x.shape[0] >= 4 and x.shape[0] == len(res)          # of 24 lines; bf16 rounding makes equal logits, so fewer lines pass there
    again = B.search(x, il, blank, W)
    for r, a in zip(res, again):
        assert r["margin"] >= 2 * r["bound"] > 0 and a["hyps"] == r["hyps"]


def test_edit_cases_cover_the_listed_lengths():
    cases = B.edit_cases()
    lens = {(len(a), len(b)) for a, b in cases}
    assert {(0, 0), (1, 512), (63, 512), (64, 512), (65, 512), (512, 512)} <= lens
    assert any(len(a) == 0 and len(b) > 0 for a, b in cases) and any(a == b and a for a, b in cases)
    assert ctc_ref.levenshtein([1, 2, 3, 4, 5], [1, 3, 4, 9, 5, 6]) == 3


# ---------------------------------------------------------------------------------------------- the library's host side
@pytest.fixture(scope="module")
def h():
    from pero_pretraining_amd import _lib
    return _lib.lib()


def _beam(h, *, ptrs=True, N=2, S=8, C=5, blank=0, W=4, dtype=0):
    p = [ctypes.c_void_p(64)] * 15 if ptrs else [None] * 15          # never dereferenced: every call below fails its host checks
    return h.pero_ctc_beam(*p, N, S, C, blank, W, dtype, None)


def test_beam_search_validates_its_arguments_without_a_gpu(h):
    assert _beam(h, ptrs=False) == -1 and b"null pointer" in h.pero_last_error()
    assert _beam(h, blank=5) == -1 and b"blank" in h.pero_last_error()
    assert _beam(h, blank=-1) == -1
    assert _beam(h, dtype=2) == -1 and b"dtype" in h.pero_last_error()
    for bad in ({"N": 0}, {"S": 0}, {"C": 1}, {"W": 0}, {"W": -3}):
        assert _beam(h, **bad) == -1 and b"bad sizes" in h.pero_last_error(), bad
    for big in ({"S": 513}, {"C": 8193}, {"W": 33}):
        assert _beam(h, **big) == -2 and b"supported up to" in h.pero_last_error(), big
    assert _beam(h, N=1 << 23, S=512) == -1 and b"2^31" in h.pero_last_error()


def test_edit_distance_validates_its_arguments_without_a_gpu(h):
    p = ctypes.c_void_p(64)
    assert h.pero_edit_distance(None, None, None, None, None, None, 2, 4, 4, None) == -1 and b"null pointer" in h.pero_last_error()
    assert h.pero_edit_distance(None, p, p, p, p, None, 2, 4, 4, None) == -1          # a is needed for La > 0
    assert h.pero_edit_distance(p, p, p, p, p, None, 0, 4, 4, None) == -1 and b"bad sizes" in h.pero_last_error()
    assert h.pero_edit_distance(p, p, p, p, p, None, 2, -1, 4, None) == -1
    assert h.pero_edit_distance(p, p, p, p, p, None, 2, 513, 4, None) == -2 and b"supported up to" in h.pero_last_error()
    assert h.pero_edit_distance(p, p, p, p, p, None, 2, 4, 513, None) == -2


def test_python_wrappers_reject_host_tensors_and_bad_widths():
    from pero_pretraining_amd import _lib, ops, recognition
    with pytest.raises(_lib.PeroHipError):
        ops.ctc_beam(torch.zeros(8, 5), torch.tensor([4, 4]), 4)
    with pytest.raises(_lib.PeroHipError):
        ops.edit_distance(torch.zeros(2, 3, dtype=torch.int64), torch.tensor([1, 1]), torch.zeros(2, 3, dtype=torch.int64), torch.tensor([1, 1]))
    with pytest.raises(ValueError):
        recognition.beam_decode(torch.zeros(2, 4, 5), beam_width=4, nbest=5)
    assert ops.ctc_beam_workspace(256, 512, 16) == (17, 8192) and ops.ctc_beam_workspace(4, 3, 32) == (2, 256)
