"""CPU: tests/edit_ops_ref.py itself - its distance against recognition.levenshtein, its scripts replayed, the count identities, minimality
against brute force, the hand-written tie cases, the split into words - then recognition.top_confusions, the host-side argument
validation of pero_edit_ops (no GPU is touched) and the argument errors of ops.edit_ops."""
import ctypes

import pytest
import torch

import edit_ops_ref as E


def test_distance_script_and_counts_of_the_reference():
    from pero_pretraining_amd.recognition import levenshtein
    pairs = E.random_pairs(300, 12, 2, seed=0) + E.random_pairs(300, 12, 5, seed=1) + [([], []), ([1], []), ([], [1])]
    for a, b in pairs:
        codes = E.script(a, b)
        sub, ins, dele, hit = E.counts(codes)
        assert sub + ins + dele == E.table(a, b)[len(a)][len(b)] == levenshtein(a, b), (a, b)
        assert hit + sub + ins == len(a) and hit + sub + dele == len(b), (a, b)
        assert E.replay(a, b, codes) == b, (a, b, codes)          # hits on equal elements, substitutions on unequal ones: replay raises otherwise
        assert len(codes) <= len(a) + len(b)


def test_scripts_are_minimal_against_brute_force():
    strings = E.small_strings(4, 2)
    assert len(strings) == 31
    for a in strings:
        for b in strings:
            sub, ins, dele, _ = E.counts(E.script(a, b))
            assert sub + ins + dele == E.all_scripts_minimum(a, b), (a, b)


def test_tie_rule_on_the_hand_written_cases():
    a, b = 0, 1
    assert E.script([a, b], [b, a]) == [1, 1]
    assert E.script([a, a, b], [a, b]) == [2, 0, 0]
    assert E.script([a, b], [a, a, b]) == [3, 0, 0]
    assert E.script([], [a, b]) == [3, 3] and E.script([a, b], []) == [2, 2] and E.script([], []) == []
    # the diagonal wins a tie against both gaps: D(1, 1) = 1 is reached three ways
    assert E.script([a], [b]) == [1]
    # a deletion wins against an insertion: at (3, 3) of aba / bab the diagonal costs 3, D(3, 2) + 1 = D(2, 3) + 1 = 2
    assert E.script([a, b, a], [b, a, b]) == [2, 0, 0, 3]


def test_words_are_maximal_runs_between_separators():
    C, seps = E.WORD_C, E.sep_table(E.WORD_SEPS, E.WORD_C)
    assert seps == [1, 0, 0, 0, 0, 0, 0, 1]
    assert E.words([0, 1, 2, 0, 3, 0], seps, C) == [(1, 3), (4, 5)]                    # separators at both ends
    assert E.words([1, 2, 0, 0, 7, 0, 3, 4], seps, C) == [(0, 2), (6, 8)]              # runs of separators
    assert E.words([0, 7, 0, 0], seps, C) == [] and E.words([], seps, C) == []         # separators only
    assert E.words([1, -1, 2, 0, 3, 11], seps, C) == [(0, 3), (4, 6)]                  # labels outside [0, C) belong to words
    assert E.words([8, 0, 15], seps, C) == [(0, 1), (2, 3)]
    want = {0: ([0, 0], [0, 0, 0, 2]),   # per case: the script over words and (substitutions, insertions, deletions, hits)
            2: ([3, 3], [0, 0, 2, 0]),
            3: ([], [0, 0, 0, 0]),
            4: ([1, 0], [1, 0, 0, 1]),   # 1 2 against 1 2 3: one substitution, the equal prefix does not make them equal
            5: ([1, 0], [1, 0, 0, 1]),   # equal except for the last label
            6: ([0, 1, 0], [1, 0, 0, 2])}
    for k, (codes, counts) in want.items():
        hyp, ref = E.WORD_CASES[k]
        a, a_len = E.pad([hyp], max(len(hyp), 1))
        b, b_len = E.pad([ref], max(len(ref), 1))
        out = E.expected(a, a_len, b, b_len, C=C, separators=E.WORD_SEPS)
        assert out["script"][0, :int(out["script_len"][0])].tolist() == codes and out["counts"][0].tolist() == counts, k
    a, a_len = E.pad([E.WORD_CASES[0][0]], 6)
    out = E.expected(a, a_len, a, a_len, C=C, separators=E.WORD_SEPS)
    assert out["a_spans"].tolist() == [[[1, 3], [4, 5], [-1, -1]]] and out["totals"].tolist() == [0, 0, 0, 2, 1, 0]


def test_confusion_counts_of_the_reference():
    a, a_len = E.pad([[1, 2, 9, 3], [2]], 4)
    b, b_len = E.pad([[1, 3, 3], [2, -1]], 3)
    out = E.expected(a, a_len, b, b_len, C=4, confusion=True)
    # line 0, from the end: 3 = 3; 9 for 3 (D(2, 1) + 1 = D(3, 2) = 2: the diagonal; 9 is outside [0, 4): skipped); 2 inserted (D(2, 1) = 1 is
    # neither D(1, 0) + 1 nor D(2, 0) + 1); 1 = 1.  line 1: 2 = 2, then -1 deleted: skipped
    assert out["script"][0, :4].tolist() == [0, 2, 1, 0] and out["script"][1, :2].tolist() == [0, 3]
    m = torch.zeros(5, 5, dtype=torch.int64)
    m[1, 1], m[4, 2], m[3, 3], m[2, 2] = 1, 1, 1, 1
    assert torch.equal(out["confusion"], m)
    assert out["totals"].tolist() == [1, 1, 1, 3, 2, 2]


def test_top_confusions_orders_by_count_then_reference_then_hypothesis():
    from pero_pretraining_amd.recognition import top_confusions
    m = torch.zeros(4, 4, dtype=torch.int64)          # C = 3; index 3 is the gap
    m[0, 0], m[1, 1] = 100, 50                         # the diagonal is no confusion
    m[2, 1], m[0, 3], m[3, 2], m[1, 0], m[0, 1] = 7, 5, 5, 5, 5
    assert top_confusions(m) == [(2, 1, 7), (0, 1, 5), (0, None, 5), (1, 0, 5), (None, 2, 5)]
    assert top_confusions(m, k=2) == [(2, 1, 7), (0, 1, 5)]
    assert top_confusions(m, k=3, symbols="abc") == [("c", "b", 7), ("a", "b", 5), ("a", None, 5)]
    assert top_confusions(torch.zeros(3, 3, dtype=torch.int64)) == []


def test_pairs_of_a_script_are_the_walks_indices():
    """EditOperations.pairs() is plain tensor arithmetic on the codes: here on host tensors, against the walk's own (i, j)."""
    from pero_pretraining_amd.recognition import EditOperations
    cases = E.random_pairs(20, 9, 2, seed=3) + [([], []), ([1, 1], []), ([], [0])]
    a, a_len = E.pad([c[0] for c in cases], 9)
    b, b_len = E.pad([c[1] for c in cases], 9)
    out = E.expected(a, a_len, b, b_len)
    r = EditOperations(out["counts"], out["script"], out["script_len"])
    pairs = r.pairs()
    assert pairs.shape == (len(cases), 18, 2) and pairs.dtype == torch.int32
    assert r.distance.tolist() == [E.table(x, y)[len(x)][len(y)] for x, y in cases]
    for n, (x, y) in enumerate(cases):
        steps = E.walk(x, y)
        assert pairs[n, :len(steps)].tolist() == [[i - 1, j - 1] for _, i, j in steps] and bool((pairs[n, len(steps):] == -1).all())


# ---------------------------------------------------------------------------------------------- the library's host side
@pytest.fixture(scope="module")
def h():
    from pero_pretraining_amd import _lib
    return _lib.lib()


def _ops(h, *, a=True, a_len=True, b=True, b_len=True, is_sep=False, counts=True, script=False, script_len=False, a_spans=False, b_spans=False,
         totals=False, confusion=False, N=2, La=4, Lb=4, C=5):
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its host checks
    given = [a, a_len, b, b_len, is_sep, counts, script, script_len, a_spans, b_spans, totals, confusion]
    return h.pero_edit_ops(*[p if g else None for g in given], N, La, Lb, C, None)


def test_edit_ops_validates_its_arguments_without_a_gpu(h):
    for missing in ("a", "a_len", "b", "b_len", "counts"):
        assert _ops(h, **{missing: False}) == -1 and b"null pointer" in h.pero_last_error(), missing
    for bad in ({"N": 0}, {"N": -1}, {"La": -1}, {"Lb": -1}, {"N": 1 << 31}):
        assert _ops(h, **bad) == -1 and b"bad sizes" in h.pero_last_error(), bad
    assert _ops(h, La=513) == -2 and b"supported up to" in h.pero_last_error()
    assert _ops(h, Lb=513) == -2
    assert _ops(h, script=True) == -1 and b"script" in h.pero_last_error()          # script without script_len
    assert _ops(h, script_len=True) == -1
    assert _ops(h, confusion=True, is_sep=True) == -1 and b"symbol level" in h.pero_last_error()
    assert _ops(h, confusion=True, C=0) == -1 and b"bad sizes" in h.pero_last_error()
    assert _ops(h, is_sep=True, C=0) == -1 and _ops(h, is_sep=True, C=-4) == -1
    assert _ops(h, a_spans=True) == -1 and b"word level" in h.pero_last_error()      # spans without is_sep


def test_python_wrapper_rejects_host_tensors_and_bad_arguments(monkeypatch):
    from pero_pretraining_amd import _lib, ops
    i64 = torch.int64
    a, n = torch.zeros(2, 3, dtype=i64), torch.tensor([1, 1])
    with pytest.raises(_lib.PeroHipError):
        ops.edit_ops(a, n, a, n)
    monkeypatch.setattr(ops, "_req_cuda", lambda *ts: None)          # the remaining checks come before any launch
    monkeypatch.setattr(ops, "call", lambda *args: pytest.fail("launched"))
    for bad in [dict(a=a[0]), dict(a=a[:1]), dict(b_len=torch.tensor([1])), dict(a=a.int()), dict(a=a.t().contiguous().t()), dict(a_len=n.int())]:
        with pytest.raises(ValueError):
            ops.edit_ops(**{**dict(a=a, a_len=n, b=a, b_len=n), **bad})
    for bad in [dict(totals=torch.zeros(2, dtype=i64)), dict(totals=torch.zeros(6, dtype=torch.int32)),
                dict(confusion=torch.zeros(4, 5, dtype=i64)), dict(confusion=torch.zeros(5, 5, dtype=i64), num_classes=5),
                dict(confusion=torch.zeros(5, 5, dtype=i64), separators=[0], num_classes=4), dict(separators=[0]), dict(want_spans=True),
                dict(separators=torch.zeros(3, dtype=torch.uint8), num_classes=4)]:
        with pytest.raises(ValueError):
            ops.edit_ops(a, n, a, n, **bad)
    assert ops.edit_separator_table([0, 3, 3, 9, -1], 5, "cpu").tolist() == [1, 0, 0, 1, 0]
