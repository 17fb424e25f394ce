"""CPU: tests/ctc_align_ref.py against itself and against ctc_ref.py.  On integer-valued logits every partial sum is exact, so the
float32 recursion must pick the very path an enumeration of all paths picks, tie rule included; on random logits its path is within the
derived bound of the f64 optimum; on a line's greedy string its value is the f32 sum of the row maxima, bit for bit."""
import math

import numpy as np
import pytest
import torch

import ctc_align_ref as A
import ctc_ref
from parity_ref import U32


def one_line(x, labels, T, blank=0, Lmax=None):
    """align_f32 of a single line: x (S, C)"""
    Lmax = max(len(labels), 1) if Lmax is None else Lmax
    targets = torch.full((1, Lmax), ctc_ref.SENTINEL, dtype=torch.int64)
    targets[0, :len(labels)] = torch.tensor(labels, dtype=torch.int64)
    x = torch.as_tensor(x).float()
    res = A.align_f32(x[None], targets, [T], [len(labels)], blank)
    return res, targets


STRINGS = [[], [1], [2], [1, 2], [1, 1], [2, 2, 1], [1, 2, 1], [1, 1, 1], [0, 1], [1, 0, 1]]   # C = 3; 0 is the blank when blank = 0


@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 7])
def test_integer_logits_agree_with_the_enumeration_of_all_paths(T, blank):
    """T <= 7, L <= 3, C = 3, integer logits in [-8, 8] (many ties), the all-zero line among them"""
    gen = torch.Generator().manual_seed(100 * T + blank)
    lines = [torch.zeros(T, 3)] + [torch.randint(-8, 9, (T, 3), generator=gen).float() for _ in range(3)]
    lines.append(torch.randint(-1, 2, (T, 3), generator=gen).float())          # three values only: ties everywhere
    for x in lines:
        for labels in STRINGS:
            res, targets = one_line(x, labels, T, blank)
            value, path = A.brute_force(x.numpy(), targets[0].numpy(), T, len(labels), blank)
            if path is None:
                assert not res["feasible"][0] and res["path_logit"][0] == -math.inf
                assert (res["states"] == -1).all() and (res["spans"] == -1).all()
                continue
            assert res["feasible"][0]
            assert res["states"][0, :T].tolist() == path, (x.tolist(), labels, path)
            assert float(res["path_logit"][0]) == value
            assert (res["spans"][0] == A.spans_of(path, T, targets.shape[1])).all()


def test_the_all_zero_line_advances_as_early_as_it_can():
    res, _ = one_line(torch.zeros(7, 3), [1, 2], 7)
    assert res["states"][0].tolist() == [1, 3, 4, 4, 4, 4, 4]          # both labels at once (they differ: the blank is skipped), then the last blank
    assert res["spans"][0].tolist() == [[0, 1], [1, 2]] and float(res["path_logit"][0]) == 0.0
    res, _ = one_line(torch.zeros(7, 3), [1, 1], 7)
    assert res["states"][0].tolist() == [1, 2, 3, 4, 4, 4, 4]          # a repeated label needs the blank between
    res, _ = one_line(torch.zeros(3, 3), [1, 1], 3)
    assert res["states"][0].tolist() == [1, 2, 3]                      # T = L + repeats exactly: one path


@pytest.mark.parametrize("scale", [4.0, 30.0])
@pytest.mark.parametrize("name", ["mixed-C37-blank0", "mixed-C2-blank1", "mixed-C130-blank129"])
def test_random_logits_are_within_the_bound_of_the_f64_optimum(name, scale):
    c = ctc_ref.case(f"{name}-x{int(scale)}")
    res = A.align_f32(c["logits"], c["targets"], c["input_lengths"], c["target_lengths"], c["blank"])
    ref = A.align_f64(c["logits"], c["targets"], c["input_lengths"], c["target_lengths"], c["blank"], res["states"], res["feasible"])
    assert res["feasible"].tolist() == [n not in c["infeasible"] for n in range(6)]
    for n in range(6):
        if not res["feasible"][n]:
            assert float(ref["optimum"][n]) == -math.inf
            continue
        # the optimum's own path obeys the same bound; its partial sums are no larger than the sum of the rows' largest magnitudes
        T = int(c["input_lengths"][n])
        worst = T * float(c["logits"][n, :T].abs().max(-1).values.double().sum())
        bound = 2 * max(float(ref["path_units"][n]), worst) * U32
        gap = float(ref["optimum"][n] - ref["path_logit"][n])
        assert -1e-9 <= gap <= bound, (n, gap, bound)
        assert abs(float(res["path_logit"][n]) - float(ref["path_logit"][n])) <= float(ref["path_units"][n]) * U32
        # spans: consecutive, in label order, every label at least one frame
        L = int(c["target_lengths"][n])
        sp = res["spans"][n, :L]
        assert (sp[:, 1] > sp[:, 0]).all() and (sp[1:, 0] >= sp[:-1, 1]).all() and (res["spans"][n, L:] == -1).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_greedy_string_aligns_to_the_row_maxima(dtype):
    """The path of the per-row maxima spells the greedy string, and an f32 sum is monotone in its terms: no path has a larger value."""
    gen = torch.Generator().manual_seed(3)
    x = (4 * torch.randn(4, 24, 11, generator=gen)).to(dtype).float()
    il = torch.tensor([24, 17, 1, 24])
    x[3, :, 0] += 20.0          # an all-blank line: the empty string
    for blank in (0, 10):
        if blank == 10:
            x[3, :, 10] += 40.0
        labels, lengths = ctc_ref.greedy(x, il, blank)
        res = A.align_f32(x, labels, il, lengths, blank)
        assert res["feasible"].all() and int(lengths[3]) == 0
        for n in range(4):
            acc = None
            for t in range(int(il[n])):
                m = np.float32(x[n, t].max())
                acc = m if acc is None else np.float32(acc + m)
            assert res["path_logit"][n].tobytes() == np.float32(acc).tobytes()
            st = res["states"][n, :int(il[n])]
            cls = A.state_classes(labels[n].numpy(), int(lengths[n]), 11, blank)
            assert (x[n, torch.arange(int(il[n])), torch.from_numpy(cls[st])] == x[n, :int(il[n])].max(-1).values).all()


def test_infeasible_and_empty_lines():
    x = torch.randn(6, 3, generator=torch.Generator().manual_seed(1))
    res, _ = one_line(x, [1, 1], 2)                       # needs 3 frames
    assert not res["feasible"][0] and res["path_logit"][0] == -math.inf and (res["states"] == -1).all() and (res["spans"] == -1).all()
    res, _ = one_line(x, [1, 1], 3)
    assert res["feasible"][0] and res["states"][0].tolist() == [1, 2, 3, -1, -1, -1]
    res, _ = one_line(x, [], 0)                           # T = 0, L = 0: the empty path, value 0
    assert res["feasible"][0] and float(res["path_logit"][0]) == 0.0 and (res["states"] == -1).all()
    res, _ = one_line(x, [1], 0)                          # T = 0, L > 0
    assert not res["feasible"][0] and res["path_logit"][0] == -math.inf
    res, targets = one_line(x, [], 4, Lmax=2)             # L = 0: every frame in state 0
    assert res["feasible"][0] and res["states"][0].tolist() == [0, 0, 0, 0, -1, -1] and (res["spans"] == -1).all()
    assert res["path_logit"][0] == np.float32(np.float32(np.float32(x[0, 0] + x[1, 0]) + x[2, 0]) + x[3, 0])
    res, _ = one_line(x, [1, 7], 6)                       # a label outside [0, C)
    assert not res["feasible"][0]
    y = x.clone()
    y[2, :] = -math.inf                                   # a frame nothing can emit in
    res, _ = one_line(y, [1], 6)
    assert not res["feasible"][0]
    y = x.clone()
    y[:, 1] = -math.inf
    y[4, 1] = 0.5                                         # the label can sit in frame 4 only
    res, targets = one_line(y, [1], 6)
    assert res["feasible"][0] and res["spans"][0].tolist() == [[4, 5]] and res["states"][0].tolist() == [0, 0, 0, 0, 1, 2]
    ref = A.align_f64(y[None], targets, [6], [1], 0, res["states"], res["feasible"])
    lp = torch.log_softmax(y.double(), -1)
    assert abs(float(ref["label_logp"][0, 0]) - float(lp[4, 1])) < 1e-12
    want = float(lp[[0, 1, 2, 3, 5], 0].sum() + lp[4, 1])
    assert abs(float(ref["score"][0]) - want) < 1e-10
    # lengths beyond the matrices are clamped
    res2 = A.align_f32(y[None], targets, [1000], [1000], 0)
    assert (res2["states"] == res["states"]).all()
