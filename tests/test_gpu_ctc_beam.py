"""GPU: pero_ctc_beam (csrc/ctc_decode.hip) and pero_edit_distance (csrc/edit.hip) and their users in the recognition package against
tests/ctc_beam_ref.py, whose search test_ctc_beam_ref_cpu.py pins to the CTC likelihood.  Every case goes through the REPLAY check
(the kernel's own trace, replayed in f64: no line is left out, no margin is needed); the lines whose decisions have a margin of
2 x the bound are also compared string by string with the independent search.  Every bound is the one ctc_beam_ref's docstring
derives; integer outputs and repeated calls are compared exactly.  bf16 logits are rounded once on the host; the reference sees
the rounded values."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import ctc_beam_ref as B
import ctc_ref
import parity_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    yield _ops
    print("\nPARITY_RATIOS " + json.dumps({k: round(v, 4) for k, v in sorted(R.RATIOS.items())}))


def beam(ops, x, il, blank, W, dtype):
    """x (N, S, C) f32 holding values exact in `dtype`.  The five results of ops.ctc_beam with the trace."""
    N, S, C = x.shape
    return ops.ctc_beam(x.to(dtype).cuda().reshape(N * S, C).contiguous(), il.cuda(), W, blank, return_trace=True)


def specified(x, il, result):
    """The parts of the outputs and of the trace that the header specifies, as exact (integer) tensors, for bit comparisons."""
    out, lengths, scores, count, tr = result
    parts = [out.cpu(), lengths.cpu(), scores.cpu().view(torch.int32), count.cpu(), tr["node_count"].cpu()]
    for n, T in enumerate(il.clamp(0, x.shape[1]).tolist()):
        k = int(tr["node_count"][n])
        parts += [tr["node_parent"][n, :k].cpu(), tr["node_label"][n, :k].cpu(), tr["beam_node"][n, :T].cpu(),
                  tr["beam_score"][n, :T].cpu().view(torch.int32)]
    return parts


def check_replay(ops, x, il, blank, W, dtype):
    result = beam(ops, x, il, blank, W, dtype)
    out, lengths, scores, count, tr = result
    N, S, C = x.shape
    assert out.shape == (N, W, S) and out.dtype == torch.int64 and lengths.shape == (N, W) and scores.shape == (N, W) and scores.dtype == F32
    out, lengths, scores, count = out.cpu().tolist(), lengths.cpu().tolist(), scores.cpu().tolist(), count.cpu().tolist()
    worst = 0.0
    for n in range(N):
        T = min(max(int(il[n]), 0), S)
        stats = B.replay(x[n], T, blank, W, B.trace_line(tr, n), out[n], lengths[n], scores[n], count[n])
        worst = max(worst, stats["ratio"])
    key = "ctc beam scores [bf16 logits]" if dtype == torch.bfloat16 else "ctc beam scores [f32]"
    R.RATIOS[key] = max(R.RATIOS.get(key, 0.0), worst)
    # two calls, the same bits: outputs and trace
    again = beam(ops, x, il, blank, W, dtype)
    for a, b in zip(specified(x, il, result), specified(x, il, again)):
        assert torch.equal(a, b)
    return result


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [1, 3, 16, 32])
@pytest.mark.parametrize("C,blank", [(2, 0), (2, 1), (37, 0), (37, 36), (130, 0), (130, 129)])
def test_replay_of_the_trace(ops, C, blank, W, dtype):
    """T = 0, 1, S and S - 3 in one batch; a planted string with repeated labels; a line of wide-range logits."""
    x, il, blank = B.planted_case(C, blank, dtype=dtype)
    out, lengths, scores, count, _ = check_replay(ops, x, il, blank, W, dtype)
    assert int(count[0]) == 1 and int(lengths[0, 0]) == 0 and float(scores[0, 0]) == 0.0          # T = 0: the empty string, score 0
    assert bool((scores[0, 1:] == -math.inf).all()) and bool((out[0] == -1).all())
    if C > 2:   # the planted line decodes to its string: a a b b a with the repeats kept apart
        labels = [c for c in range(C) if c != blank]
        a, b = labels[0], labels[-1]
        assert out[3, 0, :int(lengths[3, 0])].tolist() == [a, a, b, b, a, a][:6]


@pytest.mark.parametrize("dtype", DTYPES)
def test_replay_of_a_long_line(ops, dtype):
    x, il, blank, W = B.long_case(dtype)
    check_replay(ops, x, il, blank, W, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(B.REENTRY_CASES))
def test_replay_where_a_prefix_returns_to_the_beam(ops, name, dtype):
    """The re-entry cases: a split string shows as "two nodes spell the same string" or "kept twice" in the replay; these lines also
    have one right answer often enough to be compared with the search where the margin allows."""
    x, il, blank, W = B.reentry_case(name, dtype)
    res = B.search(x, il, blank, W)[0]
    assert res["reentries"] >= 1
    out, lengths, scores, count, _ = check_replay(ops, x, il, blank, W, dtype)
    if res["margin"] >= 2 * res["bound"]:
        compare_with_search(res, out[0].cpu(), lengths[0].cpu(), scores[0].cpu(), int(count[0]))


def compare_with_search(res, out, lengths, scores, count):
    assert count == len(res["hyps"])
    for k, (s, v) in enumerate(res["hyps"]):
        assert int(lengths[k]) == len(s) and tuple(out[k, :len(s)].tolist()) == s, (k, s, out[k].tolist())
        assert abs(float(scores[k]) - v) <= res["bound"], (k, float(scores[k]), v, res["bound"])


@functools.lru_cache(maxsize=None)
def exact(dtype):
    return B.exact_case(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_comparison_with_the_independent_search(ops, dtype):
    x, il, blank, W, res = exact(dtype)
    out, lengths, scores, count, _ = beam(ops, x, il, blank, W, dtype)
    out, lengths, scores = out.cpu(), lengths.cpu(), scores.cpu()
    for n, r in enumerate(res):          # every line of the built batch
        compare_with_search(r, out[n], lengths[n], scores[n], int(count[n]))
        for k in range(W):
            assert bool((out[n, k, int(lengths[n, k]):] == -1).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_unpruned_search_scores_every_string_like_the_ctc_loss(ops, dtype):
    """C = 3, T = 4, W = 32: all 15 feasible strings come back, and each score is -nll of pero_ctc_fwd for that string on the same logits,
    within the sum of the two kernels' bounds (each is within its own bound of the f64 value)."""
    x, il, blank, W = B.exhaustive_case(dtype)
    out, lengths, scores, count, _ = check_replay(ops, x, il, blank, W, dtype)
    strings = B.feasible_strings(3, 4, blank)
    assert int(count[0]) == len(strings) == 15
    got = {tuple(out[0, k, :int(lengths[0, k])].tolist()): float(scores[0, k]) for k in range(15)}
    assert sorted(got) == sorted(strings)
    targets, tl = B.pad(strings, 4, fill=ctc_ref.SENTINEL)
    lg = x.to(dtype).cuda().reshape(4, 3).repeat(15, 1).contiguous()
    il15 = torch.full((15,), 4)
    nll = ops.ctc_fwd(lg, targets.cuda(), il15.cuda(), tl.cuda(), blank)[0].cpu()
    ref, mag = ctc_ref.ctc(x.expand(15, 4, 3), targets, il15, tl, blank)
    res = B.search(x, il, blank, W)[0]
    for k, s in enumerate(strings):
        loss_bound = float(R.bound(ref["nll"][k], mag["nll"][k], int(mag["nll_terms"][k]), F32))
        assert abs(got[s] + float(nll[k])) <= res["bound"] + loss_bound, (s, got[s], float(nll[k]), res["bound"], loss_bound)


def test_edit_distance_is_exact(ops):
    cases = B.edit_cases()
    a, a_len = B.pad([c[0] for c in cases], 512)          # the padding holds a label that occurs in the strings
    b, b_len = B.pad([c[1] for c in cases], 512)
    want = torch.tensor([ctc_ref.levenshtein(x, y) for x, y in cases])
    totals = torch.zeros(2, dtype=torch.int64).cuda()
    dist = ops.edit_distance(a.cuda(), a_len.cuda(), b.cuda(), b_len.cuda(), totals)
    assert dist.dtype == torch.int64 and torch.equal(dist.cpu(), want)
    assert totals.tolist() == [int(want.sum()), int(b_len.sum())]
    ops.edit_distance(a.cuda(), a_len.cuda(), b.cuda(), b_len.cuda(), totals)          # accumulated over two calls
    assert totals.tolist() == [2 * int(want.sum()), 2 * int(b_len.sum())]
    # the transposed problem, narrow matrices (La = 65 != Lb = 40), lengths beyond the width are clamped, no totals
    small = [(x[:65], y[:40]) for x, y in cases]
    a, a_len = B.pad([c[0] for c in small], 65)
    b, b_len = B.pad([c[1] for c in small], 40)
    want = torch.tensor([ctc_ref.levenshtein(x, y) for x, y in small])
    assert torch.equal(ops.edit_distance(b.cuda(), b_len.cuda(), a.cuda(), a_len.cuda()).cpu(), want)
    full = [(a[n].tolist(), b[n].tolist()) for n in range(len(small))]
    want = torch.tensor([ctc_ref.levenshtein(x, y) for x, y in full])
    assert torch.equal(ops.edit_distance(a.cuda(), (a_len + 1000).cuda(), b.cuda(), (b_len + 1000).cuda()).cpu(), want)
    # a zero-width matrix: every distance is the other length
    empty = torch.zeros((len(small), 0), dtype=torch.int64).cuda()
    assert torch.equal(ops.edit_distance(empty, a_len.cuda(), b.cuda(), b_len.cuda()).cpu(), b_len)


# ------------------------------------------------------------------------------------------------ the recognition package
class _Planted(torch.nn.Module):
    """A recogniser whose logits are planted (the construction of test_gpu_ctc.py)."""

    def __init__(self, logits, loss):
        super().__init__()
        self.logits, self.loss = logits, loss

    def forward(self, images, targets=None, target_lengths=None, input_lengths=None):
        out = self.logits[:images.shape[0]]
        return {"output": out, "loss": self.loss(out, targets, input_lengths, target_lengths)}


def _planted():
    # 3 3 - 7 7 7 - 7 1 - 9 4 4 (blank 0), cut to its first 11 frames (88 px): 3 7 7 1 9; the second line is noisier and shorter
    frames = [3, 3, 0, 7, 7, 7, 0, 7, 1, 0, 9, 4, 4, 0, 0, 0]
    logits = torch.zeros(2, 16, 12)
    logits[:, torch.arange(16), torch.tensor(frames)] = 8.0
    logits[1] += torch.randn(16, 12, generator=torch.Generator().manual_seed(2))
    batch = {"images": np.zeros((2, 40, 128, 3), np.uint8), "targets": np.array([[3, 7, 5, 1, 9, 0], [3, 7, 7, 1, 2, 2]]),
             "target_lengths": np.array([5, 6]), "widths": np.array([88, 72])}
    return logits, batch, torch.tensor([11, 9])


@pytest.mark.parametrize("beam_width", [None, 4])
def test_tester_counts_errors_on_the_device(beam_width):
    """Tester: the loss and the character error rate of planted logits.  Expected here from the f64 CTC reference and from host greedy
    decoding + the textbook edit distance; the planted strings are so peaked that the beam search's best string is the greedy one."""
    from pero_pretraining_amd.recognition import BatchOperator, CTCLoss, Tester
    logits, batch, il = _planted()
    model = _Planted(logits.cuda(), CTCLoss(blank=0))
    tester = Tester(BatchOperator(torch.device("cuda")), model, [batch, batch, batch], beam_width=beam_width)
    result = tester.test()
    assert set(result) == {"loss", "cer"} and model.training
    targets, tl = torch.from_numpy(batch["targets"]), torch.from_numpy(batch["target_lengths"])
    res, mag = ctc_ref.ctc(logits, targets, il, tl, 0)
    want, want_mag = ctc_ref.reduce(res["nll"], tl, "mean", mag_nll=mag["nll"])
    R.assert_within(torch.tensor(result["loss"]), want, want_mag, int(mag["nll_terms"].max()) + 2 + 3, F32, what="Tester loss")
    decoded, lengths = ctc_ref.greedy(logits, il, 0)
    assert decoded[0, :5].tolist() == [3, 7, 7, 1, 9] and int(lengths[0]) == 5
    distance = sum(ctc_ref.levenshtein(decoded[n, :int(lengths[n])].tolist(), targets[n, :int(tl[n])].tolist()) for n in range(2))
    assert distance >= 2 and result["cer"] == (3 * distance) / (3 * 11)
    # max_lines stops the loop as before: two lines per batch, the second batch is the last
    short = Tester(BatchOperator(torch.device("cuda")), model, [batch, batch, batch], max_lines=3, beam_width=beam_width).test()
    assert short["cer"] == result["cer"]


def test_beam_decode_returns_the_planted_strings_and_nbest_lists():
    from pero_pretraining_amd import recognition
    logits, _, il = _planted()
    labels, lengths, scores = recognition.beam_decode(logits.cuda(), il.cuda(), blank=0, beam_width=4)
    assert labels.shape == (2, 16) and lengths.shape == (2,) and scores.shape == (2,) and scores.dtype == F32
    assert labels[0, :5].tolist() == [3, 7, 7, 1, 9] and int(lengths[0]) == 5 and bool((labels[0, 5:] == -1).all())
    res = B.search(logits, il, 0, 4)
    for n in range(2):
        assert tuple(labels[n, :int(lengths[n])].tolist()) == res[n]["hyps"][0][0]
        assert abs(float(scores[n]) - res[n]["hyps"][0][1]) <= res[n]["bound"]
    labels3, lengths3, scores3 = recognition.beam_decode(logits.cuda(), il.cuda(), blank=0, beam_width=4, nbest=3)
    assert labels3.shape == (2, 3, 16) and lengths3.shape == (2, 3) and scores3.shape == (2, 3)
    assert torch.equal(labels3[:, 0], labels) and torch.equal(scores3[:, 0], scores) and bool((scores3[:, :-1] >= scores3[:, 1:]).all())
    # without input_lengths every line has S frames
    full = recognition.beam_decode(logits.cuda(), beam_width=4)[0]
    assert full[0, :6].tolist() == [3, 7, 7, 1, 9, 4]


def test_recogniser_decode_keeps_greedy_by_default():
    from pero_pretraining_amd.recognition import greedy_decode, init_model
    torch.manual_seed(0)
    model = init_model(torch.device("cuda"), {"type": "vit", "num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128},
                       {"type": "linear", "in_features": 64, "out_features": 37}, blank=0).eval()
    images = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (2, 40, 192, 3), dtype=np.uint8)).cuda()
    il = torch.tensor([24, 17]).cuda()
    offsets = np.array([5, 9])
    model.backbone.set_offsets(offsets)
    plain = model.decode(images, il)
    with torch.no_grad():
        model.backbone.set_offsets(offsets)
        output = model(images, input_lengths=il)["output"]
    want = greedy_decode(output, il, 0)
    assert isinstance(plain, tuple) and len(plain) == 2 and torch.equal(plain[0], want[0]) and torch.equal(plain[1], want[1])
    model.backbone.set_offsets(offsets)
    labels, lengths, scores = model.decode(images, il, beam_width=8)
    assert labels.shape == (2, 24) and lengths.shape == (2,) and scores.shape == (2,)
    res = B.search(output.float().cpu(), il.cpu(), 0, 8)
    for n in range(2):          # an untrained model: near-ties are likely, so the string is compared only where the margin allows
        assert bool((labels[n, int(lengths[n]):] == -1).all()) and float(scores[n]) <= 0.0
        if res[n]["margin"] >= 2 * res[n]["bound"]:
            assert tuple(labels[n, :int(lengths[n])].tolist()) == res[n]["hyps"][0][0]
