"""GPU: pero_ctc_beam_lm (csrc/ctc_decode.hip) and its users in the recognition package against tests/ctc_beam_lm_ref.py, which
test_ctc_lm_ref_cpu.py pins to an exhaustive enumeration.  As in test_gpu_ctc_beam.py every case goes through the REPLAY check (the kernel's
own trace replayed in f64 with the language-model term: no margin needed), the lines with a decision margin of 2 x the bound are compared
string by string with the independent search, and integer outputs and repeated calls are compared exactly.  What the header fixes as a
chain of f32 operations - the nodes' LM state and weight, out_lm - is compared as bits.  Every bound is the one ctc_beam_lm_ref's docstring
derives.  bf16 logits are rounded once on the host; the reference sees the rounded values."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import ctc_beam_lm_ref as L
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


@functools.lru_cache(maxsize=None)
def model(C, blank, order=3):
    return L.fitted(C, blank, order=order)


def rows(x, dtype):
    N, S, C = x.shape
    return x.to(dtype).cuda().reshape(N * S, C).contiguous()


def beam_lm(ops, x, il, blank, W, K, lm, alpha, beta, use_final, dtype):
    """x (N, S, C) f32 holding values exact in `dtype`.  The six results of ops.ctc_beam_lm with the trace."""
    return ops.ctc_beam_lm(rows(x, dtype), il.cuda(), W, lm, alpha, beta, K, use_final, blank, return_trace=True)


def specified(x, il, result, lm_parts=True):
    """The parts of the outputs and of the trace that the header specifies, as exact (integer) tensors.  lm_parts False: those that
    pero_ctc_beam has as well."""
    out, lengths, scores, count, out_lm, tr = result
    parts = [out.cpu(), lengths.cpu(), scores.cpu().view(torch.int32), count.cpu(), tr["node_count"].cpu()]
    if lm_parts:
        parts.append(out_lm.cpu().view(torch.int32))
    for n, T in enumerate(il.clamp(0, x.shape[1]).tolist()):
        k = int(tr["node_count"][n])
        parts += [tr["node_parent"][n, :k].cpu(), tr["node_label"][n, :k].cpu(), tr["beam_node"][n, :T].cpu(),
                  tr["beam_score"][n, :T].cpu().view(torch.int32)]
        if lm_parts:
            parts += [tr["node_lm_state"][n, :k].cpu(), tr["node_lm_weight"][n, :k].cpu().view(torch.int32)]
    return parts


def check_replay(ops, x, il, blank, W, K, lm, alpha, beta, use_final, dtype):
    args = (ops, x, il, blank, W, K, lm, alpha, beta, use_final, dtype)
    result = beam_lm(*args)
    out, lengths, scores, count, out_lm, tr = result
    N, S, C = x.shape
    assert out.shape == (N, W, S) and out.dtype == torch.int64 and lengths.shape == (N, W) and scores.shape == (N, W) and scores.dtype == F32
    assert out_lm.shape == (N, W) and out_lm.dtype == F32 and tr["node_lm_state"].shape == (N, S * W + 1)
    out, lengths, scores, count, out_lm = (v.cpu().tolist() for v in (out, lengths, scores, count, out_lm))
    worst, stats = 0.0, []
    for n in range(N):
        T = min(max(int(il[n]), 0), S)
        stats.append(L.replay(x[n], T, blank, W, K, lm, alpha, beta, use_final, L.trace_line(tr, n), out[n], lengths[n], scores[n], out_lm[n],
                              count[n]))
        worst = max(worst, stats[-1]["ratio"])
    key = "ctc beam lm scores [bf16 logits]" if dtype == torch.bfloat16 else "ctc beam lm scores [f32]"
    R.RATIOS[key] = max(R.RATIOS.get(key, 0.0), worst)
    again = beam_lm(*args)          # two calls, the same bits: outputs and trace
    for a, b in zip(specified(x, il, result), specified(x, il, again)):
        assert torch.equal(a, b)
    return result, stats


# ------------------------------------------------------------------------------------------------ the null model is pero_ctc_beam
def _identity_case(name, dtype):
    if name == "C37-S12-W8":
        gen = torch.Generator().manual_seed(37)
        x = (2 * torch.randn(6, 12, 37, generator=gen)).to(dtype).float()
        return x, torch.tensor([12, 9, 12, 0, 1, 12]), 0, 8
    return B.reentry_case(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["C37-S12-W8", "C3-S10-W3-x4", "C3-S12-W4-x6"])
def test_null_model_is_the_plain_search_bit_for_bit(ops, name, dtype):
    """alpha = 0, beta = 0, no final term, K = min(W + 1, C - 1): w = +0 and x + 0 = x, so every output and trace entry pero_ctc_beam
    specifies is equal as an integer."""
    x, il, blank, W = _identity_case(name, dtype)
    C = x.shape[-1]
    plain = ops.ctc_beam(rows(x, dtype), il.cuda(), W, blank, return_trace=True)
    got = beam_lm(ops, x, il, blank, W, min(W + 1, C - 1), model(C, blank), 0.0, 0.0, False, dtype)
    ref = specified(x, il, plain[:4] + (None,) + plain[4:], lm_parts=False)
    for k, (a, b) in enumerate(zip(specified(x, il, got, lm_parts=False), ref)):
        assert a.dtype == b.dtype and torch.equal(a, b), k
    live = torch.arange(W)[None] < got[3].cpu()[:, None]
    assert bool((got[4].cpu()[live].view(torch.int32) == 0).all()) and bool((got[4].cpu()[~live] == 0).all())          # out_lm: sums of +0


# ------------------------------------------------------------------------------------------------ replay
SETTINGS = [(0.5, 0.0, True), (2.0, 1.5, False), (0.5, -1.0, True), (2.0, 0.0, False), (0.5, 1.5, True), (2.0, -1.0, True)]   # alpha, beta, final


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [1, 3, 16, 32])
@pytest.mark.parametrize("C,blank", [(5, 0), (5, 4), (37, 0), (37, 36)])
def test_replay_of_the_trace(ops, C, blank, W, dtype):
    """ctc_beam_ref.planted_case (T = 0, 1, S and S - 3 in one batch; a planted string with repeats; a line of wide-range logits) under an
    order-3 model, with K = 1, W + 1 and C - 1 (the largest K the kernel takes where W C exceeds its 1088 candidates); alpha in {0.5, 2},
    beta in {0, 1.5, -1} and the final term on and off rotate through the cases so that each value meets each K."""
    x, il, blank = B.planted_case(C, blank, dtype=dtype)
    lm = model(C, blank)
    walk_start = float(lm.final[lm.start])
    for i, kind in enumerate(["1", "W+1", "C-1"]):
        alpha, beta, use_final = SETTINGS[(i + [1, 3, 16, 32].index(W) + (C == 37) + 2 * (blank != 0)) % len(SETTINGS)]
        K = L.class_top(kind, W, C)
        (out, lengths, scores, count, out_lm, _), _ = check_replay(ops, x, il, blank, W, K, lm, alpha, beta, use_final, dtype)
        # T = 0: the empty string; its score is the final term of the start state, or 0
        want = float(np.float32(alpha) * np.float32(walk_start)) if use_final else 0.0
        assert int(count[0]) == 1 and int(lengths[0, 0]) == 0 and float(scores[0, 0]) == want == float(out_lm[0, 0])
        assert bool((scores[0, 1:] == -math.inf).all()) and bool((out[0] == -1).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_replay_of_a_long_line(ops, dtype):
    """S = 264 frames (more than a workgroup has threads), C = 37, W = 4, K = 20."""
    x, il, blank, W = B.long_case(dtype)
    check_replay(ops, x, il, blank, W, 20, model(37, 0), 0.5, 1.5, True, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_class_without_a_unigram_arc_is_forbidden(ops, dtype):
    """The planted line spells a a b b a; without an arc for b in state 0 no hypothesis and no node holds b, whatever the logits say.  (The
    replay also refuses such a node.)"""
    C, blank = 5, 0
    x, il, blank = B.planted_case(C, blank, dtype=dtype)
    lm = L.without_class(model(C, blank), 4)
    for W, K in [(3, 4), (16, 2)]:
        (out, lengths, _, count, _, tr), stats = check_replay(ops, x, il, blank, W, K, lm, 0.5, 0.0, True, dtype)
        assert not bool((out == 4).any())
        for n in range(x.shape[0]):
            assert not bool((tr["node_label"][n, :int(tr["node_count"][n])] == 4).any())
        assert int(count[3]) >= 1 and int(lengths[3, 0]) >= 1          # the line still decodes to something


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_order_one_model_has_a_single_state(ops, dtype):
    lm = model(37, 0, order=1)
    assert lm.num_states == 1
    x, il, blank = B.planted_case(37, 0, dtype=dtype)
    (_, _, _, _, _, tr), _ = check_replay(ops, x, il, blank, 8, 12, lm, 2.0, -1.0, True, dtype)
    for n in range(x.shape[0]):
        assert not bool(tr["node_lm_state"][n, :int(tr["node_count"][n])].any())


# ------------------------------------------------------------------------------------------------ the independent search
def compare_with_search(res, out, lengths, scores, out_lm, count):
    assert count == len(res["hyps"])
    for k, (s, v) in enumerate(res["hyps"]):
        assert int(lengths[k]) == len(s) and tuple(out[k, :len(s)].tolist()) == s, (k, s, out[k].tolist())
        assert abs(float(scores[k]) - v) <= res["bound"], (k, float(scores[k]), v, res["bound"])
        assert L.bits(out_lm[k]) == L.bits(res["lm"][k]), (k, float(out_lm[k]), float(res["lm"][k]))


@functools.lru_cache(maxsize=None)
def exact(dtype):
    return L.exact_case(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_comparison_with_the_independent_search(ops, dtype):
    x, il, blank, W, K, lm, alpha, beta, use_final, res, lines = exact(dtype)
    if dtype == F32:
        assert 4 * len(res) >= 3 * lines, (len(res), lines)          # a test that skips most lines shows nothing
    assert len(res) >= 1
    out, lengths, scores, count, out_lm, _ = beam_lm(ops, x, il, blank, W, K, lm, alpha, beta, use_final, dtype)
    out, lengths, scores, out_lm = out.cpu(), lengths.cpu(), scores.cpu(), out_lm.cpu()
    for n, r in enumerate(res):
        compare_with_search(r, out[n], lengths[n], scores[n], out_lm[n], int(count[n]))
        for k in range(W):
            assert bool((out[n, k, int(lengths[n, k]):] == -1).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(B.REENTRY_CASES))
def test_a_prefix_that_returns_keeps_its_node_and_its_lm_state(ops, name, dtype):
    """Under REENTRY_LM both re-entry cases keep a prefix that leaves the beam and comes back (asserted on the reference).  In the kernel's
    trace the returning prefix must be the SAME node - the replay refuses two nodes that spell one string - and the node's LM state and weight,
    which the kernel takes from the node and does not look up again, are the walk's (replay: as bits); the line also has a margin, so the
    hypotheses are the independent search's."""
    x, il, blank, W = B.reentry_case(name, dtype)
    alpha, beta, K = L.REENTRY_LM
    lm = model(3, 0)
    res = L.search(x, il, blank, W, K, lm, alpha, beta, True)[0]
    want = L.returns([[s for s, _, _ in f] for f in res["frames"]])
    assert res["reentries"] >= 1 and len(want) >= 1 and res["margin"] >= 2 * res["bound"]
    (out, lengths, scores, count, out_lm, tr), stats = check_replay(ops, x, il, blank, W, K, lm, alpha, beta, True, dtype)
    line = L.trace_line(tr, 0)
    got = L.returns([[k for k in row if k >= 0] for row in line["beam_node"][:x.shape[1]]])
    strings, walk = stats[0]["strings"], L.Walk(lm, alpha, beta)
    assert [(t, strings[k]) for t, k in got] == want
    for _, k in got:
        assert line["node_lm_state"][k] == walk.of(strings[k])[0]
    compare_with_search(res, out[0].cpu(), lengths[0].cpu(), scores[0].cpu(), out_lm[0].cpu(), int(count[0]))


def test_the_model_changes_the_winner_on_the_device(ops):
    """ctc_beam_lm_ref.winner_case: 1 3 without the model, 1 2 with it (test_ctc_lm_ref_cpu.py asserts the precondition on the reference)."""
    x, il, blank, lm, alpha = L.winner_case()
    plain = ops.ctc_beam(rows(x, F32), il.cuda(), 8, blank)
    assert plain[0][0, 0, :int(plain[1][0, 0])].tolist() == [1, 3]
    (out, lengths, _, _, _, _), _ = check_replay(ops, x, il, blank, 8, 3, lm, alpha, 0.0, True, F32)
    assert out[0, 0, :int(lengths[0, 0])].tolist() == [1, 2]


def test_class_top_default_and_limit(ops):
    x, il, blank = B.planted_case(130, 0)
    lm = model(130, 0, order=1)
    with pytest.raises(ValueError, match="1088"):
        ops.ctc_beam_lm(rows(x, F32), il.cuda(), 16, lm, class_top=68)
    with pytest.raises(ValueError, match="classes"):
        ops.ctc_beam_lm(rows(x, F32), il.cuda(), 16, model(37, 0))
    default = ops.ctc_beam_lm(rows(x, F32), il.cuda(), 16, lm)          # None: min(C - 1, 1088 // W - 1) = 67
    explicit = ops.ctc_beam_lm(rows(x, F32), il.cuda(), 16, lm, class_top=67)
    assert len(default) == 5 and all(torch.equal(a, b) for a, b in zip(default, explicit))
    beyond = ops.ctc_beam_lm(rows(x, F32), il.cuda(), 4, lm, class_top=1000)          # clamped to C - 1 = 129: 4 * 130 candidates
    assert all(torch.equal(a, b) for a, b in zip(beyond, ops.ctc_beam_lm(rows(x, F32), il.cuda(), 4, lm, class_top=129)))


# ------------------------------------------------------------------------------------------------ the recognition package
def test_beam_decode_without_a_model_is_unchanged_and_with_one_returns_the_shapes():
    from pero_pretraining_amd import ops, recognition
    x, il, blank = B.planted_case(37, 0)
    lm = model(37, 0)
    want = ops.ctc_beam(rows(x, F32), il.cuda(), 4, blank)
    for nbest in (1, 3):
        got = recognition.beam_decode(x.cuda(), il.cuda(), blank=0, beam_width=4, nbest=nbest, lm=None)
        assert len(got) == 3
        for a, b in zip(got, want):
            b = b[:, 0] if nbest == 1 else b[:, :nbest]
            assert torch.equal(a.view(torch.int32) if a.dtype == F32 else a, b.view(torch.int32) if b.dtype == F32 else b)
    labels, lengths, scores, lm_scores = recognition.beam_decode(x.cuda(), il.cuda(), 0, 4, nbest=3, lm=lm, lm_weight=0.5, length_bonus=1.5,
                                                                 return_lm_scores=True)
    assert labels.shape == (5, 3, 16) and lengths.shape == (5, 3) and scores.shape == (5, 3) and lm_scores.shape == (5, 3)
    full = ops.ctc_beam_lm(rows(x, F32), il.cuda(), 4, lm, 0.5, 1.5)
    assert torch.equal(labels, full[0][:, :3]) and torch.equal(scores, full[2][:, :3]) and torch.equal(lm_scores, full[4][:, :3])
    one = recognition.beam_decode(x.cuda(), il.cuda(), 0, 4, lm=lm, lm_weight=0.5, length_bonus=1.5)
    assert len(one) == 3 and one[0].shape == (5, 16) and torch.equal(one[0], labels[:, 0]) and torch.equal(one[2], scores[:, 0])
    with pytest.raises(ValueError):
        recognition.beam_decode(x.cuda(), il.cuda(), 1, 4, lm=lm)          # the model's blank is 0
    with pytest.raises(ValueError):
        recognition.beam_decode(x.cuda()[..., :36], il.cuda(), 0, 4, lm=lm)
    with pytest.raises(ValueError):
        recognition.beam_decode(x.cuda(), il.cuda(), 0, 4, return_lm_scores=True)


def test_recogniser_and_tester_decode_with_a_model():
    """A two-layer d = 64 recogniser: decode, transcribe and Tester(beam_width = 4, lm = ...) use the same search; the Tester's character
    error rate is the one counted on the host from the decoded strings."""
    from pero_pretraining_amd.recognition import BatchOperator, Tester, beam_decode, init_model, levenshtein
    torch.manual_seed(0)
    C = 37
    net = init_model(torch.device("cuda"), {"type": "vit", "num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128},
                     {"type": "linear", "in_features": 64, "out_features": C}, blank=0).eval()
    lm = model(C, 0)
    rng = np.random.default_rng(0)
    batch = {"images": rng.integers(0, 256, (3, 40, 192, 3), dtype=np.uint8), "targets": rng.integers(1, C, (3, 7)),
             "target_lengths": np.array([7, 5, 6]), "widths": np.array([192, 130, 77])}
    operator = BatchOperator(torch.device("cuda"))
    images, targets, target_lengths, il = operator.prepare_batch(batch)
    kw = dict(lm=lm, lm_weight=0.5, length_bonus=1.0, class_top=12)
    labels, lengths, scores, lm_scores = net.decode(images, il, beam_width=4, return_lm_scores=True, **kw)
    assert labels.shape == (3, 24) and lengths.shape == (3,) and scores.shape == (3,) and lm_scores.shape == (3,)
    with torch.no_grad():
        output = net(images, input_lengths=il)["output"]
    direct = beam_decode(output, il, 0, 4, return_lm_scores=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip((labels, lengths, scores, lm_scores), direct))
    plain = net.decode(images, il, beam_width=4)
    assert len(plain) == 3
    t_labels, t_lengths, alignment = net.transcribe(images, il, beam_width=4, **kw)
    assert torch.equal(t_labels, labels) and torch.equal(t_lengths, lengths) and alignment.spans.shape[0] == 3
    result = Tester(operator, net, [batch, batch], beam_width=4, **kw).test()
    decoded = [labels[n, :int(lengths[n])].tolist() for n in range(3)]
    distance = sum(levenshtein(decoded[n], batch["targets"][n, :batch["target_lengths"][n]].tolist()) for n in range(3))
    assert result["cer"] == (2 * distance) / (2 * int(batch["target_lengths"].sum()))
