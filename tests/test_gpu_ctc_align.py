"""GPU: pero_ctc_align (csrc/ctc_align.hip) and its users in the recognition package against tests/ctc_align_ref.py.  states, spans
and path_logit are compared with the float32 restatement as INTEGERS (the recursion holds f32 additions and comparisons only: no
margin); score and label_logp are compared with their f64 values on the kernel's own path within the bounds ctc_align_ref's docstring
derives.  Every call goes to the C entry point with poisoned outputs and workspaces, twice, and the two results are compared as integers.
bf16 logits are rounded once on the host; the references see the rounded values.  The module prints its worst error / bound per
label (PARITY_RATIOS); DESIGN.md section 13 quotes them."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import ctc_align_ref as A
import ctc_ref
import parity_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
F32 = torch.float32
GLOBAL_BACK = 1            # PERO_CTC_ALIGN_GLOBAL_BACK
LDS_BACK_BYTES = 96 * 1024   # PERO_CTC_ALIGN_LDS_BACK_BYTES


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    yield _ops
    print("\nPARITY_RATIOS " + json.dumps({k: round(v, 4) for k, v in sorted(R.RATIOS.items())}))


def raw_align(x, targets, il, tl, blank, flags=0, poison=0x5a):
    """The C entry point on x (N, S, C) (a tensor of the kernel's dtype) with every output and workspace poisoned; the full `back`
    workspace is always passed.  Returns the five outputs on the host."""
    from pero_pretraining_amd import _lib
    from pero_pretraining_amd.ops import dt, ptr, stream
    N, S, C = x.shape
    Lmax = targets.shape[1]
    lg = x.cuda().reshape(N * S, C).contiguous()
    tg, ild, tld = targets.cuda(), torch.as_tensor(il).cuda(), torch.as_tensor(tl).cuda()

    def poisoned(shape, dtype):
        return torch.full((int(np.prod(shape)) * dtype.itemsize,), poison, dtype=torch.uint8, device="cuda").view(dtype).view(shape)

    states, spans = poisoned((N, S), torch.int32), poisoned((N, Lmax, 2), torch.int32)
    path_logit, score, label_logp = poisoned((N,), F32), poisoned((N,), F32), poisoned((N, Lmax), F32)
    row_lse, back = poisoned((N * S,), F32), poisoned((N * S * (2 * Lmax + 1),), torch.uint8)
    _lib.call("pero_ctc_align", ptr(lg), ptr(tg), ptr(ild), ptr(tld), ptr(states), ptr(spans), ptr(path_logit), ptr(score), ptr(label_logp),
              ptr(row_lse), ptr(back), N, S, C, Lmax, blank, flags, dt(lg), stream())
    return {"states": states.cpu(), "spans": spans.cpu(), "path_logit": path_logit.cpu(), "score": score.cpu(), "label_logp": label_logp.cpu()}


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def check(c, dtype, flags=0):
    """One case against both references.  c: logits (N, S, C) f32, targets, input_lengths, target_lengths, blank."""
    x = c["logits"].to(dtype)
    xf, tg, il, tl, blank = x.float(), c["targets"], c["input_lengths"], c["target_lengths"], c["blank"]
    N, S, C = xf.shape
    Lmax = tg.shape[1]
    got = raw_align(x, tg, il, tl, blank, flags, poison=0x5a)
    again = raw_align(x, tg, il, tl, blank, flags, poison=0xc3)
    assert same_bits(got, again)                                                     # two calls, other poison: the same bits
    want = A.align_f32(xf, tg, il, tl, blank)
    assert np.array_equal(got["states"].numpy(), want["states"])
    assert np.array_equal(got["spans"].numpy(), want["spans"])
    assert np.array_equal(got["path_logit"].numpy().view(np.int32), want["path_logit"].view(np.int32))
    if "infeasible" in c:
        assert [n for n in range(N) if not want["feasible"][n]] == list(c["infeasible"])
    ref = A.align_f64(xf, tg, il, tl, blank, got["states"].numpy(), want["feasible"])
    ok = torch.from_numpy(want["feasible"])
    assert bool((got["score"][~ok] == -math.inf).all()) and int(torch.count_nonzero(got["label_logp"][~ok])) == 0
    tag = " [bf16 logits]" if dtype == torch.bfloat16 else ""
    R.assert_within(got["score"][ok], ref["score"][ok], torch.ones(int(ok.sum())), ref["score_units"][ok], F32, what="ctc align score" + tag)
    has = ok[:, None] & (torch.arange(Lmax)[None, :] < torch.as_tensor(tl).clamp(0, Lmax)[:, None])
    assert int(torch.count_nonzero(got["label_logp"][~has])) == 0                    # behind L: exact zeros
    R.assert_within(got["label_logp"][has], ref["label_logp"][has], torch.ones(int(has.sum())), ref["label_units"][has], F32,
                    what="ctc align label_logp" + tag)
    return got, want


def poison_rows_behind_T(c, value=1e30):
    """large finite values in the rows t >= T: reading one would change a result"""
    c = dict(c)
    x = c["logits"].clone()
    for n, T in enumerate(torch.as_tensor(c["input_lengths"]).tolist()):
        x[n, max(T, 0):] = value
    c["logits"] = x
    return c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(ctc_ref.CASES))
def test_alignment_matches_the_references(name, dtype):
    """ctc_ref's case list: C in {2, 37, 130}, blank first and last, 4 randn and 30 randn, N = 6 with L = 0 | 1 | 5 at T = 9 < S | repeats |
    L = T | infeasible; S = 72; S = 264 with L = 130 (L' = 261 > 256 threads, more than 64 KiB of LDS)."""
    check(poison_rows_behind_T(ctc_ref.case(name)), dtype)


def special_case(C, blank):
    """S = 12, Lmax = 6: T exactly L + repeats | one frame fewer | T = 0 with L = 0 | T = 0 with L > 0 | a label >= C | a negative
    label | a label equal to blank | a label that -inf logits confine to frames 2, 3 | lengths beyond the matrices (clamped)."""
    gen = torch.Generator().manual_seed(7 + C + blank)
    a, b = [c for c in range(C) if c != blank][:2] if C > 2 else ([c for c in range(C) if c != blank] * 2)
    lines = [[a, a, b, b], [a, a, b, b], [], [a, b], [a, C + 4, b], [a, -5], [a, blank, b], [b, a], [a, b, a, b, a, b]]
    il = [6, 5, 0, 0, 12, 12, 12, 10, 1000]
    N, S, Lmax = len(lines), 12, 6
    x = 4 * torch.randn(N, S, C, generator=gen)
    x[7, :, b] = -math.inf
    x[7, 2:4, b] = 1.0
    targets = torch.full((N, Lmax), ctc_ref.SENTINEL, dtype=torch.int64)
    for n, l in enumerate(lines):
        targets[n, :len(l)] = torch.tensor(l, dtype=torch.int64)
    tl = [len(l) for l in lines]
    tl[8] = 1000
    infeasible = [1, 3, 4, 5] if a != b else [0, 1, 3, 4, 5, 7]          # C = 2: a = b, so a a a a needs 7 frames and a a cannot sit in two
    return {"logits": x, "targets": targets, "input_lengths": torch.tensor(il), "target_lengths": torch.tensor(tl), "blank": blank,
            "infeasible": infeasible}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,blank", [(2, 0), (2, 1), (37, 0), (37, 36)])
def test_edge_lines(C, blank, dtype):
    c = poison_rows_behind_T(special_case(C, blank))
    got, want = check(c, dtype)
    assert float(got["path_logit"][2]) == 0.0 and float(got["score"][2]) == 0.0               # T = 0, L = 0
    if C > 2:
        assert got["states"][0, :6].tolist() == [1, 2, 3, 5, 6, 7]                            # a a b b in six frames: one path
        assert got["spans"][7, 0].tolist()[0] >= 2 and got["spans"][7, 0].tolist()[1] <= 4   # confined by the -inf logits


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_frame(dtype):
    """S = 1: L = 0, L = 1 and L = 2 (infeasible)"""
    x = torch.tensor([[[0.5, -1.0]], [[0.25, 2.0]], [[1.0, 1.0]]])
    targets = torch.tensor([[ctc_ref.SENTINEL] * 2, [1, ctc_ref.SENTINEL], [1, 1]])
    c = {"logits": x, "targets": targets, "input_lengths": torch.tensor([1, 1, 1]), "target_lengths": torch.tensor([0, 1, 2]), "blank": 0,
         "infeasible": [2]}
    got, _ = check(c, dtype)
    assert got["states"].tolist() == [[0], [1], [-1]] and got["spans"][1].tolist() == [[0, 1], [-1, -1]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_logits_follow_the_tie_rule(dtype):
    """Integer-valued logits (exact in bf16 and in every partial sum): ties at every step, the all-zero line among them."""
    gen = torch.Generator().manual_seed(11)
    N, S, C, Lmax = 6, 12, 3, 5
    x = torch.randint(-8, 9, (N, S, C), generator=gen).float()
    x[0] = 0.0
    x[1] = torch.randint(-1, 2, (S, C), generator=gen).float()
    lines = [[1, 2, 2], [1, 1, 2, 1], [2], [], [1, 2, 1, 2, 1], [2, 2, 2, 2, 2]]
    targets = torch.full((N, Lmax), ctc_ref.SENTINEL, dtype=torch.int64)
    for n, l in enumerate(lines):
        targets[n, :len(l)] = torch.tensor(l, dtype=torch.int64)
    c = {"logits": x, "targets": targets, "input_lengths": torch.tensor([12, 12, 7, 5, 9, 9]), "target_lengths": torch.tensor([len(l) for l in lines]),
         "blank": 0, "infeasible": []}
    got, _ = check(poison_rows_behind_T(c), dtype)
    assert got["states"][0].tolist() == [1, 3, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6]          # all zero: as early as it can, then the last blank
    for n in range(N):          # and the enumeration of every path, where the line is small enough
        T, L = int(c["input_lengths"][n]), len(lines[n])
        if T <= 9 and L <= 3:
            value, path = A.brute_force(x[n].numpy(), targets[n].numpy(), T, L, 0)
            assert got["states"][n, :T].tolist() == path and float(got["path_logit"][n]) == value


@functools.lru_cache(maxsize=None)
def long_case():
    """N = 2, S = 512, Lmax = 160, C = 5: 512 * 321 bytes of backpointers exceed the LDS constant"""
    gen = torch.Generator().manual_seed(5)
    N, S, C, Lmax = 2, 512, 5, 160
    assert S * (2 * Lmax + 1) > LDS_BACK_BYTES
    targets = torch.randint(1, C, (N, Lmax), generator=gen)
    return {"logits": 4 * torch.randn(N, S, C, generator=gen), "targets": targets, "input_lengths": torch.tensor([512, 400]),
            "target_lengths": torch.tensor([160, 90]), "blank": 0, "infeasible": []}


@pytest.mark.parametrize("dtype", DTYPES)
def test_backpointers_in_the_global_workspace(dtype):
    check(poison_rows_behind_T(long_case()), dtype)
    # a shape that fits LDS, forced to the workspace: the same bits as from LDS
    c = poison_rows_behind_T(ctc_ref.case("mixed-C37-blank0-x4"))
    forced, _ = check(c, dtype, flags=GLOBAL_BACK)
    assert same_bits(forced, raw_align(c["logits"].to(dtype), c["targets"], c["input_lengths"], c["target_lengths"], 0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_lse_has_the_same_bits_in_loss_aligner_and_beam(dtype):
    """include/pero_hip.h defines score, label_logp and the beam's log-probabilities with pero_ctc_fwd's row_lse: the three entry points
    write the same int32 patterns on every row t < T (T = 0, 5 and S), and the two workspaces keep their poison behind T."""
    from pero_pretraining_amd import _lib
    from pero_pretraining_amd.ops import ctc_beam_workspace, ctc_fwd, dt, ptr, stream
    N, S, C, Lmax, W, blank = 3, 12, 37, 4, 4, 0
    gen = torch.Generator().manual_seed(13)
    lg = (4 * torch.randn(N * S, C, generator=gen)).to(dtype).cuda()
    il, tl = torch.tensor([0, 5, 12]).cuda(), torch.tensor([0, 2, 4]).cuda()
    tg = torch.randint(1, C, (N, Lmax), generator=gen).cuda()
    K, H = ctc_beam_workspace(S, C, W)

    def poisoned(kind, *shape):
        return torch.full((int(np.prod(shape)) * kind.itemsize,), 0x5a, dtype=torch.uint8, device="cuda").view(kind).view(shape)

    i32, i64 = torch.int32, torch.int64
    from_fwd = ctc_fwd(lg, tg, il, tl, blank)[1]
    from_align, from_beam = poisoned(F32, N * S), poisoned(F32, N * S)
    outs = [poisoned(i32, N, S), poisoned(i32, N, Lmax, 2), poisoned(F32, N), poisoned(F32, N), poisoned(F32, N, Lmax)]
    back = poisoned(torch.uint8, N * S * (2 * Lmax + 1))
    _lib.call("pero_ctc_align", ptr(lg), ptr(tg), ptr(il), ptr(tl), *[ptr(o) for o in outs], ptr(from_align), ptr(back), N, S, C, Lmax, blank, 0,
              dt(lg), stream())
    outs = [poisoned(i64, N, W, S), poisoned(i64, N, W), poisoned(F32, N, W), poisoned(i64, N), poisoned(i32, N, S * W + 1),
            poisoned(i32, N, S * W + 1), poisoned(i32, N), poisoned(i32, N, S, W), poisoned(F32, N, S, W, 2)]
    work = [poisoned(F32, N * S, K), poisoned(i32, N * S, K), poisoned(i64, N, H)]
    _lib.call("pero_ctc_beam", ptr(lg), ptr(il), *[ptr(o) for o in outs], ptr(from_beam), *[ptr(w) for w in work], N, S, C, blank, W, dt(lg),
              stream())
    written = (torch.arange(S)[None, :] < il.cpu()[:, None]).reshape(N * S)
    assert int(written.sum()) == 17
    fwd_bits, align_bits, beam_bits = (v.cpu().view(i32) for v in (from_fwd, from_align, from_beam))
    assert bool(torch.isfinite(from_fwd).all())                                       # pero_ctc_fwd: every row
    assert torch.equal(align_bits[written], fwd_bits[written]) and torch.equal(beam_bits[written], fwd_bits[written])
    assert bool((align_bits[~written] == 0x5a5a5a5a).all()) and bool((beam_bits[~written] == 0x5a5a5a5a).all())


def test_ops_wrapper_and_argument_checks(ops):
    from pero_pretraining_amd._lib import PeroHipError
    c = ctc_ref.case("mixed-C37-blank36-x4")
    N, S, C = c["logits"].shape
    lg, tg, il, tl = c["logits"].cuda().reshape(N * S, C).contiguous(), c["targets"].cuda(), c["input_lengths"].cuda(), c["target_lengths"].cuda()
    want = raw_align(c["logits"], c["targets"], c["input_lengths"], c["target_lengths"], 36)
    for kw in ({}, {"global_back": True}):
        states, spans, path_logit, score, label_logp = ops.ctc_align(lg, tg, il, tl, 36, **kw)
        assert states.dtype == torch.int32 and states.shape == (N, S) and spans.shape == (N, tg.shape[1], 2) and score.dtype == F32
        got = {"states": states.cpu(), "spans": spans.cpu(), "path_logit": path_logit.cpu(), "score": score.cpu(), "label_logp": label_logp.cpu()}
        assert same_bits(got, want)
    with pytest.raises(ValueError):
        ops.ctc_align(lg, tg, il, tl, C)                                  # blank outside [0, C)
    with pytest.raises(ValueError):
        ops.ctc_align(lg, tg.int(), il, tl, 0)                            # targets are int64
    with pytest.raises(ValueError):
        ops.ctc_align(lg, tg.t().contiguous().t(), il, tl, 0)             # contiguous
    with pytest.raises(ValueError):
        ops.ctc_align(lg, tg, il, tl[:-1].contiguous(), 0)                # one length per line
    with pytest.raises(ValueError):
        ops.ctc_align(lg.half(), tg, il, tl, 0)                           # f32 or bf16
    with pytest.raises(ValueError):
        ops.ctc_align(lg[:-1], tg, il, tl, 0)                             # N * S rows
    one = torch.ones(1, dtype=torch.int64).cuda()
    with pytest.raises(PeroHipError, match=r"\(-2\)"):                    # PERO_E_UNSUPPORTED
        ops.ctc_align(torch.zeros(513, 4).cuda(), one.view(1, 1), one, one, 0)


# ------------------------------------------------------------------------------------------------ the recognition package
@functools.lru_cache(maxsize=None)
def tiny():
    from pero_pretraining_amd.recognition import init_model
    torch.manual_seed(0)
    model = init_model(torch.device("cuda"), {"type": "vit", "num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128},
                       {"type": "linear", "in_features": 64, "out_features": 37}, blank=0).eval()
    images = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (2, 40, 192, 3), dtype=np.uint8)).cuda()
    il = torch.tensor([24, 17]).cuda()
    offsets = np.array([5, 9])
    with torch.no_grad():
        model.backbone.set_offsets(offsets)
        output = model.encode(images)
    return model, images, il, offsets, output


def test_recogniser_align_is_forced_align_of_its_logits():
    from pero_pretraining_amd.recognition import Alignment, forced_align
    model, images, il, offsets, output = tiny()
    targets = torch.tensor([[3, 7, 7, 1, 9, 0], [4, 4, 2, -1, -1, -1]]).cuda()
    tl = torch.tensor([5, 3]).cuda()
    model.backbone.set_offsets(offsets)
    got = model.align(images, targets, tl, il)
    want = forced_align(output, targets, tl, il, blank=0)
    assert isinstance(got, Alignment) and got.nll is None and got.path_share is None
    for a, b in zip(got[:6], want[:6]):
        assert a.is_cuda and torch.equal(a, b)
    # against the references, on the logits the kernel saw
    x = output.float().cpu() if output.dtype == torch.bfloat16 else output.cpu()
    ref = A.align_f32(x, targets.cpu(), il.cpu(), tl.cpu(), 0)
    assert np.array_equal(got.states.cpu().numpy(), ref["states"]) and np.array_equal(got.spans.cpu().numpy(), ref["spans"])
    frames = (got.spans[..., 1] - got.spans[..., 0]).cpu()
    assert frames[0, :5].min() >= 1 and got.confidences.shape == (2, 6) and float(got.confidences[0, 5]) == 0.0
    conf = torch.exp(got.label_logp.cpu().double() / frames.clamp_min(1))
    assert torch.allclose(got.confidences.cpu().double()[frames > 0], conf[frames > 0], rtol=1e-6)
    assert bool((got.confidences > 0).cpu()[frames > 0].all()) and bool((got.confidences <= 1).all())


def test_recogniser_transcribe_aligns_its_own_greedy_string():
    from pero_pretraining_amd.recognition import forced_align, greedy_decode
    model, images, il, offsets, output = tiny()
    model.backbone.set_offsets(offsets)
    labels, lengths, al = model.transcribe(images, il)
    want_labels, want_lengths = greedy_decode(output, il, 0)
    assert torch.equal(labels, want_labels) and torch.equal(lengths, want_lengths)
    x = output.float().cpu()
    ref = A.align_f64(x, labels.cpu(), il.cpu(), lengths.cpu(), 0, al.states.cpu().numpy(), np.ones(2, dtype=bool))
    for n in range(2):
        T, L = int(il[n]), int(lengths[n])
        st = al.states[n, :T].cpu().tolist()
        assert bool((al.states[n, T:] == -1).all())
        collapsed = [s for t, s in enumerate(st) if s & 1 and (t == 0 or st[t - 1] != s)]
        assert collapsed == [2 * k + 1 for k in range(L)]                                   # the non-blank states spell the decoded labels, in order
        assert [int(labels[n, s >> 1]) for s in collapsed] == labels[n, :L].tolist()
        # the greedy string's best path takes every row's maximum
        top = output[n, :T].float().max(-1).values
        R.assert_within(al.path_logit[n].cpu(), top.double().sum().cpu(), torch.ones(()), ref["path_units"][n], F32, what="ctc align path_logit")
        R.assert_within(top.sum().cpu(), top.double().sum().cpu(), top.double().abs().sum().cpu(), T, F32)          # the device sum, any order
    # with_nll: the best path's share of the string's probability
    al = forced_align(output, labels, lengths, il, blank=0, with_nll=True)
    res, mag = ctc_ref.ctc(x, labels.cpu(), il.cpu(), lengths.cpu(), 0)
    for n in range(2):
        nll_bound = float(R.bound(res["nll"][n], mag["nll"][n], int(mag["nll_terms"][n]), F32))
        arg = float(ref["score_units"][n]) * R.U32 + nll_bound + max(abs(float(al.score[n])), abs(float(al.nll[n]))) * R.U32
        bound = math.exp(arg) * (1 + (R.EXPF + 1) * R.U32) - 1
        assert 0.0 < float(al.path_share[n]) <= 1.0 + bound, (float(al.path_share[n]), bound)


def test_recogniser_transcribe_with_a_beam():
    model, images, il, offsets, output = tiny()
    model.backbone.set_offsets(offsets)
    labels, lengths, al = model.transcribe(images, il, beam_width=4)
    model.backbone.set_offsets(offsets)
    want = model.decode(images, il, beam_width=4)
    assert torch.equal(labels, want[0]) and torch.equal(lengths, want[1])
    ref = A.align_f32(output.float().cpu(), labels.cpu(), il.cpu(), lengths.cpu(), 0)
    assert ref["feasible"].all() and np.array_equal(al.states.cpu().numpy(), ref["states"]) and np.array_equal(al.spans.cpu().numpy(), ref["spans"])
