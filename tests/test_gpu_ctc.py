"""GPU: pero_ctc_fwd / pero_ctc_bwd / pero_ctc_greedy (csrc/ctc.hip) and the recognition package against tests/ctc_ref.py, the f64
restatement that test_ctc_ref_cpu.py pins to torch.nn.functional.ctc_loss in f64.  Every bound is the one ctc_ref's docstring derives
(no tolerance here is a measured number); integer outputs, zero rows and repeated calls are compared exactly.  bf16 logits are
rounded once on the host; the reference sees the rounded values."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import ctc_ref
import parity_ref as R
from parity_ref import assert_within

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    yield _ops
    print("\nPARITY_RATIOS " + json.dumps({k: round(v, 4) for k, v in sorted(R.RATIOS.items())}))


def line_scales(N):
    """distinct upstream scales per line, one of them 0"""
    g = torch.linspace(-1.0, 2.0, N).float()
    g[1] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """The case, its logits as the kernels see them (rounded to `dtype` once) and the f64 reference on those values; computed once, never modified."""
    c = ctc_ref.case(name)
    x = c["logits"].to(dtype)
    g = line_scales(x.shape[0])
    res, mag = ctc_ref.ctc(x.float(), c["targets"], c["input_lengths"], c["target_lengths"], c["blank"], g=g, zero_infinity=True)
    return c, x, g, res, mag


def device_args(c, x):
    N, S, C = x.shape
    return (x.cuda().reshape(N * S, C).contiguous(), c["targets"].cuda(), c["input_lengths"].cuda(), c["target_lengths"].cuda())


def check_nll(got, res, mag, c, dtype, what):
    got = got.cpu()
    for n in range(got.numel()):
        if n in c["infeasible"]:
            assert math.isinf(float(got[n])) and float(got[n]) > 0, (n, float(got[n]))
        else:
            assert_within(got[n], res["nll"][n], mag["nll"][n], int(mag["nll_terms"][n]), F32, what=what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(ctc_ref.CASES))
def test_ctc_kernels_match_the_f64_reference(ops, name, dtype):
    c, x, g, res, mag = reference(name, dtype)
    N, S, C = x.shape
    lg, tg, il, tl = device_args(c, x)
    nll, row_lse, alpha = ops.ctc_fwd(lg, tg, il, tl, c["blank"])
    check_nll(nll, res, mag, c, dtype, "ctc nll")
    valid = torch.arange(S)[None, :] < c["input_lengths"][:, None]
    # row_lse: an absolute error of row_units units (ctc_ref's docstring), so the magnitude is 1
    assert_within(row_lse.cpu().view(N, S)[valid], res["row_lse"][valid], torch.ones(int(valid.sum())), mag["row_units"], F32, what="ctc row_lse")
    gd = g.cuda()
    dl = ops.ctc_bwd(lg, tg, il, tl, row_lse, alpha, nll, gd, c["blank"], zero_infinity=True)
    assert dl.dtype == dtype and dl.shape == lg.shape
    dlc = dl.cpu().view(N, S, C)
    for n in range(N):
        assert_within(dlc[n], res["grad"][n], mag["grad"][n], mag["grad_terms"], dtype, extra_ulps=mag["grad_units"][n], what="ctc dlogits")
        assert int(torch.count_nonzero(dlc[n, int(c["input_lengths"][n]):])) == 0          # rows behind the line's frames: exact zeros
    for n in c["infeasible"]:
        assert int(torch.count_nonzero(dlc[n])) == 0                                       # zero_infinity: exact zeros
    # two calls, the same bits
    again = ops.ctc_bwd(lg, tg, il, tl, row_lse, alpha, nll, gd, c["blank"], zero_infinity=True)
    assert torch.equal(again.view(torch.int32 if dtype == F32 else torch.int16), dl.view(torch.int32 if dtype == F32 else torch.int16))
    # without zero_infinity the infeasible line's rows are unspecified; every other line keeps its bits
    if c["infeasible"]:
        feasible = [n for n in range(N) if n not in c["infeasible"]]
        plain = ops.ctc_bwd(lg, tg, il, tl, row_lse, alpha, nll, gd, c["blank"], zero_infinity=False).cpu().view(N, S, C)
        assert torch.equal(plain[feasible], dlc[feasible])


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_path_line(ops, dtype):
    """L = T = 24 distinct labels: one path, nll = -sum of its log-probabilities (formed here in f64, independently of the recursion)."""
    c, x, g, res, mag = reference("mixed-C37-blank0-x4", dtype)
    nll = ops.ctc_fwd(*device_args(c, x), c["blank"])[0].cpu()
    lp = torch.log_softmax(x[4].double(), -1)
    want = -lp[torch.arange(24), c["targets"][4, :24]].sum()
    assert_within(nll[4], want, mag["nll"][4], int(mag["nll_terms"][4]), F32, what="ctc nll")


@pytest.mark.parametrize("dtype", DTYPES)
def test_greedy_decode_is_exact(ops, dtype):
    x, il, _ = ctc_ref.greedy_case()
    x = x.to(dtype)
    N, S, C = x.shape
    for blank in (0, C - 1):
        want, want_len = ctc_ref.greedy(x.float(), il, blank)
        out, lengths = ops.ctc_greedy(x.cuda().reshape(N * S, C).contiguous(), il.cuda(), blank)
        assert out.dtype == torch.int64 and lengths.dtype == torch.int64
        assert torch.equal(lengths.cpu(), want_len) and torch.equal(out.cpu(), want)
    assert int(want_len[3]) == 0 and bool((want[3] == -1).all())          # input_length 0
    # more classes than a wave has lanes, ragged lengths
    c, xl, _, _, _ = reference("mixed-C130-blank129-x4", dtype)
    want, want_len = ctc_ref.greedy(xl.float(), c["input_lengths"], c["blank"])
    out, lengths = ops.ctc_greedy(device_args(c, xl)[0], c["input_lengths"].cuda(), c["blank"])
    assert torch.equal(lengths.cpu(), want_len) and torch.equal(out.cpu(), want)


# ------------------------------------------------------------------------------------------------ module level
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_ctc_loss_module_and_backward_through_a_linear_head(reduction, dtype):
    """CTCLoss on the logits of a LinearHead against the f64 reference evaluated on those logits; .backward() reaches the head's weight:
    dW = dlogits^T tokens, compared in f32 mode against the f64 product of the reference gradient (N S terms more per entry)."""
    from pero_pretraining_amd.masked_pretraining.model import LinearHead
    from pero_pretraining_amd.precision import autocast
    from pero_pretraining_amd.recognition import CTCLoss
    c = ctc_ref.case("mixed-C37-blank36-x4")
    N, S, C = c["logits"].shape
    torch.manual_seed(3)
    head = LinearHead(64, C).cuda()
    with torch.no_grad():
        head.linear.weight.mul_(8.0)
    tokens = torch.randn(N, S, 64, generator=torch.Generator().manual_seed(4)).cuda()
    loss_fn = CTCLoss(blank=c["blank"], reduction=reduction, zero_infinity=True)
    with autocast(dtype == torch.bfloat16):
        output = head(tokens)
        loss = loss_fn(output, c["targets"].cuda(), c["input_lengths"].cuda(), c["target_lengths"].cuda())
    assert output.dtype == dtype and output.shape == (N, S, C) and loss.dtype == F32
    # upstream scale of each line under this reduction, with a distinct weight per line for "none"
    w = line_scales(N).double()
    (loss * w.float().cuda()).sum().backward() if reduction == "none" else loss.backward()
    tl = c["target_lengths"].double().clamp_min(1)
    g = {"none": w, "sum": torch.ones(N, dtype=torch.float64), "mean": 1.0 / (tl * N)}[reduction]
    res, mag = ctc_ref.ctc(output.detach().float(), c["targets"], c["input_lengths"], c["target_lengths"], c["blank"], g=g, zero_infinity=True)
    want, want_mag = ctc_ref.reduce(res["nll"], c["target_lengths"], reduction, True, mag_nll=mag["nll"])
    assert_within(loss.detach(), want, want_mag, int(mag["nll_terms"].max()) + N, F32, what=f"CTCLoss {reduction}")
    assert head.linear.weight.grad is not None and bool(torch.isfinite(head.linear.weight.grad).all())
    if dtype == F32:
        t64 = tokens.cpu().double().reshape(N * S, 64)
        dw = res["grad"].reshape(N * S, C).t() @ t64
        dw_mag = mag["grad"].reshape(N * S, C).t() @ t64.abs()
        assert_within(head.linear.weight.grad, dw, dw_mag, N * S + mag["grad_terms"], F32, extra_ulps=max(mag["grad_units"]), what="CTCLoss head dW")


def _recogniser(C=37):
    from pero_pretraining_amd.recognition import init_model
    torch.manual_seed(0)
    return init_model(torch.device("cuda"), {"type": "vit", "num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128},
                      {"type": "linear", "in_features": 64, "out_features": C}, blank=0)


def _batch(N=4, W=192, C=37, seed=0):
    rng = np.random.default_rng(seed)
    widths = np.array([W, W - 8, W - 61, W])[:N]
    lengths = np.array([7, 5, 3, 0])[:N]
    targets = np.zeros((N, 8), np.int64)
    for n in range(N):
        targets[n, :lengths[n]] = rng.integers(1, C, lengths[n])
    return {"images": rng.integers(0, 256, (N, 40, W, 3), dtype=np.uint8), "targets": targets, "target_lengths": lengths, "widths": widths}


@pytest.mark.parametrize("bfloat16", [False, True])
def test_recogniser_takes_three_train_steps(bfloat16):
    from pero_pretraining_amd.common.lr_scheduler import WarmupSchleduler
    from pero_pretraining_amd.optim import FusedAdam
    from pero_pretraining_amd.recognition import BatchOperator, Trainer
    model = _recogniser().train()
    optimizer = FusedAdam(model.parameters(), lr=1e-3)
    trainer = Trainer(BatchOperator(torch.device("cuda")), model, None, optimizer, WarmupSchleduler(optimizer, 1e-3, 1, 1), bfloat16=bfloat16)
    outputs = []
    hook = model.register_forward_hook(lambda mod, args, result: outputs.append(result["output"].detach().float().cpu()))
    batch = _batch()
    losses = [float(trainer.train_step(batch)) for _ in range(3)]
    hook.remove()
    assert all(math.isfinite(v) for v in losses) and losses[2] < losses[0], losses
    assert outputs[0].shape == (4, 24, 37)
    input_lengths = torch.tensor([24, 23, 17, 24])            # ceil(width / 8)
    res, mag = ctc_ref.ctc(outputs[0], batch["targets"], input_lengths, batch["target_lengths"], 0)
    want, want_mag = ctc_ref.reduce(res["nll"], batch["target_lengths"], "mean", mag_nll=mag["nll"])
    assert_within(torch.tensor(losses[0]), want, want_mag, int(mag["nll_terms"].max()) + 4, F32, what="recogniser step-1 loss")


def test_recogniser_attends_to_valid_positions_only_when_asked():
    """attend_valid_only: the key ranges [0, input_length) reach the encoder layers - the valid outputs of a line no longer depend on the pixels behind its width."""
    model = _recogniser().eval()
    model.attend_valid_only = True
    batch = _batch(N=2)
    images = torch.from_numpy(batch["images"]).cuda()
    other = images.clone()
    other[1, :, 184:] = 255 - other[1, :, 184:]                # line 1 is 184 px wide: 23 positions
    il = torch.tensor([24, 23]).cuda()
    offsets = np.array([5, 9])
    with torch.no_grad():
        model.backbone.set_offsets(offsets)
        a = model(images, input_lengths=il)["output"]
        model.backbone.set_offsets(offsets)
        b = model(other, input_lengths=il)["output"]
        assert torch.equal(a[1, :23], b[1, :23]) and not torch.equal(a[1, 23], b[1, 23])
        model.attend_valid_only = False
        model.backbone.set_offsets(offsets)
        a = model(images, input_lengths=il)["output"]
        model.backbone.set_offsets(offsets)
        b = model(other, input_lengths=il)["output"]
        assert not torch.equal(a[1, :23], b[1, :23])


class _Planted(torch.nn.Module):
    """A recogniser whose logits are planted: Tester and pero_ctc_greedy see a known string per line."""

    def __init__(self, logits, loss):
        super().__init__()
        self.logits, self.loss = logits, loss

    def forward(self, images, targets=None, target_lengths=None, input_lengths=None):
        n = images.shape[0]
        out = self.logits[:n]
        return {"output": out, "loss": self.loss(out, targets, input_lengths, target_lengths)}


def test_tester_reports_loss_and_character_error_rate():
    from pero_pretraining_amd.recognition import BatchOperator, CTCLoss, Tester
    # (a) a real recogniser whose head is rigged: zero weight, a bias that makes every position emit class 11 -> the line decodes to [11]
    model = _recogniser()
    with torch.no_grad():
        model.head.linear.weight.zero_()
        model.head.linear.bias.zero_()
        model.head.linear.bias[11] = 10.0
    batch = _batch(N=2)
    batch["targets"] = np.array([[11], [11]])
    batch["target_lengths"] = np.array([1, 1])
    tester = Tester(BatchOperator(torch.device("cuda")), model, [batch, batch])
    result = tester.test()
    assert result["cer"] == 0 and math.isfinite(result["loss"]) and model.training
    batch["targets"] = np.array([[11], [12]])
    assert tester.test()["cer"] == 0.5                                   # one of two characters substituted
    # (b) a known string of L = 5 per line, written into the logits: 3 3 - 7 7 7 - 7 1 - 9 4 4 (blank 0) -> 3 7 7 1 9 4 is cut to its first 11 frames (88 px): 3 7 7 1 9
    frames = [3, 3, 0, 7, 7, 7, 0, 7, 1, 0, 9, 4, 4, 0, 0, 0]
    logits = torch.zeros(2, 16, 12)
    logits[:, torch.arange(16), torch.tensor(frames)] = 8.0
    planted = _Planted(logits.cuda(), CTCLoss(blank=0))
    truth = np.array([[3, 7, 7, 1, 9], [3, 7, 7, 1, 9]])
    batch = {"images": np.zeros((2, 40, 128, 3), np.uint8), "targets": truth, "target_lengths": np.array([5, 5]), "widths": np.array([88, 88])}
    tester = Tester(BatchOperator(torch.device("cuda")), planted, [batch])
    result = tester.test()
    assert result["cer"] == 0 and math.isfinite(result["loss"])
    batch["targets"] = np.array([[3, 7, 5, 1, 9], [3, 7, 7, 1, 2]])      # one substituted character per line
    assert tester.test()["cer"] == 1 / 5
