"""Kernel-level tests of csrc/latent.hip: every entry point called through its ops wrapper at the smallest shapes that reach each of its
paths, in the bounds style of tests/test_gpu_kernel_parity.py - the f64 restatement of tests/latent_ref.py and `assert_within`, the bound
derived from the kernel's own chain of roundings in the comment next to each call; no tolerance here is a measured number.  The EMA is a
chain of three correctly rounded f32 operations per element and is compared bit for bit with the same chain in numpy float32.  Rows and
elements a call must not touch, and pad rows, are compared bit for bit.  bf16 inputs are rounded once on the host; the reference sees the
rounded values.  Each test prints the measured error beside its bound (as error / bound)."""
import numpy as np
import pytest
import torch

import latent_ref as LR
from parity_ref import DIVF, SQRTF, assert_within

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
WIDTHS = [64, 72, 520]     # one chunk of 256 columns partly filled, not a multiple of 8, three chunks with the last partly filled


def gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


def f32r(v):
    return float(np.float32(v))


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------ pero_ema_update
EMA_SIZES = [1, 7, 8, 4095, 4096, 4097, 3 * 4096 + 5]   # the sizes of tests/test_gpu_layerwise_optim.py: below / at / above a tile, several tiles


def _ema_case():
    g = gen(1, 2, 3)
    srcs, offs, total = [], [], 0
    for i, n in enumerate(EMA_SIZES):
        if i == 3:   # this source starts 4 bytes into its allocation: not 16-byte aligned, the scalar branch
            base = torch.empty(n + 1, device="cuda", dtype=F32)
            t = base[1:]
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.empty(n, device="cuda", dtype=F32)
        t.copy_(torch.randn(n, generator=g))
        srcs.append(t)
        offs.append(total)
        total += ((n + 7) // 8) * 8
    avg0 = torch.zeros(total)
    for o, n in zip(offs, EMA_SIZES):
        avg0[o:o + n] = torch.randn(n, generator=g)
    return srcs, offs, total, avg0


def test_ema_update_is_bit_equal_to_the_f32_formula(ops):
    srcs, offs, total, avg0 = _ema_case()
    table, tiles = ops.ema_table([(s, o, s.numel()) for s, o in zip(srcs, offs)], torch.device("cuda"))
    assert tiles == sum((n + 4095) // 4096 for n in EMA_SIZES) and table.shape == (len(EMA_SIZES), 4)
    avg, lp = avg0.cuda(), torch.zeros(total, device="cuda", dtype=BF16)
    plain = avg0.cuda()                     # the same updates without the bf16 destination
    ref = avg0.numpy().copy()
    for step, tau in enumerate((0.9, 0.999)):   # two successive updates with different tau; the sources move in between
        w = f32r(1.0 - tau)
        ops.ema_update(avg, table, tiles, w, lp)
        ops.ema_update(plain, table, tiles, w)
        for s, o in zip(srcs, offs):
            ref[o:o + s.numel()] = LR.ema_update_f32(ref[o:o + s.numel()], s.cpu().numpy(), w)
        got = avg.cpu()
        # a + w * (p - a): three f32 operations, each correctly rounded, none contracted (-ffp-contract=off): the bits of numpy float32
        assert torch.equal(got, torch.from_numpy(ref)), (step, float((got - torch.from_numpy(ref)).abs().max()))
        assert torch.equal(lp.cpu(), torch.from_numpy(ref).to(BF16))      # round-to-nearest-even of the new average, same launch
        assert torch.equal(plain.cpu(), got)
        for s in srcs:
            s.mul_(0.5).add_(0.25)
    pad = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offs, EMA_SIZES):
        pad[o:o + n] = False
    assert int(pad.sum()) > 0 and not avg.cpu()[pad].any() and not lp.cpu()[pad].any()   # the padding between the segments stays 0
    print(f"\npero_ema_update: max |got - numpy f32| = 0 over {total} elements, {tiles} tiles (bound: bit equality)")


@pytest.mark.parametrize("sizes", [[4097], [4097, 7], [4097, 7, 4096]], ids=lambda s: f"{len(s)}seg")
def test_ema_update_finds_the_segment_in_tables_of_one_two_and_three(ops, sizes):
    """Tables of 1, 2 and 3 segments (first tiles 0 / 0, 2 / 0, 2, 3) are where a wrong midpoint of the segment search first shows:
    every segment against the f32 formula, bit for bit, and zero pads."""
    g = gen(4, len(sizes))
    offs = [sum(((m + 7) // 8) * 8 for m in sizes[:i]) for i in range(len(sizes))]
    total = offs[-1] + ((sizes[-1] + 7) // 8) * 8
    srcs = [torch.randn(n, generator=g).cuda() for n in sizes]
    avg0 = torch.zeros(total)
    for o, n in zip(offs, sizes):
        avg0[o:o + n] = torch.randn(n, generator=g)
    table, tiles = ops.ema_table([(s, o, s.numel()) for s, o in zip(srcs, offs)], torch.device("cuda"))
    assert tiles == sum((n + 4095) // 4096 for n in sizes)
    avg, lp = avg0.cuda(), torch.zeros(total, device="cuda", dtype=BF16)
    w = f32r(1.0 - 0.99)
    ops.ema_update(avg, table, tiles, w, lp)
    ref = avg0.numpy().copy()
    for s, o in zip(srcs, offs):
        ref[o:o + s.numel()] = LR.ema_update_f32(ref[o:o + s.numel()], s.cpu().numpy(), w)   # the pads of avg0 are zeros and stay untouched
    assert torch.equal(avg.cpu(), torch.from_numpy(ref))
    assert torch.equal(lp.cpu(), torch.from_numpy(ref).to(BF16))


# ------------------------------------------------------------------------------------------------ pero_latent_targets
def _targets_case(d, K, n, dtype):
    g = gen(d, K, n, dtype == F32)
    mats = [(torch.randn(53, d, generator=g) * (0.5 + k) + 0.4 * k).to(dtype) for k in range(K)]
    index = torch.randperm(53, generator=g)[:n]      # unique, unsorted
    return mats, index


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("n", [1, 29])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("d", WIDTHS)
def test_latent_targets(ops, d, K, n, dtype):
    mats, index = _targets_case(d, K, n, dtype)
    n_pad = n + 3
    y = ops.latent_targets([m.cuda() for m in mats], index.cuda(), n_pad, 1e-5)
    ref, mag = LR.latent_targets(mats, index, n_pad, f32r(1e-5))
    # per matrix: mu is an f32 sum of d terms (error <= d u mean|x|, carried into every deviation: the mean|x| rs part of mag); the variance
    # is a sum of d squares, and rs = 1 / sqrt(var / d + eps) takes half its relative error: together <= d u on |x - mu| rs.  Then K terms
    # are added.  n_terms = d + K; extra: the divisions by d (2 DIVF), the sqrt, the reciprocal (DIVF), the rounded 1 / K (1); the
    # deviation, its square, the product with rs and the product with 1 / K are the 4 of assert_within.
    worst = assert_within(y, ref, mag, d + K, F32, extra_ulps=3 * DIVF + SQRTF + 1, what="pero_latent_targets")
    assert torch.equal(y[n:].cpu(), torch.zeros(3, d))                                  # pad rows: exact zeros
    # rows outside the index do not influence the result: overwritten with NaN, the same bits come out
    poisoned = []
    for m in mats:
        p = torch.full_like(m, float("nan"))
        p[index] = m[index]
        poisoned.append(p.cuda())
    assert torch.equal(ops.latent_targets(poisoned, index.cuda(), n_pad, 1e-5), y)
    print(f"\npero_latent_targets d={d} K={K} n={n} {dtype}: error / bound = {worst:.4f} (bound ({d + K} + 4 + 5) 2^-24 mag)")


def test_latent_targets_refuses_unsupported_widths(ops):
    """No scalar path: a width that is no multiple of 4, or wider than the header allows, is the library's error, not garbage."""
    from pero_pretraining_amd._lib import PeroHipError
    idx = torch.zeros(1, device="cuda", dtype=torch.int64)
    for d in (19, ops.LATENT_MAX_D + 4):
        with pytest.raises(PeroHipError, match=r"\(-1\).*multiple of 4"):
            ops.latent_targets([torch.zeros(2, d, device="cuda")], idx, 1)
    with pytest.raises(PeroHipError, match=r"\(-1\)"):
        ops.latent_targets([torch.zeros(2, 64, device="cuda")] * (ops.LATENT_MAX_K + 1), idx, 1)
    wide = ops.latent_targets([torch.randn(3, ops.LATENT_MAX_D, device="cuda")], torch.tensor([2], device="cuda"), 1)   # the widest supported row
    assert abs(float(wide.mean())) < 1e-5 and abs(float(wide.var(unbiased=False)) - 1.0) < 1e-3


# ------------------------------------------------------------------------------------------------ pero_latent_loss_fwd / _bwd
def _loss_case(d, n, beta, dtype):
    g = gen(d, n, int(beta * 10), dtype == F32)
    n_pad = n + 3
    y = torch.randn(n_pad, d, generator=g)
    pred = (y + torch.randn(n_pad, d, generator=g) * 1.5).to(dtype)
    # an element within 1e-3 beta of the branch point of l' goes to |e| = 2 beta, where the rounding of a bf16 prediction (2^-8 |p|, more than
    # the margin) cannot bring it back; the count of offenders left is asserted to be 0
    bad = LR.branch_offenders(pred.float(), y, beta)
    away = (y + torch.sign(pred.float() - y) * 2 * beta).to(dtype)
    pred = torch.where(bad, away, pred)
    assert int(LR.branch_offenders(pred.float(), y, beta).sum()) == 0
    return pred, y, n_pad


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("beta", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("n", [1, 29])
@pytest.mark.parametrize("d", WIDTHS)
def test_latent_loss_fwd_bwd(ops, d, n, beta, dtype):
    pred, y, n_pad = _loss_case(d, n, beta, dtype)
    p, t = pred.cuda(), y.cuda()
    loss = ops.latent_loss_fwd(p, t, n, beta)
    ref, mag = LR.latent_loss(pred.float(), y, n, beta)
    # a row sum of d terms in f32; the sum of the n row sums is in f64 (no f32 rounding) and is rounded to f32 once (1) after one division
    # (DIVF); the difference, the two products and the division by beta of a term are the 4 of assert_within
    worst = assert_within(loss, ref.reshape(1), mag.reshape(1), d, F32, extra_ulps=DIVF + 1, what="pero_latent_loss_fwd")
    assert torch.equal(ops.latent_loss_fwd(p, t, n, beta), loss)                         # the same bits on a second run
    dloss = torch.full((1,), 0.375, device="cuda")                                       # a dloss that is not 1
    dp = ops.latent_loss_bwd(p, t, n, beta, dloss)
    gref = LR.latent_loss_grad(pred.float(), y, n, beta, 0.375)
    # one term: e (1), e / beta or 2 e (1, DIVF), g = dloss * coef with coef rounded (2), g * l' (1): 5 roundings = the 1 + 4; written in pred's dtype
    wb = assert_within(dp, gref, gref.abs(), 1, dtype, extra_ulps=DIVF, what="pero_latent_loss_bwd")
    assert dp.dtype == dtype and torch.equal(dp[n:].cpu().float(), torch.zeros(3, d))    # pad rows: exact zeros
    assert torch.equal(ops.latent_loss_bwd(p, t, n, beta, dloss), dp)
    one = ops.latent_loss_bwd(p, t, n, beta)                                             # dloss = null means 1
    assert_within(one, LR.latent_loss_grad(pred.float(), y, n, beta, 1.0), gref.abs() / 0.375, 1, dtype, extra_ulps=DIVF, what="pero_latent_loss_bwd")
    print(f"\npero_latent_loss d={d} n={n} beta={beta} {dtype}: fwd error / bound = {worst:.4f} (({d} + 4 + 2) 2^-24 loss), "
          f"bwd error / bound = {wb:.4f} ((1 + 4 + 1) 2^-24 |g|{' + 2^-8 |g|' if dtype == BF16 else ''})")


def test_latent_loss_refuses_unsupported_widths_and_empty_selection_is_nan(ops):
    from pero_pretraining_amd._lib import PeroHipError
    z = torch.zeros(4, 19, device="cuda")
    with pytest.raises(PeroHipError, match=r"\(-1\).*multiple of 4"):
        ops.latent_loss_fwd(z, z, 4, 1.0)
    with pytest.raises(PeroHipError, match=r"\(-1\).*multiple of 4"):
        ops.latent_loss_bwd(z, z, 4, 1.0)
    z = torch.zeros(4, 64, device="cuda")
    assert torch.isnan(ops.latent_loss_fwd(z, z, 0, 1.0)).all()          # the mean over nothing
    assert torch.equal(ops.latent_loss_bwd(z + 1, z, 0, 1.0), z)
