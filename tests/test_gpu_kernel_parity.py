"""Kernel-level parity of csrc/losses.hip, csrc/bnorm.hip and the small utilities of csrc/misc.hip / csrc/rowops.hip: every entry point
called directly, at the smallest shapes that reach each of its branches, and held to the f64 restatement of tests/parity_ref.py through
`assert_within` (the bound is derived per call in the comment next to it; no tolerance here is a measured number).  Outputs the header
describes as accumulated are pre-filled; rows / bytes a call must not touch are compared bit for bit; integer, copy and cast outputs with
torch.equal.  bf16 inputs are rounded once on the host; the reference sees the rounded values."""
import json

import numpy as np
import pytest
import torch

import parity_ref as R
from parity_ref import DIVF, EXPF, LOGF, SQRTF, assert_within

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    yield _ops
    print("\nPARITY_RATIOS " + json.dumps({k: round(v, 4) for k, v in sorted(R.RATIOS.items())}))


def call(name, *args):
    from pero_pretraining_amd._lib import call as _call
    return _call(name, *args)


def gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


def f32r(v):
    """A float as the C ABI receives it (c_float): the reference computes with the rounded value."""
    return float(np.float32(v))


def shifted(t, elems=4):
    """A device copy of `t` that starts `elems` elements into its allocation (4 bf16 = 8 bytes: rows are no longer 16-byte aligned)."""
    base = torch.empty(t.numel() + 2 * elems, device="cuda", dtype=t.dtype)
    v = base[elems:elems + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == elems * t.element_size() % 16
    return v


def scalar(v):
    return None if v is None else torch.full((1,), v, device="cuda", dtype=F32)


# ------------------------------------------------------------------------------------------------ VICReg invariance
def _sqdiff_inputs(d, n, dtype):
    g = gen(d, n, dtype == F32)
    x = torch.randn(53, d, generator=g).to(dtype)
    y = (torch.randn(47, d, generator=g) * 0.8 + 0.2).to(dtype)
    ix, iy = torch.randperm(53, generator=g)[:n], torch.randperm(47, generator=g)[:n]   # unique, unsorted
    dx0, dy0 = torch.randn(53, d, generator=g).to(dtype), torch.randn(47, d, generator=g).to(dtype)
    return x, y, ix, iy, dx0, dy0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,n", [(72, 29), (520, 29), (19, 29), (72, 1)])   # vector branch, second trip of its loop, scalar branch, one row
def test_sqdiff_rows_fwd_bwd(ops, dtype, d, n):
    x, y, ix, iy, dx0, dy0 = _sqdiff_inputs(d, n, dtype)
    scale = f32r(1.0 / (n * d))
    out = ops.sqdiff_rows(x.cuda(), ix.cuda(), y.cuda(), iy.cuda(), scale)
    ref, mag = R.sqdiff(x, ix, y, iy, scale)
    # header: partial[n] row sums (d terms each), then the sum of the n partials; the difference, its square and the final scale are in the 4
    assert_within(out, ref, mag, d + n, F32, what="pero_sqdiff_rows")
    for gval in (None, 0.5):
        dx, dy = dx0.cuda(), dy0.cuda()
        ops.sqdiff_rows_bwd(x.cuda(), ix.cuda(), y.cuda(), iy.cuda(), dx, dy, scalar(gval), 0.375)
        (rdx, rdy), (mx, my) = R.sqdiff_bwd(x, ix, y, iy, dx0, dy0, gval, 0.375)
        # three terms per element: the old value, c x, c y (c = coef g: one more rounding, in the 4)
        assert_within(dx, rdx, mx, 3, dtype, what="pero_sqdiff_rows_bwd")
        assert_within(dy, rdy, my, 3, dtype, what="pero_sqdiff_rows_bwd")
        keep_x, keep_y = torch.ones(53, dtype=torch.bool), torch.ones(47, dtype=torch.bool)
        keep_x[ix], keep_y[iy] = False, False
        assert torch.equal(dx.cpu()[keep_x], dx0[keep_x]) and torch.equal(dy.cpu()[keep_y], dy0[keep_y])   # rows not listed: untouched
        assert not torch.equal(dx.cpu()[ix], dx0[ix])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,n", [(72, 29), (520, 29), (19, 29), (72, 1)])
def test_scatter_add_rows_scaled(ops, dtype, d, n):
    g = gen(d, n, 3)
    src = torch.randn(n, d, generator=g).to(dtype)
    dst0 = torch.randn(53, d, generator=g).to(dtype)
    index = torch.randperm(53, generator=g)[:n]
    for gval in (None, 0.5):
        dst = dst0.cuda()
        ops.scatter_add_rows_scaled(src.cuda(), index.cuda(), dst, scalar(gval))
        ref, mag = R.scatter_add_scaled(src, index, dst0, gval)
        assert_within(dst, ref, mag, 2, dtype, what="pero_scatter_add_rows_scaled")   # old value + g src
        keep = torch.ones(53, dtype=torch.bool)
        keep[index] = False
        assert torch.equal(dst.cpu()[keep], dst0[keep])


def test_losses_rows_not_16_byte_aligned_take_the_scalar_branch_with_the_same_bits(ops):
    """bf16, d = 72, every operand a view that starts 8 bytes into its allocation: the 16-byte branch must step aside.  The elementwise
    results (sqdiff backward, scaled scatter) are the aligned run's bit for bit; the forward sum is added in another order and is held to
    the reference's bound instead."""
    d, n, dtype = 72, 29, torch.bfloat16
    x, y, ix, iy, dx0, dy0 = _sqdiff_inputs(d, n, dtype)
    scale = f32r(1.0 / (n * d))
    out = ops.sqdiff_rows(shifted(x), ix.cuda(), shifted(y), iy.cuda(), scale)
    ref, mag = R.sqdiff(x, ix, y, iy, scale)
    assert_within(out, ref, mag, d + n, F32, what="pero_sqdiff_rows")
    dx_a, dy_a, dx_s, dy_s = dx0.cuda(), dy0.cuda(), shifted(dx0), shifted(dy0)
    ops.sqdiff_rows_bwd(x.cuda(), ix.cuda(), y.cuda(), iy.cuda(), dx_a, dy_a, scalar(0.5), 0.375)
    ops.sqdiff_rows_bwd(shifted(x), ix.cuda(), shifted(y), iy.cuda(), dx_s, dy_s, scalar(0.5), 0.375)
    assert torch.equal(dx_a, dx_s) and torch.equal(dy_a, dy_s)
    src = x[:n].contiguous()
    sc_a, sc_s = dx0.cuda(), shifted(dx0)
    ops.scatter_add_rows_scaled(src.cuda(), ix.cuda(), sc_a, scalar(0.5))
    ops.scatter_add_rows_scaled(shifted(src), ix.cuda(), sc_s, scalar(0.5))
    assert torch.equal(sc_a, sc_s) and not torch.equal(sc_a.cpu(), dx0)


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_sum_scale(ops, n):
    p = torch.randn(n, generator=gen(n))
    scale = f32r(0.3)
    ref, mag = R.sum_scale(p, scale)
    assert_within(ops.sum_scale(p.cuda(), scale), ref, mag, n, F32, what="pero_sum_scale")


# ------------------------------------------------------------------------------------------------ VICReg variance / covariance
VIC_SHAPES = [(130, 192, 72), (515, 576, 264), (2, 64, 8)]   # one block; two column blocks x five row slabs; the smallest m


def _vic_rows(m, m_pad, d, dtype):
    g = gen(m, m_pad, d)
    z = torch.full((m_pad, d), 7.0)     # padding rows: the call must not read them into its output
    z[:m] = torch.randn(m, d, generator=g) * torch.linspace(0.25, 1.75, d) + 0.3
    return z.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,m_pad,d", VIC_SHAPES)
def test_center_cols(ops, dtype, m, m_pad, d):
    z = _vic_rows(m, m_pad, d, dtype)
    cs = z[:m].double().sum(0).float()
    sumsq0 = torch.rand(d, generator=gen(d, 5)) * 50 + 1
    zc = torch.full((m_pad, d), 3.0, device="cuda", dtype=dtype)
    sumsq, zd, csd = sumsq0.cuda(), z.cuda(), cs.cuda()
    call("pero_center_cols", ops.ptr(zd), ops.ptr(csd), ops.ptr(zc), ops.ptr(sumsq), m, m_pad, d, ops.dt(dtype), ops.stream())
    (rzc, rsq), (mzc, msq) = R.center_cols(z, cs, m, sumsq0)
    assert_within(zc, rzc, mzc, 2, dtype, what="pero_center_cols zc")         # z - colsum / m (the division is in the 4)
    assert float(zc[m:].float().abs().max()) == 0.0                            # padding rows: exact zeros
    # old value + m squares; extra 6: the rounding of the difference inside each square (parity_ref.center_cols)
    assert_within(sumsq, rsq, msq, m + 1, F32, extra_ulps=6, what="pero_center_cols sumsq")
    assert float((sumsq.cpu() - sumsq0).min()) > 0                             # added to, not overwritten


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,m_pad,d", VIC_SHAPES)
def test_vicreg_var(ops, dtype, m, m_pad, d):
    z = _vic_rows(m, m_pad, d, dtype)
    (_, rsq), _ = R.center_cols(z, z[:m].double().sum(0).float(), m, torch.zeros(d))
    sumsq, thr, eps = rsq.float(), 1.0, f32r(1e-5)
    std = R.vicreg_std(sumsq, m, eps)
    # the f32 error of std is at most (m + 8) * 2^-24 (3e-5 at m = 515): no column may sit that close to the hinge
    assert float((thr - std).abs().min()) > 1e-4
    cvar, loss = ops.vicreg_var(sumsq.cuda(), m, thr, eps)
    (rcvar, rloss), (mcvar, mloss) = R.vicreg_var(sumsq, m, thr, eps)
    assert 0 < int((rcvar == 0).sum()) < d                                     # columns on both sides of the hinge
    assert torch.equal(cvar.cpu() == 0, rcvar == 0)                            # exactly 0 on the inactive side
    # loss: d terms; std = sqrt(sumsq / (m - 1) + eps): a division, an addition, a square root
    assert_within(loss, rloss, mloss, d, F32, extra_ulps=DIVF + 1 + SQRTF, what="pero_vicreg_var loss")
    # cvar: one term; std's three roundings, two products, one division
    assert_within(cvar, rcvar, mcvar, 1, F32, extra_ulps=DIVF + 1 + SQRTF + 2 + DIVF, what="pero_vicreg_var cvar")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wv,wc", [(1.0, 1.0), (25.0, 1.0)])
@pytest.mark.parametrize("d", [8, 72, 264, 520])
def test_vicreg_cov(ops, dtype, wv, wc, d):
    g = gen(d, 11)
    a = torch.randn(d, d, generator=g)
    cov = ((a + a.t()) * 0.5).contiguous()
    cvar = -torch.rand(d, generator=g) * 0.01
    cvar[::3] = 0.0
    m = 130
    G, loss = ops.vicreg_cov(cov.cuda(), cvar.cuda(), m, wv, wc, dtype)
    (rG, rloss), (mG, mloss) = R.vicreg_cov(cov, cvar, m, wv, wc)
    # G: one term; the coefficient wc 4 / (d (m - 1)) is two products and a division, then one product
    assert_within(G, rG, mG, 1, dtype, extra_ulps=3 + DIVF, what="pero_vicreg_cov G")
    assert_within(torch.diagonal(G), wv * cvar.double(), (wv * cvar.double()).abs(), 1, dtype, what="pero_vicreg_cov G diagonal")
    # header: rowpart[d] row sums of d - 1 squares, then the sum of the d row sums
    assert_within(loss, rloss, mloss, 2 * d, F32, what="pero_vicreg_cov loss")


# ------------------------------------------------------------------------------------------------ NT-Xent
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [19, 72, 520])
@pytest.mark.parametrize("rows", [1, 5, 130])
def test_rownorm_fwd_bwd(ops, dtype, rows, d):
    g = gen(rows, d, 13)
    x = (torch.randn(rows, d, generator=g) * 1.5 + 0.2).to(dtype)
    zero_row = 3 if rows > 1 else None
    if zero_row is not None:
        x[zero_row] = 0.0
    dxn = torch.randn(rows, d, generator=g).to(dtype)
    xn, inv = ops.rownorm_fwd(x.cuda())
    (rxn, rinv), (mxn, minv) = R.rownorm(x)
    # d squares; a square root, a reciprocal and the product x inv
    assert_within(inv, rinv, minv, d, F32, extra_ulps=SQRTF + DIVF, what="pero_rownorm_fwd inv")
    assert_within(xn, rxn, mxn, d, dtype, extra_ulps=SQRTF + DIVF + 1, what="pero_rownorm_fwd xn")
    if zero_row is not None:
        assert abs(float(inv[zero_row]) - 1e12) <= 1e12 * 2.0 ** -22 and float(xn[zero_row].float().abs().max()) == 0.0
    # the out= form into halves of one buffer (the second half starts at rows * d elements: 16-byte aligned or not)
    both = torch.full((2 * rows, d), 9.0, device="cuda", dtype=dtype)
    inv2 = torch.full((2 * rows,), 9.0, device="cuda")
    ops.rownorm_fwd(x.cuda(), out=(both[rows:], inv2[rows:]))
    assert torch.equal(both[rows:], xn) and torch.equal(inv2[rows:], inv)
    assert float((both[:rows].float() - 9.0).abs().max()) == 0.0 and float((inv2[:rows] - 9.0).abs().max()) == 0.0
    ops.rownorm_fwd(x.cuda(), out=(both[:rows], inv2[:rows]))
    assert torch.equal(both[:rows], xn) and torch.equal(inv2[:rows], inv) and torch.equal(both[rows:], xn)
    for gval in (None, 0.5):
        dx = ops.rownorm_bwd(xn, dxn.cuda(), inv, scalar(gval))
        rdx, mdx = R.rownorm_bwd(xn, dxn, inv, gval)
        assert bool(torch.isfinite(dx.float()).all())
        assert_within(dx, rdx, mdx, d + 1, dtype, what="pero_rownorm_bwd")    # d products of the dot, and dxn; inv g is in the 4


def _sim(lines, S):
    g = gen(lines, S, 17)
    sim = torch.rand(lines, S, S, generator=g) * 20 - 10
    sim[0, 3, 7] = 60.0                      # one dominant entry: every other term of its column is ~e^-50
    sim[lines - 1, :, 2] = 4.25              # a column of identical values
    return sim, g


@pytest.mark.parametrize("grad_dtype", [None, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("lines,S", [(3, 32), (5, 100), (2, 257)])   # S > 256: a thread owns more than one column
def test_ntxent_cols(ops, grad_dtype, lines, S):
    sim, _ = _sim(lines, S)
    loss, line_loss, dsim = ops.ntxent_cols(sim.cuda(), grad_dtype)
    res, mag = R.ntxent_cols(sim)
    ulps = mag["ulps"] + EXPF + LOGF          # argument errors (parity_ref._lse_units), one expf per term, one logf
    # S exponentials per column, then S columns (then `lines` line losses)
    assert_within(line_loss, res["line_loss"], mag["line_loss"], 2 * S, F32, extra_ulps=ulps, what="pero_ntxent_cols line_loss")
    assert_within(loss, res["loss"], mag["loss"], 2 * S + lines, F32, extra_ulps=ulps, what="pero_ntxent_cols loss")
    if grad_dtype is None:
        assert dsim is None
    else:   # p = exp(s - lse): lse carries the S-term sum; the second expf, the subtraction and the weight
        assert_within(dsim, res["dsim"], mag["dsim"], S, grad_dtype, extra_ulps=ulps + EXPF + 2, what="pero_ntxent_cols dsim")


@pytest.mark.parametrize("grad_dtype", DTYPES)
@pytest.mark.parametrize("lines,S,L,own0", [(3, 32, 3, 0), (2, 100, 70, 5), (2, 257, 8, 6), (1, 16, 1, 0)])   # L > 64: a lane owns two negatives
def test_ntxent_cols_cross(ops, grad_dtype, lines, S, L, own0):
    sim, g = _sim(lines, S)
    cross = torch.rand(lines * S, L, generator=g) * 20 - 10
    for l in range(lines):
        cross[l * S:(l + 1) * S, own0 + l] = 1e4      # the line's own pooled embedding: must influence nothing
    loss, line_loss, dsim, dcross = ops.ntxent_cols_cross(sim.cuda(), cross.cuda(), own0, grad_dtype)
    res, mag = R.ntxent_cols_cross(sim, cross, own0)
    # as ntxent_cols with S + L - 1 exponentials per column; the two partial sums are joined by one more expf and a product
    ulps = mag["ulps"] + 2 * EXPF + LOGF + 2
    assert_within(line_loss, res["line_loss"], mag["line_loss"], 2 * S + L, F32, extra_ulps=ulps, what="pero_ntxent_cols_cross line_loss")
    assert_within(loss, res["loss"], mag["loss"], 2 * S + L + lines, F32, extra_ulps=ulps, what="pero_ntxent_cols_cross loss")
    assert_within(dsim, res["dsim"], mag["dsim"], S + L, grad_dtype, extra_ulps=ulps + EXPF + 2, what="pero_ntxent_cols_cross dsim")
    assert_within(dcross, res["dcross"], mag["dcross"], S + L, grad_dtype, extra_ulps=ulps + EXPF + 2, what="pero_ntxent_cols_cross dcross")
    for l in range(lines):
        assert float(dcross[l * S:(l + 1) * S, own0 + l].float().abs().max()) == 0.0
    if L == 1:   # no negatives at all: the loss of pero_ntxent_cols on the same sim, within that entry point's bound
        plain, pmag = R.ntxent_cols(sim)
        assert_within(loss, plain["loss"], pmag["loss"], 2 * S + L + lines, F32, extra_ulps=pmag["ulps"] + 2 * EXPF + LOGF + 2,
                      what="pero_ntxent_cols_cross loss")
        assert_within(ops.ntxent_cols(sim.cuda())[0], plain["loss"], pmag["loss"], 2 * S + lines, F32, extra_ulps=pmag["ulps"] + EXPF + LOGF)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lines,S,d", [(3, 5, 8), (2, 33, 2056)])   # d / 8 = 257: a second block along x
def test_line_mean_and_add_line_rows(ops, dtype, lines, S, d):
    g = gen(lines, S, d)
    x = (torch.randn(lines * S, d, generator=g) + 0.4).to(dtype)
    ref, mag = R.line_mean(x, lines, S)
    assert_within(ops.line_mean(x.cuda(), lines, S), ref, mag, S + 1, F32, what="pero_line_mean")   # S rows, then the product with 1 / S
    src = torch.randn(lines, d, generator=g)
    for scale in (1.0, f32r(1.0 / S)):
        dst = x.cuda()
        ops.add_line_rows_(dst, src.cuda(), lines, S, scale)
        ref, mag = R.add_line_rows(x, src, lines, S, scale)
        assert_within(dst, ref, mag, 2, dtype, what="pero_add_line_rows")     # old value + scale src
        assert not torch.equal(dst.cpu(), x)


# ------------------------------------------------------------------------------------------------ BatchNorm1d (+ ReLU)
BN_SHAPES = [(37, 72), (301, 200), (2, 64), (5, 1), (4100, 520)]   # two strips; four; two rows; one column; past the 8192-block grid cap


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows,d", BN_SHAPES)
def test_bn_fwd_bwd(ops, dtype, relu, rows, d):
    g = gen(rows, d, relu)
    eps, mom = f32r(1e-5), f32r(0.1)
    xs = [(torch.randn(rows, d, generator=g) * torch.linspace(0.5, 2.0, d) + 0.3).to(dtype) for _ in range(2)]
    w, b = torch.randn(d, generator=g), torch.randn(d, generator=g) * 0.5
    rm0, rv0 = torch.randn(d, generator=g), torch.rand(d, generator=g) + 0.5
    dy = torch.randn(rows, d, generator=g).to(dtype)
    wd, bd = w.cuda(), b.cuda()
    rm, rv = rm0.cuda(), rv0.cuda()
    r_rm, r_rv, r_mag = rm0, rv0, None
    for step, x in enumerate(xs):
        y, mean, rstd = ops.bn_fwd(x.cuda(), wd, bd, rm, rv, eps, mom, True, relu)
        res, mag = R.bn_fwd(x, w, b, r_rm, r_rv, eps, mom, True, relu, running_mag=r_mag)
        r_rm, r_rv, r_mag = res["running_mean"], res["running_var"], (mag["running_mean"], mag["running_var"])
        # mean: `rows` terms.  rstd: `rows` squares (each from a rounded difference: 3 units), a division by the count, + eps, sqrt, reciprocal
        assert_within(mean, res["mean"], mag["mean"], rows, F32, what="pero_bn_fwd save_mean")
        assert_within(rstd, res["rstd"], mag["rstd"], rows, F32, extra_ulps=3 + DIVF + 1 + SQRTF + DIVF, what="pero_bn_fwd save_rstd")
        # y: the mean's chain and the variance's chain (rows terms each) and rstd's extras above, then two products and the bias
        assert_within(y, res["y"], mag["y"], 2 * rows, dtype, extra_ulps=3 + DIVF + 1 + SQRTF + DIVF + 3, what="pero_bn_fwd y")
        # running statistics after step + 1 calls: each call adds the batch chain (rows terms + the unbiased division) and two products
        assert_within(rm, r_rm, r_mag[0], (step + 1) * (rows + 2), F32, what="pero_bn_fwd running_mean")
        assert_within(rv, r_rv, r_mag[1], (step + 1) * (rows + 2), F32, extra_ulps=3 + DIVF, what="pero_bn_fwd running_var")
        y_free, mean_free, rstd_free = ops.bn_fwd(x.cuda(), wd, bd, None, None, eps, mom, True, relu)   # no running buffers: same batch statistics
        assert torch.equal(y_free, y) and torch.equal(mean_free, mean) and torch.equal(rstd_free, rstd)
    # backward of the second step: the reference gates on the y the forward kernel stored (checked above)
    for accumulate in (False, True):
        dw = torch.full((d,), 3.0, device="cuda") if accumulate else None
        db = torch.full((d,), -2.0, device="cuda") if accumulate else None
        dx = ops.bn_bwd(dy.cuda(), x.cuda(), y, wd, mean, rstd, dw, db, relu)
        bres, bmag = R.bn_bwd(dy, x, y, w, mean, rstd, None if dw is None else torch.full((d,), 3.0),
                              None if db is None else torch.full((d,), -2.0), relu)
        # dx: g, the mean of g (rows terms) and xhat times the mean of g xhat (rows terms, each from a rounded difference), four products
        assert_within(dx, bres["dx"], bmag["dx"], 2 * rows + 1, dtype, extra_ulps=6, what="pero_bn_bwd dx")
        if accumulate:   # old value + rows terms (+ the product with rstd)
            assert_within(dw, bres["dweight"], bmag["dweight"], rows + 1, F32, extra_ulps=2, what="pero_bn_bwd dweight")
            assert_within(db, bres["dbias"], bmag["dbias"], rows + 1, F32, what="pero_bn_bwd dbias")
            assert float((db + 2.0).abs().max()) > 0
    # evaluation: the running statistics the two training calls left; the buffers keep their bits
    rm_before, rv_before = rm.clone(), rv.clone()
    y, mean, rstd = ops.bn_fwd(x.cuda(), wd, bd, rm, rv, eps, mom, False, relu)
    res, mag = R.bn_fwd(x, w, b, rm, rv, eps, mom, False, relu)
    assert torch.equal(rm, rm_before) and torch.equal(rv, rv_before) and torch.equal(mean, rm)
    assert_within(rstd, res["rstd"], mag["rstd"], 1, F32, extra_ulps=1 + SQRTF + DIVF, what="pero_bn_fwd eval rstd")
    assert_within(y, res["y"], mag["y"], 2, dtype, extra_ulps=1 + SQRTF + DIVF + 3, what="pero_bn_fwd eval y")


# ------------------------------------------------------------------------------------------------ utilities
@pytest.mark.parametrize("pitch", [400, 512])
def test_rowdot_blocks(ops, pitch):
    g = gen(pitch, 19)
    rows, cols = 37, 384
    x = torch.randn(rows, pitch, generator=g).bfloat16()
    y = torch.randn(rows, pitch + 16, generator=g).bfloat16()
    out, xd, yd = torch.full((rows, cols // 128), 5.0, device="cuda"), x.cuda(), y.cuda()
    call("pero_rowdot_blocks", ops.ptr(xd), ops.ptr(yd), ops.ptr(out), rows, cols, pitch, pitch + 16, ops.stream())
    ref, mag = R.rowdot_blocks(x[:, :cols], y[:, :cols])
    assert_within(out, ref, mag, 128, F32, what="pero_rowdot_blocks")


@pytest.mark.parametrize("rows,cols,pitch", [(5, 19, 24), (64, 512, 640)])
def test_cast_pad_f32_bf16(ops, rows, cols, pitch):
    src = torch.randn(rows, cols, generator=gen(rows, cols))
    dst = ops.cast_pad_to_bf16(src.cuda(), pitch)
    assert torch.equal(dst[:, :cols].cpu(), src.bfloat16()) and float(dst[:, cols:].float().abs().max()) == 0.0


def test_add_rows2d(ops):
    g = gen(23)
    rows, cols = 7, 33
    dst0, src = torch.randn(rows, 40, generator=g), torch.randn(rows, 36, generator=g)
    dst = dst0.cuda()
    ops.add_rows2d(dst, src.cuda(), cols)
    assert torch.equal(dst.cpu()[:, :cols], dst0[:, :cols] + src[:, :cols])    # one f32 addition per element: exact
    assert torch.equal(dst.cpu()[:, cols:], dst0[:, cols:])                    # columns beyond `cols`: untouched


@pytest.mark.parametrize("offset,nbytes", [(64, 8192 * 256 * 16 + 4096 * 16), (64, 16 * 100 + 5), (66, 1600)])
def test_zero_fill(ops, offset, nbytes):
    """16-byte aligned and a whole number of 16-byte pieces, past grid x block pieces (the stride loop); aligned with five odd bytes;
    misaligned by two bytes.  64 guard bytes on each side keep their value."""
    buf = torch.full((offset + nbytes + 64,), 0xAB, device="cuda", dtype=torch.uint8)
    assert buf.data_ptr() % 16 == 0
    call("pero_zero_fill", buf.data_ptr() + offset, nbytes, ops.stream())
    assert int(buf[offset:offset + nbytes].max()) == 0
    assert int(buf[:offset].min()) == 0xAB and int(buf[offset + nbytes:].min()) == 0xAB and buf[offset + nbytes:].numel() == 64


def _special_f32(n, g):
    x = torch.randn(n, generator=g)
    bits = x[:4096].view(torch.int32).clone()
    bits = (bits & ~0xFFFF) | 0x8000           # exact ties between two bf16 neighbours, even and odd upper halves alike
    x[:4096] = bits.view(torch.float32)
    x[4096], x[4097], x[4098], x[4099], x[4100] = float("inf"), float("-inf"), float("nan"), 0.0, -0.0
    x[4101] = 3.4e38             # rounds up to inf
    x[4102] = 1e-40                             # subnormal
    return x


def test_casts_bit_exact_with_tail_and_special_values(ops):
    n = 100003                                  # not a multiple of 8: the tail of the vector loop
    src = _special_f32(n, gen(29))
    dst = torch.full((n + 8,), 1.5, device="cuda", dtype=torch.bfloat16)
    ops.cast_to_bf16(src.cuda(), dst[:n])
    got, want = dst[:n].cpu().view(torch.int16), src.bfloat16().view(torch.int16)
    # (torch's own f32 -> bf16 of a NaN depends on the host's code path - 0x7fc0 from the scalar one, 0xffff from the AVX-512 one - so at the
    #  NaN the kernel is held to the truncation of the source's quiet NaN instead: sign and quiet bit kept, 0x7fc0; every other element,
    #  the ties, the infinities, the overflow and the subnormal included, to torch bit for bit)
    assert int(got[4098]) == 0x7FC0 and bool(torch.isnan(src.bfloat16()[4098]))
    want[4098] = 0x7FC0
    bad = torch.nonzero(got != want).reshape(-1)[:8].tolist()
    assert not bad, [(i, hex(int(src.view(torch.int32)[i]) & 0xFFFFFFFF), hex(int(got[i]) & 0xFFFF), hex(int(want[i]) & 0xFFFF)) for i in bad]
    assert float((dst[n:].float() - 1.5).abs().max()) == 0.0
    back = torch.full((n + 8,), 2.5, device="cuda")
    call("pero_cast_bf16_f32", ops.ptr(dst), ops.ptr(back), n, ops.stream())
    assert torch.equal(back[:n].cpu().view(torch.int32), dst[:n].cpu().float().view(torch.int32))
    assert float((back[n:] - 2.5).abs().max()) == 0.0


def test_scale_bf16(ops):
    x = torch.randn(100003, generator=gen(31)).bfloat16()
    y = x.cuda()
    ops.scale_(y, f32r(0.3))
    assert torch.equal(y.cpu(), (x.float() * f32r(0.3)).bfloat16())      # one f32 product, one rounding: exact


@pytest.mark.parametrize("dtype,rows,cols,pitch", [(torch.float32, 45, 19, 19), (torch.bfloat16, 45, 19, 19),      # cols % 8 != 0
                                                   (torch.bfloat16, 45, 72, 76),                                     # rows not 16-byte aligned
                                                   (torch.float32, 300, 72, 80), (torch.bfloat16, 300, 72, 80)])   # the fast path, three slabs
def test_colsum_paths(ops, dtype, rows, cols, pitch):
    g = gen(rows, cols, pitch)
    x = (torch.randn(rows, pitch, generator=g) + 0.25).to(dtype)
    out0 = torch.randn(cols, generator=g)
    out = out0.cuda()
    ops.colsum(x.cuda()[:, :cols], out)
    ref, mag = R.colsum(x[:, :cols], out0)
    assert_within(out, ref, mag, rows + 1, F32, what="pero_colsum")            # old value + `rows` terms


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_scatter_rows_scalar_branch(ops, dtype):
    g = gen(37, dtype == F32)
    d = 19
    src = torch.randn(50, d, generator=g).to(dtype)
    index = torch.randperm(50, generator=g)[:21]
    out = ops.gather_rows(src.cuda(), index.cuda(), 24)
    assert torch.equal(out[:21].cpu(), src[index]) and float(out[21:].float().abs().max()) == 0.0
    dst = src.cuda()
    ops.scatter_add_rows(out, index.cuda(), dst)
    ref = src.float()
    ref[index] += src[index].float()
    assert torch.equal(dst.cpu(), ref.to(dtype))                               # one addition, one rounding: exact
    none = torch.full((6, d), 4.0, device="cuda", dtype=dtype)
    ops.gather_rows(src.cuda(), index.cuda()[:0], 6, out=none)                 # n_idx = 0: every output row is padding
    assert float(none.float().abs().max()) == 0.0
