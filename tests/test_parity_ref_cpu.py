"""The f64 restatements of tests/parity_ref.py must be right before a GPU kernel is held to them: each is pinned here, on the
CPU, to the oracle (oracle/pero_oracle.py) or to torch autograd / torch.nn in f64, chained the way the library chains the
entry points."""
import pytest
import torch

import parity_ref as R
from oracle import pero_oracle as O

TOL = 1e-10


def close(a, b, tol=TOL):
    a, b = R.f64(a), R.f64(b)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_vicreg_pieces_chain_to_the_oracle_loss_and_its_gradients():
    """gather -> colsum -> center_cols -> zc^T zc / (m - 1) -> vicreg_var -> vicreg_cov; gradient zc @ G scattered back plus sqdiff_bwd."""
    g = torch.Generator().manual_seed(1)
    N, S, D = 3, 7, 16
    x = (torch.randn(N, S, D, generator=g, dtype=torch.float64) * torch.linspace(0.25, 1.75, D, dtype=torch.float64) + 0.3).requires_grad_(True)
    y = (torch.randn(N, S, D, generator=g, dtype=torch.float64) * torch.linspace(0.25, 1.75, D, dtype=torch.float64) - 0.1).requires_grad_(True)
    im1 = (torch.rand(N, S, generator=g) < 0.8).long()
    im2 = (torch.rand(N, S, generator=g) < 0.8).long()
    sm1 = torch.zeros(N, S, dtype=torch.long)
    sm2 = torch.zeros(N, S, dtype=torch.long)
    sm1[:, 1:5] = 1
    sm2[:, 2:6] = 1
    wv, wi, wc, thr, eps = 25.0, 15.0, 2.0, 1.0, 1e-5
    ref = O.vicreg_loss(x, y, im1, im2, sm1, sm2, wv, wi, wc, thr, eps)
    ref["loss"].backward()

    x2, y2 = x.detach().reshape(N * S, D), y.detach().reshape(N * S, D)
    ix, iy = torch.nonzero(sm1.reshape(-1) == 1).reshape(-1), torch.nonzero(sm2.reshape(-1) == 1).reshape(-1)
    i1, i2 = torch.nonzero(im1.reshape(-1) == 1).reshape(-1), torch.nonzero(im2.reshape(-1) == 1).reshape(-1)
    n = ix.numel()
    inv, mag = R.sqdiff(x2, ix, y2, iy, 1.0 / (n * D))
    assert close(inv, ref["loss.invariance"]) and close(mag, inv)
    m = i1.numel() + i2.numel()
    m_pad = m + 5
    z = torch.zeros(m_pad, D, dtype=torch.float64)
    z[:i1.numel()] = x2[i1]
    z[i1.numel():m] = y2[i2]
    cs, _ = R.colsum(z, torch.zeros(D))
    (zc, sumsq), (mag_zc, _) = R.center_cols(z, cs, m, torch.zeros(D))
    assert float(zc[m:].abs().max()) == 0.0 and bool((mag_zc >= zc.abs()).all())
    (cvar, lvar), _ = R.vicreg_var(sumsq, m, thr, eps)
    assert close(lvar, ref["loss.variance"])
    assert 0 < int((cvar == 0).sum()) < D, "the scale ramp must put columns on both sides of the hinge"
    cov = zc.t() @ zc / (m - 1)
    (G, lcov), _ = R.vicreg_cov(cov, cvar, m, wv, wc)
    assert close(lcov, ref["loss.covariance"])
    assert close(wv * lvar + wi * inv + wc * lcov, ref["loss"])
    dz = zc @ G
    dx0, dy0 = torch.zeros(N * S, D, dtype=torch.float64), torch.zeros(N * S, D, dtype=torch.float64)
    dx1, _ = R.scatter_add_scaled(dz[:i1.numel()], i1, dx0, None)
    dy1, _ = R.scatter_add_scaled(dz[i1.numel():m], i2, dy0, 1.0)
    (dx, dy), _ = R.sqdiff_bwd(x2, ix, y2, iy, dx1, dy1, torch.tensor(1.0), wi * 2.0 / (n * D))
    assert close(dx, x.grad.reshape(N * S, D)) and close(dy, y.grad.reshape(N * S, D))
    # a pre-filled accumulator and an upstream gradient scale
    (dxg, _), _ = R.sqdiff_bwd(x2, ix, y2, iy, dx1 + 1.0, dy1, torch.tensor(0.5), 4.0)
    assert close(dxg - 1.0 - dx1, 0.5 * 4.0 / (wi * 2.0 / (n * D)) * (dx - dx1))
    out, mag = R.sum_scale(torch.tensor([1.0, -2.0, 4.0]), 0.5)
    assert float(out) == 1.5 and float(mag) == 3.5


def _ntxent_inputs(L, S, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(L, S, D, generator=g, dtype=torch.float64).requires_grad_(True)
    y = (torch.randn(L, S, D, generator=g, dtype=torch.float64) * 0.5 + 0.7 * x.detach()).requires_grad_(True)
    return x, y


def test_ntxent_pieces_chain_to_the_oracle_loss_and_its_gradients():
    L, S, D, T = 3, 6, 10, 0.1
    x, y = _ntxent_inputs(L, S, D, 2)
    ones = torch.ones(L, S, dtype=torch.long)
    ref = O.ntxent_loss(x, y, ones, ones, ones, ones, T)["loss"]
    ref.backward()
    (xn, invx), _ = R.rownorm(x.detach().reshape(L * S, D))
    (yn, invy), _ = R.rownorm(y.detach().reshape(L * S, D))
    sim = torch.einsum("lid,ljd->lij", xn.reshape(L, S, D), yn.reshape(L, S, D)) / T
    res, mag = R.ntxent_cols(sim)
    assert close(res["loss"], ref) and close(res["line_loss"].mean(), ref)
    assert bool((mag["dsim"] >= res["dsim"].abs()).all()) and mag["ulps"] > 0
    dxn = torch.einsum("lij,ljd->lid", res["dsim"], yn.reshape(L, S, D)).reshape(L * S, D) / T
    dyn = torch.einsum("lij,lid->ljd", res["dsim"], xn.reshape(L, S, D)).reshape(L * S, D) / T
    dx, _ = R.rownorm_bwd(xn, dxn, invx, None)
    dy, _ = R.rownorm_bwd(yn, dyn, invy, torch.tensor(1.0))
    assert close(dx, x.grad.reshape(L * S, D)) and close(dy, y.grad.reshape(L * S, D))
    # an all-zero row: inv is the reciprocal of the floor, the row stays zero, nothing is NaN in either direction
    xz = x.detach().reshape(L * S, D).clone()
    xz[4] = 0.0
    (xnz, invz), _ = R.rownorm(xz)
    assert abs(float(invz[4]) - 1e12) < 1e12 * 2.0 ** -23 and float(xnz[4].abs().max()) == 0.0
    dz, _ = R.rownorm_bwd(xnz, dxn, invz, None)
    assert bool(torch.isfinite(dz).all())


def test_ntxent_cross_pieces_chain_to_the_oracle_loss_and_its_gradients():
    L, S, D, T = 4, 5, 8, 0.1
    x, y = _ntxent_inputs(L, S, D, 3)
    ref, _ = O.ntxent_cross_loss(x, y, 2, T)
    ref.backward()
    (xn, invx), _ = R.rownorm(x.detach().reshape(L * S, D))
    (yn, invy), _ = R.rownorm(y.detach().reshape(L * S, D))
    pm, _ = R.line_mean(xn, L, S)
    (p, invp), _ = R.rownorm(pm)
    sim = torch.einsum("lid,ljd->lij", xn.reshape(L, S, D), yn.reshape(L, S, D)) / T
    cross = yn @ p.t() / T
    poisoned = cross.clone()
    for l in range(L):
        poisoned[l * S:(l + 1) * S, l] = 1e4       # the line's own pooled embedding is left out: it influences nothing
    res, mag = R.ntxent_cols_cross(sim, poisoned, 0)
    assert close(res["loss"], ref)
    for l in range(L):
        assert float(res["dcross"][l * S:(l + 1) * S, l].abs().max()) == 0.0
    dxn = torch.einsum("lij,ljd->lid", res["dsim"], yn.reshape(L, S, D)).reshape(L * S, D) / T
    dyn = torch.einsum("lij,lid->ljd", res["dsim"], xn.reshape(L, S, D)).reshape(L * S, D) / T + res["dcross"] @ p / T
    dp = res["dcross"].t() @ yn / T
    dpm, _ = R.rownorm_bwd(p, dp, invp, None)
    dxn, _ = R.add_line_rows(dxn, dpm, L, S, 1.0 / S)
    dx, _ = R.rownorm_bwd(xn, dxn, invx, None)
    dy, _ = R.rownorm_bwd(yn, dyn, invy, None)
    assert close(dx, x.grad.reshape(L * S, D)) and close(dy, y.grad.reshape(L * S, D))
    # a single line has no negatives: the cross form is the plain one
    one, _ = R.ntxent_cols_cross(sim[:1], torch.full((S, 1), 1e4, dtype=torch.float64), 0)
    plain, _ = R.ntxent_cols(sim[:1])
    assert close(one["loss"], plain["loss"]) and close(one["dsim"], plain["dsim"])


@pytest.mark.parametrize("relu", [False, True])
def test_bn_matches_torch_batchnorm1d(relu):
    g = torch.Generator().manual_seed(4)
    rows, d, eps, mom = 9, 5, 1e-5, 0.1
    bn = torch.nn.BatchNorm1d(d, eps=eps, momentum=mom).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(d, generator=g, dtype=torch.float64))
        bn.bias.copy_(torch.randn(d, generator=g, dtype=torch.float64))
    w, b = bn.weight.detach().clone(), bn.bias.detach().clone()
    rm, rv, rmag = torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64), None
    for step in range(2):
        x = (torch.randn(rows, d, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
        dy = torch.randn(rows, d, generator=g, dtype=torch.float64)
        bn.zero_grad()
        yt = torch.relu(bn(x)) if relu else bn(x)
        yt.backward(dy)
        res, mag = R.bn_fwd(x.detach(), w, b, rm, rv, eps, mom, True, relu, running_mag=rmag)
        assert close(res["y"], yt) and bool((mag["y"] >= res["y"].abs() - 1e-12).all()) and bool((mag["rstd"] >= res["rstd"]).all())
        rm, rv, rmag = res["running_mean"], res["running_var"], (mag["running_mean"], mag["running_var"])
        assert close(rm, bn.running_mean) and close(rv, bn.running_var)
        bres, bmag = R.bn_bwd(dy, x.detach(), res["y"], w, res["mean"], res["rstd"], torch.full((d,), 3.0), torch.full((d,), -2.0), relu)
        assert close(bres["dx"], x.grad) and close(bres["dweight"] - 3.0, bn.weight.grad) and close(bres["dbias"] + 2.0, bn.bias.grad)
        assert bool((bmag["dx"] >= bres["dx"].abs() - 1e-12).all())
    free, _ = R.bn_fwd(x.detach(), w, b, None, None, eps, mom, True, relu)     # training without running buffers
    assert close(free["y"], yt) and "running_mean" not in free
    bn.eval()
    ye = torch.relu(bn(x)) if relu else bn(x)
    res, _ = R.bn_fwd(x.detach(), w, b, rm, rv, eps, mom, False, relu)
    assert close(res["y"], ye) and "running_mean" not in res


def test_softmax_masked_ce_and_small_sums_match_autograd():
    g = torch.Generator().manual_seed(5)
    s = (torch.randn(6, 11, generator=g, dtype=torch.float64) * 40).requires_grad_(True)
    dp = torch.randn(6, 11, generator=g, dtype=torch.float64)
    pt = torch.softmax(s * 0.3, -1)
    pt.backward(dp)
    p, mag = R.softmax(s.detach(), 0.3)
    ds, _ = R.softmax_bwd(p, dp, 0.3)
    assert close(p, pt) and close(ds, s.grad) and mag["ulps"] > 0
    rows, V = 12, 9
    lg = (torch.randn(rows, V, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[10:] = -1
    mask = torch.tensor([1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 0])
    for uw in (None, 0.25):
        lg.grad = None
        ref = O.masked_cross_entropy(lg[None], labels[None], mask[None], uw)
        ref.backward()
        (loss, grad), mag = R.masked_ce(lg.detach(), labels, mask, uw, dloss=torch.tensor(0.5))
        assert close(loss, ref) and close(grad, 0.5 * lg.grad) and bool((mag["grad"] >= grad.abs()).all())
    x, y = torch.randn(3, 256, generator=g), torch.randn(3, 256, generator=g)
    out, _ = R.rowdot_blocks(x, y)
    assert close(out, (x.double() * y.double()).reshape(3, 2, 128).sum(-1))
    out, mag = R.colsum(x, torch.ones(256))
    assert close(out, 1 + x.double().sum(0)) and bool((mag >= out.abs()).all())


def test_assert_within_rejects_twice_its_bound_and_accepts_half():
    ref = torch.tensor([1.0, -3.0, 0.0, 100.0], dtype=torch.float64)
    mag = torch.tensor([2.0, 3.0, 1.0, 400.0], dtype=torch.float64)
    for dtype in (torch.float32, torch.bfloat16):
        b = R.bound(ref, mag, 10, dtype, extra_ulps=2)
        want = 16 * 2.0 ** -24 * mag + 2.0 ** -126 + (2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0)
        assert torch.equal(b, want)
        assert R.assert_within(ref + 0.5 * b, ref, mag, 10, dtype, extra_ulps=2) == pytest.approx(0.5)
        R.assert_within(ref - 0.5 * b, ref, mag, 10, dtype, extra_ulps=2)
        for k in range(4):           # ONE element at twice its bound is enough
            bad = ref.clone()
            bad[k] += 2.0 * b[k]
            with pytest.raises(AssertionError, match=rf"element \({k},\)"):
                R.assert_within(bad, ref, mag, 10, dtype, extra_ulps=2, what="probe")
    with pytest.raises(AssertionError):   # NaN is never within a bound
        R.assert_within(torch.tensor([float("nan")]), torch.tensor([1.0]), torch.tensor([1.0]), 1, torch.float32)
    with pytest.raises(AssertionError):   # without magnitude only the underflow step (2^-126) is left
        R.assert_within(torch.tensor([1e-30]), torch.tensor([0.0]), torch.tensor([0.0]), 1, torch.float32)
