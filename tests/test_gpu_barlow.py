"""GPU: BarlowTwinsLoss and the five kernels of csrc/barlow.hip against the f64 restatement of tests/barlow_ref.py.

Bounds.  f32 mode: values within 1e-4 |ref| + 1e-7, gradients within 1e-4 max|ref| + 1e-8 - those of test_vicreg_matches_reference_golden
(same GEMM, same kind of statistics); the same arithmetic in torch f32 on the CPU differs from f64 by at most 1.2e-6 / 5e-6 of the maximum
at these shapes.  bf16 mode: values within 2e-2 |ref| + 1e-6, gradient cosine above 0.995 - those of test_vicreg_bf16_large_uses_fast_syrk;
with inputs and zh rounded to bf16 the CPU restatement differs by 3.2e-4 / 8.2e-3 and a cosine of 0.99998 (the rounding of G and d zh
to bf16 was not simulated).  Every case prints its figures before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import barlow_ref as B  # noqa: E402

TILE_ROWS = 1024   # PERO_BARLOW_TILE_ROWS: the rows of one partial of the column reductions (asserted below)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def masks_ab(n, s, tail):
    """Shift mask 1 with its last `tail` positions 0 and one position per line set to 2; shift mask 2 is its reverse."""
    m1 = np.ones((n, s), np.uint8)
    m1[:, s - tail:] = 0
    if n > 1:
        for l in range(n):
            m1[l, 5 + l] = 2
    return m1, m1[:, ::-1].copy()


# name -> (N, S, D, shift, noise, masks)
CASES = {
    "a": (1, 40, 24, 0.0, 0.3, lambda: masks_ab(1, 40, 3)),        # 37 pairs: n % 64 != 0, one partial row tile, D % 8 == 0 but tiny
    "a20": (1, 40, 20, 0.0, 0.3, lambda: masks_ab(1, 40, 3)),      # D % 8 != 0: the element-by-element path of every kernel
    "b": (4, 64, 256, 0.0, 0.3, lambda: masks_ab(4, 64, 2)),       # 244 pairs, 16-byte path; bf16: the tile GEMM
    "c": (4, 64, 256, 5.0, 0.3, lambda: masks_ab(4, 64, 2)),       # as b, column offsets of 5 (6 x std)
    "d": (33, 64, 64, 0.0, 1.0, lambda: (np.ones((33, 64), np.uint8),) * 2),   # 2112 pairs = 2 full row tiles of 1024 + one of 64
}


@functools.lru_cache(maxsize=None)
def case(name, bf16):
    """(x, y, m1, m2, ref) - float32 inputs (bf16-rounded values when bf16), the masks, and the f64 restatement's loss parts and gradients
    on exactly those values.  Computed once per (case, mode) and shared; nothing in it is modified."""
    N, S, D, shift, noise, mk = CASES[name]
    rng = np.random.default_rng(0)
    x = 0.8 * rng.standard_normal((N, S, D))
    if shift:
        x = x + shift * rng.standard_normal((1, 1, D))
    y = x + noise * rng.standard_normal((N, S, D))
    xt, yt = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.float32))
    if bf16:
        xt, yt = xt.bfloat16().float(), yt.bfloat16().float()
    m1, m2 = mk()
    xo, yo = xt.double().requires_grad_(True), yt.double().requires_grad_(True)
    res = B.barlow_loss(xo, yo, m1, m2)
    res["loss"].backward()
    ref = {k: float(v) for k, v in res.items()}
    ref["grad_x"], ref["grad_y"] = xo.grad.clone(), yo.grad.clone()
    return xt, yt, m1, m2, ref


KEYS = ("loss", "loss.on_diagonal", "loss.off_diagonal")


def run(name, bf16, scale=1.0, stacked=False, lam=0.0051):
    import pero_pretraining_amd as P
    from pero_pretraining_amd.joint_embedding_pretraining.losses import BarlowTwinsLoss
    xt, yt, m1, m2, ref = case(name, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    loss = BarlowTwinsLoss(lambda_offdiag=lam)
    masks = [cu(m) for m in (np.ones_like(m1), np.ones_like(m2), m1, m2)]
    with P.autocast(bf16):
        if stacked:
            xy = torch.cat([xt, yt]).to(dt).cuda().requires_grad_(True)
            res = loss.forward_stacked(xy, *masks)
        else:
            xg, yg = xt.to(dt).cuda().requires_grad_(True), yt.to(dt).cuda().requires_grad_(True)
            res = loss(xg, yg, *masks)
    (scale * res["loss"]).backward()
    if stacked:
        n = xt.shape[0]
        return res, xy.grad[:n], xy.grad[n:], ref
    return res, xg.grad, yg.grad, ref


def test_tile_height_is_the_one_the_cases_were_sized_for():
    from pero_pretraining_amd import ops
    assert ops.BARLOW_TILE_ROWS == TILE_ROWS
    n = int((CASES["d"][5]()[0] == 1).sum())
    assert n > 2 * TILE_ROWS and n % TILE_ROWS != 0   # at least three row tiles, the last one partial


@pytest.mark.parametrize("name", ["a", "a20", "b", "c", "d"])
def test_f32_matches_f64_restatement(name):
    res, gx, gy, ref = run(name, False)
    assert set(res) == set(KEYS)
    assert not res["loss.on_diagonal"].requires_grad and not res["loss.off_diagonal"].requires_grad
    for k in KEYS:
        print(f"{name} f32 {k}: got {float(res[k]):.9g} ref {ref[k]:.9g} rel {abs(float(res[k]) - ref[k]) / abs(ref[k]):.3g}")
    for g, r, w in ((gx, ref["grad_x"], "x"), (gy, ref["grad_y"], "y")):
        err = float((g.double().cpu() - r).abs().max())
        print(f"{name} f32 grad_{w}: max err {err:.3g} of max {float(r.abs().max()):.3g} -> {err / float(r.abs().max()):.3g}")
    for k in KEYS:
        assert abs(float(res[k]) - ref[k]) < 1e-4 * abs(ref[k]) + 1e-7, (k, float(res[k]), ref[k])
    for g, r in ((gx, ref["grad_x"]), (gy, ref["grad_y"])):
        assert float((g.double().cpu() - r).abs().max()) < 1e-4 * float(r.abs().max()) + 1e-8


@pytest.mark.parametrize("name", ["b", "c", "d"])
def test_bf16_matches_f64_restatement(name):
    res, gx, gy, ref = run(name, True)
    assert gx.dtype == torch.bfloat16
    cos = []
    for g, r in ((gx, ref["grad_x"]), (gy, ref["grad_y"])):
        g = g.float().cpu().double()
        cos.append(float((g.flatten() @ r.flatten()) / (g.norm() * r.norm())))
    for k in KEYS:
        print(f"{name} bf16 {k}: got {float(res[k]):.9g} ref {ref[k]:.9g} rel {abs(float(res[k]) - ref[k]) / abs(ref[k]):.3g}")
    print(f"{name} bf16 gradient cosines: {cos[0]:.6f} {cos[1]:.6f}")
    for k in KEYS:
        assert abs(float(res[k]) - ref[k]) < 2e-2 * abs(ref[k]) + 1e-6, (k, float(res[k]), ref[k])
    assert min(cos) > 0.995, cos


def test_stats_kernel_keeps_a_small_variance_on_a_large_mean():
    """z = 0.1 N(0, 1) + 10: a plain sum of squares minus the squared mean is off by 2e-2 in the variance here, a centred form by 1e-6."""
    from pero_pretraining_amd import ops
    rng = np.random.default_rng(0)
    z1 = (0.1 * rng.standard_normal((500, 64)) + 10.0).astype(np.float32)
    z2 = (0.1 * rng.standard_normal((500, 64)) + 10.0).astype(np.float32)
    idx = torch.arange(500, device="cuda")
    perm = torch.from_numpy(np.random.default_rng(1).permutation(500)).cuda()
    mean, rstd = ops.barlow_stats(cu(z1), idx, cu(z2), perm, 1e-5)
    for v, z in enumerate((z1, z2)):
        z64 = z.astype(np.float64)
        rs = 1.0 / np.sqrt(z64.var(axis=0) + 1e-5)
        err = np.abs(rstd[v].cpu().numpy() - rs) / rs
        print(f"view {v}: rstd rel err max {err.max():.3g}; mean abs err max {np.abs(mean[v].cpu().numpy() - z64.mean(axis=0)).max():.3g}")
        assert err.max() < 1e-4
        assert np.abs(mean[v].cpu().numpy() - z64.mean(axis=0)).max() < 1e-5


def test_forward_stacked_gives_the_bits_of_forward():
    res, gx, gy, _ = run("b", False)
    res2, gx2, gy2, _ = run("b", False, stacked=True)
    for k in KEYS:
        assert torch.equal(res[k], res2[k]), k
    assert torch.equal(gx, gx2) and torch.equal(gy, gy2)


def test_gradients_outside_the_pairs_are_exact_zeros_and_scale_with_the_seed():
    _, _, m1, m2, _ = case("b", False)
    assert (m1 == 2).sum() == 4 and (m2 == 2).sum() == 4
    res, gx, gy, _ = run("b", False)
    res3, gx3, gy3, _ = run("b", False, scale=3.0)
    for g, m in ((gx, m1), (gy, m2)):
        out = torch.from_numpy(m != 1).cuda()
        assert float(g[out].abs().max()) == 0.0 and int(out.sum()) == 12
        assert float(g[~out].abs().sum(dim=-1).min()) > 0.0   # every paired position has a gradient
    # the seed multiplies inside one f32 product chain: g * rstd * (...) - a few ulp of the largest entry
    for g, g3 in ((gx, gx3), (gy, gy3)):
        assert float((g3 - 3.0 * g).abs().max()) <= 4 * 2.0 ** -23 * float(g3.abs().max())


@pytest.mark.parametrize("name,bf16", [("b", False), ("d", False), ("b", True), ("d", True)])
def test_every_op_repeats_its_bits(name, bf16):
    """Case d: three row tiles, so the merge order of the partials is in play; case b: 244 -> 256 rows, so the padding rows are."""
    from pero_pretraining_amd import ops
    xt, yt, m1, m2, _ = case(name, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    D = xt.shape[-1]
    x2, y2 = xt.reshape(-1, D).to(dt).cuda(), yt.reshape(-1, D).to(dt).cuda()
    ix, iy = (cu(i) for i in B.pairs(m1, m2))
    n, n_pad = ix.numel(), ((ix.numel() + 63) // 64) * 64

    def twice(f):
        a, b = f(), f()
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        assert all(torch.equal(p, q) for p, q in zip(a, b)), f
        return a if len(a) > 1 else a[0]

    mean, rstd = twice(lambda: ops.barlow_stats(x2, ix, y2, iy, 1e-5))
    zh = twice(lambda: ops.barlow_standardize(x2, ix, y2, iy, mean, rstd, n_pad))
    if n_pad > n:   # the padding rows are stored zeros
        assert zh.shape == (2, n_pad, D) and float(zh[:, n:].abs().max()) == 0.0 and bool(torch.isfinite(zh).all())
    c = ops.gemm(zh[0].float(), zh[1].float(), trans_a=True, trans_b=True, alpha=1.0 / n, out_dtype=torch.float32)
    out, G = twice(lambda: ops.barlow_corr(c, n, 0.0051, dt))
    dzh = torch.stack([ops.gemm(zh[1], G), ops.gemm(zh[0], G, trans_b=True)])
    a, b = twice(lambda: ops.barlow_bwd_stats(dzh, zh, n))
    g = torch.ones(1, device="cuda")

    def bwd():
        dx, dy = ops.zeros(x2.shape, x2.device, dt), ops.zeros(y2.shape, y2.device, dt)
        ops.barlow_standardize_bwd(dzh, zh, rstd, a, b, ix, iy, dx, dy, g)
        return dx, dy
    twice(bwd)


def test_errors_and_the_single_pair():
    from pero_pretraining_amd.joint_embedding_pretraining.losses import BarlowTwinsLoss, VICRegLoss
    loss = BarlowTwinsLoss()
    rng = np.random.default_rng(2)
    x, y = cu(rng.standard_normal((2, 8, 16)).astype(np.float32)), cu(rng.standard_normal((2, 8, 16)).astype(np.float32))
    ones = np.ones((2, 8), np.uint8)
    short = ones.copy()
    short[0, 0] = 0
    with pytest.raises(RuntimeError) as e1:
        loss(x, y, ones, ones, ones, short)
    with pytest.raises(RuntimeError) as e2:
        VICRegLoss()(x, y, ones, ones, ones, short)
    assert str(e1.value) == str(e2.value) and "must match the size of tensor b (15)" in str(e1.value)
    with pytest.raises(ValueError):
        loss(x, y, ones, ones, 2 * ones, 2 * ones)
    one1, one2 = np.zeros((2, 8), np.uint8), np.zeros((2, 8), np.uint8)
    one1[0, 3], one2[1, 6] = 1, 1
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    res = loss(xg, yg, ones, ones, one1, one2)
    res["loss"].backward()
    assert float(res["loss"]) == 16.0 and float(res["loss.on_diagonal"]) == 16.0 and float(res["loss.off_diagonal"]) == 0.0
    assert float(xg.grad.abs().max()) == 0.0 and float(yg.grad.abs().max()) == 0.0


def test_model_step_with_barlow_loss_and_init_model():
    from pero_pretraining_amd.joint_embedding_pretraining import model as J
    from pero_pretraining_amd.joint_embedding_pretraining.losses import BarlowTwinsLoss
    from pero_pretraining_amd.joint_embedding_pretraining.train import init_model
    from pero_pretraining_amd.optim import FusedAdam
    torch.manual_seed(0)
    bb = {"num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128}
    hd = {"type": "linear", "in_features": 64, "out_features": 80}
    model = J.JointEmbeddingTransformerEncoder(J.init_backbone(dict(bb)), J.init_head(dict(hd)), BarlowTwinsLoss()).cuda().train()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    rng = np.random.default_rng(0)
    im1 = cu(rng.integers(0, 256, (2, 40, 128, 3), dtype=np.uint8))
    im2 = cu(rng.integers(0, 256, (2, 40, 128, 3), dtype=np.uint8))
    ones = torch.ones((2, 16), dtype=torch.uint8, device="cuda")
    before = model.head.linear.weight.detach().clone()
    opt.zero_grad()
    res = model(im1, im2, ones, ones, ones, ones)
    assert set(KEYS) <= set(res) and bool(torch.isfinite(res["loss"]))
    assert abs(float(res["loss"]) - (float(res["loss.on_diagonal"]) + 0.0051 * float(res["loss.off_diagonal"]))) <= 1e-5 * float(res["loss"])
    res["loss"].backward()
    opt.step()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert not torch.equal(before, model.head.linear.weight.detach())
    built = init_model(torch.device("cuda", 0), dict(bb, type="vit"), dict(hd), loss_type="barlow", barlow_lambda=0.02)
    assert isinstance(built.loss, BarlowTwinsLoss) and built.loss.lambda_offdiag == 0.02
    with pytest.raises(ValueError, match="Unknown loss type: nope"):
        init_model(torch.device("cuda", 0), dict(bb, type="vit"), dict(hd), loss_type="nope")
