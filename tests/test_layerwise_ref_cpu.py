"""CPU: the f64 restatement of the layer-wise optimizers (tests/layerwise_ref.py) is torch.optim.AdamW / torch.optim.SGD in f64 when
the adaptation is off, gives the trust ratios worked out by hand when it is on, and 1 in the degenerate cases; ops.layer_table's tile
arithmetic; constructor validation; layerwise_groups; the new C-ABI entries refuse bad arguments on the host."""
import math

import pytest
import torch

import layerwise_ref as L

SHAPES = [(7, 5), (11,), (3, 4, 2)]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("maximize", [False, True])
def test_lamb_without_adaptation_is_adamw_in_f64(maximize):
    """r = 1: p - lr (mhat / denom + wd p) = p (1 - lr wd) - lr mhat / denom, AdamW's step with sqrt(v / bc2) = sqrt(v) / sqrt(bc2)."""
    gen = torch.Generator().manual_seed(3)
    mine = [torch.randn(s, generator=gen, dtype=torch.float64) for s in SHAPES]
    theirs = [torch.nn.Parameter(p.clone()) for p in mine]
    opt = torch.optim.AdamW(theirs, lr=1e-3, eps=1e-6, weight_decay=0.05, maximize=maximize)
    ms, vs = [torch.zeros_like(p) for p in mine], [torch.zeros_like(p) for p in mine]
    for step in range(1, 4):
        lr = 1e-3 * step
        opt.param_groups[0]["lr"] = lr
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * (10.0 if step % 2 else 0.01) for s in SHAPES]
        for q, g in zip(theirs, grads):
            q.grad = g.clone()
        opt.step()
        stats = L.lamb_step(mine, grads, ms, vs, step, lr, eps=1e-6, weight_decay=0.05, maximize=maximize, layer_adaptation=False)
        assert all(r == 1.0 for _, _, r in stats)
    worst = max(_rel(p, q.detach()) for p, q in zip(mine, theirs))
    print(f"worst relative |restatement - AdamW| = {worst:.3e}")
    assert worst <= 1e-12
    for q, m, v in zip(theirs, ms, vs):
        assert _rel(m, opt.state[q]["exp_avg"]) <= 1e-12 and _rel(v, opt.state[q]["exp_avg_sq"]) <= 1e-12


@pytest.mark.parametrize("wd,maximize", [(0.0, False), (0.05, False), (0.05, True)])
def test_lars_without_adaptation_is_sgd_in_f64(wd, maximize):
    gen = torch.Generator().manual_seed(4)
    mine = [torch.randn(s, generator=gen, dtype=torch.float64) for s in SHAPES]
    theirs = [torch.nn.Parameter(p.clone()) for p in mine]
    opt = torch.optim.SGD(theirs, lr=0.1, momentum=0.9, weight_decay=wd, maximize=maximize)
    bufs = [torch.zeros_like(p) for p in mine]
    for step in range(1, 4):
        lr = 0.1 * step
        opt.param_groups[0]["lr"] = lr
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) for s in SHAPES]
        for q, g in zip(theirs, grads):
            q.grad = g.clone()
        opt.step()
        stats = L.lars_step(mine, grads, bufs, lr, momentum=0.9, weight_decay=wd, maximize=maximize, layer_adaptation=False)
        assert all(r == 1.0 for _, _, r in stats)
    worst = max(_rel(p, q.detach()) for p, q in zip(mine, theirs))
    print(f"worst relative |restatement - SGD| = {worst:.3e}")
    assert worst <= 1e-12
    for q, b in zip(theirs, bufs):
        assert _rel(b, opt.state[q]["momentum_buffer"]) <= 1e-12


def test_two_tensor_example_by_hand():
    """p0 = (3, 4), |p0| = 5; p1 = (0, 0, 2), |p1| = 2.  LARS, wd = 0, mu = 0: the step is lr c |p| g / |g|, whatever |g| is."""
    p = [torch.tensor([3.0, 4.0], dtype=torch.float64), torch.tensor([0.0, 0.0, 2.0], dtype=torch.float64)]
    g = [torch.tensor([0.6, 0.8], dtype=torch.float64), torch.tensor([2.0, 0.0, 0.0], dtype=torch.float64)]   # |g0| = 1, |g1| = 2
    lr, c = 0.5, 0.1
    q = [x.clone() for x in p]
    stats = L.lars_step(q, g, [torch.zeros_like(x) for x in p], lr, momentum=0.0, weight_decay=0.0, trust_coefficient=c)
    assert stats[0] == pytest.approx((5.0, 1.0, 0.5), rel=1e-14) and stats[1] == pytest.approx((2.0, 2.0, 0.1), rel=1e-14)
    assert torch.allclose(q[0], torch.tensor([3.0 - 0.5 * 0.5 * 0.6, 4.0 - 0.5 * 0.5 * 0.8], dtype=torch.float64), rtol=1e-15, atol=0)
    assert torch.allclose(q[1], torch.tensor([-0.5 * 0.1 * 2.0, 0.0, 2.0], dtype=torch.float64), rtol=1e-15, atol=0)   # lr c |p| g / |g| = 0.1 e0
    for x, y, gg in zip(q, p, g):
        assert torch.allclose(y - x, lr * c * y.norm() * gg / gg.norm(), rtol=1e-14, atol=0)
    # the gradient of tensor 0 a thousand times larger: the same step, and tensor 1 is untouched by it
    q2 = [x.clone() for x in p]
    stats2 = L.lars_step(q2, [g[0] * 1e3, g[1]], [torch.zeros_like(x) for x in p], lr, momentum=0.0, weight_decay=0.0, trust_coefficient=c)
    assert stats2[0][2] == pytest.approx(0.5e-3, rel=1e-14)
    assert torch.allclose(q2[0], q[0], rtol=1e-14, atol=0) and torch.equal(q2[1], q[1])
    # LAMB at step 1 with eps = 0, wd = 0: mhat / sqrt(vhat) = sign(g), so |u| = sqrt(non-zero entries) and the step is lr |p| / |u| sign(g)
    q3 = [x.clone() for x in p]
    stats3 = L.lamb_step(q3, g, [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p], 1, lr, eps=1e-300, weight_decay=0.0)
    assert stats3[0][1] == pytest.approx(math.sqrt(2.0), rel=1e-12) and stats3[0][2] == pytest.approx(5.0 / math.sqrt(2.0), rel=1e-12)
    assert stats3[1][1] == pytest.approx(1.0, rel=1e-12) and stats3[1][2] == pytest.approx(2.0, rel=1e-12)
    assert torch.allclose(q3[0], p[0] - lr * 5.0 / math.sqrt(2.0), rtol=1e-12, atol=0)
    assert torch.allclose(q3[1], torch.tensor([-1.0, 0.0, 2.0], dtype=torch.float64), rtol=1e-12, atol=1e-300)


def test_degenerate_norms_give_ratio_one():
    z, one = torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    # |p| = 0 with a gradient: r = 1, a plain step
    p = [z.clone()]
    assert L.lars_step(p, [one], [z.clone()], 0.1, momentum=0.0)[0] == (0.0, 2.0, 1.0) and torch.equal(p[0], -0.1 * one)
    p = [z.clone()]
    st = L.lamb_step(p, [one], [z.clone()], [z.clone()], 1, 0.1, weight_decay=0.0)[0]
    assert st[0] == 0.0 and st[2] == 1.0 and float(p[0].abs().max()) > 0
    # |u| = 0: a zero gradient with wd = 0 at step 1 - r = 1 and p keeps its value
    p = [one.clone()]
    assert L.lars_step(p, [z], [z.clone()], 0.1)[0] == (2.0, 0.0, 1.0) and torch.equal(p[0], one)
    p = [one.clone()]
    assert L.lamb_step(p, [z], [z.clone()], [z.clone()], 1, 0.1, weight_decay=0.0)[0] == (2.0, 0.0, 1.0) and torch.equal(p[0], one)
    # a NaN norm fails both comparisons
    assert L.trust_ratio(float("nan"), 1.0, 1.0, True) == 1.0 and L.trust_ratio(1.0, float("nan"), 1.0, True) == 1.0
    assert L.trust_ratio(2.0, 4.0, 0.5, True) == 0.25 and L.trust_ratio(2.0, 4.0, 0.5, False) == 1.0


def test_layer_table_tile_arithmetic():
    from pero_pretraining_amd import _lib, ops
    assert ops.LAYER_TILE == _lib.DEFINES["PERO_LAYER_TILE"] == 4096 and ops.layer_chain() == 15
    sizes = [1, 7, 8, 4095, 4096, 4097, 3 * 4096 + 5]
    assert [ops.layer_tiles(n) for n in sizes] == [1, 1, 1, 1, 1, 2, 4]
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 7) // 8 * 8
    table, tiles = ops.layer_table(list(zip(offs, sizes)), "cpu")
    assert table.dtype == torch.int64 and table.shape == (7, 3) and tiles == 11
    assert table._pero_extent == offs[-1] + sizes[-1]       # what the wrappers hold the flat buffers' lengths to
    assert table[:, 0].tolist() == offs and table[:, 1].tolist() == sizes and table[:, 2].tolist() == [0, 1, 2, 3, 4, 5, 7]
    # tiles start at the tensor: a tensor alone has the layout it has among the others
    alone, t1 = ops.layer_table([(0, 3 * 4096 + 5)], "cpu")
    assert alone.tolist() == [[0, 3 * 4096 + 5, 0]] and t1 == 4
    for bad in ([(4, 8)], [(0, 0)], []):
        with pytest.raises(ValueError):
            ops.layer_table(bad, "cpu")


def test_constructor_validation():
    from pero_pretraining_amd.optim import FusedAdam, FusedLAMB, FusedLARS
    assert issubclass(FusedLAMB, FusedAdam) and issubclass(FusedLARS, FusedAdam)
    p = [torch.nn.Parameter(torch.zeros(4, 4))]
    with pytest.raises(ValueError, match="amsgrad"):
        FusedLAMB(p, amsgrad=True)
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-0.1), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            FusedLAMB(p, **kw)
    with pytest.raises(TypeError):
        FusedLARS(p)   # lr is required, as in torch.optim.SGD
    for kw in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-0.1), dict(lr=0.1, trust_coefficient=-1.0),
               dict(lr=0.1, max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            FusedLARS(p, **kw)
    for make in (lambda: FusedLAMB(p), lambda: FusedLARS(p, 0.1)):   # valid arguments: the flat buffers live on the GPU, nowhere else
        with pytest.raises(RuntimeError, match="GPU"):
            make()


def test_layerwise_groups():
    from pero_pretraining_amd.optim import decay_groups, layerwise_groups
    model = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3), torch.nn.Conv1d(3, 2, 3), torch.nn.BatchNorm1d(2))
    groups, plain = layerwise_groups(model, 0.05), decay_groups(model, 0.05)
    assert [(g["weight_decay"], g["layer_adaptation"]) for g in groups] == [(0.05, True), (0.0, False)]
    assert [[id(p) for p in g["params"]] for g in groups] == [[id(p) for p in g["params"]] for g in plain]
    assert all(p.dim() >= 2 for p in groups[0]["params"]) and all(p.dim() < 2 for p in groups[1]["params"])
    torch.optim.SGD(groups, lr=0.1)   # the same groups feed torch's optimizer (it keeps the unknown key)


def test_layerwise_entries_validate_arguments_without_gpu():
    import ctypes
    from pero_pretraining_amd import _lib
    lib = _lib.lib()
    E = _lib.DEFINES["PERO_E_INVALID"]
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    a = ctypes.c_void_p(base + (-base) % 16)
    off = ctypes.c_void_p(a.value + 4)          # 4-byte aligned only
    tab = (ctypes.c_int64 * 3)(0, 8, 0)
    lamb1 = lambda p=a, g=a, m=a, v=a, t=tab, n=1, tiles=1, part=a, step=1, maxi=0, gn=None, mx=0.0: lib.pero_lamb_stage1(  # noqa: E731
        p, g, m, v, t, n, tiles, part, 0.9, 0.999, step, 1e-6, 1.0, 0.01, maxi, gn, mx, None)
    lamb2 = lambda p=a, m=a, v=a, pb=None, t=tab, n=1, tiles=1, st=a, step=1: lib.pero_lamb_stage2(  # noqa: E731
        p, m, v, pb, t, n, tiles, st, 1e-3, 0.9, 0.999, step, 1e-6, 0.01, None)
    lars1 = lambda p=a, g=a, t=tab, n=1, tiles=1, part=a, maxi=0, gn=None, mx=0.0: lib.pero_lars_stage1(  # noqa: E731
        p, g, t, n, tiles, part, 1.0, 0.0, maxi, gn, mx, None)
    lars2 = lambda p=a, g=a, b=a, pb=None, t=tab, n=1, tiles=1, st=a, maxi=0, gn=None, mx=0.0: lib.pero_lars_stage2(  # noqa: E731
        p, g, b, pb, t, n, tiles, st, 0.1, 0.9, 1.0, 0.0, maxi, gn, mx, None)
    fin = lambda part=a, t=tab, n=1, adapt=1, st=a: lib.pero_layer_ratio_finish(part, t, n, 1.0, adapt, st, None)  # noqa: E731
    cases = {
        "pero_lamb_stage1": [lambda: lamb1(p=None), lambda: lamb1(t=None), lambda: lamb1(part=None), lambda: lamb1(m=off), lambda: lamb1(step=0),
                             lambda: lamb1(maxi=2), lambda: lamb1(gn=a, mx=-1.0), lambda: lamb1(n=0), lambda: lamb1(tiles=0),
                             lambda: lamb1(tiles=1 << 31), lambda: lamb1(n=2, tiles=1)],
        "pero_lamb_stage2": [lambda: lamb2(p=None), lambda: lamb2(st=None), lambda: lamb2(v=off), lambda: lamb2(pb=off), lambda: lamb2(step=0),
                             lambda: lamb2(tiles=1 << 31)],
        "pero_lars_stage1": [lambda: lars1(g=None), lambda: lars1(t=None), lambda: lars1(p=off), lambda: lars1(maxi=-1), lambda: lars1(gn=a, mx=-1.0),
                             lambda: lars1(tiles=1 << 31)],
        "pero_lars_stage2": [lambda: lars2(b=None), lambda: lars2(st=None), lambda: lars2(b=off), lambda: lars2(pb=off), lambda: lars2(maxi=2),
                             lambda: lars2(tiles=0)],
        "pero_layer_ratio_finish": [lambda: fin(part=None), lambda: fin(t=None), lambda: fin(st=None), lambda: fin(n=0), lambda: fin(n=1 << 31),
                                    lambda: fin(adapt=2)],
    }
    for name, calls in cases.items():
        for i, c in enumerate(calls):
            assert c() == E, (name, i)
            assert name.encode() in lib.pero_last_error(), (name, i)
