"""GPU: FusedAdam's weight decay (coupled / decoupled), amsgrad, maximize and fused global-norm clip.  The kernels (csrc/optim.hip) are
held to the f64 restatement tests/optim_ref.py, which tests/test_optim_ref_cpu.py pins to torch; the optimizer and the Trainer to
torch.optim.Adam / AdamW + clip_grad_norm_ in f64.

Bounds.  p, m: 1e-6 and v, vmax: 2e-6 relative (the bounds of test_gpu_ops.py::test_adam_matches_oracle); 2e-6 absolute on parameters
against torch (test_gpu_next_rows.py's interchange test).  The norm: (chain + 2) * 2^-24 relative, where chain = ops.sumsq_chain(n) is
the longest run of f32 additions one partial sum goes through in the kernel's layout (every addition and the squaring contribute at
most one rounding of 2^-24 to a sum of positive terms; the root and the final rounding make the 2; the f64 finish adds nothing at this
scale).  A clipped gradient carries the norm's error once, so m widens by that bound and v (its square) by twice it."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import optim_ref as R  # noqa: E402

U = 2.0 ** -24
FLAGS = list(itertools.product([0.0, 0.05], [False, True], [False, True], [False, True]))   # wd, decoupled, amsgrad, maximize
BIG = 4096 * 1024 + 1027   # the smallest size at which the Adam grid (4096 workgroups x 1024 elements) walks a second stride, with a tail


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    return _ops


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def norm_bound(ops, *sizes):
    return (max(ops.sumsq_chain(n) for n in sizes) + 2) * U


def device_norm(ops, buffers, scale=1.0):
    counts = [ops.sumsq_num_partials(b.numel()) for b in buffers]
    work = torch.empty(sum(counts), device="cuda")
    out = torch.zeros(1, device="cuda")
    start = 0
    for b, c in zip(buffers, counts):
        ops.sumsq_partials(b, work[start:start + c])
        start += c
    ops.grad_norm_finish(work, scale, out)
    return out


@pytest.fixture(scope="module")
def adam_inputs():
    """The parameters and the four gradients of test_adam_matches_oracle (n = 10007: not a multiple of 4, the scalar tail runs)."""
    g = torch.Generator().manual_seed(6)
    n = 10007
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (0.1 if step % 2 else 10) for step in range(1, 5)]
    return p, grads, [g_.cuda() for g_ in grads]


def run_kernel_case(ops, adam_inputs, wd, decoupled, amsgrad, maximize, max_norm):
    """Four steps on the device and in the f64 restatement; returns the worst coefficient of the clip and the error ratios."""
    p, grads, dgrads = adam_inputs
    n = p.numel()
    pd, md, vd = p.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    xd = torch.zeros(n, device="cuda") if amsgrad else None
    pb = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    po, mo, vo = p.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    xo = torch.zeros(n, dtype=torch.float64) if amsgrad else None
    coefs = []
    for step in range(1, 5):
        norm64, dnorm = None, None
        if max_norm is not None:
            norm64 = R.global_norm([grads[step - 1]])
            coefs.append(R.clip_coefficient(norm64, max_norm))
            dnorm = device_norm(ops, [dgrads[step - 1]])
        R.adam_step_ex(po, grads[step - 1], mo, vo, xo, step, 1e-3 * step, weight_decay=wd, decoupled=decoupled, maximize=maximize,
                       grad_norm=norm64, max_norm=max_norm)
        ops.adam_step_ex(pd, dgrads[step - 1], md, vd, pb, 1e-3 * step, 0.9, 0.999, 1e-8, step, weight_decay=wd, decoupled=decoupled,
                         vmax=xd, maximize=maximize, grad_norm=dnorm, max_norm=max_norm or 0.0)
    errs = {"p": rel_err(pd, po), "m": rel_err(md, mo), "v": rel_err(vd, vo)}
    if amsgrad:
        errs["vmax"] = rel_err(xd, xo)
    assert torch.equal(pb.cpu(), pd.cpu().bfloat16())
    return coefs, errs


@pytest.mark.parametrize("wd,decoupled,amsgrad,maximize", FLAGS)
def test_kernel_matches_restatement(ops, adam_inputs, wd, decoupled, amsgrad, maximize):
    _, errs = run_kernel_case(ops, adam_inputs, wd, decoupled, amsgrad, maximize, None)
    print("errors", errs)
    assert errs["p"] < 1e-6 and errs["m"] < 1e-6 and errs["v"] < 2e-6
    assert errs.get("vmax", 0.0) < 2e-6


@pytest.mark.parametrize("max_norm,active", [(1.0, True), (1e6, False)])
@pytest.mark.parametrize("wd,decoupled,amsgrad,maximize", FLAGS)
def test_kernel_clips_by_the_device_norm(ops, adam_inputs, wd, decoupled, amsgrad, maximize, max_norm, active):
    """The clip reads the norm the two norm launches left on the device; the reference clips by the f64 norm."""
    coefs, errs = run_kernel_case(ops, adam_inputs, wd, decoupled, amsgrad, maximize, max_norm)
    print("coefficients", coefs, "errors", errs)
    assert all(c < 0.9 for c in coefs) if active else all(c == 1.0 for c in coefs)
    nb = norm_bound(ops, adam_inputs[0].numel())
    assert errs["p"] < 1e-6 and errs["m"] < 1e-6 + nb and errs["v"] < 2e-6 + 2 * nb
    assert errs.get("vmax", 0.0) < 2e-6 + 2 * nb


@pytest.mark.parametrize("n", [10007, BIG])
def test_defaults_are_the_bits_of_adam_step(ops, n):
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    p = torch.randn(n, device="cuda", generator=g)
    a = [p.clone(), torch.zeros_like(p), torch.zeros_like(p), torch.empty(n, device="cuda", dtype=torch.bfloat16)]
    b = [p.clone(), torch.zeros_like(p), torch.zeros_like(p), torch.empty(n, device="cuda", dtype=torch.bfloat16)]
    for step in range(1, 4):
        gr = torch.randn(n, device="cuda", generator=g) * (0.1 if step % 2 else 10)
        ops.adam_step(a[0], gr, a[1], a[2], a[3], 1e-3 * step, 0.9, 0.999, 1e-8, step, 0.5)
        ops.adam_step_ex(b[0], gr, b[1], b[2], b[3], 1e-3 * step, 0.9, 0.999, 1e-8, step, 0.5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a[3], a[0].bfloat16()) and float(a[2].min()) > 0


def _spread(n, seed):
    """Magnitudes from 1e-4 to 1e3, both signs."""
    g = torch.Generator().manual_seed(seed)
    x = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 7 - 4) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    return x.float()


@pytest.mark.parametrize("n", [1, 1027, 10007, BIG])
def test_global_norm(ops, n):
    one = [_spread(n, 1)]
    three = [_spread(n, 2), _spread(n // 2 + 3, 3), _spread(13, 4)]
    for bufs in (one, three):
        dev = [b.cuda() for b in bufs]
        want = R.global_norm(bufs)
        got = device_norm(ops, dev)
        bound = norm_bound(ops, *[b.numel() for b in bufs])
        err = abs(float(got.double()) - want) / want
        print(f"n {[b.numel() for b in bufs]}: relative error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        assert torch.equal(device_norm(ops, dev), got)                     # the same bits from call to call
        half = device_norm(ops, [b * 2 for b in dev], scale=0.5)           # the DataParallel form: a doubled sum, scale 1 / world
        assert abs(float(half) - float(got)) <= float(np.spacing(np.float32(float(got))))
        assert abs(float(device_norm(ops, dev, scale=0.25).double()) - 0.25 * want) <= bound * 0.25 * want


# ---- the optimizer against torch ---------------------------------------------------------------------------------------
SHAPES = [(24, 32), (24,), (7, 5, 3), (1,), (64, 64)]


def _grads_like(params, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(p.shape, device="cuda", generator=gen) * 0.1 for p in params]


def _two_groups(params, wd):
    return [{"params": [p for p in params if p.dim() >= 2], "weight_decay": wd}, {"params": [p for p in params if p.dim() < 2], "weight_decay": 0.0}]


def _feed(opt, mine, theirs, grads, dtype=None):
    opt.zero_grad()
    for p, q, g in zip(mine, theirs, grads):
        p.grad.copy_(g)
        q.grad = g.clone().to(dtype or q.dtype)


@pytest.mark.parametrize("kind", ["adamw", "adam_coupled_amsgrad_maximize"])
def test_optimizer_matches_torch_with_two_groups_and_clip(ops, kind):
    from pero_pretraining_amd.optim import FusedAdam, FusedAdamW
    torch.manual_seed(0)
    mine = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in SHAPES]
    theirs = [torch.nn.Parameter(p.detach().double()) for p in mine]    # torch in f64: the comparison measures this optimizer's error alone
    max_norm = 1.0
    if kind == "adamw":
        fa = FusedAdamW(_two_groups(mine, 0.05), lr=3e-3, max_grad_norm=max_norm)
        ta = torch.optim.AdamW(_two_groups(theirs, 0.05), lr=3e-3)
        assert fa.param_groups[0]["decoupled_weight_decay"] and fa.defaults["weight_decay"] == 1e-2
    else:
        fa = FusedAdam(_two_groups(mine, 0.05), lr=3e-3, amsgrad=True, maximize=True, max_grad_norm=max_norm)
        ta = torch.optim.Adam(_two_groups(theirs, 0.05), lr=3e-3, amsgrad=True, maximize=True)
    assert [g["weight_decay"] for g in fa.param_groups] == [0.05, 0.0]
    sizes = [f["g"].numel() for f in fa._flat]
    for step in range(4):
        grads = _grads_like(mine, step)
        _feed(fa, mine, theirs, grads)
        want = float(torch.nn.utils.clip_grad_norm_(theirs, max_norm))
        fa.step(); ta.step()
        got = float(fa.grad_norm.double())
        assert got > max_norm                                           # the clip is active
        assert abs(got - want) <= norm_bound(ops, *sizes) * want
        for p, g in zip(mine, grads):
            assert torch.equal(p.grad, g)                               # .grad stays unscaled (unlike clip_grad_norm_)
        worst = max(float((p.detach().double() - q.detach()).abs().max()) for p, q in zip(mine, theirs))
        print(f"{kind} step {step}: norm {got:.6f} (torch {want:.6f}), worst parameter difference {worst:.3e}")
        assert worst < 2e-6


def test_amsgrad_state_dict_interchanges_with_torch_adam():
    """An amsgrad state moves FusedAdam -> torch.optim.Adam -> FusedAdam and continues (max_exp_avg_sq per parameter, real group keys)."""
    from pero_pretraining_amd.optim import FusedAdam
    torch.manual_seed(0)
    shapes = SHAPES[:4]
    mine = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    fa = FusedAdam(_two_groups(mine, 0.05), lr=3e-3, amsgrad=True, max_grad_norm=None)
    ta = torch.optim.Adam(_two_groups(theirs, 0.0), lr=1.0)
    assert fa.state_dict()["state"] == {}
    for step in range(2):
        _feed(fa, mine, theirs, [g * (10.0 if step == 0 else 1.0) for g in _grads_like(mine, step)])   # a shrinking v: vmax differs from v
        fa.step()
    sd = fa.state_dict()
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"} for st in sd["state"].values()) and len(sd["state"]) == 4
    assert [(g["weight_decay"], g["amsgrad"], g["maximize"], g["decoupled_weight_decay"]) for g in sd["param_groups"]] == \
        [(0.05, True, False, False), (0.0, True, False, False)]
    assert any(bool((st["max_exp_avg_sq"] > st["exp_avg_sq"]).any()) for st in sd["state"].values())
    for p, q in zip(mine, theirs):
        q.data.copy_(p.data)
    ta.load_state_dict(sd)                                               # FusedAdam -> torch.optim.Adam
    assert ta.param_groups[0]["amsgrad"] and ta.param_groups[0]["weight_decay"] == 0.05 and ta.param_groups[0]["lr"] == 3e-3
    for step in range(2, 4):
        _feed(fa, mine, theirs, _grads_like(mine, step))
        fa.step(); ta.step()
    for p, q in zip(mine, theirs):
        assert (p - q).abs().max() < 2e-6
    fresh = [torch.nn.Parameter(q.detach().clone()) for q in theirs]
    fb = FusedAdam(_two_groups(fresh, 0.0), lr=1.0)
    fb.load_state_dict(ta.state_dict())                                  # torch.optim.Adam -> FusedAdam
    assert fb.param_groups[0]["lr"] == 3e-3 and fb.param_groups[0]["amsgrad"] and fb.param_groups[0]["weight_decay"] == 0.05
    assert fb._flat[0]["step"] == 4 and fb._flat[1]["step"] == 4
    _feed(fb, fresh, theirs, _grads_like(mine, 9))
    fb.step(); ta.step()
    for p, q in zip(fresh, theirs):
        assert (p - q).abs().max() < 2e-6
    tw = torch.optim.AdamW([torch.nn.Parameter(q.detach().clone()) for q in theirs], lr=1.0)   # and AdamW takes a FusedAdamW state
    from pero_pretraining_amd.optim import FusedAdamW
    fw = FusedAdamW([torch.nn.Parameter(q.detach().clone()) for q in theirs], lr=2e-3, max_grad_norm=0.5)
    tw.load_state_dict(fw.state_dict())
    assert tw.param_groups[0]["decoupled_weight_decay"] and tw.param_groups[0]["weight_decay"] == 1e-2 and tw.param_groups[0]["max_grad_norm"] == 0.5


def test_grad_scale_is_the_data_parallel_contract(ops):
    """grad_scale = 0.5 on a doubled flat gradient (two ranks' sum) steps like grad_scale = 1 on the gradient itself, the clip included."""
    from pero_pretraining_amd.optim import FusedAdamW
    torch.manual_seed(1)
    base = [torch.randn(s, device="cuda") for s in SHAPES]
    runs = []
    for scale in (0.5, 1.0):
        params = [torch.nn.Parameter(b.clone()) for b in base]
        opt = FusedAdamW(_two_groups(params, 0.05), lr=3e-3, max_grad_norm=1.0)
        opt.grad_scale = scale
        norms = []
        for step in range(3):
            opt.zero_grad()
            for p, g in zip(params, _grads_like(params, step)):
                p.grad.copy_(g)
            for flat in opt.flat_grads().values():
                flat.mul_(1.0 / scale)
            opt.step()
            norms.append(float(opt.grad_norm))
        assert all(nrm > 1.0 for nrm in norms)
        runs.append((params, norms))
    for p, q in zip(runs[0][0], runs[1][0]):
        assert rel_err(p, q) < 1e-6
    for a, b in zip(runs[0][1], runs[1][1]):
        assert abs(a - b) <= 1.2e-7 * b


# ---- constructor behaviour -----------------------------------------------------------------------------------------------
def test_constructor_takes_torch_adams_arguments():
    from pero_pretraining_amd.optim import FusedAdam, FusedAdamW
    p = [torch.nn.Parameter(torch.randn(8, 8, device="cuda"))]
    opt = FusedAdam(p, weight_decay=0.1)                                 # raised ValueError before
    assert opt.param_groups[0]["weight_decay"] == 0.1 and not opt.param_groups[0]["decoupled_weight_decay"]
    opt = FusedAdam([torch.nn.Parameter(torch.randn(8, device="cuda"))], amsgrad=True, maximize=True, decoupled_weight_decay=True, max_grad_norm=2.0)
    g = opt.param_groups[0]
    assert g["amsgrad"] and g["maximize"] and g["decoupled_weight_decay"] and g["max_grad_norm"] == 2.0 and opt._flat[0]["vmax"] is not None
    assert issubclass(FusedAdamW, FusedAdam)
    with pytest.raises(ValueError):
        FusedAdam([torch.nn.Parameter(torch.randn(8, device="cuda"))], weight_decay=-1.0)


def test_defaults_step_exactly_as_before(ops):
    """FusedAdam with every new argument at its default: three steps give the bits of the launch it made before (pero_adam_step over the
    same flat buffers)."""
    from pero_pretraining_amd.optim import FusedAdam
    torch.manual_seed(2)
    base = [torch.randn(s, device="cuda") for s in SHAPES]
    new = [torch.nn.Parameter(b.clone()) for b in base]
    old = [torch.nn.Parameter(b.clone()) for b in base]
    explicit = [torch.nn.Parameter(b.clone()) for b in base]
    fn, fo = FusedAdam(new, lr=2e-3), FusedAdam(old, lr=2e-3)
    fe = FusedAdam(explicit, lr=2e-3, weight_decay=0, amsgrad=False, maximize=False, decoupled_weight_decay=False, max_grad_norm=None)
    for step in range(3):
        grads = _grads_like(new, step)
        for opt, params in ((fn, new), (fo, old), (fe, explicit)):
            opt.zero_grad()
            for p, g in zip(params, grads):
                p.grad.copy_(g)
        fn.step(); fe.step()
        f = fo._flat[0]
        f["step"] += 1
        ops.adam_step(f["p"], f["g"], f["m"], f["v"], f["lp"], 2e-3, 0.9, 0.999, 1e-8, f["step"], 1.0)
    assert fn.grad_norm is None and fn._flat[0]["vmax"] is None
    for a, b, c in zip(new, old, explicit):
        assert torch.equal(a, b) and torch.equal(a, c)
    for k in ("p", "m", "v", "lp"):
        assert torch.equal(fn._flat[0][k], fo._flat[0][k])


def test_clip_over_groups_on_two_devices_is_refused():
    from pero_pretraining_amd.optim import FusedAdam

    class Elsewhere:   # stands in for a flat gradient buffer on a second GPU
        device = torch.device("cuda", 1)

        def numel(self):
            return 8

    params = [torch.nn.Parameter(torch.randn(4, 4, device="cuda")), torch.nn.Parameter(torch.randn(4, device="cuda"))]
    opt = FusedAdam(_two_groups(params, 0.1), max_grad_norm=1.0)
    opt.zero_grad()
    opt._flat[1] = dict(opt._flat[1], g=Elsewhere())
    with pytest.raises(RuntimeError, match="one device"):
        opt._global_norm()


# ---- through the Trainer ---------------------------------------------------------------------------------------------------
BB32 = {"type": "vit", "num_blocks": 2, "model_dim": 32, "num_heads": 4, "feedforward_dim": 64}
HD32 = {"type": "linear", "in_features": 32, "out_features": 24}
WD, MAX_NORM = 0.05, 0.05


def _batches():
    rng = np.random.default_rng(5)   # the batches of test_resume_continues_the_trajectory
    return [{"images": rng.integers(0, 256, (2, 40, 64, 3), dtype=np.uint8), "labels": rng.integers(0, 24, (2, 8))} for _ in range(6)]


def _make_trainer(seed, data, ckpts, bfloat16=False, testers=None):
    from pero_pretraining_amd.masked_pretraining import train as T
    torch.manual_seed(seed)
    model = T.init_model(torch.device("cuda"), dict(BB32), dict(HD32))
    bop = T.init_batch_operator(torch.device("cuda"), 0.4)
    trn_t, tst_t = T.init_testers(bop, model, testers, testers) if testers is not None else (None, None)
    trainer = T.init_training(bop, model, data, trn_t, tst_t, 2e-3, 4, ckpts, bfloat16=bfloat16, weight_decay=WD, max_grad_norm=MAX_NORM)
    return trainer, model


@pytest.mark.parametrize("bfloat16", [False, True])
def test_trainer_steps_match_torch_adamw_with_clip(ops, tmp_path, bfloat16):
    """init_training(weight_decay, max_grad_norm): before each optimizer step the parameters and gradients go to f64 CPU clones, torch's
    AdamW over the same two groups + clip_grad_norm_ takes the step there, and the f32 (master) weights agree afterwards; in bf16 mode the
    bf16 and transposed bf16 copies the kernels read are the rounded masters, bit for bit."""
    from pero_pretraining_amd import lowp
    from pero_pretraining_amd.optim import FusedAdamW
    np.random.seed(3)
    trainer, model = _make_trainer(1, None, str(tmp_path), bfloat16=bfloat16)
    opt = trainer.optimizer
    assert isinstance(opt, FusedAdamW) and len(opt.param_groups) == 2
    assert [g["weight_decay"] for g in opt.param_groups] == [WD, 0.0] and all(g["max_grad_norm"] == MAX_NORM for g in opt.param_groups)
    assert all(p.dim() >= 2 for p in opt.param_groups[0]["params"]) and all(p.dim() < 2 for p in opt.param_groups[1]["params"])
    assert [id(p) for g in opt.param_groups for p in g["params"]] == \
        [id(p) for p in model.parameters() if p.dim() >= 2] + [id(p) for p in model.parameters() if p.dim() < 2]
    clones = [[torch.nn.Parameter(p.detach().double().cpu()) for p in g["params"]] for g in opt.param_groups]
    ta = torch.optim.AdamW([{"params": c, "weight_decay": g["weight_decay"]} for c, g in zip(clones, opt.param_groups)], lr=2e-3)
    fused_step, seen = opt.step, []

    def checked_step():
        for group, cl, tg in zip(opt.param_groups, clones, ta.param_groups):
            tg["lr"] = group["lr"]
            for p, q in zip(group["params"], cl):
                q.data.copy_(p.detach().double().cpu())
                q.grad = p.grad.detach().double().cpu()
        want = float(torch.nn.utils.clip_grad_norm_([q for cl in clones for q in cl], MAX_NORM))
        ta.step()
        fused_step()
        got = float(opt.grad_norm)
        worst = max(float((p.detach().double().cpu() - q.detach()).abs().max()) for g, cl in zip(opt.param_groups, clones) for p, q in zip(g["params"], cl))
        print(f"bf16 {bfloat16}: norm {got:.6f} (torch {want:.6f}), worst parameter difference {worst:.3e}")
        assert got > MAX_NORM and abs(got - want) <= norm_bound(ops, *[f["g"].numel() for f in opt._flat]) * want
        assert worst < 2e-6
        seen.append(got)

    opt.step = checked_step
    for i, batch in enumerate(_batches()[:3]):
        trainer.scheduler.update_learning_rate(i + 1)   # warm-up over 4 iterations: three different rates, none zero
        loss = trainer.train_step(batch)
        assert math.isfinite(float(loss))
    assert len(seen) == 3
    for p in model.parameters():
        assert torch.equal(lowp.get(p), p.detach().bfloat16())
        if p.dim() >= 2:
            assert torch.equal(lowp.weight_t(p), p.detach().bfloat16().view(p.shape[0], -1).t())
    for f in opt._flat:
        assert torch.equal(f["lp"], f["p"].bfloat16())


def test_hip_graph_steps_equal_eager_steps_with_decay_and_clip(tmp_path):
    """The same three steps under Trainer(hip_graph=True) (the optimizer's launches, the norm's included, stay outside the captured
    graph) against the eager Trainer, held to what test_gpu_model.py::test_hip_graph_step_equals_eager_step holds the plain optimizer
    to: losses to 1e-5 relative, weights to 1e-4 (the step's f32 atomics are not ordered), the rounding-noise key-bias slice left out."""
    from pero_pretraining_amd.masked_pretraining.trainer import Trainer
    runs = {}
    for name, flag in (("eager", False), ("graph", True)):
        np.random.seed(3)
        built, model = _make_trainer(1, None, str(tmp_path), bfloat16=True)
        model.eval()   # no offset draws: both runs see the same inputs
        trainer = Trainer(built.batch_operator, model, None, built.optimizer, built.scheduler, bfloat16=True, hip_graph=flag)
        losses, norms = [], []
        for i, batch in enumerate(_batches()[:3]):
            trainer.scheduler.update_learning_rate(i + 1)
            losses.append(float(trainer.train_step(batch)))
            norms.append(float(trainer.optimizer.grad_norm))
        torch.cuda.synchronize()
        if flag:
            assert len(trainer._graphs) == 1
        runs[name] = (losses, norms, {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()})
    print("losses", runs["eager"][0], runs["graph"][0], "norms", runs["eager"][1], runs["graph"][1])
    for a, b in zip(runs["eager"][0], runs["graph"][0]):
        assert np.isfinite(a) and abs(a - b) <= 1e-5 * abs(a)
    for a, b in zip(runs["eager"][1], runs["graph"][1]):
        assert a > MAX_NORM and abs(a - b) <= 1e-4 * a
    for k, v in runs["eager"][2].items():
        w = runs["graph"][2][k]
        if k.endswith("in_proj_bias"):
            d = v.shape[0] // 3
            v, w = np.delete(v, np.s_[d:2 * d]), np.delete(w, np.s_[d:2 * d])
        assert np.abs(v - w).max() <= 1e-4, k


def test_resume_continues_the_trajectory_with_decay_and_clip(golden, tmp_path):
    """Save, resume, step on: the training-state file carries both groups' moments and keys, and the resumed run ends where the
    uninterrupted one does (the bound of test_gpu_next_rows.py::test_resume_continues_the_trajectory)."""
    from pero_pretraining_amd.masked_pretraining import train as T
    g = golden("g12_tester.npz")
    tst = [{"images": g["b2.images"], "labels": g["b2.labels"]}]
    batches, ckpts = _batches(), str(tmp_path)
    np.random.seed(3); torch.manual_seed(3)
    trainer, model = _make_trainer(1, batches, ckpts, testers=tst)
    trainer.train(end_iteration=4, start_iteration=0, view_step=3)
    want = {k: v.clone() for k, v in model.state_dict().items()}
    assert os.path.exists(T.get_training_state_path(ckpts, 3))
    saved = torch.load(T.get_training_state_path(ckpts, 3), map_location="cpu", weights_only=True)["optimizer"]
    assert [(gr["weight_decay"], gr["decoupled_weight_decay"], gr["max_grad_norm"]) for gr in saved["param_groups"]] == [(WD, True, MAX_NORM), (0.0, True, MAX_NORM)]
    np.random.seed(1234); torch.manual_seed(1234)
    trainer2, model2 = _make_trainer(2, batches[4:], ckpts, testers=tst)
    start = T.resume(trainer2, ckpts, 3)
    assert start == 4 and [f["step"] for f in trainer2.optimizer._flat] == [4, 4]
    trainer2.train(end_iteration=4, start_iteration=start, view_step=1000)
    for k, v in model2.state_dict().items():
        assert (v - want[k]).abs().max() <= 1e-5 * max(1.0, float(want[k].abs().max())), k
