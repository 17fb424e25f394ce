"""GPU: FusedLAMB / FusedLARS and their kernels (csrc/optim_layerwise.hip) against the f64 restatement tests/layerwise_ref.py, which
tests/test_layerwise_ref_cpu.py pins to torch and to ratios worked out by hand.

Bounds (U = 2^-24), as the issue sets them.  They start from tests/test_gpu_optim.py's: p, m (and LARS's momentum buffer) 1e-6, v 2e-6,
relative to the largest magnitude; a clipped gradient carries the global norm's error nb = norm_bound (there) once, so m widens by nb
and v by 2 nb.  They are widened by the derived bound of the tile sums and by nothing else:
  * a tile partial goes through chain = ops.layer_chain() f32 additions (the lane's four pieces, the fold, the butterfly, the waves)
    and one squaring, each at most one rounding of a sum of positive terms; the f64 finish adds nothing at this scale; the root and the
    rounding to f32 make 2: tile = (chain + 2) U = 1.01e-6 bounds |p| and |u|; under a clip |u| scales with the coefficient and
    carries nb as m does;
  * the ratio r = c |p| / |u| carries that bound for both norms and its own two roundings: rb = bound(|p|) + bound(|u|) + 2 U;
  * the step lr r u is smaller than p, so p widens by rb, and so does LARS's buffer (r u summed with momentum).
That is 1.0e-6 for the norms, 2.1e-6 for r and 3.1e-6 for p without a clip.  The bounds of u's roundings are relative to its two
terms (the quotient, LARS: g', and weight_decay * p), so the inputs are chosen not to cancel: kappa = | |term 1| + |term 2| | / |u|,
taken from the restatement (its `terms`), is asserted to stay below 2 for every tensor, and the one-element tensor, where a random draw
cancels almost completely now and then, has hand-picked values (gradients of one sign, a decay term a tenth of the gradient).
Every test prints the measured error beside its bound."""
import itertools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import layerwise_ref as L  # noqa: E402
import optim_ref as R  # noqa: E402

U = 2.0 ** -24
KAPPA_MAX = 2.0
SIZES = [1, 7, 8, 4095, 4096, 4097, 2 * 4096, 3 * 4096 + 5]   # a short tile, an exact tile, one element over, many tiles: ~37 k in all
E_P, E_M, E_V = 1e-6, 1e-6, 2e-6
MAX_NORM = 1.0


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    return _ops


def bounds(ops, kind, nb):
    """The docstring's bounds; nb = the bound of the clip's global norm (0 without a clip)."""
    tile = (ops.layer_chain() + 2) * U
    b_pn, b_un = tile, tile + nb
    rb = b_pn + b_un + 2 * U
    return {"p": E_P + rb, "m": E_M + nb, "v": E_V + 2 * nb, "buf": E_M + nb + rb, "pn": b_pn, "un": b_un, "r": rb}


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def offsets_of(sizes):
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 7) // 8 * 8
    return offs, total


class Flat:
    """The flat device buffers of one group over tensors of `sizes`, filled from lists of CPU f32 tensors."""

    def __init__(self, ops, sizes, params):
        self.ops, self.sizes = ops, sizes
        self.offs, self.total = offsets_of(sizes)
        z = lambda: torch.zeros(self.total, device="cuda")  # noqa: E731
        self.p, self.g, self.m, self.v = z(), z(), z(), z()
        self.lp = torch.zeros(self.total, device="cuda", dtype=torch.bfloat16)
        self.table, self.tiles = ops.layer_table(list(zip(self.offs, sizes)), "cuda")
        self.partials = torch.empty(2 * self.tiles, device="cuda")
        self.stats = torch.zeros(len(sizes), 3, device="cuda")
        self.put(self.p, params)

    def put(self, flat, tensors):
        for o, t in zip(self.offs, tensors):
            flat[o:o + t.numel()].copy_(t.reshape(-1))

    def get(self, flat):
        return [flat[o:o + n].clone() for o, n in zip(self.offs, self.sizes)]

    def norm(self, scale=1.0):
        """The clip's global norm of the flat gradient, as FusedAdam._global_norm leaves it on the device."""
        part = torch.empty(self.ops.sumsq_num_partials(self.total), device="cuda")
        out = torch.zeros(1, device="cuda")
        self.ops.sumsq_partials(self.g, part)
        self.ops.grad_norm_finish(part, scale, out)
        return out

    def step(self, kind, grads, step, lr, *, wd, maximize, clip, adapt=True, grad_scale=1.0, c=1e-3, mu=0.9):
        ops = self.ops
        self.put(self.g, grads)
        gn = self.norm(grad_scale) if clip else None
        kw = dict(grad_scale=grad_scale, weight_decay=wd, maximize=maximize, grad_norm=gn, max_norm=MAX_NORM if clip else 0.0)
        if kind == "lamb":
            ops.lamb_stage1(self.p, self.g, self.m, self.v, self.table, self.tiles, self.partials, 0.9, 0.999, step, 1e-6, **kw)
            ops.layer_ratio_finish(self.partials, self.table, self.tiles, 1.0, adapt, self.stats)
            ops.lamb_stage2(self.p, self.m, self.v, self.lp, self.table, self.tiles, self.stats, lr, 0.9, 0.999, step, 1e-6, wd)
        else:
            ops.lars_stage1(self.p, self.g, self.table, self.tiles, self.partials, **kw)
            ops.layer_ratio_finish(self.partials, self.table, self.tiles, c, adapt, self.stats)
            ops.lars_stage2(self.p, self.g, self.m, self.lp, self.table, self.tiles, self.stats, lr, mu, **kw)
        return self.stats.clone()


@pytest.fixture(scope="module")
def inputs():
    """The parameters and three gradients per tensor, shared and left unchanged."""
    gen = torch.Generator().manual_seed(21)
    params = [torch.randn(n, generator=gen) for n in SIZES]
    grads = [[torch.randn(n, generator=gen) * 0.1 for n in SIZES] for _ in range(3)]
    params[0] = torch.tensor([0.05])   # the one-element tensor by hand: see the module docstring
    for gs, value in zip(grads, (0.11, 0.13, 0.12)):
        gs[0] = torch.tensor([value])
    return params, grads


def lr_of(kind, step):
    return (1e-3 if kind == "lamb" else 0.1) * step


def reference(kind, params, grads, *, wd, maximize, clip, adapt=True, grad_scale=1.0):
    """Three steps of the f64 restatement; returns p, m / buf, v, the stats of every step and the cancellation kappa of every step's u."""
    p = [t.double() for t in params]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    all_stats, all_kappa = [], []
    for step in range(1, 4):
        gn = R.global_norm(grads[step - 1], grad_scale) if clip else None
        terms = []
        kw = dict(weight_decay=wd, grad_scale=grad_scale, maximize=maximize, layer_adaptation=adapt, grad_norm=gn,
                  max_norm=MAX_NORM if clip else None, terms=terms)
        if kind == "lamb":
            all_stats.append(L.lamb_step(p, grads[step - 1], m, v, step, lr_of(kind, step), **kw))
        else:
            all_stats.append(L.lars_step(p, grads[step - 1], m, lr_of(kind, step), **kw))
        all_kappa.append(kappas(terms, all_stats[-1]))
    return p, m, v, all_stats, all_kappa


def kappas(terms, stats):
    return [t / un if un > 0 else 1.0 for t, (_, un, _) in zip(terms, stats)]


def check_against_reference(ops, kind, flat, dev_stats, ref, clip, label):
    """Every tensor and step against the restatement; prints the worst error of each kind beside its bound, then asserts."""
    p, m, v, ref_stats, ref_kappa = ref
    B = bounds(ops, kind, (ops.sumsq_chain(flat.total) + 2) * U if clip else 0.0)
    kappa = max(max(k) for k in ref_kappa)
    assert kappa <= KAPPA_MAX, kappa                                  # the inputs do not cancel
    got_p, got_m = flat.get(flat.p), flat.get(flat.m)
    errs = {"p": max(rel_err(a, b) for a, b in zip(got_p, p))}
    if kind == "lamb":
        errs["m"] = rel_err(torch.cat(got_m), torch.cat(m))
        errs["v"] = rel_err(torch.cat(flat.get(flat.v)), torch.cat(v))
    else:
        errs["buf"] = max(rel_err(a, b) for a, b in zip(got_m, m))
    for name, col in (("pn", 0), ("un", 1), ("r", 2)):
        errs[name] = max(abs(float(got[t, col]) - want[t][col]) / want[t][col]
                         for got, want in zip(dev_stats, ref_stats) for t in range(len(want)) if want[t][col] > 0)
    print(label, f"kappa {kappa:.2f}", " ".join(f"{k} {errs[k]:.2e} (bound {B[k]:.2e})" for k in errs))
    for k in errs:
        assert errs[k] <= B[k], (k, errs[k], B[k])
    assert torch.equal(flat.lp, flat.p.bfloat16())   # the bf16 copy is the rounded master, pads (zero) included


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd,clip,maximize", list(itertools.product([0.0, 0.01], [False, True], [False, True])))
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_kernels_match_restatement(ops, inputs, kind, wd, clip, maximize):
    params, grads = inputs
    flat = Flat(ops, SIZES, params)
    dev_stats = [flat.step(kind, grads[s - 1], s, lr_of(kind, s), wd=wd, maximize=maximize, clip=clip).cpu() for s in range(1, 4)]
    ref = reference(kind, params, grads, wd=wd, maximize=maximize, clip=clip)
    if clip:
        assert all(R.clip_coefficient(R.global_norm(g), MAX_NORM) < 0.9 for g in grads)   # the clip is active
    assert all(0 < r != 1.0 for st in ref[3] for _, _, r in st)                            # and so is the adaptation
    check_against_reference(ops, kind, flat, dev_stats, ref, clip, f"{kind} wd {wd} clip {clip} maximize {maximize}:")


# ---- 2. degenerate tensors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_degenerate_tensors_have_ratio_one(ops, kind):
    gen = torch.Generator().manual_seed(5)
    sizes = [4097, 7, 4096]
    params = [torch.zeros(4097), torch.randn(7, generator=gen), torch.randn(4096, generator=gen)]   # tensor 0: |p| = 0
    grads = [torch.randn(4097, generator=gen), torch.zeros(7), torch.randn(4096, generator=gen)]     # tensor 1: |u| = 0 at step 1, wd = 0
    flat = Flat(ops, sizes, params)
    stats = flat.step(kind, grads, 1, lr_of(kind, 1), wd=0.0, maximize=False, clip=False).cpu()
    print(kind, "stats", stats.tolist())
    assert float(stats[0, 0]) == 0.0 and float(stats[0, 1]) > 0 and float(stats[0, 2]) == 1.0
    assert float(stats[1, 1]) == 0.0 and float(stats[1, 0]) > 0 and float(stats[1, 2]) == 1.0
    assert float(stats[2, 2]) not in (0.0, 1.0)
    got = flat.get(flat.p)
    assert torch.equal(got[1].cpu(), params[1])                     # a zero update: p keeps its bits
    assert float(got[0].abs().max()) > 0                            # a plain step from zero


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_without_adaptation_it_is_torch(ops, inputs, kind):
    """layer_adaptation=False: r == 1.0 exactly, and three steps agree with torch.optim.AdamW / torch.optim.SGD run on device f32 tensors
    (and with the restatement) within the bounds above."""
    params, grads = inputs
    flat = Flat(ops, SIZES, params)
    theirs = [torch.nn.Parameter(t.cuda()) for t in params]
    if kind == "lamb":
        opt = torch.optim.AdamW(theirs, lr=1e-3, eps=1e-6, weight_decay=0.01)
    else:
        opt = torch.optim.SGD(theirs, lr=0.1, momentum=0.9, weight_decay=0.01)
    dev_stats = []
    for s in range(1, 4):
        dev_stats.append(flat.step(kind, grads[s - 1], s, lr_of(kind, s), wd=0.01, maximize=False, clip=False, adapt=False).cpu())
        assert bool((dev_stats[-1][:, 2] == 1.0).all())
        opt.param_groups[0]["lr"] = lr_of(kind, s)
        for q, g in zip(theirs, grads[s - 1]):
            q.grad = g.cuda()
        opt.step()
    ref = reference(kind, params, grads, wd=0.01, maximize=False, clip=False, adapt=False)
    bound = bounds(ops, kind, 0.0)["p"]
    for t, (a, q) in enumerate(zip(flat.get(flat.p), theirs)):
        err = rel_err(a, q.detach())
        print(f"{kind} without adaptation, tensor of {SIZES[t]}: |p - torch| {err:.2e} (bound {bound:.2e})")
        assert err <= bound
    check_against_reference(ops, kind, flat, dev_stats, ref, False, f"{kind} without adaptation:")


def test_a_flat_buffer_shorter_than_its_table_is_refused(ops, inputs):
    """The wrappers hold every buffer the table indexes to the table's extent before anything is launched."""
    params, grads = inputs
    flat = Flat(ops, SIZES, params)
    short = flat.p[:flat.total - 8]
    short_bf16 = flat.lp[:flat.total - 8]
    calls = [lambda: ops.lamb_stage1(short, flat.g, flat.m, flat.v, flat.table, flat.tiles, flat.partials, 0.9, 0.999, 1, 1e-6),
             lambda: ops.lamb_stage2(flat.p, flat.m, short, flat.lp, flat.table, flat.tiles, flat.stats, 1e-3, 0.9, 0.999, 1, 1e-6),
             lambda: ops.lamb_stage2(flat.p, flat.m, flat.v, short_bf16, flat.table, flat.tiles, flat.stats, 1e-3, 0.9, 0.999, 1, 1e-6),
             lambda: ops.lars_stage1(flat.p, short, flat.table, flat.tiles, flat.partials),
             lambda: ops.lars_stage2(flat.p, flat.g, short, flat.lp, flat.table, flat.tiles, flat.stats, 0.1, 0.9),
             lambda: ops.lars_stage1(flat.p, flat.g, flat.table.clone(), flat.tiles, flat.partials)]   # a table of unknown extent
    for i, c in enumerate(calls):
        with pytest.raises(ValueError, match="extent"):
            c()
    assert torch.equal(flat.p.cpu(), torch.cat([torch.nn.functional.pad(t, (0, -t.numel() % 8)) for t in params]))   # nothing ran


# ---- 3. reproducible and tile-local --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_same_bits_twice_and_alone(ops, inputs, kind):
    params, grads = inputs
    runs = []
    for _ in range(2):
        flat = Flat(ops, SIZES, params)
        stats = [flat.step(kind, grads[s - 1], s, lr_of(kind, s), wd=0.01, maximize=False, clip=True) for s in range(1, 3)]
        runs.append((flat, stats))
    (a, sa), (b, sb) = runs
    for x, y in ((a.p, b.p), (a.m, b.m), (a.v, b.v), (a.lp, b.lp), (sa[0], sb[0]), (sa[1], sb[1])):
        assert torch.equal(x, y)
    # every tensor stepped alone (its own table: one tensor at offset 0): the bits of p and of its stats row among the others -
    # tiles start at the tensor, so its partials and their order are the same
    together = Flat(ops, SIZES, params)
    stats = together.step(kind, grads[0], 1, lr_of(kind, 1), wd=0.01, maximize=False, clip=False)
    for t, n in enumerate(SIZES):
        alone = Flat(ops, [n], [params[t]])
        st = alone.step(kind, [grads[0][t]], 1, lr_of(kind, 1), wd=0.01, maximize=False, clip=False)
        assert torch.equal(st[0], stats[t]), (n, st[0].tolist(), stats[t].tolist())
        assert torch.equal(alone.get(alone.p)[0], together.get(together.p)[t]), n
        assert torch.equal(alone.get(alone.m)[0], together.get(together.m)[t]), n


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_tables_of_one_two_and_three_tensors_give_the_bits_of_the_eight(ops, inputs, kind):
    """Tables of 1, 2 and 3 tensors (4097 / 4097, 7 / 4097, 7, 4096 elements: first tiles 0 / 0, 2 / 0, 2, 3) are where a wrong midpoint
    of the tile search first shows: every tensor's p, m and stats row are those of the same tensor in the run over all eight."""
    params, grads = inputs
    together = Flat(ops, SIZES, params)
    stats = together.step(kind, grads[0], 1, lr_of(kind, 1), wd=0.01, maximize=False, clip=False)
    all_p, all_m = together.get(together.p), together.get(together.m)
    for sizes in ([4097], [4097, 7], [4097, 7, 4096]):
        which = [SIZES.index(n) for n in sizes]
        few = Flat(ops, sizes, [params[t] for t in which])
        st = few.step(kind, [grads[0][t] for t in which], 1, lr_of(kind, 1), wd=0.01, maximize=False, clip=False)
        for i, (t, p, m) in enumerate(zip(which, few.get(few.p), few.get(few.m))):
            assert torch.equal(st[i], stats[t]), (sizes, i, st[i].tolist(), stats[t].tolist())
            assert torch.equal(p, all_p[t]) and torch.equal(m, all_m[t]), (sizes, i)


# ---- 4.-6. the optimizer classes -------------------------------------------------------------------------------------------------------
SHAPES = [(24, 32), (24,), (7, 5, 3), (1,), (64, 65)]


def _grads_like(params, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(p.shape, device="cuda", generator=gen) * 0.1 for p in params]


def _groups(params, wd):
    return [{"params": [p for p in params if p.dim() >= 2], "weight_decay": wd},
            {"params": [p for p in params if p.dim() < 2], "weight_decay": 0.0, "layer_adaptation": False}]


def _make(kind, params, **kw):
    from pero_pretraining_amd.optim import FusedLAMB, FusedLARS
    if kind == "lamb":
        return FusedLAMB(_groups(params, 0.01), lr=2e-3, **kw)
    return FusedLARS(_groups(params, 0.01), lr=0.1, momentum=0.9, trust_coefficient=1e-2, **kw)


def _feed(opt, params, grads):
    opt.zero_grad()
    for p, g in zip(params, grads):
        p.grad.copy_(g)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_bf16_and_transposed_copies_follow_the_step(kind):
    from pero_pretraining_amd import lowp
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in SHAPES]
    before = [p.detach().clone() for p in params]
    opt = _make(kind, params)
    for step in range(2):
        _feed(opt, params, _grads_like(params, step))
        opt.step()
    for p, q in zip(params, before):
        assert not torch.equal(p.detach(), q)
        assert torch.equal(lowp.get(p), p.detach().bfloat16())
        if p.dim() >= 2:
            assert torch.equal(lowp.weight_t(p), p.detach().bfloat16().view(p.shape[0], -1).t())
    for f in opt._flat:
        assert torch.equal(f["lp"], f["p"].bfloat16())
    stats = opt.layer_stats
    assert [tuple(s.shape) for s in stats] == [(3, 3), (2, 3)] and all(s.is_cuda for s in stats)
    assert bool((stats[1][:, 2] == 1.0).all()) and bool((stats[0][:, 2] != 1.0).all())


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_small_model_three_steps(ops, kind):
    """FusedLAMB / FusedLARS over layerwise_groups on smoke()'s model with a clip and grad_scale = 0.5 (two data-parallel ranks' summed
    gradient) against the restatement fed the same gradients: parameters within the p bound, grad_norm within the norm's."""
    from pero_pretraining_amd.masked_pretraining import model as M
    from pero_pretraining_amd.optim import FusedLAMB, FusedLARS, layerwise_groups
    torch.manual_seed(0)
    bb = M.init_backbone({"type": "vit", "num_blocks": 2, "model_dim": 128, "num_heads": 4, "feedforward_dim": 256})
    model = M.MaskedTransformerEncoder(bb, M.init_head({"type": "linear", "in_features": 128, "out_features": 256})).cuda()
    groups = layerwise_groups(model, 0.01)
    if kind == "lamb":
        opt = FusedLAMB(groups, lr=2e-3, max_grad_norm=MAX_NORM)
    else:
        opt = FusedLARS(groups, lr=0.1, momentum=0.9, trust_coefficient=1e-2, max_grad_norm=MAX_NORM)
    opt.grad_scale = 0.5
    assert [(g["weight_decay"], g["layer_adaptation"]) for g in opt.param_groups] == [(0.01, True), (0.0, False)]
    mine = [p for g in opt.param_groups for p in g["params"]]
    adapt = [g["layer_adaptation"] for g in opt.param_groups for _ in g["params"]]
    wds = [g["weight_decay"] for g in opt.param_groups for _ in g["params"]]
    ref_p = [p.detach().double().cpu() for p in mine]
    ref_m, ref_v = [torch.zeros_like(t) for t in ref_p], [torch.zeros_like(t) for t in ref_p]
    nb = (max(ops.sumsq_chain(f["g"].numel()) for f in opt._flat) + 2) * U
    bound = bounds(ops, kind, nb)["p"]
    for step in range(1, 4):
        for g in opt.param_groups:
            g["lr"] = g["lr"] * 1.5
        grads = _grads_like(mine, step)
        _feed(opt, mine, grads)
        opt.step()
        cpu_grads = [g.cpu() for g in grads]
        want_norm = R.global_norm(cpu_grads, 0.5)
        got_norm = float(opt.grad_norm.double())
        assert want_norm > MAX_NORM and abs(got_norm - want_norm) <= nb * want_norm, (got_norm, want_norm)
        for i in range(len(mine)):   # one tensor at a time: its group's weight decay and adaptation
            terms = []
            kw = dict(weight_decay=wds[i], grad_scale=0.5, layer_adaptation=adapt[i], grad_norm=want_norm, max_norm=MAX_NORM, terms=terms)
            if kind == "lamb":
                st = L.lamb_step([ref_p[i]], [cpu_grads[i]], [ref_m[i]], [ref_v[i]], step, opt.param_groups[0]["lr"], **kw)
            else:
                st = L.lars_step([ref_p[i]], [cpu_grads[i]], [ref_m[i]], opt.param_groups[0]["lr"], trust_coefficient=1e-2, **kw)
            assert not adapt[i] or kappas(terms, st)[0] <= KAPPA_MAX, (tuple(mine[i].shape), kappas(terms, st)[0])
        errs = [rel_err(p.detach(), q) for p, q in zip(mine, ref_p)]
        i = int(np.argmax(errs))
        print(f"{kind} step {step}: norm {got_norm:.6f} (f64 {want_norm:.6f}), worst relative parameter error {errs[i]:.2e} "
              f"(tensor {tuple(mine[i].shape)}, bound {bound:.2e})")
        assert errs[i] <= bound


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_state_dict_interchanges_with_torch_and_resumes_with_the_same_bits(kind):
    torch.manual_seed(0)
    base = [torch.randn(s, device="cuda") for s in SHAPES]
    mk = lambda: [torch.nn.Parameter(b.clone()) for b in base]  # noqa: E731
    straight, first = mk(), mk()
    oa, ob = _make(kind, straight, max_grad_norm=MAX_NORM), _make(kind, first, max_grad_norm=MAX_NORM)
    assert oa.state_dict()["state"] == {}
    for step in range(3):
        _feed(oa, straight, _grads_like(straight, step))
        oa.step()
    for step in range(2):
        _feed(ob, first, _grads_like(first, step))
        ob.step()
    sd = ob.state_dict()
    keys = {"step", "exp_avg", "exp_avg_sq"} if kind == "lamb" else {"momentum_buffer"}
    assert len(sd["state"]) == len(SHAPES) and all(set(st) == keys for st in sd["state"].values())
    resumed = [torch.nn.Parameter(p.detach().clone()) for p in first]
    oc = _make(kind, resumed, max_grad_norm=MAX_NORM)
    oc.load_state_dict(sd)
    _feed(oc, resumed, _grads_like(resumed, 2))
    oc.step()
    for p, q in zip(resumed, straight):
        assert torch.equal(p.detach(), q.detach())               # two steps, save, load, one step: the bits of three steps
    for fa, fc in zip(oa._flat, oc._flat):
        assert torch.equal(fa["m"], fc["m"]) and (kind == "lars" or torch.equal(fa["v"], fc["v"]))
    # this class -> torch's class -> this class
    tparams = [torch.nn.Parameter(p.detach().clone()) for p in first]
    tgroups = [{"params": [p for p in tparams if p.dim() >= 2]}, {"params": [p for p in tparams if p.dim() < 2]}]
    topt = torch.optim.Adam(tgroups, lr=1.0) if kind == "lamb" else torch.optim.SGD(tgroups, lr=1.0, momentum=0.5)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]["lr"] == ob.param_groups[0]["lr"] and topt.param_groups[0]["weight_decay"] == 0.01
    assert topt.param_groups[1]["layer_adaptation"] is False
    if kind == "lars":
        assert topt.param_groups[0]["momentum"] == 0.9 and topt.param_groups[0]["trust_coefficient"] == 1e-2
    for q, g in zip(tparams, _grads_like(tparams, 7)):
        q.grad = g
    topt.step()                                                   # torch steps on the loaded state
    back = [torch.nn.Parameter(p.detach().clone()) for p in first]
    od = _make(kind, back)
    od.load_state_dict(topt.state_dict())                         # and hands it back
    assert od.param_groups[0]["lr"] == ob.param_groups[0]["lr"] and od.param_groups[0]["max_grad_norm"] == MAX_NORM
    ordered = [p for g in od.param_groups for p in g["params"]]
    for f, group in zip(od._flat, topt.param_groups):
        assert f["step"] == (3 if kind == "lamb" else 1)
        for p, o, q in zip(f["params"], f["offsets"], group["params"]):
            want = topt.state[q]["exp_avg" if kind == "lamb" else "momentum_buffer"]
            assert torch.equal(f["m"][o:o + p.numel()].view(p.shape), want)
    _feed(od, ordered, _grads_like(ordered, 8))
    od.step()
    assert all(bool(torch.isfinite(p).all()) for p in back)


# ---- 7. Trainer and scripts --------------------------------------------------------------------------------------------------------------
BB = {"type": "vit", "num_blocks": 2, "model_dim": 128, "num_heads": 4, "feedforward_dim": 256}
HD = {"type": "linear", "in_features": 128, "out_features": 256}


def _batches():
    rng = np.random.default_rng(5)
    return [{"images": rng.integers(0, 256, (4, 40, 256, 3), dtype=np.uint8), "labels": rng.integers(0, 256, (4, 32))} for _ in range(3)]


def test_hip_graph_trainer_with_lamb_gives_the_bits_of_the_eager_trainer(tmp_path):
    """The masked Trainer at smoke()'s size with FusedLAMB: three steps under hip_graph=True (the optimizer's launches stay outside the
    captured graph) against the eager Trainer, bit for bit."""
    from pero_pretraining_amd.masked_pretraining import train as T
    from pero_pretraining_amd.masked_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedLAMB
    runs = {}
    for name, flag in (("eager", False), ("graph", True)):
        np.random.seed(3)
        torch.manual_seed(1)
        model = T.init_model(torch.device("cuda"), dict(BB), dict(HD))
        bop = T.init_batch_operator(torch.device("cuda"), 0.4)
        built = T.init_training(bop, model, None, None, None, 2e-3, 4, str(tmp_path), bfloat16=True, weight_decay=0.01, max_grad_norm=MAX_NORM, optimizer="lamb")
        assert type(built.optimizer) is FusedLAMB
        model.eval()   # no offset draws: both runs see the same inputs
        trainer = Trainer(built.batch_operator, model, None, built.optimizer, built.scheduler, bfloat16=True, hip_graph=flag)
        losses = []
        for i, batch in enumerate(_batches()):
            trainer.scheduler.update_learning_rate(i + 1)
            losses.append(float(trainer.train_step(batch)))
        torch.cuda.synchronize()
        if flag:
            assert len(trainer._graphs) == 1
        runs[name] = (losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, [s.clone() for s in trainer.optimizer.layer_stats])
    worst = max(float((v.double() - runs["graph"][1][k].double()).abs().max()) for k, v in runs["eager"][1].items())
    print("losses", runs["eager"][0], runs["graph"][0], "worst weight difference", worst)
    assert all(math.isfinite(x) for x in runs["eager"][0]) and runs["eager"][0] == runs["graph"][0]
    for k, v in runs["eager"][1].items():
        assert torch.equal(v, runs["graph"][1][k]), k
    for a, b in zip(runs["eager"][2], runs["graph"][2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("script", ["masked", "joint"])
def test_init_training_builds_the_optimizer_it_is_asked_for(tmp_path, script):
    from pero_pretraining_amd.optim import FusedAdam, FusedAdamW, FusedLAMB, FusedLARS
    if script == "masked":
        from pero_pretraining_amd.masked_pretraining import train as T
        make_bop = lambda: T.init_batch_operator(torch.device("cuda"), 0.4)  # noqa: E731
    else:
        from pero_pretraining_amd.joint_embedding_pretraining import train as T
        make_bop = lambda: T.init_batch_operator(torch.device("cuda"))  # noqa: E731
    small = {"type": "vit", "num_blocks": 1, "model_dim": 32, "num_heads": 4, "feedforward_dim": 64}
    head = {"type": "linear", "in_features": 32, "out_features": 24}

    def build(**kw):
        torch.manual_seed(0)
        model = T.init_model(torch.device("cuda"), dict(small), dict(head))
        return T.init_training(make_bop(), model, None, None, None, 1e-3, 4, str(tmp_path), **kw).optimizer, model

    opt, model = build()
    assert type(opt) is FusedAdam and len(opt.param_groups) == 1 and opt.param_groups[0]["weight_decay"] == 0   # what it builds today
    opt, _ = build(weight_decay=0.05)
    assert type(opt) is FusedAdamW and [g["weight_decay"] for g in opt.param_groups] == [0.05, 0.0]
    opt, model = build(optimizer="lamb", weight_decay=0.05, max_grad_norm=2.0)
    assert type(opt) is FusedLAMB
    assert [(g["weight_decay"], g["layer_adaptation"], g["max_grad_norm"]) for g in opt.param_groups] == [(0.05, True, 2.0), (0.0, False, 2.0)]
    assert [id(p) for g in opt.param_groups for p in g["params"]] == \
        [id(p) for p in model.parameters() if p.dim() >= 2] + [id(p) for p in model.parameters() if p.dim() < 2]
    opt, _ = build(optimizer="lars", weight_decay=1e-4, momentum=0.8)
    assert type(opt) is FusedLARS and opt._flat[0]["v"] is None
    assert [(g["weight_decay"], g["layer_adaptation"], g["momentum"]) for g in opt.param_groups] == [(1e-4, True, 0.8), (0.0, False, 0.8)]
    with pytest.raises(ValueError, match="Unknown optimizer"):
        build(optimizer="sgd")
