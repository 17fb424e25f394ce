"""CPU: the f64 restatement of the optimizer formulas (tests/optim_ref.py) is torch.optim.Adam / AdamW + clip_grad_norm_ in f64 to
1e-14, over every combination of the flags; the new C-ABI entries refuse bad arguments on the host; decay_groups splits a model the
usual way and the data-parallel gradient buckets follow its two flat buffers."""
import itertools

import pytest
import torch

import optim_ref as R

SHAPES = [(7, 5), (11,), (3, 4, 2)]
FLAGS = list(itertools.product([0.0, 0.05], [False, True], [False, True], [False, True]))   # wd, decoupled, amsgrad, maximize


@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("wd,decoupled,amsgrad,maximize", FLAGS)
def test_restatement_is_torch_in_f64(wd, decoupled, amsgrad, maximize, clip):
    gen = torch.Generator().manual_seed(17)
    mine = [torch.randn(s, generator=gen, dtype=torch.float64) for s in SHAPES]
    theirs = [torch.nn.Parameter(p.clone()) for p in mine]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    lr = 3e-3
    opt = cls(theirs, lr=lr, weight_decay=wd, amsgrad=amsgrad, maximize=maximize)
    m = [torch.zeros_like(p) for p in mine]
    v = [torch.zeros_like(p) for p in mine]
    vmax = [torch.zeros_like(p) if amsgrad else None for p in mine]
    worst = 0.0
    for step in range(1, 5):
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * (10.0 if step % 2 else 0.01) for s in SHAPES]
        for q, g in zip(theirs, grads):
            q.grad = g.clone()
        norm = None
        if clip is not None:
            norm = R.global_norm(grads)
            got = torch.nn.utils.clip_grad_norm_(theirs, clip)
            assert abs(float(got) - norm) <= 1e-14 * norm
        opt.step()
        for i, g in enumerate(grads):
            R.adam_step_ex(mine[i], g, m[i], v[i], vmax[i], step, lr, weight_decay=wd, decoupled=decoupled, maximize=maximize,
                           grad_norm=norm, max_norm=clip)
        for p, q in zip(mine, theirs):
            worst = max(worst, float((p - q.detach()).abs().max()))
    print(f"worst |restatement - torch| = {worst:.3e}")
    assert worst < 1e-14
    for i, q in enumerate(theirs):
        st = opt.state[q]
        assert float((st["exp_avg"] - m[i]).abs().max()) < 1e-14 and float((st["exp_avg_sq"] - v[i]).abs().max()) < 1e-14
        if amsgrad:
            assert float((st["max_exp_avg_sq"] - vmax[i]).abs().max()) < 1e-14
        else:
            assert "max_exp_avg_sq" not in st


def test_new_optimizer_entries_validate_arguments_without_gpu():
    import ctypes
    from pero_pretraining_amd import _lib
    L = _lib.lib()
    assert L.pero_adam_step_ex(None, None, None, None, None, 4, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, 0, None, 0, None, 0.0, None) < 0
    assert b"pero_adam_step_ex" in L.pero_last_error()
    buf = (ctypes.c_float * 16)()
    base = ctypes.addressof(buf)
    a16 = ctypes.c_void_p(base + (-base) % 16)
    assert L.pero_adam_step_ex(a16, a16, a16, a16, None, 4, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.1, 2, None, 0, None, 0.0, None) < 0   # decoupled = 2
    assert L.pero_adam_step_ex(a16, a16, a16, a16, None, 4, 1e-3, 0.9, 0.999, 1e-8, 0, 1.0, 0.1, 1, None, 0, None, 0.0, None) < 0   # step 0
    assert L.pero_adam_step_ex(a16, a16, a16, a16, None, 4, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, 0, None, 0, a16, -1.0, None) < 0   # max_norm < 0
    assert L.pero_sumsq_partials(None, 4, None, None) < 0 and b"pero_sumsq_partials" in L.pero_last_error()
    assert L.pero_sumsq_partials(ctypes.c_void_p(a16.value + 4), 4, a16, None) < 0                                                  # alignment
    assert L.pero_grad_norm_finish(None, 1, 1.0, None, None) < 0 and b"pero_grad_norm_finish" in L.pero_last_error()
    assert L.pero_grad_norm_finish(a16, 0, 1.0, a16, None) < 0


def test_partial_count_depends_on_n_alone():
    """One workgroup per 1024 16-byte pieces up to the cap: ops.py's constants restate csrc/optim.hip's layout."""
    from pero_pretraining_amd import ops
    for n in (1, 4, 5, 1027, 4096, 4097, 10007, 4096 * 1024 + 1027, 40_400_000, 2 ** 31 + 5):
        nv = (n + 3) // 4
        want = max(1, min((nv + ops.SUMSQ_PIECES_PER_BLOCK - 1) // ops.SUMSQ_PIECES_PER_BLOCK, ops.SUMSQ_MAX_BLOCKS))
        assert ops.sumsq_num_partials(n) == want, n
    assert ops.sumsq_num_partials(0) == 0
    assert ops.sumsq_chain(1) == 1 + 11 and ops.sumsq_chain(10007) == 4 + 11
    assert ops.sumsq_chain(2048 * 1024 * 4 * 3) == 12 + 11     # past the cap every lane walks further


def test_decay_groups_split_by_dimension_in_model_order():
    from pero_pretraining_amd.optim import decay_groups
    model = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3), torch.nn.Conv1d(3, 2, 3), torch.nn.BatchNorm1d(2))
    groups = decay_groups(model, 0.05)
    assert [g["weight_decay"] for g in groups] == [0.05, 0.0]
    names = {id(p): n for n, p in model.named_parameters()}
    assert [names[id(p)] for p in groups[0]["params"]] == ["0.weight", "2.weight"]
    assert [names[id(p)] for p in groups[1]["params"]] == ["0.bias", "1.weight", "1.bias", "2.bias", "3.weight", "3.bias"]
    torch.optim.AdamW(groups, lr=1e-3)   # the same groups feed torch's optimizer


def test_plan_buckets_keeps_the_two_groups_apart():
    """The gradient buckets of parallel.DataParallel over a decay / no-decay pair of flat buffers: ranges of one stage merge inside a group,
    never across groups, and every parameter's padded range is covered once."""
    from pero_pretraining_amd.parallel import plan_buckets
    prefix = "backbone.encoder_layers.layers."
    named = [("backbone.conv.weight", torch.zeros(4, 3, 2, 2)), ("backbone.conv.bias", torch.zeros(4)),
             (prefix + "0.linear.weight", torch.zeros(6, 4)), (prefix + "0.linear.bias", torch.zeros(6)), (prefix + "0.norm.weight", torch.zeros(6)),
             (prefix + "1.linear.weight", torch.zeros(5, 3)), (prefix + "1.linear.bias", torch.zeros(5)), ("head.linear.weight", torch.zeros(3, 5)),
             ("head.linear.bias", torch.zeros(3))]
    offsets, totals = {}, [0, 0]
    for name, p in named:   # FusedAdam's layout over decay_groups: group 0 = dim() >= 2, group 1 = the rest, 8-element padding
        gi = 0 if p.dim() >= 2 else 1
        offsets[id(p)] = (gi, totals[gi], p.numel())
        totals[gi] += ((p.numel() + 7) // 8) * 8
    got = plan_buckets(named, offsets, 2)
    assert got == {-1: [(0, 0, 48), (1, 0, 8)], 0: [(0, 48, 72), (1, 8, 24)], 1: [(0, 72, 88), (1, 24, 32)], "head": [(0, 88, 104), (1, 32, 40)]}
    covered = [0, 0]
    for ranges in got.values():
        for gi, a, b in ranges:
            covered[gi] += b - a
    assert covered == totals
