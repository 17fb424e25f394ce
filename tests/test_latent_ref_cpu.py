"""CPU: tests/latent_ref.py, the f64 restatement the GPU tests of the latent-target step compare with, pinned to torch itself - the targets
to F.layer_norm, the loss and its gradient to F.smooth_l1_loss / F.mse_loss under autograd, the EMA to torch.optim.swa_utils.AveragedModel,
the decay schedule's end points, the span masks - and the host-side pieces of the package that need no GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import latent_ref as LR


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("d,K,n", [(64, 1, 1), (72, 3, 29), (19, 2, 5)])
def test_targets_equal_the_mean_of_layer_norms(d, K, n):
    g = _gen(d + K + n)
    mats = [torch.randn(53, d, generator=g, dtype=torch.float64) * (k + 1) + 0.3 * k for k in range(K)]
    index = torch.randperm(53, generator=g)[:n]
    y, mag = LR.latent_targets(mats, index, n + 3, 1e-5)
    ref = sum(TF.layer_norm(m, (d,), eps=1e-5) for m in mats)[index] / K
    assert float((y[:n] - ref).abs().max()) < 1e-12
    assert torch.equal(y[n:], torch.zeros(3, d, dtype=torch.float64)) and bool((mag[:n] > 0).all())


def _loss_inputs(d, n, beta, seed):
    g = _gen(seed)
    y = torch.randn(n + 3, d, generator=g, dtype=torch.float64)
    pred = y + torch.randn(n + 3, d, generator=g, dtype=torch.float64) * 1.5
    return LR.move_off_branch(pred, y, beta), y


@pytest.mark.parametrize("beta", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("d,n", [(64, 1), (72, 29), (520, 29), (19, 29)])
def test_loss_and_gradient_equal_torch(beta, d, n):
    pred, y = _loss_inputs(d, n, beta, 7 * d + n)
    assert int(LR.branch_offenders(pred, y, beta).sum()) == 0   # no element within 1e-3 beta of the branch point of l'
    p = pred[:n].clone().requires_grad_(True)
    ref = TF.mse_loss(p, y[:n]) if beta == 0 else TF.smooth_l1_loss(p, y[:n], beta=beta)
    (0.375 * ref).backward()
    loss, mag = LR.latent_loss(pred, y, n, beta)
    assert abs(float(loss) - float(ref)) < 1e-12 * float(ref) and float(mag) == float(loss)
    grad = LR.latent_loss_grad(pred, y, n, beta, dloss=0.375)
    assert float((grad[:n] - p.grad).abs().max()) < 1e-15
    assert torch.equal(grad[n:], torch.zeros(3, d, dtype=torch.float64))


def test_move_off_branch_moves_offenders_only():
    y = torch.zeros(1, 4, dtype=torch.float64)
    pred = torch.tensor([[0.5 + 1e-5, -0.5 + 2e-4, 0.3, -2.0]], dtype=torch.float64)
    assert int(LR.branch_offenders(pred, y, 0.5).sum()) == 2
    moved = LR.move_off_branch(pred, y, 0.5)
    assert int(LR.branch_offenders(moved, y, 0.5).sum()) == 0 and torch.equal(moved[0, 2:], pred[0, 2:])
    assert int(LR.branch_offenders(pred, y, 0.0).sum()) == 0   # MSE has no branch


def test_ema_three_updates_equal_averaged_model():
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    torch.manual_seed(2)
    decay = 0.9
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.LayerNorm(7), torch.nn.Linear(7, 3)).double()
    averaged = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(decay))
    averaged.update_parameters(net)            # its first call copies: the state WeightEMA starts from
    avg = [p.detach().clone() for p in net.parameters()]
    for k in range(3):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn(p.shape, dtype=torch.float64) * 0.1)
        averaged.update_parameters(net)
        avg = LR.ema_update(avg, [p.detach() for p in net.parameters()], LR.ema_decay(k, decay))
    for a, b in zip(avg, averaged.module.parameters()):
        assert float((a - b).abs().max()) < 1e-15
    # the f32 chain of the kernel against the f64 formula: three roundings per element
    a32, p32 = np.float32(0.25), np.float32(-1.5)
    got = LR.ema_update_f32(a32, p32, 1 - decay)
    assert got.dtype == np.float32 and abs(float(got) - (0.25 + float(np.float32(1 - decay)) * (-1.75))) < 3 * 2.0 ** -24 * 1.75


def test_decay_schedule_end_points_and_ramp():
    assert LR.ema_decay(0, 0.999) == 0.999 and LR.ema_decay(10 ** 6, 0.999) == 0.999
    assert LR.ema_decay(5, 0.999, decay_start=None, ramp_updates=10) == 0.999
    assert LR.ema_decay(5, 0.999, decay_start=0.99, ramp_updates=0) == 0.999
    taus = [LR.ema_decay(k, 0.9999, 0.99, 100) for k in range(0, 151)]
    assert taus[0] == 0.99 and taus[100] == 0.9999 and taus[150] == 0.9999
    assert all(b > a for a, b in zip(taus[:100], taus[1:101]))
    assert abs(taus[50] - (0.99 + 0.0099 * 0.5)) < 1e-15
    # the class computes the same numbers (no GPU needed: a CPU module is left unflattened)
    from pero_pretraining_amd.optim import WeightEMA
    ema = WeightEMA(torch.nn.Linear(3, 2), decay=0.9999, decay_start=0.99, ramp_updates=100)
    assert [ema.decay_at(k) for k in range(151)] == taus
    assert not any(p.requires_grad for p in ema.module.parameters()) and not ema.module.training
    sd = ema.state_dict()
    assert set(sd) == {"module", "n_updates", "decay", "decay_start", "ramp_updates"} and sd["n_updates"] == 0
    with pytest.raises(RuntimeError, match="GPU"):
        ema.update()
    with pytest.raises(ValueError):
        WeightEMA(torch.nn.Linear(3, 2), decay=1.5)


@pytest.mark.parametrize("span,prob", [(1, 0.3), (3, 0.3), (33, 0.9)])   # 33: longer than a line (cut at its end)
def test_span_masks(span, prob):
    from pero_pretraining_amd.latent_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.masked_pretraining.batch_operator import BatchOperator as MaskedOperator
    labels = np.zeros((6, 32), dtype=np.int64)
    labels[1, 20:] = -1
    labels[4, 3:] = -1
    valid = (labels >= 0).astype(int)
    bop = BatchOperator(torch.device("cpu"), prob, mask_span=span)
    np.random.seed(11)
    mask = bop._create_mask({"labels": labels})
    np.random.seed(11)
    rand = np.random.rand(6, 32)
    assert np.array_equal(mask, LR.span_mask(rand, prob, span, valid))
    assert mask.sum() > 0 and not (mask * (1 - valid)).any()           # never on invalid positions
    if span == 1:
        np.random.seed(11)
        assert np.array_equal(mask, MaskedOperator(torch.device("cpu"), 0.3)._create_mask({"labels": labels}))
    else:
        starts = rand < prob / span
        assert np.array_equal(mask[0, :span], np.maximum.accumulate(starts[0, :span]).astype(int))   # a run reaches span - 1 positions on
    # without labels the validity comes from the image masks
    np.random.seed(11)
    assert np.array_equal(bop._create_mask({"image_masks": valid.astype(np.uint8)}), mask)
    images, v, m = bop.prepare_batch({"images": np.zeros((6, 40, 256, 3), np.uint8), "labels": labels})
    assert isinstance(m, np.ndarray) and torch.equal(v, torch.from_numpy(valid)) and images.dtype == torch.uint8


def test_target_std_and_trainer_refusals():
    t = torch.randn(40, 8, generator=_gen(3), dtype=torch.float64)
    assert abs(LR.target_std(t) - float(t.std(0, unbiased=False).mean())) < 1e-15
    assert LR.target_std(torch.ones(5, 8)) == 0.0                      # a collapsed teacher
    from pero_pretraining_amd.latent_pretraining.trainer import Trainer
    for kw in ({"hip_graph": True}, {"data_parallel": object()}):
        with pytest.raises(ValueError, match="not supported"):
            Trainer(None, None, None, None, None, **kw)


def test_latent_entry_points_validate_arguments_without_gpu():
    """Unsupported widths and counts return the library's error code on the host, before any launch."""
    import ctypes
    from pero_pretraining_amd import _lib, ops
    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    one = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    idx = (ctypes.c_int64 * 1)(0)
    assert ops.LATENT_MAX_K == 16 and ops.LATENT_MAX_D >= 4096
    for K, d in ((1, 19), (1, 4100), (0, 64), (17, 64)):
        assert h.pero_latent_targets(one, K, idx, buf, 1, 1, 1, d, 1e-5, 0, None) == _lib.DEFINES["PERO_E_INVALID"], (K, d)
    assert b"pero_latent_targets" in h.pero_last_error()
    assert h.pero_latent_loss_fwd(buf, buf, buf, buf, 1, 19, 1.0, 0, None) == -1
    assert h.pero_latent_loss_fwd(buf, buf, buf, buf, 1, 16, -1.0, 0, None) == -1 and b"beta" in h.pero_last_error()
    assert h.pero_latent_loss_bwd(buf, buf, None, buf, 2, 1, 16, 1.0, 0, None) == -1
    assert h.pero_ema_update(None, None, None, 1, 1, 0.5, None) == -1
    assert h.pero_ema_update(buf, None, idx, 2, 1, 0.5, None) == -1        # fewer tiles than segments
    with pytest.raises(ValueError, match="multiples of 8"):
        ops.ema_table([(4096, 4, 8)], torch.device("cpu"))
