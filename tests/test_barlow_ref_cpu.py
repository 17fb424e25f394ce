"""CPU: the f64 restatement of Barlow Twins (tests/barlow_ref.py) is consistent with itself - its staged backward, which is the kernels'
division of work, equals autograd of the loss - and behaves at the edges the GPU tests rely on."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import barlow_ref as B  # noqa: E402


def _rows(n, d, seed, shift=0.0, noise=0.3):
    rng = np.random.default_rng(seed)
    z1 = 0.8 * rng.standard_normal((n, d)) + shift * rng.standard_normal((1, d))
    z2 = z1 + noise * rng.standard_normal((n, d))
    return torch.from_numpy(z1), torch.from_numpy(z2)


def test_staged_backward_equals_autograd_f64():
    for n, d, shift, lam in ((37, 24, 0.0, 0.0051), (244, 48, 5.0, 0.0051), (100, 16, 0.0, 0.3)):
        z1, z2 = _rows(n, d, n, shift)
        a1, a2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
        loss = B.loss_from_rows(a1, a2, lam)[0]
        (3.0 * loss).backward()
        d1, d2 = B.staged_backward(z1, z2, lam, g=3.0)
        for got, ref in ((d1, a1.grad), (d2, a2.grad)):
            assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max()), (n, d, shift)


def test_masked_loss_pairs_positions_in_order():
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((2, 10, 6)))
    y = torch.from_numpy(rng.standard_normal((2, 10, 6)))
    m1 = np.ones((2, 10), np.uint8)
    m1[:, -2:] = 0
    m1[0, 3] = 2
    m2 = m1[:, ::-1].copy()
    res = B.barlow_loss(x, y, m1, m2)
    ix, iy = B.pairs(m1, m2)
    assert ix.size == iy.size == 15 and 3 not in ix and 6 not in iy
    ref = B.loss_from_rows(x.reshape(-1, 6)[ix], y.reshape(-1, 6)[iy])
    assert float(res["loss"]) == float(ref[0]) and float(res["loss.on_diagonal"]) == float(ref[1])
    assert abs(float(res["loss"]) - float(ref[1] + 0.0051 * ref[2])) < 1e-12


def test_single_pair_gives_loss_d_and_zero_gradients():
    z1, z2 = _rows(1, 12, 5)
    a1, a2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    loss, on, off, _ = B.loss_from_rows(a1, a2)
    loss.backward()
    assert float(loss) == 12.0 and float(on) == 12.0 and float(off) == 0.0
    assert float(a1.grad.abs().max()) == 0.0 and float(a2.grad.abs().max()) == 0.0
    d1, d2 = B.staged_backward(z1, z2)
    assert float(d1.abs().max()) == 0.0 and float(d2.abs().max()) == 0.0


def test_constant_column_stays_finite():
    z1, z2 = _rows(50, 8, 7)
    z1[:, 2] = 1.5
    z2[:, 2] = 1.5
    z2[:, 5] = -4.0
    a1, a2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    loss = B.loss_from_rows(a1, a2)[0]
    loss.backward()
    d1, d2 = B.staged_backward(z1, z2)
    for t in (loss, a1.grad, a2.grad, d1, d2):
        assert bool(torch.isfinite(t).all())
    assert float((d1 - a1.grad).abs().max()) <= 1e-10 * float(a1.grad.abs().max())


# ---- the host side of BarlowTwinsLoss: no GPU needed ----------------------------------------------------------------------------
def test_loss_class_refuses_the_cpu_and_init_model_knows_barlow():
    import pytest
    from pero_pretraining_amd.joint_embedding_pretraining.losses import BarlowTwinsLoss
    from pero_pretraining_amd.joint_embedding_pretraining.train import init_model
    loss = BarlowTwinsLoss()
    assert (loss.lambda_offdiag, loss.eps) == (0.0051, 1e-5)
    ones = np.ones((1, 4), np.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        loss(torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), ones, ones, ones, ones)
    bb = {"type": "vit", "num_blocks": 1, "model_dim": 64, "num_heads": 4, "feedforward_dim": 64}
    hd = {"type": "linear", "in_features": 64, "out_features": 32}
    model = init_model("cpu", bb, hd, loss_type="barlow", barlow_lambda=0.01)
    assert isinstance(model.loss, BarlowTwinsLoss) and model.loss.lambda_offdiag == 0.01
    with pytest.raises(ValueError, match="Unknown loss type: nope"):
        init_model("cpu", bb, hd, loss_type="nope")


def test_entry_points_validate_arguments_without_gpu():
    import ctypes
    import re
    from pero_pretraining_amd import _lib, ops
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    assert L.pero_barlow_stats(None, None, None, None, None, None, None, 4, 8, 1e-5, 0, None) == -1
    assert b"pero_barlow_stats" in L.pero_last_error()
    assert L.pero_barlow_stats(buf, idx, buf, idx, buf, buf, buf, 0, 8, 1e-5, 0, None) == -1               # no rows
    assert L.pero_barlow_standardize(buf, idx, buf, idx, buf, buf, buf, 4, 3, 8, 0, None) == -1             # n_pad < n
    assert L.pero_barlow_corr(buf, buf, buf, buf, 0, 4, 0.0051, 0, None) == -1                              # d == 0
    assert L.pero_barlow_bwd_stats(buf, buf, buf, buf, buf, 4, 3, 8, 0, None) == -1
    assert L.pero_barlow_standardize_bwd(buf, buf, buf, buf, buf, idx, idx, buf, None, None, 4, 4, 8, 0, None) == -1
    assert L.pero_barlow_stats(buf, idx, buf, idx, buf, buf, buf, 4, 8, 1e-5, 7, None) == -1                # dtype
    # the workspace: ops' helper against the text of the header's function-like macro
    text = open(_lib.HEADER_PATH).read()
    (body,) = re.findall(r"^#define PERO_BARLOW_PART\(n, d\)[ \t]+(.+)$", text, flags=re.M)
    assert body == "(4 * (((n) + PERO_BARLOW_TILE_ROWS - 1) / PERO_BARLOW_TILE_ROWS) * (d))"
    T = _lib.DEFINES["PERO_BARLOW_TILE_ROWS"]
    assert ops.BARLOW_TILE_ROWS == T
    for n, d in ((1, 1), (T, 24), (T + 1, 64), (5 * T - 1, 4096)):
        assert ops.barlow_part_elems(n, d) == 4 * ((n + T - 1) // T) * d
