"""The f64 restatements of tests/ntxent_ragged_ref.py (NT-Xent on collated batches) pinned on the CPU: chained, they are the literal
boolean-indexing loss and its torch-autograd gradients; at all-ones masks they are the oracle's NT-Xent; on g24 they are the reference's
own loss and gradients; and `ntxent_slots_host` (the numpy twin of pero_ntxent_slots) is the boolean-index ranks."""
import math

import numpy as np
import pytest
import torch

import ntxent_ragged_ref as RR
import parity_ref as R
from oracle import pero_oracle as O

T = 0.1
G24_MASKS = ("image_masks1", "image_masks2", "shift_masks1", "shift_masks2")


def chain(x, y, masks, Sp, cross=False):
    """Loss and gradients through the restated entry points, in the order _NTXentFn / _NTXentCrossFn call them (one rank)."""
    x, y = R.f64(x), R.f64(y)
    n, S, D = x.shape
    slot1, slot2, count = RR.slots(*masks)
    (xn, invx), _ = RR.rows_fwd(x, slot1, count, Sp)
    (yn, invy), _ = RR.rows_fwd(y, slot2, count, Sp)
    sim = torch.einsum("lid,ljd->lij", xn, yn) / T
    cr = None
    if cross:
        pm, _ = RR.line_mean_ragged(xn.reshape(n * Sp, D), count, Sp)
        (p, invp), _ = R.rownorm(pm)
        cr = (yn.reshape(n * Sp, D) @ p.t()) / T
    res, _ = RR.cols_ragged(sim, count, cr, 0)
    dxn = torch.einsum("lij,ljd->lid", res["dsim"], yn) / T
    dyn = torch.einsum("lij,lid->ljd", res["dsim"], xn) / T
    if cross:
        dc = res["dcross"]
        dyn = dyn + (dc @ p / T).reshape(n, Sp, D)
        dp = dc.t() @ yn.reshape(n * Sp, D) / T
        dpm, _ = R.rownorm_bwd(p, dp, invp, None)
        dxn = RR.add_line_rows_ragged(dxn.reshape(n * Sp, D), dpm, count, Sp)[0].reshape(n, Sp, D)
    dx, _ = RR.rows_bwd(xn, dxn, invx, slot1, count, None)
    dy, _ = RR.rows_bwd(yn, dyn, invy, slot2, count, None)
    return float(res["loss"]), dx, dy


def literal(x, y, masks, cross=False):
    xo, yo = R.f64(x).requires_grad_(True), R.f64(y).requires_grad_(True)
    l = RR.loss(xo, yo, *masks, temperature=T, cross=cross)
    l.backward()
    return float(l), xo.grad, yo.grad


def _inputs(n, S, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, S, D, generator=g, dtype=torch.float64)
    return x, x + 0.7 * torch.randn(n, S, D, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("pad", [0, 60])      # Sp = S (f32 parity mode) and a padded block (bf16 mode)
def test_restatements_chain_to_the_literal_loss_and_autograd(cross, pad):
    masks = RR.collated_masks()
    n, S = masks[0].shape
    x, y = _inputs(n, S, 16, 1)
    loss, dx, dy = chain(x, y, masks, S + pad, cross)
    ref, gx, gy = literal(x, y, masks, cross)
    assert abs(loss - ref) < 1e-12 * abs(ref)
    assert float((dx - gx).abs().max()) < 1e-12 and float((dy - gy).abs().max()) < 1e-12
    sel1, sel2 = RR.selected(masks[0], masks[2]), RR.selected(masks[1], masks[3])
    assert not sel1.all() and float(dx[torch.from_numpy(~sel1)].abs().max()) == 0.0 and float(dy[torch.from_numpy(~sel2)].abs().max()) == 0.0


def test_all_ones_masks_are_the_oracle():
    n, S, D = 4, 12, 16
    x, y = _inputs(n, S, D, 2)
    ones = np.ones((n, S), np.uint8)
    masks = (ones,) * 4
    assert abs(chain(x, y, masks, S)[0] - float(O.ntxent_loss(x, y, *masks)["loss"])) < 1e-12
    assert abs(float(RR.loss(x, y, *masks)) - float(O.ntxent_loss(x, y, *masks)["loss"])) < 1e-12
    ref = float(O.ntxent_cross_loss(x, y, n)[0])
    assert abs(chain(x, y, masks, S, cross=True)[0] - ref) < 1e-12 and abs(float(RR.loss(x, y, *masks, cross=True)) - ref) < 1e-12


def test_g24_is_the_reference(golden):
    """The reference's own NTXentLoss on the masks it accepts (shift masks all ones, image masks with equal counts): 1e-4, as for g9."""
    g = golden("g24_ntxent_image_masks.npz")
    masks = [g[k] for k in G24_MASKS]
    counts = RR.slots(*masks)[2]
    assert len(set(counts.tolist())) == 3 and counts.min() > 0 and all(bool((g[k] == 1).all()) for k in G24_MASKS[2:])
    assert not np.array_equal(masks[0][1], masks[1][1])          # one line selects different positions in the two views
    loss, dx, dy = chain(g["x"], g["y"], masks, 24)
    assert abs(loss - float(g["loss"])) < 1e-4 * float(g["loss"])
    assert np.abs(dx.numpy() - g["grad_x"]).max() < 1e-4 * np.abs(g["grad_x"]).max() + 1e-8
    assert np.abs(dy.numpy() - g["grad_y"]).max() < 1e-4 * np.abs(g["grad_y"]).max() + 1e-8
    assert abs(literal(g["x"], g["y"], masks)[0] - float(g["loss"])) < 1e-4 * float(g["loss"])
    # what the collator produces: the reference raises IndexError, the two counts of every line agree, shift == 1 implies image == 1
    assert bool(g["collated_masks_raise_indexerror"])
    cm = [g["collated_" + k] for k in G24_MASKS]
    assert np.array_equal(RR.slots(*cm)[2], g["collated_counts"]) and g["collated_counts"].tolist() == [60, 64, 50, 17, 64]


def _slot_cases():
    im1, im2, sm1, sm2 = (m.copy() for m in RR.collated_masks())
    yield "collated", (im1, im2, sm1, sm2), None
    assert (sm1 == 2).any() and (sm2 == 2).any()                 # the collated shift masks hold "shared but padding" positions
    twos = (im1.copy(), im2.copy(), sm1.copy(), sm2.copy())     # a selected position turned into a 2: one pair fewer in every line
    for l in range(len(im1)):
        twos[2][l, np.flatnonzero(RR.selected(im1[l], sm1[l]))[0]] = 2
        twos[3][l, np.flatnonzero(RR.selected(im2[l], sm2[l]))[-1]] = 2
    yield "twos", twos, [59, 63, 49, 16, 63]
    mism = (im1.copy(), im2.copy(), sm1.copy(), sm2.copy())
    mism[0][1, np.flatnonzero(RR.selected(im1[1], sm1[1]))[0]] = 0
    yield "mismatch", mism, None
    empty = (im1.copy(), im2.copy(), sm1.copy(), sm2.copy())
    empty[0][2] = 0
    empty[1][2] = 0
    yield "empty", empty, None


@pytest.mark.parametrize("name,masks,counts", list(_slot_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_ntxent_slots_host_is_the_boolean_index_ranks(name, masks, counts):
    from pero_pretraining_amd.joint_embedding_pretraining.losses import ntxent_slots_host
    got = ntxent_slots_host(*masks)
    ref = RR.slots(*masks)
    for a, b in zip(got, ref):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    if counts is not None:
        assert got[2].tolist() == counts
    if name == "collated":
        assert got[2].tolist() == [60, 64, 50, 17, 64]
    if name == "mismatch":
        assert got[2][1] == -1 and (np.delete(got[2], 1) > 0).all()
    if name == "empty":
        assert got[2][2] == 0 and (got[0][2] == -1).all() and (got[1][2] == -1).all()
    other = tuple(torch.from_numpy(m.astype(np.int64)) for m in masks)      # other integer dtypes, torch tensors
    assert all(np.array_equal(a, b) for a, b in zip(ntxent_slots_host(*other), ref))


def test_bad_lines_have_a_nan_loss_and_zero_gradients_in_the_restatement():
    sim = torch.randn(2, 6, 6, dtype=torch.float64)
    res, _ = RR.cols_ragged(sim, [4, -1])
    assert math.isnan(float(res["loss"])) and math.isnan(float(res["line_loss"][1])) and float(res["dsim"][1].abs().max()) == 0.0
    assert float(res["dsim"][0, 4:].abs().max()) == 0.0 and float(res["dsim"][0, :, 4:].abs().max()) == 0.0
