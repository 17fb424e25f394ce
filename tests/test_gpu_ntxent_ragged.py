"""NT-Xent on collated batches (NTXentLoss(apply_masks=True), csrc/ntxent_ragged.hip) on the GPU.  Kernel level: every new entry point
against its f64 restatement (tests/ntxent_ragged_ref.py) through `assert_within`, with the term counts of the dense NT-Xent kernel tests
(tests/test_gpu_kernel_parity.py) taken at the padded block size, and every entry the header calls zero compared with 0 exactly.  Loss
level: the reference's own values (g24), the f64 boolean-indexing loss on masks as the collator draws them, the equalities the
selection implies.  End to end: a collated batch of ragged widths through init_model(loss_type="ntxent", ntxent_apply_masks=True)."""
import math

import numpy as np
import pytest
import torch

import ntxent_ragged_ref as RR
import parity_ref as R
from parity_ref import DIVF, EXPF, LOGF, SQRTF, assert_within

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
F32 = torch.float32
G24_MASKS = ("image_masks1", "image_masks2", "shift_masks1", "shift_masks2")


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    return _ops


def gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(a):
    return torch.tensor(np.asarray(a), dtype=torch.int32).cuda()


def zero(t):
    return t.numel() == 0 or float(t.float().abs().max()) == 0.0


def random_masks(lines, S, seed):
    """Random image masks and three-valued shift masks; line 0 selects the same positions in both views, line 1 (if any) different
    numbers, line 2 (if any) none."""
    rng = np.random.default_rng(seed)
    im1, im2 = (rng.integers(0, 2, (lines, S)).astype(np.uint8) for _ in range(2))
    sm1, sm2 = (rng.integers(0, 3, (lines, S)).astype(np.uint8) for _ in range(2))
    im1[0, 0] = sm1[0, 0] = 1
    im2[0], sm2[0] = im1[0], sm1[0]
    if lines > 1:
        im1[1, -1] = sm1[1, -1] = 1
        im2[1], sm2[1] = im1[1], sm1[1]
        im2[1, -1] = 0
    if lines > 2:
        sm1[2] = np.where(sm1[2] == 1, 2, sm1[2])
        im2[2] = 0
    return im1, im2, sm1, sm2


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("S", [1, 5, 64, 65, 130])
def test_slots_are_exact(ops, S):
    lines = 7
    masks = random_masks(lines, S, S)
    slot, count = ops.ntxent_slots(*(cu(m) for m in masks))
    r1, r2, rc = RR.slots(*masks)
    assert slot.dtype == count.dtype == torch.int32 and slot.shape == (2 * lines, S)
    assert np.array_equal(slot[:lines].cpu().numpy(), r1) and np.array_equal(slot[lines:].cpu().numpy(), r2)
    assert np.array_equal(count.cpu().numpy(), rc)
    assert rc[0] > 0 and rc[1] == -1 and rc[2] == 0
    # masks of another integer dtype, host arrays among them
    slot2, count2 = ops.ntxent_slots(cu(masks[0].astype(np.int64)), masks[1].astype(np.int32), cu(masks[2]), torch.from_numpy(masks[3]).long())
    assert torch.equal(slot2, slot) and torch.equal(count2, count)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [12, 40, 256, 520])    # unaligned rows (scalar path), 16-byte path, half a wave of vectors, its second trip
@pytest.mark.parametrize("S", [5, 68])
def test_rows_fwd_bwd(ops, dtype, S, d):
    from pero_pretraining_amd.joint_embedding_pretraining.losses import ragged_block_rows
    n = 4
    Sp = ragged_block_rows(S, dtype)
    assert Sp == (S if dtype == F32 else 128)
    masks = list(random_masks(n, S, S + d))
    masks[0][3], masks[2][3] = 0, 1
    masks[0][3, [0, S - 2]] = 1
    masks[1][3], masks[3][3] = np.roll(masks[0][3], 1), np.roll(masks[2][3], 1)      # line 3: the same number at other positions
    slot1, slot2, count = RR.slots(*masks)
    assert count[0] > 0 and count[1] == -1 and count[2] == 0 and count[3] > 0 and not np.array_equal(slot1[3], slot2[3])
    slot_h = np.concatenate([slot1, slot2])
    slot, cnt = ops.ntxent_slots(*(cu(m) for m in masks))
    g = gen(S, d, 3)
    x = (torch.randn(2 * n, S, d, generator=g) * 1.5 + 0.2).to(dtype)
    x[0, int(np.flatnonzero(slot1[0] >= 0)[0])] = 0.0                                  # a selected all-zero row: inv = 1e12, xn = 0
    xn = torch.full((2 * n * Sp, d), 9.0, device="cuda", dtype=dtype)
    inv = torch.full((2 * n * Sp,), 9.0, device="cuda")
    ops.ntxent_rows_fwd(x.cuda().view(-1, d), slot, cnt, Sp, out=(xn, inv))            # both views stacked: one launch
    (rxn, rinv), (mxn, minv) = RR.rows_fwd(x, slot_h, count, Sp)
    # as pero_rownorm_fwd: d squares; a square root, a reciprocal and the product x inv
    assert_within(inv.view(2 * n, Sp), rinv, minv, d, F32, extra_ulps=SQRTF + DIVF, what="pero_ntxent_rows_fwd inv")
    assert_within(xn.view(2 * n, Sp, d), rxn, mxn, d, dtype, extra_ulps=SQRTF + DIVF + 1, what="pero_ntxent_rows_fwd xn")
    for l in range(2 * n):
        m = max(int(count[l % n]), 0)
        assert zero(xn.view(2 * n, Sp, d)[l, m:]) and zero(inv.view(2 * n, Sp)[l, m:]), l      # pad rows: exactly zero
    # one view alone into half of the buffers, as the two-tensor call does: the same bits
    xn2, inv2 = torch.full_like(xn, 9.0), torch.full_like(inv, 9.0)
    ops.ntxent_rows_fwd(x[n:].cuda().view(-1, d), slot[n:], cnt, Sp, out=(xn2[n * Sp:], inv2[n * Sp:]))
    assert torch.equal(xn2[n * Sp:], xn[n * Sp:]) and torch.equal(inv2[n * Sp:], inv[n * Sp:]) and float((xn2[:n * Sp].float() - 9.0).abs().max()) == 0.0
    dxn = torch.randn(2 * n, Sp, d, generator=g).to(dtype)
    for gval in (None, 0.5):
        gdev = None if gval is None else torch.full((1,), gval, device="cuda")
        dx = ops.ntxent_rows_bwd(xn, dxn.cuda().view(-1, d), inv, slot, cnt, Sp, gdev)
        rdx, mdx = RR.rows_bwd(xn.view(2 * n, Sp, d), dxn, inv.view(2 * n, Sp), slot_h, count, gval)
        assert bool(torch.isfinite(dx.float()).all())
        assert_within(dx.view(2 * n, S, d), rdx, mdx, d + 1, dtype, what="pero_ntxent_rows_bwd")   # as pero_rownorm_bwd
        unsel = torch.from_numpy((slot_h < 0) | (np.tile(count, 2)[:, None] <= 0)).cuda()
        assert bool(unsel.any()) and zero(dx.view(2 * n, S, d)[unsel])                            # unselected positions: exactly zero


def _sim(lines, Sp, counts):
    """Similarities in the m x m blocks as test_gpu_kernel_parity._sim draws them; NaN everywhere else: nothing outside a block may be read."""
    g = gen(lines, Sp, 17)
    sim = torch.full((lines, Sp, Sp), math.nan)
    for l, m in enumerate(counts):
        if m > 0:
            sim[l, :m, :m] = torch.rand(m, m, generator=g) * 20 - 10
    m0, ml = counts[0], counts[-1]
    if m0 > 7:
        sim[0, 3, 7] = 60.0                  # one dominant entry: every other term of its column is ~e^-50
    if ml > 2:
        sim[lines - 1, :ml, 2] = 4.25        # a column of identical values
    return sim, g


def _count_sets(lines, Sp):
    """Counts drawn from {1, 17, Sp - 1, Sp}: every value at least once per shape."""
    vals = [1, 17, Sp - 1, Sp]
    return [[vals[(k + l) % 4] for l in range(lines)] for k in range(4 if lines == 1 else 2 if lines == 3 else 3)]


def _check_cols(ops, sim, counts, grad_dtype, cross=None, own0=0, what="pero_ntxent_cols_ragged"):
    lines, Sp, _ = sim.shape
    L = 0 if cross is None else cross.shape[1]
    loss, line_loss, dsim, dcross = ops.ntxent_cols_ragged(sim.cuda(), i32(counts), grad_dtype, cross=None if cross is None else cross.cuda(), own0=own0)
    res, mag = RR.cols_ragged(sim, counts, cross, own0)
    # the dense kernels' counts at the block size: Sp (+ L) exponentials per column, then Sp columns (then `lines` line losses); argument
    # errors (parity_ref._lse_units), one expf per term, one logf; with negatives the two partial sums are joined by one more expf and a product
    ulps = mag["ulps"] + EXPF + LOGF + ((EXPF + 2) if cross is not None else 0)
    good = torch.tensor([m > 0 for m in counts])
    assert bool(torch.isnan(line_loss.cpu()[~good]).all())
    assert_within(line_loss.cpu()[good], res["line_loss"][good], mag["line_loss"][good], 2 * Sp + L, F32, extra_ulps=ulps, what=what + " line_loss")
    if bool(good.all()):
        assert_within(loss, res["loss"], mag["loss"], 2 * Sp + L + lines, F32, extra_ulps=ulps, what=what + " loss")
    else:
        assert math.isnan(float(loss))
    if grad_dtype is None:
        assert dsim is None and dcross is None
        return
    assert_within(dsim, res["dsim"], mag["dsim"], Sp + L, grad_dtype, extra_ulps=ulps + EXPF + 2, what=what + " dsim")
    for l, m in enumerate(counts):
        m = max(m, 0)
        assert zero(dsim[l, m:]) and zero(dsim[l, :, m:]), l                 # outside the m x m block: exactly zero
    if cross is not None:
        assert_within(dcross, res["dcross"], mag["dcross"], Sp + L, grad_dtype, extra_ulps=ulps + EXPF + 2, what=what + " dcross")
        dc = dcross.view(lines, Sp, L)
        for l, m in enumerate(counts):
            assert zero(dc[l, max(m, 0):]) and zero(dc[l, :, own0 + l]), l


@pytest.mark.parametrize("grad_dtype", [None, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("lines,Sp", [(1, 24), (3, 68), (3, 128), (2, 256)])
def test_cols_ragged(ops, grad_dtype, lines, Sp):
    for counts in _count_sets(lines, Sp):
        sim, _ = _sim(lines, Sp, counts)
        _check_cols(ops, sim, counts, grad_dtype)


@pytest.mark.parametrize("grad_dtype", DTYPES)
@pytest.mark.parametrize("bad", [-1, 0])
def test_cols_ragged_line_without_pairs(ops, grad_dtype, bad):
    counts = [17, bad, 68]
    sim, g = _sim(3, 68, counts)
    _check_cols(ops, sim, counts, grad_dtype)
    cross = torch.rand(3 * 68, 5, generator=g) * 20 - 10
    _check_cols(ops, sim, counts, grad_dtype, cross, 2)


@pytest.mark.parametrize("grad_dtype", DTYPES)
@pytest.mark.parametrize("lines,Sp,L,own0", [(1, 24, 1, 0), (3, 68, 5, 2), (3, 128, 130, 5), (2, 256, 130, 70)])   # L > 64: a lane owns two negatives
def test_cols_ragged_cross(ops, grad_dtype, lines, Sp, L, own0):
    for counts in _count_sets(lines, Sp):
        sim, g = _sim(lines, Sp, counts)
        cross = torch.full((lines, Sp, L), math.nan)
        for l, m in enumerate(counts):
            cross[l, :m] = torch.rand(m, L, generator=g) * 20 - 10
            cross[l, :m, own0 + l] = 1e4              # the line's own pooled embedding: must influence nothing
        _check_cols(ops, sim, counts, grad_dtype, cross.view(lines * Sp, L), own0)
    if L == 1:   # no negatives at all: the loss without `cross` on the same block, within that call's bound
        plain, pmag = RR.cols_ragged(sim, counts)
        got = ops.ntxent_cols_ragged(sim.cuda(), i32(counts), None, cross=cross.view(Sp, 1).cuda(), own0=0)[0]
        assert_within(got, plain["loss"], pmag["loss"], 2 * Sp + L + lines, F32, extra_ulps=pmag["ulps"] + 2 * EXPF + LOGF + 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Sp,d", [(24, 8), (128, 2056)])   # d / 8 = 257: a second block along x
def test_line_mean_and_add_line_rows_ragged(ops, dtype, Sp, d):
    counts = [1, 17, Sp, -1]
    g = gen(Sp, d, 5)
    x = (torch.randn(4 * Sp, d, generator=g) + 0.4).to(dtype)
    ref, mag = RR.line_mean_ragged(x, counts, Sp)
    got = ops.line_mean_ragged(x.cuda(), i32(counts), Sp)
    assert_within(got, ref, mag, Sp + 1, F32, extra_ulps=DIVF, what="pero_line_mean_ragged")   # up to Sp rows, then the product with 1 / count
    assert zero(got[3])
    src = torch.randn(4, d, generator=g)
    dst = x.cuda()
    ops.add_line_rows_ragged_(dst, src.cuda(), i32(counts), Sp)
    ref, mag = RR.add_line_rows_ragged(x, src, counts, Sp)
    assert_within(dst, ref, mag, 2, dtype, extra_ulps=DIVF, what="pero_add_line_rows_ragged")  # old value + src / count
    for l, m in enumerate(counts):
        m = max(m, 0)
        assert torch.equal(dst.view(4, Sp, d)[l, m:].cpu(), x.view(4, Sp, d)[l, m:])            # rows behind the count: untouched
        assert m == 0 or not torch.equal(dst.view(4, Sp, d)[l, :m].cpu(), x.view(4, Sp, d)[l, :m])


# ------------------------------------------------------------------------------------------------ loss level
def _loss_and_grads(loss_module, x, y, masks, stacked=False):
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    if stacked:
        xy = torch.cat([xg, yg]).detach().requires_grad_(True)
        loss = loss_module.forward_stacked(xy, *masks)["loss"]
        loss.backward()
        n = x.shape[0]
        return loss.detach(), xy.grad[:n], xy.grad[n:]
    loss = loss_module(xg, yg, *masks)["loss"]
    loss.backward()
    return loss.detach(), xg.grad, yg.grad


def _literal(x, y, masks, cross=False):
    xo, yo = x.detach().cpu().double().requires_grad_(True), y.detach().cpu().double().requires_grad_(True)
    ref = RR.loss(xo, yo, *masks, cross=cross)
    ref.backward()
    return float(ref), xo.grad, yo.grad


def _xy(n, S, D, seed, noise=0.7):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, S, D)).astype(np.float32)
    return cu(x), cu((x + noise * rng.standard_normal((n, S, D))).astype(np.float32))


def _close(got, ref, rel):
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else ref
    return np.abs(got.float().cpu().numpy() - ref).max() < rel * np.abs(ref).max() + 1e-8


def test_g24_reference_loss_and_gradients(golden):
    from pero_pretraining_amd.joint_embedding_pretraining.losses import NTXentLoss
    g = golden("g24_ntxent_image_masks.npz")
    masks = [cu(g[k]) for k in G24_MASKS]
    loss, gx, gy = _loss_and_grads(NTXentLoss(apply_masks=True), cu(g["x"]), cu(g["y"]), masks)
    assert abs(float(loss) - float(g["loss"])) < 1e-4 * float(g["loss"])
    assert _close(gx, g["grad_x"], 1e-4) and _close(gy, g["grad_y"], 1e-4)
    with pytest.raises(IndexError):      # the default keeps the reference's behaviour on these masks
        NTXentLoss()(cu(g["x"]), cu(g["y"]), *masks)


@pytest.fixture(scope="module")
def collated():
    """Masks as the collator draws them for widths 480, 512, 400, 130, 512 (S = 68), f32 inputs, and the f64 loss and gradients."""
    masks = RR.collated_masks()
    x, y = _xy(5, 68, 40, 11)
    return masks, x, y, _literal(x, y, masks)


def test_collated_masks_f32_match_the_f64_loss(collated):
    from pero_pretraining_amd.joint_embedding_pretraining.losses import NTXentLoss
    masks, x, y, (ref, rgx, rgy) = collated
    dev = [cu(m) for m in masks]
    loss, gx, gy = _loss_and_grads(NTXentLoss(apply_masks=True), x, y, dev)
    assert abs(float(loss) - ref) < 1e-4 * ref
    assert _close(gx, rgx, 1e-4) and _close(gy, rgy, 1e-4)
    sel1, sel2 = (torch.from_numpy(~RR.selected(masks[i], masks[i + 2])).cuda() for i in (0, 1))
    assert bool(sel1.any()) and zero(gx[sel1]) and zero(gy[sel2])               # unselected positions: exactly zero
    # stacked and two-tensor calls agree
    loss_s, gxs, gys = _loss_and_grads(NTXentLoss(apply_masks=True), x, y, dev, stacked=True)
    assert float(loss_s) == float(loss) and torch.equal(gxs, gx) and torch.equal(gys, gy)
    # masks with host twins (what BatchCreator and the batch operators hand over) and masks that exist on the device only: same values
    twins = [cu(m) for m in masks]
    for t, m in zip(twins, masks):
        t._pero_host = m
    loss_t, gxt, gyt = _loss_and_grads(NTXentLoss(apply_masks=True), x, y, twins)
    assert float(loss_t) == float(loss) and torch.equal(gxt, gx) and torch.equal(gyt, gy)


def test_collated_masks_bf16_tile_kernel():
    """n = 3, S = 132, D = 256: blocks of Sp = 256 rows, the three per-line products take the bf16 tile kernel; the bounds of
    test_gpu_joint.py::test_ntxent_bf16_batched_fast_path."""
    import pero_pretraining_amd as P
    from pero_pretraining_amd import ops
    from pero_pretraining_amd.joint_embedding_pretraining.losses import NTXentLoss, ragged_block_rows
    assert ragged_block_rows(132, torch.bfloat16) == 256
    masks = RR.collated_masks(widths=(1000, 777, 1024))
    assert masks[0].shape == (3, 132)
    x, y = _xy(3, 132, 256, 12, noise=0.5)
    xb, yb = x.bfloat16(), y.bfloat16()
    ref, rgx, _ = _literal(xb, yb, masks)
    ops.gemm_timeline = []
    try:
        with P.autocast(True):
            loss, gx, _ = _loss_and_grads(NTXentLoss(apply_masks=True), xb, yb, [cu(m) for m in masks])
        tags = [t[3] for t in ops.gemm_timeline]
    finally:
        ops.gemm_timeline = None
    assert len(tags) == 3 and all(t.startswith("gemm_bf16_tile") for t in tags), tags
    assert abs(float(loss) - ref) < 2e-2 * ref
    gx = gx.float().cpu().double()
    cos = float((gx.flatten() @ rgx.flatten()) / (gx.norm() * rgx.norm()))
    assert cos > 0.99, cos


def test_all_ones_masks_equal_the_default_loss():
    from pero_pretraining_amd.joint_embedding_pretraining.losses import NTXentLoss
    x, y = _xy(3, 24, 40, 13)
    ones = [torch.ones((3, 24), dtype=torch.uint8).cuda()] * 4
    for cross in (False, True):
        loss, gx, gy = _loss_and_grads(NTXentLoss(apply_masks=True, cross_rank_negatives=cross), x, y, ones)
        dl, dgx, dgy = _loss_and_grads(NTXentLoss(cross_rank_negatives=cross), x, y, ones)
        assert abs(float(loss) - float(dl)) <= 1e-6 * float(dl)
        assert _close(gx, dgx.cpu(), 1e-6) and _close(gy, dgy.cpu(), 1e-6)


def test_unselected_padding_columns_change_nothing(collated):
    from pero_pretraining_amd.joint_embedding_pretraining.losses import NTXentLoss
    masks, x, y, _ = collated
    loss, gx, gy = _loss_and_grads(NTXentLoss(apply_masks=True), x, y, [cu(m) for m in masks])
    pad = 9
    wide = [np.concatenate([m, np.full((5, pad), v, np.uint8)], axis=1) for m, v in zip(masks, (0, 0, 2, 0))]
    xw, yw = _xy(5, 68 + pad, 40, 14)
    xw[:, :68], yw[:, :68] = x, y
    lw, gxw, gyw = _loss_and_grads(NTXentLoss(apply_masks=True), xw, yw, [cu(m) for m in wide])
    assert abs(float(lw) - float(loss)) <= 1e-6 * float(loss)
    assert _close(gxw[:, :68], gx.cpu(), 1e-6) and _close(gyw[:, :68], gy.cpu(), 1e-6) and zero(gxw[:, 68:]) and zero(gyw[:, 68:])


def test_line_without_pairs_raises_with_host_twins_and_is_nan_without(collated):
    from pero_pretraining_amd.joint_embedding_pretraining.losses import NTXentLoss
    masks, x, y, _ = collated
    bad = [m.copy() for m in masks]
    bad[0][1, int(np.flatnonzero(RR.selected(masks[0][1], masks[2][1]))[0])] = 0       # line 1: 63 positions in view 1, 64 in view 2
    twins = [cu(m) for m in bad]
    for t, m in zip(twins, bad):
        t._pero_host = m
    with pytest.raises(ValueError, match="line 1 selects 63 positions in view 1 and 64 in view 2"):
        NTXentLoss(apply_masks=True)(x, y, *twins)
    with pytest.raises(ValueError, match="line 1"):
        NTXentLoss(apply_masks=True)(x, y, *bad)                                         # host arrays are their own twins
    loss, gx, gy = _loss_and_grads(NTXentLoss(apply_masks=True), x, y, [cu(m) for m in bad])
    assert math.isnan(float(loss)) and zero(gx[1]) and zero(gy[1]) and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all())
    assert not zero(gx[0])


def test_cross_negatives_one_rank_match_the_f64_loss(collated):
    from pero_pretraining_amd.joint_embedding_pretraining.losses import NTXentLoss
    masks, x, y, (plain, _, _) = collated
    ref, rgx, rgy = _literal(x, y, masks, cross=True)
    dev = [cu(m) for m in masks]
    loss, gx, gy = _loss_and_grads(NTXentLoss(apply_masks=True, cross_rank_negatives=True), x, y, dev)
    assert abs(float(loss) - ref) < 1e-4 * ref and ref > plain          # more negatives in every normaliser
    assert _close(gx, rgx, 1e-4) and _close(gy, rgy, 1e-4)
    loss_s, gxs, gys = _loss_and_grads(NTXentLoss(apply_masks=True, cross_rank_negatives=True), x, y, dev, stacked=True)
    assert float(loss_s) == float(loss) and torch.equal(gxs, gx) and torch.equal(gys, gy)


# ------------------------------------------------------------------------------------------------ end to end
def test_collated_batch_trains_with_ntxent():
    from pero_pretraining_amd.common.dataloader import BatchCreator
    from pero_pretraining_amd.joint_embedding_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.joint_embedding_pretraining.train import init_model
    from pero_pretraining_amd.joint_embedding_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    rng = np.random.default_rng(15)
    data = [{"image": rng.integers(0, 256, (40, w, 3), dtype=np.uint8), "image2": rng.integers(0, 256, (40, w, 3), dtype=np.uint8), "labels": None,
             "image_id": str(i)} for i, w in enumerate((480, 512, 400, 130, 512))]
    np.random.seed(3)
    batch = BatchCreator().create_batch(data)
    assert batch["image_masks"].shape == (5, 68) and not bool((batch["shift_masks"] == 1).all())
    torch.manual_seed(0)
    definitions = ({"type": "vit", "num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128},
                   {"type": "linear", "in_features": 64, "out_features": 80})
    model = init_model(torch.device("cuda", 0), *definitions, loss_type="ntxent", ntxent_apply_masks=True).train()
    bop = BatchOperator(torch.device("cuda", 0))
    prepared = bop.prepare_batch(batch)
    out = model(*prepared)
    masks = [m.cpu().numpy() for m in prepared[2:]]
    ref = float(RR.loss(out["output1"].cpu().double(), out["output2"].cpu().double(), *masks))
    assert abs(float(out["loss"]) - ref) < 1e-4 * ref
    trainer = Trainer(bop, model, None, FusedAdam(model.parameters(), lr=1e-3), None, bfloat16=False)
    losses = [float(trainer.train_step(batch)) for _ in range(2)]
    assert all(math.isfinite(l) for l in losses), losses
    plain = init_model(torch.device("cuda", 0), *definitions, loss_type="ntxent").train()
    with pytest.raises(IndexError):
        plain(*prepared)
