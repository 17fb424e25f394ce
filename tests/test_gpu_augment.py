"""GPU: pero_augment_stack_lines (csrc/augment.hip) bit for bit against tests/augment_ref.py - the numpy restatement of the formulas in
include/pero_hip.h that test_augment_ref_cpu.py anchors -, then the collator with a LineAugmenter, then one joint-embedding step on an
augmented batch.  Every comparison is np.array_equal / torch.equal; the step is only asked for a finite loss.

Kernel outputs are views inside a larger allocation (`Guarded`): 0xA5 in front and behind must survive, and the output itself starts
as 0x5C, so that a byte the kernel skipped fails the comparison."""
import math

import numpy as np
import pytest
import torch

import augment_ref as A
import datapath_ref as D

pytestmark = pytest.mark.gpu
KS = 5


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    return _ops


class Guarded:
    """`t`: a uint8 tensor of `shape` that starts `guard` bytes (a multiple of 16) into its allocation and ends `guard` bytes before
    its end."""

    def __init__(self, shape, guard):
        nbytes = int(np.prod(shape))
        assert guard % 16 == 0 and guard >= 16
        self.raw = torch.full((2 * guard + nbytes,), 0xA5, device="cuda", dtype=torch.uint8)
        self.raw[guard:guard + nbytes].fill_(0x5C)
        self.t = self.raw[guard:guard + nbytes].view(shape)
        self.guard = guard
        assert self.t.data_ptr() % 16 == 0

    def check(self):
        g = self.guard
        assert int(self.raw[:g].min()) == 0xA5 and int(self.raw[:g].max()) == 0xA5, "bytes in front of the output were written"
        assert int(self.raw[-g:].min()) == 0xA5 and int(self.raw[-g:].max()) == 0xA5, "bytes behind the output were written"
        return self.t


def _device_run(ops, packed, offsets, widths, left, params, knots, lut, H, Wt, C, ks=KS):
    """The C entry on exactly these arrays (packed: the lines and the 8 slack bytes, 0xFF - a consumed one is a wrong pixel)."""
    from pero_pretraining_amd._lib import call
    B = len(widths)
    assert packed.size == int(widths.astype(np.int64).sum()) * H * C + 8
    out = Guarded((B, H, Wt, C), (Wt * C + 16 + 15) // 16 * 16)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (packed, offsets, widths, left, params, knots)]
    lut_d = None if lut is None else torch.from_numpy(np.ascontiguousarray(lut)).cuda()
    call("pero_augment_stack_lines", *(ops.ptr(t) for t in dev), ops.ptr(lut_d), ops.ptr(out.t), B, H, Wt, C, A.P, ks, ops.stream())
    return out.check().cpu().numpy()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H", [1, 5, 40])
@pytest.mark.parametrize("line_set", range(len(A.LINE_SETS)))
def test_kernel_matches_the_reference(ops, line_set, H, C):
    lines, neutral_line = A.LINE_SETS[line_set]
    packed, offsets, widths, left, params, knots, lut = A.case(C, H, A.WT, lines, neutral_line)
    got = _device_run(ops, packed, offsets, widths, left, params, knots, lut, H, A.WT, C)
    want = A.augment_stack_lines(packed, offsets, widths, left, params, knots, lut, len(widths), H, A.WT, C, KS)
    assert np.array_equal(got, want)
    plain = D.stack_lines(packed, offsets, widths, left, len(widths), H, A.WT, C)
    assert np.array_equal(got[neutral_line], plain[neutral_line]) and not np.array_equal(got, plain)   # the neutral line is a copy


@pytest.mark.parametrize("ks", [3, 8])
def test_kernel_at_the_smallest_and_the_largest_knot_spacing(ops, ks):
    C, H = 3, 5
    lines, _ = A.LINE_SETS[1]
    packed, offsets, widths, left, params, knots, lut = A.case(C, H, A.WT, lines, None, ks)
    got = _device_run(ops, packed, offsets, widths, left, params, knots, lut, H, A.WT, C, ks)
    assert np.array_equal(got, A.augment_stack_lines(packed, offsets, widths, left, params, knots, lut, len(widths), H, A.WT, C, ks))


@pytest.mark.parametrize("C", [2, 4])            # the kernel is instantiated per channel count: the two that the cases above leave out
def test_kernel_with_two_and_four_channels(ops, C):
    H = 5
    lines, neutral_line = A.LINE_SETS[0]
    packed, offsets, widths, left, params, knots, lut = A.case(C, H, A.WT, lines, neutral_line)
    got = _device_run(ops, packed, offsets, widths, left, params, knots, lut, H, A.WT, C)
    assert np.array_equal(got, A.augment_stack_lines(packed, offsets, widths, left, params, knots, lut, len(widths), H, A.WT, C, KS))


def test_kernel_with_more_than_256_chunks_per_row(ops):
    C, Wt = A.WIDE_C, A.WIDE_WT                 # 257 chunks of 16 bytes per row: more than one block along the row
    packed, offsets, widths, left, params, knots, lut = A.case(C, 1, Wt, A.WIDE_LINES)
    assert Wt * C // 16 > 256
    got = _device_run(ops, packed, offsets, widths, left, params, knots, lut, 1, Wt, C)
    assert np.array_equal(got, A.augment_stack_lines(packed, offsets, widths, left, params, knots, lut, 2, 1, Wt, C, KS))


@pytest.mark.parametrize("C,H", [(1, 1), (3, 5), (1, 40)])
def test_extreme_parameters_only_clamp(ops, C, H):
    """INT32_MIN / INT32_MAX in every parameter and knot: the formulas index in bounds for them (asserted on the reference in
    test_augment_ref_cpu.py), so the kernel reads the line's own pixels and gives the reference's bytes."""
    for lines, _ in A.LINE_SETS:
        packed, offsets, widths, left, params, knots, lut = A.extreme_case(C, H, A.WT, lines)
        got = _device_run(ops, packed, offsets, widths, left, params, knots, lut, H, A.WT, C)
        assert np.array_equal(got, A.augment_stack_lines(packed, offsets, widths, left, params, knots, lut, len(widths), H, A.WT, C, KS))


def test_null_tone_curve_is_the_identity_curve(ops):
    C, H = 3, 5
    lines, neutral_line = A.LINE_SETS[0]
    packed, offsets, widths, left, params, knots, _ = A.case(C, H, A.WT, lines, neutral_line)
    identity = A.neutral(len(widths), A.WT, C, KS)[2]
    a = _device_run(ops, packed, offsets, widths, left, params, knots, None, H, A.WT, C)
    b = _device_run(ops, packed, offsets, widths, left, params, knots, identity, H, A.WT, C)
    assert np.array_equal(a, b)
    assert np.array_equal(a, A.augment_stack_lines(packed, offsets, widths, left, params, knots, None, len(widths), H, A.WT, C, KS))


@pytest.mark.parametrize("C,H", [(1, 1), (3, 40), (4, 3)])
def test_neutral_parameters_give_stack_lines_on_the_device(ops, C, H):
    packed, offsets, widths, left = D.stack_lines_case(C, H)                       # datapath_ref's lines: every residue modulo 4
    B, Wt = len(widths), D.STACK_LINES_WT
    packed_d, off_d, w_d, left_d = (torch.from_numpy(a).cuda() for a in (packed, offsets, widths, left))
    params, knots, lut = (torch.from_numpy(a).cuda() for a in A.neutral(B, Wt, C, KS))
    plain = ops.stack_lines(packed_d, off_d, w_d, left_d, B, H, Wt, C)
    assert torch.equal(ops.augment_stack_lines(packed_d, off_d, w_d, left_d, params, knots, lut, B, H, Wt, C, KS), plain)
    assert torch.equal(ops.augment_stack_lines(packed_d, off_d, w_d, left_d, params, knots, None, B, H, Wt, C), plain)


# ------------------------------------------------------------------------------------------------ the collator
WIDTHS = (50, 300, 128, 77, 203, 256)
ZERO = dict(max_slope=0, max_slant=0, scale_range=0, max_translate=0, warp_amplitude_y=0, warp_amplitude_x=0, brightness=0,
            contrast=0, gamma=0, channel_gain=0, noise_sigma=0)
KEYS = ("images", "images2", "image_masks", "image_masks2", "shift_masks", "shift_masks2")


def _data():
    rng = np.random.default_rng(21)
    return [{"image": rng.integers(0, 256, (40, w, 3), dtype=np.uint8), "image2": rng.integers(0, 256, (40, w, 3), dtype=np.uint8),
             "labels": rng.integers(0, 50, w // 8), "image_id": str(i)} for i, w in enumerate(WIDTHS)]


def _batch(**kwargs):
    """The batch, and the left paddings the collator drew for both views."""
    from pero_pretraining_amd.common.dataloader import BatchCreator
    np.random.seed(9)
    batch = BatchCreator(**kwargs).create_batch(_data())
    lefts = [[int(row.argmax()) for row in batch[k].cpu().numpy()] for k in ("image_masks", "image_masks2")]   # first position of the line
    return batch, lefts[0], lefts[1]


@pytest.fixture(scope="module")
def plain():
    return _batch()


def _same_layout(got, want):
    (b, l1, l2), (pb, pl1, pl2) = got, want
    assert l1 == pl1 and l2 == pl2 and b["shifts"] == pb["shifts"] and b["ids"] == pb["ids"]
    assert np.array_equal(b["labels"], pb["labels"])
    for k in KEYS[2:]:
        assert torch.equal(b[k], pb[k]) and np.array_equal(b[k]._pero_host, pb[k]._pero_host), k
    assert b["original_images"] is None and b["original_images2"] is None


def test_zero_magnitude_augmenter_changes_nothing(plain):
    from pero_pretraining_amd.common.augment import LineAugmenter
    got = _batch(augmenter=LineAugmenter(seed=1, p=1.0, **ZERO))
    _same_layout(got, plain)
    assert torch.equal(got[0]["images"], plain[0]["images"]) and torch.equal(got[0]["images2"], plain[0]["images2"])


def test_augmenter_changes_the_pixels_and_nothing_else(plain):
    from pero_pretraining_amd.common.augment import LineAugmenter
    got = _batch(augmenter=LineAugmenter(seed=1, p=1.0))
    _same_layout(got, plain)
    sub = 8
    for key, lefts in (("images", got[1]), ("images2", got[2])):
        img, ref = got[0][key].cpu().numpy(), plain[0][key].cpu().numpy()
        assert img.shape == ref.shape and img.dtype == np.uint8
        for b, (w, lp) in enumerate(zip(WIDTHS, lefts)):
            lo, hi = lp * sub, lp * sub + w
            assert not img[b, :, :lo].any() and not img[b, :, hi:].any()            # outside the line's span: zero
            assert not np.array_equal(img[b, :, lo:hi], ref[b, :, lo:hi])            # inside: augmented
    again = _batch(augmenter=LineAugmenter(seed=1, p=1.0))
    assert torch.equal(again[0]["images"], got[0]["images"]) and torch.equal(again[0]["images2"], got[0]["images2"])
    other = _batch(augmenter=LineAugmenter(seed=2, p=1.0))
    assert not torch.equal(other[0]["images"], got[0]["images"])


def test_the_two_views_get_their_own_draws(plain):
    """The same pixels in both views, the same left paddings: the views differ by their draws alone."""
    from pero_pretraining_amd.common.augment import LineAugmenter
    from pero_pretraining_amd.common.dataloader import BatchCreator
    data = _data()
    for d in data:
        d["image2"] = d["image"]
    np.random.seed(9)
    same = BatchCreator(same_left_paddings=True).create_batch(data)
    assert torch.equal(same["images"], same["images2"])
    np.random.seed(9)
    b = BatchCreator(same_left_paddings=True, augmenter=LineAugmenter(seed=1, p=1.0)).create_batch(data)
    assert not torch.equal(b["images"], b["images2"]) and not torch.equal(b["images"], same["images"])
    assert torch.equal(b["image_masks"], b["image_masks2"])


def test_augment_views_selects_the_views(plain):
    from pero_pretraining_amd.common.augment import LineAugmenter
    got = _batch(augmenter=LineAugmenter(seed=1, p=1.0), augment_views=(False, True))
    _same_layout(got, plain)
    assert torch.equal(got[0]["images"], plain[0]["images"]) and not torch.equal(got[0]["images2"], plain[0]["images2"])
    none = _batch(augmenter=LineAugmenter(seed=1, p=1.0), augment_views=(False, False))
    assert torch.equal(none[0]["images"], plain[0]["images"]) and torch.equal(none[0]["images2"], plain[0]["images2"])


# ------------------------------------------------------------------------------------------------ one step
def test_joint_embedding_step_on_an_augmented_batch():
    from pero_pretraining_amd.common.augment import LineAugmenter
    from pero_pretraining_amd.joint_embedding_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.joint_embedding_pretraining.train import init_model
    from pero_pretraining_amd.joint_embedding_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    batch, _, _ = _batch(augmenter=LineAugmenter(seed=3))
    torch.manual_seed(0)
    model = init_model(torch.device("cuda", 0), {"type": "vit", "num_blocks": 2, "model_dim": 128, "num_heads": 4, "feedforward_dim": 256},
                       {"type": "linear", "in_features": 128, "out_features": 80}, loss_type="ntxent", ntxent_apply_masks=True).train()
    trainer = Trainer(BatchOperator(torch.device("cuda", 0)), model, None, FusedAdam(model.parameters(), lr=1e-3), None, bfloat16=False)
    assert math.isfinite(float(trainer.train_step(batch)))
