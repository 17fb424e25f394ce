"""CPU: anchors of tests/augment_ref.py (the numpy restatement of pero_augment_stack_lines that test_gpu_augment.py holds the kernel
to) against things that need no formula - slice copies, shifts, np.take -, the host side of the C entry, and LineAugmenter.draw."""
import ctypes

import numpy as np
import pytest
import torch

import augment_ref as A
import datapath_ref as D

KS = 5


def _one_line(H, w, C, Wt, left=0, seed=0):
    lines = [(w, left)]
    packed, offsets, widths, left_px = D.stack_lines_case(C, H, Wt, lines, seed)
    return packed, offsets, widths, left_px, packed[:H * w * C].reshape(H, w, C)


def _run(packed, offsets, widths, left, params, knots, lut, H, Wt, C, ks=KS):
    return A.augment_stack_lines(packed, offsets, widths, left, params, knots, lut, len(widths), H, Wt, C, ks)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H", [1, 5, 40])
def test_neutral_parameters_are_stack_lines(C, H):
    for lines, _ in A.LINE_SETS:
        packed, offsets, widths, left = D.stack_lines_case(C, H, A.WT, lines)
        params, knots, lut = A.neutral(len(widths), A.WT, C, KS)
        want = D.stack_lines(packed, offsets, widths, left, len(widths), H, A.WT, C)
        assert np.array_equal(_run(packed, offsets, widths, left, params, knots, lut, H, A.WT, C), want)
        assert np.array_equal(_run(packed, offsets, widths, left, params, knots, None, H, A.WT, C), want)


@pytest.mark.parametrize("k", [-7, -2, -1, 1, 3, 6])
def test_whole_pixel_translation_is_a_row_shift_with_edge_replication(k):
    H, w, C, Wt = 5, 33, 3, 64
    packed, offsets, widths, left, line = _one_line(H, w, C, Wt, left=7)
    params, knots, lut = A.neutral(1, Wt, C, KS)
    params[0, A.TY] = 256 * k
    got = _run(packed, offsets, widths, left, params, knots, lut, H, Wt, C)
    want = np.zeros((1, H, Wt, C), dtype=np.uint8)
    want[0, :, 7:7 + w] = line[np.clip(np.arange(H) + k, 0, H - 1)]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k", [-40, -3, 1, 2, 35])
def test_constant_horizontal_knots_are_a_column_shift(k):
    H, w, C, Wt = 3, 70, 1, 96
    packed, offsets, widths, left, line = _one_line(H, w, C, Wt, left=11)
    params, knots, lut = A.neutral(1, Wt, C, KS)
    knots[0, 1, :] = 256 * k
    got = _run(packed, offsets, widths, left, params, knots, lut, H, Wt, C)
    want = np.zeros((1, H, Wt, C), dtype=np.uint8)
    want[0, :, 11:11 + w] = line[:, np.clip(np.arange(w) + k, 0, w - 1)]
    assert np.array_equal(got, want)


def test_tone_curve_alone_is_np_take():
    H, w, C, Wt = 5, 31, 3, 32
    packed, offsets, widths, left, line = _one_line(H, w, C, Wt, left=1)
    params, knots, lut = A.neutral(1, Wt, C, KS)
    lut[0] = np.random.default_rng(3).integers(0, 256, (C, 256), dtype=np.uint8)
    got = _run(packed, offsets, widths, left, params, knots, lut, H, Wt, C)
    for c in range(C):
        assert np.array_equal(got[0, :, 1:1 + w, c], np.take(lut[0, c], line[:, :, c]))
    assert not np.array_equal(got[0, :, 1:1 + w], line)


def test_half_pixel_taps_average():
    H, w, C, Wt = 2, 2, 1, 16
    packed = np.array([10, 20, 10, 20] + [0xFF] * 8, dtype=np.uint8)
    offsets, widths, left = np.array([0], dtype=np.int64), np.array([w], dtype=np.int32), np.array([0], dtype=np.int32)
    params, knots, lut = A.neutral(1, Wt, C, KS)
    knots[0, 1, :] = 128                                      # half a pixel to the right
    got = _run(packed, offsets, widths, left, params, knots, lut, H, Wt, C)
    assert got[0, :, 0, 0].tolist() == [15, 15] and got[0, :, 1, 0].tolist() == [20, 20]      # the second column's +1 tap is the edge
    packed[:4] = [10, 10, 20, 20]
    knots[:] = 0
    params[0, A.TY] = 128                                     # half a pixel down
    got = _run(packed, offsets, widths, left, params, knots, lut, H, Wt, C)
    assert got[0, 0, :2, 0].tolist() == [15, 15] and got[0, 1, :2, 0].tolist() == [20, 20]


def test_zero_noise_amplitude_adds_nothing():
    C, H = 3, 5
    lines, _ = A.LINE_SETS[1]
    packed, offsets, widths, left, params, knots, lut = A.case(C, H, A.WT, lines)
    params[:, A.NOISE_AMP] = 0
    quiet = _run(packed, offsets, widths, left, params, knots, lut, H, A.WT, C)
    params[:, A.SEED_LO:] += 12345                            # the seed is not read either
    assert np.array_equal(_run(packed, offsets, widths, left, params, knots, lut, H, A.WT, C), quiet)
    params[:, A.NOISE_AMP] = A.noise_amp(4.0)
    assert not np.array_equal(_run(packed, offsets, widths, left, params, knots, lut, H, A.WT, C), quiet)


# with this seed (lo, hi) the 81 920 noise values of the test below have mean -0.0187 and standard deviation 8.0126
NOISE_SEED = (20261, 7)


def test_noise_has_the_documented_mean_and_deviation():
    H, w, C = 40, 2048, 1
    packed = np.concatenate([np.full(H * w, 128, dtype=np.uint8), np.full(8, 0xFF, dtype=np.uint8)])
    offsets, widths, left = np.array([0], dtype=np.int64), np.array([w], dtype=np.int32), np.array([0], dtype=np.int32)
    params, knots, lut = A.neutral(1, w, C, KS)
    params[0, A.NOISE_AMP] = A.noise_amp(8.0)
    assert params[0, A.NOISE_AMP] == 3547
    params[0, A.SEED_LO], params[0, A.SEED_HI] = NOISE_SEED
    n = _run(packed, offsets, widths, left, params, knots, lut, H, w, C)[0, :, :, 0].astype(np.int64) - 128
    assert -28 <= n.min() and n.max() <= 28                             # |s| <= 510: 510 * 3547 / 65536 = 27.6, nothing clamps at 128
    mean, std = float(n.mean()), float(n.std())
    print(f"noise mean {mean:.4f} std {std:.4f}")
    assert abs(mean) <= 0.1 and abs(std - 8.0) <= 0.05 * 8.0
    # two seeds give two fields, and the field does not repeat from row to row
    params[0, A.SEED_HI] += 1
    other = _run(packed, offsets, widths, left, params, knots, lut, H, w, C)[0, :, :, 0].astype(np.int64) - 128
    assert abs(float(np.corrcoef(n.reshape(-1), other.reshape(-1))[0, 1])) < 0.02
    assert abs(float(np.corrcoef(n[0], n[1])[0, 1])) < 0.1


@pytest.mark.parametrize("C,H", [(1, 1), (3, 5), (1, 40)])
def test_extreme_parameters_index_in_bounds(C, H):
    for lines, _ in A.LINE_SETS:
        packed, offsets, widths, left, params, knots, lut = A.extreme_case(C, H, A.WT, lines)
        assert set(np.unique(params)) == {A.INT32_MIN, A.INT32_MAX} == set(np.unique(knots))
        NK = A.num_knots(A.WT, KS)
        for b, w in enumerate(widths.tolist()):
            ys, xs, y0, y1, x0, x1, j = A.taps(w, H, params[b], knots[b], KS)
            assert ys.dtype == np.int64 and float(np.abs(ys.astype(np.float64)).max()) < 2.0 ** 58           # far from wrapping
            assert float(np.abs(xs.astype(np.float64)).max()) < 2.0 ** 58
            for v, n in ((y0, H), (y1, H), (x0, w), (x1, w), (j, NK - 1)):
                assert int(v.min()) >= 0 and int(v.max()) < n
        out = _run(packed, offsets, widths, left, params, knots, lut, H, A.WT, C)       # numpy would raise on a positive overrun
        for b, (w, lp) in enumerate(zip(widths.tolist(), left.tolist())):
            assert not out[b, :, :lp].any() and not out[b, :, lp + w:].any()


# ------------------------------------------------------------------------------------------------ the C entry's host side
def test_entry_validates_its_arguments_without_a_gpu():
    from pero_pretraining_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(64)                                   # never dereferenced: every call below fails its host checks

    def entry(ptrs=(p,) * 8, B=2, H=5, Wt=96, C=1, P=A.P, ks=5):
        return h.pero_augment_stack_lines(*ptrs, B, H, Wt, C, P, ks, None)
    name = b"pero_augment_stack_lines"
    assert entry((None,) * 8) < 0 and name + b": null pointer" in h.pero_last_error()
    for i in (0, 1, 2, 3, 4, 5, 7):                           # every pointer but the tone curve, which may be null
        assert entry(tuple(None if k == i else p for k in range(8))) < 0 and name + b": null pointer" in h.pero_last_error()
    for ks in (2, 9, -1):
        assert entry(ks=ks) < 0 and name in h.pero_last_error() and b"knot_shift" in h.pero_last_error()
    assert entry(P=8) < 0 and name in h.pero_last_error() and b"params" in h.pero_last_error()
    assert entry(Wt=100) < 0 and name in h.pero_last_error() and b"16-byte" in h.pero_last_error()
    for bad in ({"B": 0}, {"H": 0}, {"H": 65536}, {"C": 0}, {"C": 5, "Wt": 80}, {"Wt": 1 << 24}):
        assert entry(**bad) < 0 and name + b": bad sizes" in h.pero_last_error(), bad


def test_ops_wrapper_checks_on_the_host():
    from pero_pretraining_amd import ops
    B, H, Wt, C = 2, 5, 96, 3
    params, knots, lut = (torch.from_numpy(a) for a in A.neutral(B, Wt, C, KS))
    packed = torch.zeros(100, dtype=torch.uint8)
    offsets, widths, left = torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    good = dict(packed=packed, offsets=offsets, widths=widths, left_px=left, params=params, knots=knots, lut=lut)
    for key, bad in (("offsets", offsets.int()), ("widths", widths.long()), ("params", params[:, :6].contiguous()),
                     ("params", params.long()), ("knots", knots[:, :, 1:].contiguous()), ("knots", knots.transpose(0, 1)),
                     ("lut", lut[:, :1].contiguous()), ("lut", lut.int()), ("packed", packed.int())):
        with pytest.raises(ValueError, match=key):
            ops.augment_stack_lines(**{**good, key: bad}, B=B, H=H, Wt=Wt, C=C)
    with pytest.raises(ValueError, match="GPU"):              # everything well formed, but on the host
        ops.augment_stack_lines(**good, B=B, H=H, Wt=Wt, C=C)


# ------------------------------------------------------------------------------------------------ LineAugmenter.draw
def _draw(aug, B=16, H=40, Wt=512, C=3):
    return aug.draw([Wt - 7] * B, H, Wt, C)


def test_draw_is_reproducible_and_leaves_numpy_alone():
    from pero_pretraining_amd.common.augment import LineAugmenter
    np.random.seed(5)
    state = np.random.get_state()
    a, b = _draw(LineAugmenter(seed=11)), _draw(LineAugmenter(seed=11))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = _draw(LineAugmenter(seed=12))
    assert not any(torch.equal(x, y) for x, y in zip(a, c))
    aug = LineAugmenter(seed=11)
    first, second = _draw(aug), _draw(aug)                    # one augmenter: a new draw per call (the two views differ)
    assert all(torch.equal(x, y) for x, y in zip(a, first)) and not any(torch.equal(x, y) for x, y in zip(first, second))
    now = np.random.get_state()
    assert now[0] == state[0] and np.array_equal(now[1], state[1]) and now[2:] == state[2:]
    params, knots, lut = a
    assert params.dtype == torch.int32 and params.shape == (16, A.P) and params.is_contiguous() and not params.is_cuda
    assert knots.dtype == torch.int32 and knots.shape == (16, 2, A.num_knots(512, 5)) and knots.is_contiguous()
    assert lut.dtype == torch.uint8 and lut.shape == (16, 3, 256) and lut.is_contiguous()


def test_draw_stays_inside_the_documented_ranges():
    from pero_pretraining_amd.common.augment import LineAugmenter
    kw = dict(max_slope=0.03, max_slant=0.2, scale_range=0.1, max_translate=2.0, warp_amplitude_y=1.5, warp_amplitude_x=3.0,
              noise_sigma=5.0, p=1.0)
    params, knots, lut = (t.numpy().astype(np.int64) for t in _draw(LineAugmenter(seed=0, **kw), B=512))
    up = lambda v: int(np.ceil(256 * v))
    for col, bound, centre in ((A.SY, up(0.1), 256), (A.TY, up(2.0), 0), (A.SLOPE, up(0.03), 0), (A.SLANT, up(0.2), 0)):
        d = params[:, col] - centre
        assert d.min() >= -bound and d.max() <= bound and d.min() < -bound // 2 and d.max() > bound // 2, col   # and it uses the range
    assert params[:, A.NOISE_AMP].min() >= 0 and params[:, A.NOISE_AMP].max() <= A.noise_amp(5.0)
    assert len(np.unique(params[:, A.SEED_LO])) == 512
    assert np.abs(knots[:, 0]).max() <= up(1.5) and np.abs(knots[:, 1]).max() <= up(3.0) < 8 * 256
    assert np.abs(knots[:, 0]).max() > up(1.5) // 2 and np.abs(knots[:, 1]).max() > up(3.0) // 2
    # smooth: neighbouring knots are 32 px apart on a smoothstep between draws 64 px apart (slope at most 1.5 x the draws' difference
    # per 64 px): they differ by at most 1.5 x amplitude, where independent knots would differ by up to 2 x amplitude
    assert np.abs(np.diff(knots[:, 1], axis=1)).max() <= 1.5 * up(3.0) + 1
    assert (np.diff(lut, axis=2) >= 0).all()                 # every tone curve is monotone
    from pero_pretraining_amd.common.dataloader import BatchCreator
    with pytest.raises(ValueError, match="patch"):            # a pixel must not leave its label
        BatchCreator(augmenter=LineAugmenter(warp_amplitude_x=8.0))
    assert BatchCreator(subsampling_factor=16, augmenter=LineAugmenter(warp_amplitude_x=8.0)).augment_views == (True, True)
    with pytest.raises(ValueError, match="warp_period"):
        LineAugmenter(warp_period=16)


def test_zero_magnitudes_and_p_zero_draw_the_neutral_values():
    from pero_pretraining_amd.common.augment import LineAugmenter
    zero = dict(max_slope=0, max_slant=0, scale_range=0, max_translate=0, warp_amplitude_y=0, warp_amplitude_x=0, brightness=0,
                contrast=0, gamma=0, channel_gain=0, noise_sigma=0)
    want = A.neutral(16, 512, 3, 5)
    for aug in (LineAugmenter(seed=1, p=1.0, **zero), LineAugmenter(seed=1, p=0.0)):
        got = _draw(aug)
        for g, w in zip(got, want):
            assert np.array_equal(g.numpy(), w)
    # a neutral line differs from an augmented one in the seed columns too: all of `params` is neutral, not only what the kernel reads
    assert int(want[0][:, A.SEED_LO:].max()) == 0


def test_p_selects_its_share_of_the_lines():
    from pero_pretraining_amd.common.augment import LineAugmenter
    n = 4096
    for p in (0.25, 0.8):
        params, knots, lut = _draw(LineAugmenter(seed=4, p=p), B=n, Wt=64, C=1)
        neutral_params = (params.numpy() == A.neutral(1, 64, 1, 5)[0]).all(axis=1)
        neutral_knots = (knots.numpy() == 0).all(axis=(1, 2))
        assert np.array_equal(neutral_params, neutral_knots)
        share = 1 - neutral_params.mean()
        assert abs(share - p) < 4 * np.sqrt(p * (1 - p) / n)          # four standard deviations of the binomial share
