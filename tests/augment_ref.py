"""A numpy restatement, in int64, of pero_augment_stack_lines as include/pero_hip.h states it ("line augmentation fused into
collation"), and the builders of the cases that test_augment_ref_cpu.py anchors and test_gpu_augment.py runs on the device (not a test
module; it never imports the library).  Every comparison made with it is np.array_equal."""
import numpy as np

import datapath_ref as D

P = 7                                     # PERO_AUGMENT_PARAMS
SY, TY, SLOPE, SLANT, NOISE_AMP, SEED_LO, SEED_HI = range(P)
I64 = np.int64
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
NOISE_UNIT_STD = (4 * (256 ** 2 - 1) / 12) ** 0.5      # 147.8


def num_knots(Wt, knot_shift):
    return (Wt >> knot_shift) + 2


def neutral(B, Wt, C, knot_shift):
    params = np.zeros((B, P), dtype=np.int32)
    params[:, SY] = 256
    return params, np.zeros((B, 2, num_knots(Wt, knot_shift)), dtype=np.int32), np.tile(np.arange(256, dtype=np.uint8), (B, C, 1))


def noise_amp(sigma):
    return int(round(sigma * 65536 / NOISE_UNIT_STD))


def fmix32(h):
    """murmur3's finaliser on u32 values held in uint64 arrays"""
    M = np.uint64(0xFFFFFFFF)
    h = h & M
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M
    h ^= h >> np.uint64(16)
    return h


def taps(w, H, params_b, knots_b, knot_shift):
    """(ys, xs, y0, y1, x0, x1, j) of every output pixel (y, x) of one line, (H, w) int64 arrays (j: (w,)); the integers are exactly
    the header's.  The caller indexes the line with y0, y1, x0, x1 and the knot table with j, j + 1."""
    K, NK = 1 << knot_shift, knots_b.shape[1]
    sy, ty, slope, slant = (I64(int(params_b[i])) for i in (SY, TY, SLOPE, SLANT))
    k = knots_b.astype(I64)
    x = np.arange(w, dtype=I64)
    y = np.arange(H, dtype=I64)[:, None]
    cy, xc = I64((H - 1) * 128), I64(w // 2)
    j = np.clip(x >> knot_shift, 0, NK - 2)
    t = x & (K - 1)
    dy = (k[0][j] * (K - t) + k[0][j + 1] * t) >> knot_shift
    dx = (k[1][j] * (K - t) + k[1][j + 1] * t) >> knot_shift
    yr = (y << 8) - cy
    ys = cy + ((yr * sy) >> 8) + ty + slope * (x - xc) + dy
    xs = (x << 8) + ((yr * slant) >> 8) + dx
    y0, y1 = np.clip(ys >> 8, 0, H - 1), np.clip((ys >> 8) + 1, 0, H - 1)
    x0, x1 = np.clip(xs >> 8, 0, w - 1), np.clip((xs >> 8) + 1, 0, w - 1)
    return ys, xs, y0, y1, x0, x1, j


def noise(v, index, params_b):
    """v: int64 values after the tone curve; index: of the same shape, each value's byte index in the output batch."""
    amp = I64(int(params_b[NOISE_AMP]))
    if amp == 0:
        return v
    i = np.asarray(index).astype(np.uint64)
    M = np.uint64(0xFFFFFFFF)
    lo, hi = np.uint64(int(params_b[SEED_LO]) & 0xFFFFFFFF), np.uint64(int(params_b[SEED_HI]) & 0xFFFFFFFF)
    h = fmix32(fmix32((i & M) ^ lo) ^ (i >> np.uint64(32)) ^ hi)
    s = ((h & np.uint64(255)) + ((h >> np.uint64(8)) & np.uint64(255)) + ((h >> np.uint64(16)) & np.uint64(255))
         + (h >> np.uint64(24))).astype(I64) - 510
    return np.clip(v + ((s * amp + 32768) >> 16), 0, 255)


def augment_stack_lines(packed, offsets, widths, left_px, params, knots, lut, B, H, Wt, C, knot_shift):
    """The (B, H, Wt, C) u8 batch of the header's formulas; lut None = identity."""
    packed = np.asarray(packed, dtype=np.uint8)
    out = np.zeros((B, H, Wt, C), dtype=np.uint8)
    for b in range(B):
        w, lp, o = int(widths[b]), int(left_px[b]), int(offsets[b])
        line = packed[o:o + H * w * C].reshape(H, w, C).astype(I64)
        ys, xs, y0, y1, x0, x1, _ = taps(w, H, params[b], knots[b], knot_shift)
        fx, fy = (xs & 255)[:, :, None], (ys & 255)[:, :, None]
        p00, p01, p10, p11 = line[y0, x0], line[y0, x1], line[y1, x0], line[y1, x1]                 # (H, w, C)
        v = ((p00 * (256 - fx) + p01 * fx) * (256 - fy) + (p10 * (256 - fx) + p11 * fx) * fy + 32768) >> 16
        if lut is not None:
            v = np.stack([np.asarray(lut[b][c]).astype(I64)[v[:, :, c]] for c in range(C)], axis=2)
        yy, xx, cc = np.meshgrid(np.arange(H, dtype=I64), np.arange(w, dtype=I64) + lp, np.arange(C, dtype=I64), indexing="ij")
        v = noise(v, ((b * H + yy) * Wt + xx) * C + cc, params[b])
        out[b, :, lp:lp + w, :] = v.astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ the cases the GPU test runs
WT = 96
# (width, left_px) at Wt = 96: the widths 1, 2, 31, 33 and 70 - one and two pixels (every tap clamps), one short of a knot (K = 32), one
# past it, and more than two knots - with left paddings 0, 1, 2, 3 (every residue of left_px C modulo 4 for C = 1 and C = 3) and a
# line that ends with the row.  The second entry is the index of the line that gets the neutral values.
LINE_SETS = [([(1, 0), (2, 1), (31, 2), (33, 3)], 0),
             ([(70, 5), (1, 80), (2, 94), (31, 7)], 3)]
WIDE_WT, WIDE_C, WIDE_LINES = 1028, 4, [(1028, 0), (5, 1023)]        # datapath_ref's wide case: 257 16-byte chunks per row


def random_params(rng, B, Wt, C, knot_shift):
    """Different values per line, growing with the line's index, large enough that taps leave the line on every side (the clamps work)
    and that the tone curve and the noise saturate some bytes."""
    params, knots, lut = neutral(B, Wt, C, knot_shift)
    for b in range(B):
        m = b + 1
        params[b, SY] = 256 + rng.integers(-40, 41) * m
        params[b, TY] = rng.integers(-300, 301) * m
        params[b, SLOPE] = rng.integers(-30, 31) * m
        params[b, SLANT] = rng.integers(-100, 101) * m
        params[b, NOISE_AMP] = noise_amp(4.0 * m)
        params[b, SEED_LO:] = rng.integers(INT32_MIN, INT32_MAX + 1, 2)
        knots[b] = rng.integers(-400 * m, 400 * m + 1, knots[b].shape)
        lut[b] = rng.integers(0, 256, (C, 256), dtype=np.uint8)
    return params, knots, lut


def case(C, H, Wt=WT, lines=None, neutral_line=None, knot_shift=5, seed=0):
    """packed, offsets, widths, left_px (datapath_ref.stack_lines_case) and params, knots, lut for them."""
    packed, offsets, widths, left = D.stack_lines_case(C, H, Wt, lines, seed)
    B = len(widths)
    rng = np.random.default_rng(7000 + 100 * C + H + seed)
    params, knots, lut = random_params(rng, B, Wt, C, knot_shift)
    if neutral_line is not None:
        n = neutral(1, Wt, C, knot_shift)
        params[neutral_line], knots[neutral_line], lut[neutral_line] = n[0][0], n[1][0], n[2][0]
    return packed, offsets, widths, left, params, knots, lut


def extreme_case(C, H, Wt=WT, lines=None, knot_shift=5, seed=0):
    """Every parameter and every knot is INT32_MIN or INT32_MAX (both occur in every column over the lines)."""
    packed, offsets, widths, left, params, knots, lut = case(C, H, Wt, lines, None, knot_shift, seed)
    rng = np.random.default_rng(9000 + seed)
    ext = np.array([INT32_MIN, INT32_MAX], dtype=np.int64)
    params[:] = ext[rng.integers(0, 2, params.shape)]
    params[0], params[1] = INT32_MIN, INT32_MAX
    knots[:] = ext[rng.integers(0, 2, knots.shape)]
    return packed, offsets, widths, left, params, knots, lut
