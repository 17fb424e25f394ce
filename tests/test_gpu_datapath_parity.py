"""Kernel-level parity of the data path around the GEMMs: the front end (csrc/misc.hip), the collator (csrc/collate.hip), the quantizer
(csrc/vq.hip), the evaluation rank kernel (csrc/eval.hip) and the wide-row LayerNorm instantiations (csrc/rowops.hip).  Every entry
point is called directly at the smallest shapes that reach each of its shape-, pitch- or alignment-gated branches (the branch a case is
there for is asserted on the CPU, tests/test_datapath_ref_cpu.py) and held to the restatement of tests/datapath_ref.py: integer, byte,
copy and cast results bit for bit, float results through parity_ref.assert_within with a bound derived next to the call (no tolerance
here is a measured number).

Every output is a view inside a larger allocation (`Guarded`): the bytes in front of it and behind it hold 0xA5 and must keep it - a
store one row or one 16-byte piece too far lands there -, and every element the call is documented to write is pre-filled with 0x5C
bytes (2.5e17 as a float: no reference value), so that an element the kernel skipped fails the comparison."""
import json
import math

import numpy as np
import pytest
import torch

import datapath_ref as D
import parity_ref as R
from parity_ref import DIVF, SQRTF, assert_within

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
F32 = torch.float32
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    yield _ops
    print("\nPARITY_RATIOS " + json.dumps({k: round(v, 4) for k, v in sorted(R.RATIOS.items())}))


def call(name, *args):
    from pero_pretraining_amd._lib import call as _call
    return _call(name, *args)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).cuda()


class Guarded:
    """`t`: a tensor of `shape` / `dtype` that starts `guard` bytes (a multiple of 16, at least one row plus 16 bytes wherever it is
    used) into its allocation and ends `guard` bytes before its end.  `init`: values to start from (an accumulated output)."""

    def __init__(self, shape, dtype, guard, init=None):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        assert guard % 16 == 0 and guard >= 16
        self.raw = torch.full((2 * guard + nbytes,), 0xA5, device="cuda", dtype=torch.uint8)
        body = self.raw[guard:guard + nbytes]
        body.fill_(0x5C)
        self.t = body.view(dtype).view(shape)
        self.guard = guard
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(torch.as_tensor(init).to(dtype))

    def check(self):
        g = self.guard
        assert int(self.raw[:g].min()) == 0xA5 and int(self.raw[:g].max()) == 0xA5, "bytes in front of the output were written"
        assert int(self.raw[-g:].min()) == 0xA5 and int(self.raw[-g:].max()) == 0xA5, "bytes behind the output were written"
        return self.t


def row_guard(row_elems, dtype):
    """one row plus one 16-byte piece, rounded up to 16 bytes"""
    return (row_elems * torch.empty((), dtype=dtype).element_size() + 16 + 15) // 16 * 16


def same_bits(got, want, dtype):
    """bit-for-bit equality of a device tensor with a host f32 reference rounded to `dtype`"""
    w = torch.as_tensor(want).to(dtype)
    return torch.equal(got.cpu().view(BITS[dtype]), w.view(BITS[dtype]).reshape(got.shape))


# ------------------------------------------------------------------------------------------------ front end
def _patch_inputs(case):
    H, C, P, W, pitch, shift = D.PATCH_CASES[case]
    rng = np.random.default_rng(case)
    N, S = 2, W // P
    images = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
    flat = images.reshape(-1)
    flat[:min(256, flat.size)] = np.arange(min(256, flat.size))          # every byte value where there is room
    tile = rng.standard_normal((C, H, P)).astype(np.float32)
    ld = C * H * P + (0 if pitch is None else pitch)
    return N, H, C, P, W, S, ld, shift, images, tile, D.patch_mask(N, S)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(D.PATCH_CASES)))
def test_patches_from_u8(ops, case, dtype):
    N, H, C, P, W, S, ld, shift, images, tile, mask = _patch_inputs(case)
    raw = torch.zeros(images.size + 32, device="cuda", dtype=torch.uint8)
    img = raw[16 + shift:16 + shift + images.size].view(N, H, W, C)
    img.copy_(torch.from_numpy(images))
    assert img.data_ptr() % 16 == shift
    tile_d, mask_d = dev(tile), dev(mask)
    for m, t in ((mask, tile), (None, None)):       # with the mask; with `mask` and `tile` null
        out = Guarded((N * S, ld), dtype, row_guard(ld, dtype))
        call("pero_patches_from_u8", ops.ptr(img), None if m is None else ops.ptr(mask_d), None if t is None else ops.ptr(tile_d),
             ops.ptr(out.t), N, H, W, C, P, ld, ops.dt(dtype), ops.stream())
        # exact: one IEEE division per pixel (f32), one rounding to nearest even of that quotient or of the tile value (bf16), zeros behind
        assert same_bits(out.check(), D.patches_u8(images, m, t, P, ld), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(D.PATCH_CASES)))
def test_patches_from_f32_and_apply_mask(ops, case, dtype):
    N, H, C, P, W, S, ld, _, _, tile, mask = _patch_inputs(case)
    x = np.random.default_rng(100 + case).standard_normal((N, C, H, W)).astype(np.float32)
    x_d, tile_d, mask_d = dev(x), dev(tile), dev(mask)
    for m, t in ((mask, tile), (None, None)):
        out = Guarded((N * S, ld), dtype, row_guard(ld, dtype))
        call("pero_patches_from_f32", ops.ptr(x_d), None if m is None else ops.ptr(mask_d), None if t is None else ops.ptr(tile_d),
             ops.ptr(out.t), N, H, W, C, P, ld, ops.dt(dtype), ops.stream())
        assert same_bits(out.check(), D.patches_f32(x, m, t, P, ld), dtype)          # a copy (f32) or one rounding (bf16)
    if dtype == F32:   # the in-place mask is f32 only; every pixel is documented as kept or replaced, so the input is the pre-fill
        img = Guarded((N, C, H, W), F32, row_guard(W, F32), init=torch.from_numpy(x))
        call("pero_apply_mask_f32", ops.ptr(img.t), ops.ptr(mask_d), ops.ptr(tile_d), N, H, W, C, P, ops.stream())
        want = D.apply_mask(x, mask, tile, P)
        assert same_bits(img.check(), want, F32) and not np.array_equal(want, x)


@pytest.mark.parametrize("n", [1, 8, 2051])      # below one 8-element piece; exactly one; pieces and a tail of three
def test_cast_f32_bf16_direct(ops, n):
    src = torch.randn(n, generator=torch.Generator().manual_seed(n))
    src[0] = 1.00390625                          # a tie between two bf16 neighbours: to even
    out = Guarded((n,), torch.bfloat16, 32)
    src_d = src.cuda()
    call("pero_cast_f32_bf16", ops.ptr(src_d), ops.ptr(out.t), n, ops.stream())
    assert same_bits(out.check(), src, torch.bfloat16)


@pytest.mark.parametrize("rows,cols,pitch", [(3, 5, 9), (2, 8, 8), (33, 17, 24)])   # odd pitch; no padding; more than one block
def test_cast_pad_f32_bf16_direct(ops, rows, cols, pitch):
    src = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows * cols))
    out = Guarded((rows, pitch), torch.bfloat16, row_guard(pitch, torch.bfloat16))
    src_d = src.cuda()
    call("pero_cast_pad_f32_bf16", ops.ptr(src_d), ops.ptr(out.t), rows, cols, pitch, ops.stream())
    want = torch.zeros(rows, pitch)
    want[:, :cols] = src
    assert same_bits(out.check(), want, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ collation
def _run_stack_lines(ops, packed, offsets, widths, left, B, H, Wt, C):
    out = Guarded((B, H, Wt, C), torch.uint8, row_guard(Wt * C, torch.uint8))
    packed_d = dev(packed)                       # exactly the lines and the 8 slack bytes (0xFF: a consumed one is a wrong pixel)
    assert packed_d.numel() == int(widths.astype(np.int64).sum()) * H * C + 8
    off_d, w_d, left_d = dev(offsets), dev(widths), dev(left)   # named: a temporary's block would be reused by the next upload before the launch
    call("pero_stack_lines", ops.ptr(packed_d), ops.ptr(off_d), ops.ptr(w_d), ops.ptr(left_d), ops.ptr(out.t), B, H, Wt, C, ops.stream())
    assert np.array_equal(out.check().cpu().numpy(), D.stack_lines(packed, offsets, widths, left, B, H, Wt, C))


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("H", [1, 3])
def test_stack_lines_every_residue(ops, C, H):
    packed, offsets, widths, left = D.stack_lines_case(C, H)
    lo, hi, src = D.stack_lines_residues(offsets, widths, left, H, C)
    full = {0, 1, 2, 3} if C % 4 else {0}        # four bytes per pixel: every span is dword aligned, whatever the lines
    assert lo == full and hi == full and src == full
    _run_stack_lines(ops, packed, offsets, widths, left, len(widths), H, D.STACK_LINES_WT, C)


def test_stack_lines_second_block_along_the_row(ops):
    C, Wt = 4, 1028                              # 257 chunks of 16 bytes per row: block 1 of the x dimension has one live thread
    lines = [(1028, 0), (5, 1023)]
    packed, offsets, widths, left = D.stack_lines_case(C, 1, Wt, lines)
    _run_stack_lines(ops, packed, offsets, widths, left, 2, 1, Wt, C)


@pytest.mark.parametrize("sub", [8, 4])
def test_line_masks_unpaired_and_crop_shifts(ops, sub):
    S = 16
    cs = np.array([-40, -17, -16, -15, -5, -1, 0, 1, 5, 15, 16, 17, 40, 3, -2, 0], dtype=np.int32)
    B = len(cs)
    rng = np.random.default_rng(sub)
    left1 = rng.integers(0, 6, B).astype(np.int32)
    left2 = left1.copy()
    left2[-3:] = left1[-3:] + np.array([2, -left1[-2], 1], dtype=np.int32)        # the last three lines: the paddings differ as well
    widths1 = np.array([rng.integers(1, (S - l) * sub + 1) for l in left1], dtype=np.int32)
    widths2 = np.array([rng.integers(1, (S - l) * sub + 1) for l in left2], dtype=np.int32)
    widths1[0], widths1[1] = 1, (S - left1[1]) * sub                               # one label position; up to the row end
    want = D.line_masks(widths1, left1, S, sub, widths2, left2, cs)
    sh = want[4]
    assert (sh < -S).any() and ((sh > -S) & (sh < 0)).any() and (sh == 0).any() and ((sh > 0) & (sh < S)).any() and (sh > S).any()
    assert (np.abs(sh) == S).any() and {0, 1, 2} == set(np.unique(want[2]).tolist())
    w1, w2, l1, l2, cs_d = dev(widths1), dev(widths2), dev(left1), dev(left2), dev(cs)
    # unpaired: every second-view pointer null, only image_masks1 is written
    im1 = Guarded((B, S), torch.uint8, 32)
    call("pero_line_masks", ops.ptr(w1), None, ops.ptr(l1), None, None, ops.ptr(im1.t), None, None, None, None, B, S, sub, ops.stream())
    assert np.array_equal(im1.check().cpu().numpy(), want[0])
    for crop in (cs, None):
        want = D.line_masks(widths1, left1, S, sub, widths2, left2, crop)
        outs = [Guarded((B, S), torch.uint8, 32) for _ in range(4)] + [Guarded((B,), torch.int32, 32)]
        call("pero_line_masks", ops.ptr(w1), ops.ptr(w2), ops.ptr(l1), ops.ptr(l2), None if crop is None else ops.ptr(cs_d),
             *[ops.ptr(o.t) for o in outs], B, S, sub, ops.stream())
        for o, w in zip(outs, want):
            assert np.array_equal(o.check().cpu().numpy(), w)


# ------------------------------------------------------------------------------------------------ quantizer
def _argmin(ops, x_d, e_d, M, K, Dm):
    idx, best = Guarded((M,), torch.int64, 64), Guarded((M,), F32, 64)
    work = torch.full((M + K,), 7.0, device="cuda")
    call("pero_vq_argmin", ops.ptr(x_d), ops.ptr(e_d), ops.ptr(idx.t), ops.ptr(best.t), ops.ptr(work), M, K, Dm, ops.stream())
    return idx.check().cpu().numpy(), best.check().cpu()


def _shifted4(a):
    """a device copy of the f32 array that starts 4 bytes into its allocation"""
    base = torch.zeros(a.size + 8, device="cuda")
    v = base[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("M,K,Dm", D.VQ_SHAPES)
def test_vq_argmin(ops, M, K, Dm):
    x, e, plants = D.vq_case(M, K, Dm)
    ref = D.vq_distances(x, e, [hi for _, _, hi in plants])
    sure, planted = D.vq_sure_rows(ref, Dm, plants)
    assert int((~sure & ~planted).sum()) <= D.NEAR_TIE_CAP * M              # near ties: at most 2 % of the rows (also on the CPU)
    # one f32 distance is within vq_rounding_bound = (2 D + 4) 2^-24 (|x|^2 + |e|^2) of the exact one (derived there: D squares for each
    # norm, their sum, a D-term dot doubled, the last subtraction); `mag` takes the largest |e_k|^2 of the codebook
    tol = D.vq_rounding_bound(ref["mag"], Dm)
    fast = M % 64 == 0 and K % 128 == 0 and Dm % 32 == 0
    runs = [(dev(x), "")] + ([(_shifted4(x), " (x 4 bytes into its allocation)")] if fast else [])
    first, e_d = None, dev(e)
    for x_d, tag in runs:
        idx, best = _argmin(ops, x_d, e_d, M, K, Dm)
        assert idx.min() >= 0 and idx.max() < K
        # where the f64 margin exceeds the bounds of both distances the f64 argmin must come back ...
        assert np.array_equal(idx[sure], ref["index"][sure]), tag
        # ... and everywhere the code that came back is within those two bounds of the best
        assert np.all(ref["dist"][np.arange(M), idx] - ref["best"] <= 2.0 * tol), tag
        # a min over values that are each within the bound of theirs: within the bound of the min (n_terms 2 D, see above)
        assert_within(best, ref["best"], ref["mag"], 2 * Dm, F32, what="pero_vq_argmin best_dist")
        # duplicates compute bit-identical distances: the lower index wins, in the planted rows and wherever a copied code is nearest
        for row, lo, hi in plants:
            assert idx[row] == lo, (tag, row, lo, hi, int(idx[row]))
        assert not np.isin(idx[sure], [hi for _, _, hi in plants]).any(), tag
        if first is None:
            first = idx
        assert np.array_equal(idx, first), tag                                # the generic kernel on the fast kernel's shape: same indices


@pytest.mark.parametrize("M,Dm", [(5, 1), (5, 65)])       # one column; a second trip of the 64-lane column loop
def test_vq_gather(ops, M, Dm):
    rng = np.random.default_rng(M * Dm)
    K = 7
    x, e = rng.standard_normal((M, Dm)).astype(np.float32), rng.standard_normal((K, Dm)).astype(np.float32)
    idx = np.array([6, 0, 3, 3, 5], dtype=np.int64)        # within [0, K): the call does not clamp
    q = Guarded((M, Dm), F32, row_guard(Dm, F32))
    x_d, e_d, idx_d = dev(x), dev(e), dev(idx)
    call("pero_vq_gather", ops.ptr(x_d), ops.ptr(e_d), ops.ptr(idx_d), ops.ptr(q.t), M, Dm, ops.stream())
    assert same_bits(q.check(), D.vq_gather(x, e, idx), F32)               # x + (e - x): two f32 roundings, exact


def _ema_indices(M, K, rng):
    if K == 3:
        return np.array([2, 0, 2, 2, 0, 2, 2], dtype=np.int64)             # code 1 has no rows
    if K == 8:
        return np.full(M, 5, dtype=np.int64)                               # every row on one code: 512 additions into each entry
    used = np.concatenate([[0, 1023, 1024, 1029], rng.choice(np.arange(1, 1023), 36, replace=False)])   # 40 of 1030 codes have rows
    idx = rng.choice(used, M)
    idx[:4] = [0, 1023, 1024, 1029]
    return idx.astype(np.int64)


@pytest.mark.parametrize("M,K,Dm", [(7, 3, 1), (301, 1030, 70), (512, 8, 70)])
def test_vq_ema_update(ops, M, K, Dm):
    """(301, 1030, 70): the stride loop of the one-workgroup cluster kernel (K > 1024), a second trip of the scatter's column loop
    (D > 64), a last scatter block of one row, most codes without rows.  (512, 8, 70): every row on one code."""
    rng = np.random.default_rng(M + K + Dm)
    decay, epsilon = 0.99, 1e-5
    x = rng.standard_normal((M, Dm)).astype(np.float32)
    idx = _ema_indices(M, K, rng)
    assert idx.min() >= 0 and idx.max() < K                                # the call does not clamp
    cluster0 = (rng.random(K) * 2.5 + 0.5).astype(np.float32)
    ema_w0 = rng.standard_normal((K, Dm)).astype(np.float32)
    cluster = Guarded((K,), F32, 64, init=torch.from_numpy(cluster0))
    ema_w = Guarded((K, Dm), F32, row_guard(Dm, F32), init=torch.from_numpy(ema_w0))
    codebook = Guarded((K, Dm), F32, row_guard(Dm, F32))                   # overwritten: starts from the pre-fill pattern
    work = Guarded((K + K * Dm,), F32, row_guard(Dm, F32))                 # "zeroed by the call": starts from the pre-fill pattern too
    x_d, idx_d = dev(x), dev(idx)
    call("pero_vq_ema_update", ops.ptr(x_d), ops.ptr(idx_d), ops.ptr(cluster.t), ops.ptr(ema_w.t), ops.ptr(codebook.t), ops.ptr(work.t),
         M, K, Dm, decay, epsilon, ops.stream())
    res, mag = D.vq_ema_update(x, idx, cluster0, ema_w0, decay, epsilon)
    n = torch.from_numpy(res["counts"])[:, None]                           # rows on each code
    # the workspace holds the counts and the per-code sums (csrc/vq.hip: counts = work, dw = work + K)
    w = work.check().cpu()
    assert torch.equal(w[:K].double(), n[:, 0])                            # integers below 2^24: exact in f32
    # a sum of n f32 values by atomics, in any order: within n 2^-24 sum|x| (n_terms n - 4: bound() adds 4 for roundings of the terms,
    # and these terms are the inputs themselves); an entry without rows stays an exact zero
    assert_within(w[K:].view(K, Dm), res["dw"], mag["dw"], n - 4, F32, what="pero_vq_ema_update dw")
    assert float(w[K:].view(K, Dm)[n[:, 0] == 0].abs().max() if bool((n == 0).any()) else 0.0) == 0.0
    # ema_w = ema_w0 decay + (1 - decay) dw: the sum's n units, two products and one addition (in the 4)
    assert_within(ema_w.check(), res["ema_w"], mag["ema_w"], n, F32, what="pero_vq_ema_update ema_w")
    # cluster = (pre + eps) / (total + K eps) total, pre = cluster0 decay + (1 - decay) counts (3 units), + eps (1), total = a K-term sum of
    # the pre (K + 2), twice; + K eps, the division, the product (3): 2 K + 11 units of a value whose terms are all positive
    assert_within(cluster.check(), res["cluster"], mag["cluster"], 2 * K, F32, extra_ulps=10, what="pero_vq_ema_update cluster")
    # codebook = ema_w / cluster: ema_w's n + 4 units of its magnitude, cluster's 2 K + 14 and the division's one of the quotient
    assert_within(codebook.check(), res["codebook"], mag["codebook"], n + 2 * K, F32, extra_ulps=15, what="pero_vq_ema_update codebook")


# ------------------------------------------------------------------------------------------------ evaluation
def _rank_inputs(V, dtype):
    rng = np.random.default_rng(V)
    rows = 12
    lg = (np.round(rng.standard_normal((rows, V)) * 8) / 4).astype(np.float32)     # multiples of 0.25 below 16: exact in bf16, many ties
    lg[3] = 1.5                                                                     # a row of all-equal values
    lg[4, ::3] = -np.inf
    lg[5, 1::2] = -np.inf                                                           # the label itself sits on a -inf
    labels = np.array([0, V - 1, 5, 7, 3, 1, -1, V, 2, 9, 256, V - 2], dtype=np.int64)
    mask = np.array([1, 1, 1, 1, 1, 1, 1, 1, 2, 0, 1, 1], dtype=np.int64)
    wide = torch.full((rows, V + 9), math.inf, dtype=dtype)                         # the columns behind V hold +inf: not to be counted
    wide[:, :V] = torch.from_numpy(lg).to(dtype)
    assert torch.equal(wide[:, :V].float(), torch.from_numpy(lg))
    return lg, labels, mask, wide


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [257, 1000])       # one column in the second trip of the 256-thread loop; a partly filled fourth trip
def test_label_rank(ops, V, dtype):
    lg, labels, mask, wide = _rank_inputs(V, dtype)
    rows, ld = wide.shape
    logits = wide.cuda()[:, :V]
    assert logits.stride(0) == ld > V
    lab_d, mask_d = dev(labels), dev(mask)
    want = D.label_ranks(lg, labels, mask)
    assert want[6].tolist() == [V, 0, 0] and want[7].tolist() == [V, 0, 0] and want[8].tolist() == [-1, -1, -1] and want[3].tolist() == [0, 7, V - 8]
    ks = np.array([1, 2, 3, 5, 10, 100, V, V + 1], dtype=np.int32)                  # nk = 8 = PERO_MAX_TOPK
    start = np.arange(100, 100 + 1 + len(ks), dtype=np.int64)                       # counters are accumulated into
    cnt_want = D.rank_counters(want, ks)
    out_of_row = (cnt_want[1:-1] >= 2).all()                                         # labels -1 and V: an error for every k <= V
    assert out_of_row and cnt_want[0] == 10

    def run(r0, r1, ks_d, nk, counters, ranks):
        call("pero_label_rank", ops.ptr(logits[r0:r1]), ld, ops.ptr(lab_d[r0:r1]), ops.ptr(mask_d[r0:r1]), r1 - r0, V,
             None if ks_d is None else ops.ptr(ks_d), nk, None if counters is None else ops.ptr(counters.t),
             None if ranks is None else ops.ptr(ranks.t), ops.dt(dtype), ops.stream())

    # ranks and eight counters
    ranks, counters = Guarded((rows, 3), torch.int32, 32), Guarded((1 + len(ks),), torch.int64, 32, init=torch.from_numpy(start))
    run(0, rows, dev(ks), len(ks), counters, ranks)
    assert np.array_equal(ranks.check().cpu().numpy(), want)
    assert np.array_equal(counters.check().cpu().numpy(), start + cnt_want)
    # counters null, ranks wanted, nk == 0
    ranks = Guarded((rows, 3), torch.int32, 32)
    run(0, rows, None, 0, None, ranks)
    assert np.array_equal(ranks.check().cpu().numpy(), want)
    # nk == 0 with counters: the length alone; no ranks
    counters = Guarded((1,), torch.int64, 32, init=torch.from_numpy(start[:1]))
    run(0, rows, None, 0, counters, None)
    assert counters.check().cpu().tolist() == [100 + 10]
    # one row, and a second call into the same counters
    ranks, counters = Guarded((1, 3), torch.int32, 32), Guarded((3,), torch.int64, 32, init=torch.from_numpy(start[:3]))
    for _ in range(2):
        run(2, 3, dev(ks[:2]), 2, counters, ranks)
    assert np.array_equal(ranks.check().cpu().numpy(), want[2:3])
    assert np.array_equal(counters.check().cpu().numpy(), start[:3] + 2 * D.rank_counters(want[2:3], ks[:2]))


# ------------------------------------------------------------------------------------------------ LayerNorm, wide rows
LN_ROWS, LN_EPS = 5, float(np.float32(1e-5))
# rstd = 1 / sqrt(var + eps) beyond the d-term sum of the squares: each square comes from a rounded difference (3 units), the division
# by d, + eps, the square root and the reciprocal (parity_ref's BatchNorm chain)
LN_RSTD_ULPS = 3 + DIVF + 1 + SQRTF + DIVF


def _ln_inputs(d, dtype, rows=LN_ROWS):
    g = torch.Generator().manual_seed(d + (dtype == F32))
    x = (torch.randn(rows, d, generator=g) * 2 + 0.3).to(dtype)
    dy = torch.randn(rows, d, generator=g).to(dtype)
    gamma = (torch.rand(d, generator=g) + 0.5) * torch.where(torch.arange(d) % 7 == 1, -1.0, 1.0)   # away from zero, both signs
    beta = torch.randn(d, generator=g) * 0.3
    return x, dy, gamma, beta


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1032, 2048, 2056, 4096])   # NCH = 4 with two idle chunks; NCH = 4 full; NCH = 8 with a partly filled fifth chunk; NCH = 8 full
def test_layernorm_fwd_wide_rows(ops, d, dtype):
    x, _, gamma, beta = _ln_inputs(d, dtype)
    y = Guarded((LN_ROWS, d), dtype, row_guard(d, dtype))
    mean, rstd = Guarded((LN_ROWS,), F32, 32), Guarded((LN_ROWS,), F32, 32)
    x_d, gamma_d, beta_d = x.cuda(), gamma.cuda(), beta.cuda()
    call("pero_layernorm_fwd", ops.ptr(x_d), ops.ptr(gamma_d), ops.ptr(beta_d), None, None, ops.ptr(y.t), ops.ptr(mean.t),
         ops.ptr(rstd.t), LN_ROWS, d, 1, LN_EPS, ops.dt(dtype), ops.stream())
    res, mag = D.layernorm_fwd(x, gamma, beta, LN_EPS)
    # n_terms = d throughout: the mean is a d-term sum; rstd a d-term sum of squares and LN_RSTD_ULPS; y carries both sums (its
    # magnitude adds the mean's share and the variance's, datapath_ref.layernorm_fwd), rstd's extras, two products and the bias
    assert_within(mean.check(), res["mean"], mag["mean"], d, F32, what="pero_layernorm_fwd mean")
    assert_within(rstd.check(), res["rstd"], mag["rstd"], d, F32, extra_ulps=LN_RSTD_ULPS, what="pero_layernorm_fwd rstd")
    assert_within(y.check(), res["y"], mag["y"], d, dtype, extra_ulps=LN_RSTD_ULPS + 3, what="pero_layernorm_fwd y")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("from_out", [False, True])
@pytest.mark.parametrize("d", [1032, 2048])               # NCH = 4 with an idle last chunk and a partly filled third; NCH = 4 full
def test_layernorm_bwd_wide_rows(ops, d, from_out, dtype):
    x, dy, gamma, beta = _ln_inputs(d, dtype)
    fwd, _ = D.layernorm_fwd(x, gamma, beta, LN_EPS)
    mean, rstd = fwd["mean"].float(), fwd["rstd"].float()                  # the saved statistics are inputs: rounded once, seen by both sides
    t = fwd["y"].to(dtype)                                                  # the layer's output as the forward pass stores it
    g = torch.Generator().manual_seed(d)
    dg0, db0, dxs0 = (torch.randn(d, generator=g) for _ in range(3))
    work = torch.empty(3 * 512 * d, device="cuda")
    dy_d, x_d, t_d, mean_d, rstd_d, gamma_d, beta_d = (v.cuda() for v in (dy, x, t, mean, rstd, gamma, beta))
    for with_dxsum in (True, False):
        dx = Guarded((LN_ROWS, d), dtype, row_guard(d, dtype))
        dgamma, dbeta, dxsum = (Guarded((d,), F32, 64, init=v) for v in (dg0, db0, dxs0))
        if from_out:
            call("pero_layernorm_bwd_out", ops.ptr(dy_d), ops.ptr(t_d), ops.ptr(rstd_d), ops.ptr(gamma_d), ops.ptr(beta_d),
                 ops.ptr(dx.t), ops.ptr(dgamma.t), ops.ptr(dbeta.t), ops.ptr(dxsum.t) if with_dxsum else None, ops.ptr(work), LN_ROWS, d,
                 ops.dt(dtype), ops.stream())
            res, mag = D.layernorm_bwd_out(dy, t, rstd, gamma, beta, dg0, db0, dxs0 if with_dxsum else None)
        else:
            call("pero_layernorm_bwd", ops.ptr(dy_d), ops.ptr(x_d), ops.ptr(mean_d), ops.ptr(rstd_d), ops.ptr(gamma_d),
                 ops.ptr(dx.t), ops.ptr(dgamma.t), ops.ptr(dbeta.t), ops.ptr(dxsum.t) if with_dxsum else None, ops.ptr(work), LN_ROWS, d,
                 ops.dt(dtype), ops.stream())
            res, mag = D.layernorm_bwd(dy, x, mean, rstd, gamma, dg0, db0, dxs0 if with_dxsum else None)
        name = "pero_layernorm_bwd_out" if from_out else "pero_layernorm_bwd"
        # xhat: a difference and a product (2 units of its magnitude, which datapath_ref takes from the operands), from the output a
        # reciprocal more; it enters each of dx's three terms once more than the 4 covers
        xu = 4 if from_out else 3
        # dx = rstd (g - mean g - xhat mean (g xhat)): two d-term sums
        assert_within(dx.check(), res["dx"], mag["dx"], d, dtype, extra_ulps=xu, what=name + " dx")
        # dgamma / dbeta: the old value and LN_ROWS terms - d is far above that count; xhat's units on top
        assert_within(dgamma.check(), res["dgamma"], mag["dgamma"], d, F32, extra_ulps=xu, what=name + " dgamma")
        assert_within(dbeta.check(), res["dbeta"], mag["dbeta"], d, F32, what=name + " dbeta")
        if with_dxsum:   # column sums of the f32 dx before it is stored: dx's own d + 4 + xu units, the old value and LN_ROWS additions
            assert_within(dxsum.check(), res["dxsum"], mag["dxsum"], d, F32, extra_ulps=xu + LN_ROWS + 1, what=name + " dxsum")
        else:
            assert torch.equal(dxsum.check().cpu(), dxs0)                    # a null dxsum: nothing else takes the column sums


def test_layernorm_fwd_bf16_positional_table_stays_off_the_four_row_kernel(ops):
    """bf16, d <= 512, 4097 rows WITH a positional table and offsets: the four-rows-per-wave kernel takes no table, so the call must
    stay on the one-row-per-wave kernel - the rows, means and rstds are those of the same rows in chunks below 4096, bit for bit (the
    form of test_layernorm_fwd_four_rows_per_wave_equals_one_row_per_wave), and the table is in the result."""
    rows, d, S, max_len = 4097, 64, 1, 50
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, d, generator=g) * 2 + 0.3).bfloat16().cuda()
    gamma, beta = torch.randn(d, generator=g).cuda(), torch.randn(d, generator=g).cuda()
    pe = torch.randn(max_len, d, generator=g).cuda()
    offsets = torch.randint(0, max_len, (rows,), generator=g).cuda()
    y = Guarded((rows, d), torch.bfloat16, row_guard(d, torch.bfloat16))
    mean, rstd = Guarded((rows,), F32, 32), Guarded((rows,), F32, 32)
    call("pero_layernorm_fwd", ops.ptr(x), ops.ptr(gamma), ops.ptr(beta), ops.ptr(pe), ops.ptr(offsets), ops.ptr(y.t), ops.ptr(mean.t),
         ops.ptr(rstd.t), rows, d, S, LN_EPS, ops.dt(torch.bfloat16), ops.stream())
    for lo in range(0, rows, 2049):
        y1, m1, r1 = ops.layernorm_fwd(x[lo:lo + 2049].contiguous(), gamma, beta, LN_EPS, pe=pe, offsets=offsets[lo:lo + 2049].contiguous(), S=S)
        assert torch.equal(y.t[lo:lo + 2049], y1) and torch.equal(mean.t[lo:lo + 2049], m1) and torch.equal(rstd.t[lo:lo + 2049], r1)
    y.check(), mean.check(), rstd.check()
    res, mag = D.layernorm_fwd(x[:64].cpu(), gamma.cpu(), beta.cpu(), LN_EPS, pe.cpu(), offsets[:64].cpu(), S)
    assert_within(y.t[:64], res["y"], mag["y"], d, torch.bfloat16, extra_ulps=LN_RSTD_ULPS + 4, what="pero_layernorm_fwd y")   # + the table's addition
    plain, _, _ = ops.layernorm_fwd(x[:64].contiguous(), gamma, beta, LN_EPS)
    assert not torch.equal(plain, y.t[:64])
