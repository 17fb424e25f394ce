"""tests/datapath_ref.py against what the project already trusts (the oracle and the reference's golden files), and the conditions on the
INPUTS of tests/test_gpu_datapath_parity.py that can be checked without a GPU: every code path a case is there for is the one its sizes
select, the collation lines cover every address residue, and the quantizer cases stay inside the near-tie cap."""
import numpy as np
import pytest
import torch

import datapath_ref as D
from oracle import pero_oracle as O
from parity_ref import assert_within

F32 = torch.float32


# ------------------------------------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize("W", [8, 128, 200])
def test_patch_reference_is_the_oracle_front_end(W):
    rng = np.random.default_rng(W)
    N, H, C, P = 2, 40, 3, 8
    images = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
    images[0, 0, :min(W, 256), 0] = np.arange(min(W, 256))            # every byte value once where the width allows
    tile = rng.standard_normal((C, H, P)).astype(np.float32)
    mask = D.patch_mask(N, W // P)
    x = O.prepare_images(torch.from_numpy(images))
    want = O.patches(O.apply_mask(x, torch.from_numpy(mask), torch.from_numpy(tile), P), P).numpy()
    got = D.patches_u8(images, mask, tile, P, C * H * P + 8)
    assert np.array_equal(got[:, :C * H * P], want) and not got[:, C * H * P:].any()
    assert np.array_equal(D.patches_u8(images, None, None, P, C * H * P), O.patches(x, P).numpy())
    xn = x.contiguous().numpy()
    assert np.array_equal(D.patches_f32(xn, mask, tile, P, C * H * P), want)
    assert np.array_equal(D.apply_mask(xn, mask, tile, P), O.apply_mask(x, torch.from_numpy(mask), torch.from_numpy(tile), P).numpy())
    assert (mask == 1).any() and (mask == 0).any() and ((mask == 2).any() or W == 8)


def test_collation_reference_is_the_oracle_collator():
    rng = np.random.default_rng(3)
    H, C, sub, Wt = 3, 3, 8, 64
    widths, lp = [5, 17, 64, 1, 30], [2, 0, 0, 7, 4]
    lines = [rng.integers(1, 255, (H, w, C), dtype=np.uint8) for w in widths]
    packed = np.concatenate([l.reshape(-1) for l in lines] + [np.full(8, 0xFF, dtype=np.uint8)])
    offsets = np.concatenate([[0], np.cumsum([l.size for l in lines])[:-1]])
    images, masks = O.collate_view(lines, lp, Wt, sub)
    assert np.array_equal(D.stack_lines(packed, offsets, widths, [sub * v for v in lp], len(lines), H, Wt, C), images)
    lp2 = [0, 3, 0, 1, 4]
    _, masks2 = O.collate_view(lines, lp2, Wt, sub)
    im1, im2, sm1, sm2, shifts = D.line_masks(widths, lp, Wt // sub, sub, widths, lp2)
    assert np.array_equal(im1, masks) and np.array_equal(im2, masks2)
    s1, s2 = O.shift_masks([a - b for a, b in zip(lp, lp2)], masks, masks2)
    assert np.array_equal(sm1, s1) and np.array_equal(sm2, s2) and shifts.tolist() == [a - b for a, b in zip(lp, lp2)]
    only = D.line_masks(widths, lp, Wt // sub, sub)
    assert np.array_equal(only[0], masks) and only[1:] == (None, None, None, None)
    # crop shifts beyond the row on both sides: the slices clamp
    cs = [-20, 20, -8, 8, 0]
    _, _, sm1, sm2, shifts = D.line_masks(widths, lp, Wt // sub, sub, widths, lp2, cs)
    s1, s2 = O.shift_masks(shifts.tolist(), masks, masks2)
    assert np.array_equal(sm1, s1) and np.array_equal(sm2, s2)


def _rank_rows(V, seed):
    rng = np.random.default_rng(seed)
    lg = (np.round(rng.standard_normal((9, V)) * 8) / 4).astype(np.float32)     # multiples of 0.25: many exact ties, exact in bf16
    lg[3] = 1.5
    lg[4, ::3] = -np.inf
    labels = np.array([0, V - 1, 5, 7, 3, -1, V, 2, 9])
    mask = np.array([1, 1, 1, 1, 1, 1, 1, 2, 0])
    return lg, labels, mask


@pytest.mark.parametrize("V", [12, 257])
def test_rank_reference_is_the_oracle_rank(V):
    lg, labels, mask = _rank_rows(V, V)
    ranks = D.label_ranks(lg, labels, mask)
    assert np.array_equal(ranks, O.label_ranks(lg, labels, mask))
    assert ranks[5].tolist() == [V, 0, 0] and ranks[6].tolist() == [V, 0, 0] and ranks[7].tolist() == [-1, -1, -1]
    ks = (1, 2, 3, V)
    errs, n = O.errors_from_ranks(ranks, ks)
    assert D.rank_counters(ranks, ks).tolist() == [n] + [errs[f"errors_{k}"] for k in ks]


@pytest.mark.parametrize("M,K,Dm", D.VQ_SHAPES)
def test_vq_reference_agrees_with_the_oracle_outside_near_ties_and_stays_inside_the_cap(M, K, Dm):
    x, e, plants = D.vq_case(M, K, Dm)
    ref = D.vq_distances(x, e, [hi for _, _, hi in plants])
    sure, planted = D.vq_sure_rows(ref, Dm, plants)
    idx, dist = O.vq_nearest(x, e)
    assert np.array_equal(idx[sure], ref["index"][sure])
    assert np.all(np.abs(dist.min(1) - ref["best"]) <= D.vq_rounding_bound(ref["mag"], Dm))
    # the cap on exempted rows, from the f64 reference alone
    assert int((~sure & ~planted).sum()) <= D.NEAR_TIE_CAP * M, (M, K, Dm, int((~sure & ~planted).sum()))
    # the planted rows: two bit-identical codes, the row equal to both, every other code clearly farther
    for row, lo, hi in plants:
        assert np.array_equal(e[lo], e[hi]) and np.array_equal(x[row], e[lo]) and ref["index"][row] == lo and ref["dist"][row, lo] == ref["dist"][row, hi]
        others = np.delete(ref["dist"][row], [lo, hi])
        assert others.size == 0 or others.min() > 4 * D.vq_rounding_bound(ref["mag"][row], Dm)
    want = [d for c, d in D.VQ_PLANTS if c + d < K][:M]
    assert [hi - lo for _, lo, hi in plants] == want
    if (M, K, Dm) == (128, 256, 64):
        assert sorted(set(want)) == [4, 32, 64, 128]


def test_vq_gather_reference_rounds_twice():
    x, e = np.float32([[1.0, 3e-8]]), np.float32([[1e-8, 1.0]])
    q = D.vq_gather(x, e, [0])
    assert q.dtype == np.float32 and np.array_equal(q, x + (e - x)) and float(q[0, 0]) == 0.0


def test_ema_reference_agrees_with_the_oracle_and_the_golden_file(golden):
    g = golden("g16_vq_ema.npz")
    decay = float(g["decay"])
    cb, ew, cs = g["codebook0"], g["ema_w0"], g["ema_cluster_size0"]
    for step in range(2):
        flat = np.ascontiguousarray(g[f"s{step}.features"].transpose(0, 2, 3, 1)).reshape(-1, 32)
        idx = g[f"s{step}.indices"]
        res, mag = D.vq_ema_update(flat, idx, cs, ew, decay, 1e-5)
        K = cs.shape[0]
        n = torch.from_numpy(res["counts"])[:, None]
        for other in (O.vq_ema_update(flat, idx, cs, ew, decay, 1e-5), (g[f"s{step}.ema_cluster_size"], g[f"s{step}.ema_w"], g[f"s{step}.codebook"])):
            # f32 evaluations of the same formula: the bounds test_gpu_datapath_parity.py derives for the kernel
            assert_within(other[0], res["cluster"], mag["cluster"], 2 * K, F32, extra_ulps=10)
            assert_within(other[1], res["ema_w"], mag["ema_w"], n + 2, F32)
            assert_within(other[2], res["codebook"], mag["codebook"], n + 2 * K, F32, extra_ulps=15)
        assert res["counts"].sum() == flat.shape[0] and np.array_equal(res["counts"], np.bincount(idx, minlength=K))
        cb, ew, cs = g[f"s{step}.codebook"], g[f"s{step}.ema_w"], g[f"s{step}.ema_cluster_size"]
    # the scalar rules: (float)(1 - decay) is not 1 - (float)decay
    res, _ = D.vq_ema_update(np.ones((1, 1)), [0], [0.0], [[0.0]], 0.99, 0.0)
    assert res["ema_w"][0, 0] == float(np.float32(1 - 0.99)) != 1.0 - float(np.float32(0.99))


@pytest.mark.parametrize("d", [64, 1032])
def test_layernorm_reference_agrees_with_the_oracle(d):
    g = torch.Generator().manual_seed(d)
    rows, eps = 5, 1e-5
    x = torch.randn(rows, d, generator=g, dtype=torch.float64) * 2 + 0.3
    dy = torch.randn(rows, d, generator=g, dtype=torch.float64)
    gamma = (torch.rand(d, generator=g, dtype=torch.float64) + 0.5) * torch.where(torch.arange(d) % 7 == 1, -1.0, 1.0)
    beta = torch.randn(d, generator=g, dtype=torch.float64) * 0.3
    res, mag = D.layernorm_fwd(x, gamma, beta, eps)
    assert float((res["y"] - O.layer_norm(x, gamma, beta, eps)).abs().max()) < 1e-12
    assert bool((mag["y"] >= res["y"].abs() - 1e-12).all()) and bool((mag["rstd"] >= res["rstd"]).all())
    rdx, rdg, rdb, rdxs, _, _ = O.layer_norm_bwd_f64(x, dy, gamma, eps)
    zero = torch.zeros(d, dtype=torch.float64)
    for b, bm in (D.layernorm_bwd(dy, x, res["mean"], res["rstd"], gamma, zero, zero, zero),
                  D.layernorm_bwd_out(dy, res["y"], res["rstd"], gamma, beta, zero, zero, zero)):
        for key, want in (("dx", rdx), ("dgamma", rdg), ("dbeta", rdb), ("dxsum", rdxs)):
            assert float((b[key] - want).abs().max()) < 1e-10, key
            assert bool((bm[key] >= b[key].abs() - 1e-12).all()), key
    # accumulation and the optional column sums
    one = torch.ones(d, dtype=torch.float64)
    b, _ = D.layernorm_bwd(dy, x, res["mean"], res["rstd"], gamma, one, 2 * one)
    assert "dxsum" not in b and float((b["dgamma"] - rdg - 1).abs().max()) < 1e-10 and float((b["dbeta"] - rdb - 2).abs().max()) < 1e-10
    # the positional rows: pe[offsets[row / S] + row % S]
    pe = torch.randn(40, d, generator=g, dtype=torch.float64)
    res2, _ = D.layernorm_fwd(x[:4], gamma, beta, eps, pe, torch.tensor([7, 30]), 2)
    assert float((res2["y"] - res["y"][:4] - pe[[7, 8, 30, 31]]).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ conditions on the GPU cases
def test_patch_cases_select_the_branches_they_are_there_for():
    f32, bf16 = 4, 2
    want = [({"stage16", "block>0:stage16", "pow2", "store16", "nopad"}, bf16),
            ({"stage4", "block>0:stage4", "pow2", "store16", "nopad"}, bf16),
            ({"stage1", "block>0:stage1", "pow2", "store1", "nopad"}, bf16),
            ({"stage1", "pow2", "store16", "nopad"}, bf16),
            ({"stage4", "block>0:stage4", "tall", "store1", "nopad"}, bf16),
            ({"stage16", "pow2", "store16", "nopad"}, bf16),
            ({"stage16", "pow2", "store16", "nopad"}, bf16),
            ({"stage16", "pow2", "store1", "pad1"}, bf16),
            ({"stage16", "pow2", "store1", "pad1"}, bf16),
            ({"stage16", "pow2", "store1", "pad16"}, bf16),
            ({"stage16", "pow2", "store16", "nopad"}, bf16)]
    assert len(want) == len(D.PATCH_CASES)
    for (H, C, P, W, pitch, shift), (branches, item) in zip(D.PATCH_CASES, want):
        assert D.patch_branches(H, C, P, W, pitch, shift, item) == branches, (H, C, P, W, pitch, shift)
        assert "store16" not in D.patch_branches(H, C, P, W, pitch, shift, f32)
        S = W // P
        m = D.patch_mask(2, S)
        for s0 in range(0, S, D.PT_TOK):        # both mask values in every block; a one-token block differs between the lines
            blk = m[:, s0:s0 + D.PT_TOK] == 1
            assert (blk.any(1).all() and (~blk).any(1).all()) if blk.shape[1] > 1 else (blk[0, 0] != blk[1, 0])
    H, C, P, W = D.PATCH_CASES[2][:4]
    assert W * C == 51 and W // P == 17
    # a wider default pitch (the module's GEMM-friendly 1024): the 16-byte padding with the 16-byte store
    assert {"store16", "pad16"} <= D.patch_branches(40, 3, 8, 128, 64, 0, bf16)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("H", [1, 3])
def test_collation_lines_cover_every_address_residue(C, H):
    packed, offsets, widths, left = D.stack_lines_case(C, H)
    lo, hi, src = D.stack_lines_residues(offsets, widths, left, H, C)
    if C % 4:
        assert lo == {0, 1, 2, 3} and hi == {0, 1, 2, 3} and src == {0, 1, 2, 3}
    else:   # four bytes per pixel: every span and every back-to-back offset is a multiple of 4, only the aligned path can run
        assert lo == {0} and hi == {0} and src == {0}
    assert len(widths) >= 6 and {1, 2, 5} <= set(widths.tolist()) and D.STACK_LINES_WT in (widths + left).tolist()
    assert int(widths.min()) * C < 4 or C == 4                      # a line narrower than one dword
    assert packed.size == int(widths.astype(np.int64).sum()) * H * C + 8 and packed[-8:].tolist() == [0xFF] * 8
    assert 0 < int(packed[:-8].min()) and int(packed[:-8].max()) < 0xFF
    ref = D.stack_lines(packed, offsets, widths, left, len(widths), H, D.STACK_LINES_WT, C)
    assert int((ref != 0).sum()) == packed.size - 8                 # every pixel placed once, zero elsewhere


def test_wide_collation_case_needs_a_second_block():
    C, Wt = 4, 1028
    assert Wt * C % 16 == 0 and Wt * C // 16 == 257                  # 256 chunks per block: block 1 has one live thread
    lines = [(1028, 0), (5, 1023)]
    packed, offsets, widths, left = D.stack_lines_case(C, 1, Wt, lines)
    assert (widths + left).tolist() == [Wt, Wt]
    ref = D.stack_lines(packed, offsets, widths, left, 2, 1, Wt, C)
    assert ref[0, 0, -4:].all() and ref[1, 0, -5:].all() and not ref[1, 0, :-5].any()
