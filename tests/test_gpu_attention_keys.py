"""Fused attention with per-line key ranges (pero_attention_fwd_keys / pero_attention_bwd_keys, head_dim 128 and 64) and the row softmax with
ranges (pero_softmax_fwd_keys) against the f64 yardstick of tests/attention_keys_ref.py on the same bf16 inputs.

The allocations are the guarded ones of tests/test_gpu_attention_ragged.py (NaN rows behind the inputs, a bit pattern behind the outputs).  The
inputs follow its recipe - randn * 0.7 with a spiked query row and spiked key rows - and the K and V rows OUTSIDE each line's range are then
multiplied by 2^10: finite, but one leaked key would dominate every sum it enters.  Shapes: the smallest that reach each branch of the tile
walk (a dead second tile, a dead first tile, straddling ranges, a middle tile only, a single key, S % 128 == 0, four tiles).  Tolerances are
those of test_ragged_attention_matches_the_oracle_and_stays_inside_the_line."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_keys_ref as KR  # noqa: E402
from test_gpu_attention_ragged import Guarded, rel_err  # noqa: E402

CASES = [
    (1, 1, 1, ((0, 1),)),
    (2, 4, 4, ((0, 4), (1, 3))),
    (3, 132, 4, ((3, 100), (128, 132), (120, 131))),      # second tile dead; first tile dead; straddling
    (3, 260, 2, ((129, 255), (0, 260), (5, 6))),          # middle tile only; full; a single key
    (2, 256, 4, ((0, 256), (64, 200))),                   # S % 128 == 0
    (1, 388, 1, ((130, 300),)),
]
HDS = [128, 64]
IDS = [f"n{n}-s{s}-h{h}" for n, s, h, _ in CASES]


def ranges_tensor(ranges):
    return torch.tensor(ranges, dtype=torch.int32, device="cuda")


def inputs(n, s, h, hd, ranges):
    d = h * hd
    g = torch.Generator().manual_seed(n * 1000 + s + h + hd)
    qkv = (torch.randn(n * s, 3 * d, generator=g) * 0.7).bfloat16()
    qkv[min(5, n * s - 1), :d] *= 6.0
    qkv[min(s // 2 + 3, s - 1), d:2 * d] *= 6.0
    for b, (k0, k1) in enumerate(ranges):
        qkv[b * s + (k0 + k1) // 2, d:2 * d] *= 6.0          # a spiked key inside every range
        dead = torch.ones(s, dtype=torch.bool)
        dead[k0:k1] = False
        rows = b * s + torch.nonzero(dead).flatten()
        qkv[rows, d:] = (qkv[rows, d:].float() * 1024.0).bfloat16()
    assert bool(torch.isfinite(qkv.float()).all())
    dout = torch.randn(n * s, d, generator=g).bfloat16()
    return qkv, dout


def work_for(n, s, h):
    return torch.empty(3 * n * h * ((s + 127) // 128) * 128, device="cuda")


def fwd(qkv, kr, n, s, h, hd):
    from pero_pretraining_amd import ops
    out = Guarded(n * s, h * hd, torch.bfloat16)
    lse = Guarded(n * h, s, torch.float32, guard_rows=128 // s + 2)
    if kr is None:
        ops.call("pero_attention_fwd", qkv.t.data_ptr(), out.t.data_ptr(), lse.t.data_ptr(), n, s, h, hd, ops.PERO_BF16, ops.stream())
    else:
        ops.call("pero_attention_fwd_keys", qkv.t.data_ptr(), kr.data_ptr(), out.t.data_ptr(), lse.t.data_ptr(), n, s, h, hd, ops.PERO_BF16, ops.stream())
    return out, lse


def bwd(qkv, kr, out, dout, lse, n, s, h, hd, dvec=None, dbias=None):
    """out given: D is computed and stored (two launches); dvec given: D handed in (head_dim 128: the paired launch)."""
    from pero_pretraining_amd import ops
    dqkv = Guarded(n * s, 3 * h * hd, torch.bfloat16)
    if dvec is None:
        dvec = Guarded(n * s, h, torch.float32)
    work = work_for(n, s, h) if dbias is not None else None
    tail = (None if out is None else out.t.data_ptr(), dout.t.data_ptr(), lse.t.data_ptr(), dvec.t.data_ptr(), dqkv.t.data_ptr(), ops.ptr(dbias), ops.ptr(work),
            n, s, h, hd, ops.PERO_BF16, ops.stream())
    if kr is None:
        ops.call("pero_attention_bwd", qkv.t.data_ptr(), *tail)
    else:
        ops.call("pero_attention_bwd_keys", qkv.t.data_ptr(), kr.data_ptr(), *tail)
    return dqkv, dvec


@functools.lru_cache(maxsize=None)
def case(i, hd):
    """Inputs, the f64 reference and the kernels' results of one case, computed once and shared (read-only) by the tests."""
    n, s, h, ranges = CASES[i]
    d = h * hd
    qkv_c, dout_c = inputs(n, s, h, hd, ranges)
    ref_in = qkv_c.double().requires_grad_(True)
    ref = KR.attention(ref_in, ranges, n, s, h)
    ref.backward(dout_c.double())
    lse_ref = KR.lse2(qkv_c.double(), ranges, n, s, h)
    qkv = Guarded(n * s, 3 * d, torch.bfloat16, data=qkv_c.cuda())
    dout = Guarded(n * s, d, torch.bfloat16, data=dout_c.cuda())
    kr = ranges_tensor(ranges)
    out, lse = fwd(qkv, kr, n, s, h, hd)
    dqkv, dvec = bwd(qkv, kr, out, dout, lse, n, s, h, hd)
    torch.cuda.synchronize()
    return dict(qkv=qkv, dout=dout, kr=kr, out=out, lse=lse, dqkv=dqkv, dvec=dvec, ref=ref.detach(), gref=ref_in.grad, lse_ref=lse_ref)


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_key_range_attention_matches_the_reference_and_stays_inside_the_line(i, hd):
    n, s, h, ranges = CASES[i]
    c = case(i, hd)
    d = h * hd
    out, lse, dqkv, dvec = c["out"], c["lse"], c["dqkv"], c["dvec"]
    for name in ("out", "lse", "dqkv", "dvec"):
        assert bool(torch.isfinite(c[name].t.float()).all()), name + ": not finite (a leaked dead key, or a read behind the line's last row)"
        assert c[name].intact(), name + ": guard rows changed (a store behind the line's last row)"
    err = rel_err(out.t, c["ref"])
    lerr = float((lse.t.cpu().double().reshape(n, h, s) - c["lse_ref"]).abs().max())
    print(f"\nKEYS hd={hd} n={n} S={s} h={h}: out rel {err:.3e}  lse abs {lerr:.3e}", end="")
    assert err < 2 ** -7
    assert lerr < 2e-3
    want_d = (out.t.float() * c["dout"].t.float()).reshape(n * s, h, hd).sum(-1)
    assert float((dvec.t - want_d).abs().max()) <= 1e-3 * max(1.0, float(want_d.abs().max()))
    qkv_d, dout_d = c["qkv"].t.double().cpu(), c["dout"].t.double().cpu()
    for name, sl in (("dq", slice(0, d)), ("dk", slice(d, 2 * d)), ("dv", slice(2 * d, 3 * d))):
        if name != "dv":
            # A line with ONE key: P = 1 whatever q and k are, so its dq and dk are 0 exactly and no relative error against them exists.  The kernels
            # form dS = P (dP - D) / sqrt(hd) with dP = dO . v and D = dO . O, O = v exactly (P = 1, l = 1): two f32 sums of the same hd products in
            # different orders, each within hd x 2^-24 of the sum of the products' magnitudes.  So per query |dq| <= 2 hd 2^-24 |k| sum_d |dO_d v_d| /
            # sqrt(hd) - the bound of the ragged test's S = 1 case - and dk, a sum over the line's S queries, S times that with q for k.
            for b, (k0, k1) in enumerate(ranges):
                if k1 - k0 != 1:
                    continue
                rows = slice(b * s, (b + 1) * s)
                assert float(c["gref"][rows, sl].abs().max()) < 1e-12
                v = qkv_d[b * s + k0, 2 * d:]
                unc = float((dout_d[rows].abs() * v.abs()[None]).reshape(s, h, hd).sum(-1).max()) / math.sqrt(hd)
                other = float(qkv_d[b * s + k0, d:2 * d].abs().max()) if name == "dq" else float(qkv_d[rows, :d].abs().max()) * s
                got = float(dqkv.t[rows, sl].double().abs().max())
                print(f"  {name}[line {b}] abs {got:.3e} (bound {2 * hd * 2.0 ** -24 * unc * other:.3e})", end="")
                assert got <= 2 * hd * 2.0 ** -24 * unc * other, (name, b, got)
        if float(c["gref"][:, sl].abs().max()) < 1e-12:
            continue   # every line has one key: bounded absolutely above
        e = rel_err(dqkv.t[:, sl], c["gref"][:, sl])
        a, b_ = dqkv.t[:, sl].double().cpu().flatten(), c["gref"][:, sl].flatten()
        cos = float(a @ b_ / (a.norm() * b_.norm()))
        print(f"  {name} rel {e:.3e} cos {cos:.6f}", end="")
        assert e < 3e-2, (name, e)
        assert cos > 0.9995, (name, cos)
    # dK and dV rows outside a line's range: exact zeros
    for b, (k0, k1) in enumerate(ranges):
        dead = torch.ones(s, dtype=torch.bool)
        dead[k0:k1] = False
        rows = b * s + torch.nonzero(dead).flatten().cuda()
        assert bool((dqkv.t[rows, d:] == 0).all()), f"line {b}: a dK / dV row outside the range is not zero"
        assert float(c["gref"][rows.cpu(), d:].abs().max()) == 0.0 if rows.numel() else True
    # in_proj's bias gradient, accumulated into a pre-filled vector: the column sums of the stored dqkv
    dbias = torch.full((3 * d,), 2.0, device="cuda")
    dqkv2, dvec2 = bwd(c["qkv"], c["kr"], out, c["dout"], lse, n, s, h, hd, dbias=dbias)
    assert torch.equal(dqkv2.t, dqkv.t) and dqkv2.intact() and dvec2.intact()
    want = 2.0 + dqkv.t.float().sum(0)
    assert float((dbias - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))
    # D handed in (head_dim 128: the paired launch): the same dqkv bit for bit, and the same bias gradient
    dvec_in = Guarded(n * s, h, torch.float32, data=dvec.t)
    dbias3 = torch.full((3 * d,), 2.0, device="cuda")
    dqkv3, _ = bwd(c["qkv"], c["kr"], None, c["dout"], lse, n, s, h, hd, dvec=dvec_in, dbias=dbias3)
    assert torch.equal(dqkv3.t, dqkv.t) and dqkv3.intact() and torch.equal(dvec_in.t, dvec.t)
    assert float((dbias3 - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_full_ranges_give_the_bits_of_the_calls_without_ranges(i, hd):
    """[0, S) on every line: the same tiles, the same MFMAs in the same order, and no select fires - out, lse and dqkv equal those of
    pero_attention_fwd / pero_attention_bwd bit for bit, with D computed and with D handed in."""
    n, s, h, _ = CASES[i]
    c = case(i, hd)
    kr = ranges_tensor([(0, s)] * n)
    out_k, lse_k = fwd(c["qkv"], kr, n, s, h, hd)
    out_u, lse_u = fwd(c["qkv"], None, n, s, h, hd)
    assert torch.equal(out_k.t, out_u.t) and torch.equal(lse_k.t, lse_u.t)
    dq_k, dvec_k = bwd(c["qkv"], kr, out_k, c["dout"], lse_k, n, s, h, hd)
    dq_u, dvec_u = bwd(c["qkv"], None, out_u, c["dout"], lse_u, n, s, h, hd)
    assert torch.equal(dq_k.t, dq_u.t) and torch.equal(dvec_k.t, dvec_u.t)
    d = h * hd
    db_k, db_u = torch.zeros(3 * d, device="cuda"), torch.zeros(3 * d, device="cuda")
    dvec_in = Guarded(n * s, h, torch.float32, data=dvec_u.t)
    pair_k, _ = bwd(c["qkv"], kr, None, c["dout"], lse_k, n, s, h, hd, dvec=dvec_in, dbias=db_k)
    pair_u, _ = bwd(c["qkv"], None, None, c["dout"], lse_u, n, s, h, hd, dvec=dvec_in, dbias=db_u)
    assert torch.equal(pair_k.t, pair_u.t) and torch.equal(pair_k.t, dq_u.t)
    assert float((db_k - db_u).abs().max()) <= 1e-3 * max(1.0, float(db_u.abs().max()))
    for g in (out_k, lse_k, dq_k, dvec_k, pair_k):
        assert g.intact() and bool(torch.isfinite(g.t.float()).all())


@pytest.mark.parametrize("hd", HDS)
def test_lines_with_ranges_are_independent(hd):
    """Three lines with three kinds of range in one call equal the three one-line calls, bit for bit."""
    i = 2
    n, s, h, ranges = CASES[i]
    c = case(i, hd)
    d = h * hd
    for b in range(n):
        rows = slice(b * s, (b + 1) * s)
        qkv = Guarded(s, 3 * d, torch.bfloat16, data=c["qkv"].t[rows])
        dout = Guarded(s, d, torch.bfloat16, data=c["dout"].t[rows])
        kr = ranges_tensor([ranges[b]])
        out, lse = fwd(qkv, kr, 1, s, h, hd)
        dqkv, dvec = bwd(qkv, kr, out, dout, lse, 1, s, h, hd)
        assert torch.equal(out.t, c["out"].t[rows]), b
        assert torch.equal(lse.t, c["lse"].t[b * h:(b + 1) * h]), b
        assert torch.equal(dqkv.t, c["dqkv"].t[rows]), b
        assert torch.equal(dvec.t, c["dvec"].t[rows]), b
        assert out.intact() and lse.intact() and dqkv.intact() and dvec.intact()


@pytest.mark.parametrize("hd", HDS)
def test_a_bad_range_is_clamped_by_the_kernels(hd):
    """Nothing on the host reads the ranges: k0 is clamped into [0, S - 1], k1 into [k0 + 1, S].  Empty, inverted and out-of-line ranges
    give the results of their clamped forms, bit for bit."""
    n, s, h = 4, 132, 2
    bad = [(50, 50), (90, 10), (-7, 300), (500, 600)]
    good = [(50, 51), (90, 91), (0, 132), (131, 132)]
    qkv_c, dout_c = inputs(n, s, h, hd, good)
    qkv = Guarded(n * s, 3 * h * hd, torch.bfloat16, data=qkv_c.cuda())
    dout = Guarded(n * s, h * hd, torch.bfloat16, data=dout_c.cuda())
    res = []
    for ranges in (bad, good):
        kr = ranges_tensor(ranges)
        out, lse = fwd(qkv, kr, n, s, h, hd)
        dqkv, dvec = bwd(qkv, kr, out, dout, lse, n, s, h, hd)
        assert out.intact() and lse.intact() and dqkv.intact() and dvec.intact() and bool(torch.isfinite(dqkv.t.float()).all())
        res.append((out.t, lse.t, dqkv.t))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_softmax_with_key_ranges(dtype):
    """pero_softmax_fwd_keys against f64: exact zeros outside the line's range, inside it the tolerance of test_gpu_ops.py::test_softmax_fwd_bwd; the
    unchanged pero_softmax_bwd on these probabilities gives the gradient of the masked softmax."""
    from pero_pretraining_amd import ops
    n, h, s = 3, 2, 100
    ranges = [(3, 90), (99, 100), (0, 100)]
    g = torch.Generator().manual_seed(1)
    sc = torch.randn(n * h * s, s, generator=g) * 4
    for b, (k0, k1) in enumerate(ranges):   # scores outside the range: large, a leak would take the whole row
        sc[b * h * s:(b + 1) * h * s, :k0] += 60.0
        sc[b * h * s:(b + 1) * h * s, k1:] += 60.0
    dead = KR.key_padding_mask(ranges, s).repeat_interleave(h * s, dim=0)
    sr = sc.double().requires_grad_(True)
    p_ref = torch.softmax((sr * 0.3).masked_fill(dead, float("-inf")), -1)
    dp = torch.randn(n * h * s, s, generator=g)
    p_ref.backward(dp.double())
    p = ops.softmax_fwd(sc.cuda().view(n * h, s, s), 0.3, dtype, key_ranges=ranges_tensor(ranges), rows_per_line=h * s).view(n * h * s, s)
    assert bool((p[dead.cuda()] == 0).all())
    assert rel_err(p, p_ref.detach()) < (1e-6 if dtype == torch.float32 else 2 ** -8)
    ds = ops.softmax_bwd(p, dp.cuda(), 0.3)
    assert bool((ds[dead.cuda()] == 0).all())
    assert rel_err(ds, sr.grad) < (1e-5 if dtype == torch.float32 else 2 ** -6)
