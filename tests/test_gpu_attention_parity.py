"""The fused attention kernels (pero_attention_fwd / _bwd and their _keys forms, head_dim 128 and 64) against the f64 restatement of the header's
formulas in tests/attention_ref.py, element by element: |got - ref| <= the bound derived there (P's and dS's bf16 rounding, the f32 roundings of
exp2's argument, the f32 accumulations, the output's bf16 rounding - nothing measured, no safety factor).  tests/test_attention_ref_cpu.py pins
the restatement, shows that a CPU model of the kernels' arithmetic stays inside the bound on these inputs, and that defects of a few per cent in one
query block or one key row - which the norm-wise tolerances of the other attention tests let through - do not.

The four entry points are called directly; every tensor is a guarded allocation of tests/test_gpu_attention_ragged.py (NaN rows behind the inputs,
a bit pattern behind the outputs).  Inputs: that file's recipe, and with ranges that of tests/test_gpu_attention_keys.py (a spiked key inside every
range, dead K / V rows x 2^10).  Cases (attention_ref.all_cases): the smallest (n, S, h) that reach each instantiation at both head widths - one ragged
tile, S % 128 = 0 with one and two key tiles, a 4-key last tile, four tiles - and the six range cases of the keys test.

Per case: out and lse against `forward`; the backward twice - with the host-rounded REFERENCE out / lse handed in and `out` passed (D computed; the
backward is then independent of the forward kernel), then with the forward kernel's own out / lse and D handed in (`out` null: the paired launch at
head_dim 128), the reference re-evaluated on exactly those tensors; D, dQ, dK, dV against `backward`; exact zeros in the dK / dV rows outside a
range; guards intact, outputs finite; the bias gradient, accumulated into a pre-filled vector, against the column sums of the stored dqkv
(parity_ref.assert_within, n_terms = N S).  Without ranges, one call with the full range [0, S) gives the same bits."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_ref as A  # noqa: E402
import parity_ref as R  # noqa: E402
from test_gpu_attention_keys import bwd, fwd, ranges_tensor  # noqa: E402
from test_gpu_attention_ragged import Guarded  # noqa: E402

CASES = A.all_cases()
IDS = [A.case_id(c) for c in CASES]
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    yield _ops
    print("\nPARITY_RATIOS " + json.dumps({k: round(v, 4) for k, v in sorted(R.RATIOS.items())}))


def sound(*tensors):
    for t in tensors:
        assert t.intact(), "guard rows changed (a store behind the line's last row)"
        assert bool(torch.isfinite(t.t.float()).all()), "not finite (a leaked dead key, or a read behind the line's last row)"


def check_backward(tag, dqkv, ref, bnd, d, dead_rows):
    got = dqkv.t.cpu()
    for j, name in enumerate(("dq", "dk", "dv")):
        A.assert_inside(got[:, j * d:(j + 1) * d], ref[name], bnd[name], tag + " " + name, BF16)
    # the dK and dV rows outside the line's range are exact zeros (header), in the reference and in the kernel
    if dead_rows.numel():
        assert float(ref["dk"][dead_rows].abs().max()) == 0.0 and float(ref["dv"][dead_rows].abs().max()) == 0.0
        assert bool((got[dead_rows][:, d:] == 0).all()), "a dK / dV row outside the range is not zero"


def check_dbias(tag, dbias, dqkv, n, s):
    # N S stored bf16 values per column, converted exactly and added in f32 in some order (per-workgroup partial rows, then one reduction), onto the 2.0
    want, mag = R.colsum(dqkv.t.float(), torch.full((dqkv.t.shape[1],), 2.0))
    R.assert_within(dbias, want, mag, n * s, F32, what=tag + " dbias")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_attention_kernels_stay_inside_the_f64_bound(ops, i):
    hd, n, s, h, ranges = CASES[i]
    d = h * hd
    keys = "_keys" if ranges is not None else ""
    tag_f, tag_b = f"attention_fwd{keys} hd{hd}", f"attention_bwd{keys} hd{hd}"
    qkv_c, dout_c = A.inputs(hd, n, s, h, ranges)
    qkv = Guarded(n * s, 3 * d, BF16, data=qkv_c.cuda())
    dout = Guarded(n * s, d, BF16, data=dout_c.cuda())
    kr = None if ranges is None else ranges_tensor(ranges)
    dead_rows = torch.nonzero(~A.live_keys(ranges, n, s).reshape(n * s)).flatten()

    # ---- forward
    ref_f, bnd_f = A.forward(qkv_c, n, s, h, hd, ranges)
    out, lse = fwd(qkv, kr, n, s, h, hd)
    sound(out, lse)
    A.assert_inside(out.t, ref_f["out"], bnd_f["out"], tag_f + " out", BF16)
    A.assert_inside(lse.t, ref_f["lse2"], bnd_f["lse2"], tag_f + " lse2", F32)
    if ranges is None:   # the full range [0, S) on every line: the bits of the call without ranges
        out_k, lse_k = fwd(qkv, ranges_tensor([(0, s)] * n), n, s, h, hd)
        assert torch.equal(out_k.t, out.t) and torch.equal(lse_k.t, lse.t) and out_k.intact() and lse_k.intact()

    # ---- backward, independent of the forward kernel: the host-rounded reference out and lse handed in, `out` passed so that D is computed
    out_c, lse_c = ref_f["out"].bfloat16(), ref_f["lse2"].float()
    out_g = Guarded(n * s, d, BF16, data=out_c.cuda())
    lse_g = Guarded(n * h, s, F32, guard_rows=128 // s + 2, data=lse_c.cuda())
    ref_b, bnd_b = A.backward(qkv_c, out_c, dout_c, lse_c, n, s, h, hd, ranges)
    dbias = torch.full((3 * d,), 2.0, device="cuda")
    dqkv, dvec = bwd(qkv, kr, out_g, dout, lse_g, n, s, h, hd, dbias=dbias)
    sound(dqkv, dvec)
    A.assert_inside(dvec.t, ref_b["dvec"], bnd_b["dvec"], tag_b + " D", F32)
    check_backward(tag_b, dqkv, ref_b, bnd_b, d, dead_rows)
    check_dbias(tag_b, dbias, dqkv, n, s)

    # ---- backward on the forward kernel's own out and lse, D handed in (`out` null; head_dim 128: the paired launch); the reference on those tensors
    out_h, lse_h = out.t.cpu(), lse.t.cpu()
    d_in = (dout_c.double() * out_h.double()).reshape(n * s, h, hd).sum(-1).float()
    ref_p, bnd_p = A.backward(qkv_c, out_h, dout_c, lse_h, n, s, h, hd, ranges, dvec_given=d_in)
    dvec_in = Guarded(n * s, h, F32, data=d_in.cuda())
    dbias_p = torch.full((3 * d,), 2.0, device="cuda")
    dqkv_p, _ = bwd(qkv, kr, None, dout, lse, n, s, h, hd, dvec=dvec_in, dbias=dbias_p)
    sound(dqkv_p)
    assert torch.equal(dvec_in.t.cpu(), d_in)   # (D is read, not rewritten)
    check_backward(tag_b + " D given", dqkv_p, ref_p, bnd_p, d, dead_rows)
    check_dbias(tag_b + " D given", dbias_p, dqkv_p, n, s)
