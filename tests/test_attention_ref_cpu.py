"""CPU: tests/attention_ref.py, the yardstick of tests/test_gpu_attention_parity.py, at every case that test runs.

* The restatement is pinned: the forward to the oracle's attention (and, with ranges, to tests/attention_keys_ref.py) at rtol 1e-12, the backward -
  with the exact f64 `out` and `lse` handed in - to torch autograd in f64 at 1e-10.
* A CPU model of the kernels' arithmetic (f32 scores from the bf16 operands, p = exp2(fma(s, c, -m c)) per 128-key tile with the online rescale,
  l summed from the unrounded p, P and dS rounded to bf16 in front of their products, f32 accumulators, bf16 outputs) stays inside the bound at every
  case: the condition on the inputs, reference and model alone must stay below 1.
* Teeth: defects planted in the model - P of the second 128-query block weighing 2 % less in dV, dS of the line's last key 10 % off, the line's last key
  dropped from P V - are rejected by the bound; the first two pass the norm-wise metrics of the earlier attention tests (max|got - ref| / max|ref| <
  3e-2 and cosine > 0.9995) at S = 260, which is why this file exists."""
import functools
import math

import pytest
import torch

import attention_keys_ref as KR
import attention_ref as A
from oracle import pero_oracle as O

CASES = A.all_cases()
IDS = [A.case_id(c) for c in CASES]


def bf16(x):
    return x.bfloat16().float()


def fma32(s, c, z):
    """f32 fma(s, c, z): the product of two f32 values is exact in f64; one rounding of the sum to f64 sits far below the one to f32."""
    return (s.double() * float(c) + z.double()).float()


def model_forward(qkv, n, s, h, hd, ranges=None, defect=None):
    """The forward kernels' arithmetic, line by line over the key tiles that hold a live key.  defect "drop_last_key": the line's last live key does not
    enter P V (it still enters l)."""
    d = h * hd
    c = torch.tensor(A.LOG2E / math.sqrt(hd), dtype=torch.float64).float()
    kr = A.clamp_ranges(ranges, n, s)
    out = torch.empty(n * s, d, dtype=torch.bfloat16)
    lse = torch.empty(n * h, s, dtype=torch.float32)
    x = qkv.float().reshape(n, s, 3, h, hd).permute(2, 0, 3, 1, 4)
    for b in range(n):
        q, k, v = x[0, b], x[1, b], x[2, b]                  # (h, S, hd) f32
        k0, k1 = int(kr[b, 0]), int(kr[b, 1])
        m = torch.full((h, s), -math.inf)
        l = torch.zeros(h, s)
        o = torch.zeros(h, s, hd)
        for kt in range(k0 // 128, (k1 + 127) // 128):
            lo, hi = kt * 128, min(s, kt * 128 + 128)
            sc = q @ k[:, lo:hi].transpose(-1, -2)
            pos = torch.arange(lo, hi)
            sc = sc.masked_fill(~((pos >= k0) & (pos < k1))[None, None, :], -math.inf)
            mn = torch.maximum(m, sc.max(-1).values)
            alpha = torch.exp2((m - mn) * c)
            mc = mn * c
            p = torch.exp2(fma32(sc, c, -mc[..., None]))
            l = l * alpha + p.sum(-1)
            pb = bf16(p)
            if defect == "drop_last_key" and lo <= k1 - 1 < hi:
                pb[..., k1 - 1 - lo] = 0.0
            o = o * alpha[..., None] + pb @ v[:, lo:hi]
            m = mn
        inv = 1.0 / l
        out[b * s:(b + 1) * s] = (o * inv[..., None]).permute(1, 0, 2).reshape(s, d).bfloat16()
        lse[b * h:(b + 1) * h] = m * c + torch.log2(l)
    return out, lse


def model_backward(qkv, out_given, dout, lse_given, n, s, h, hd, ranges=None, defect=None):
    """The backward kernels' arithmetic.  Defects: "dv_second_block" - the P packed for dV weighs 2 % less for the queries 128 .. 255; "ds_last_key" - dS of
    the line's last live key is 10 % off."""
    d = h * hd
    c = torch.tensor(A.LOG2E / math.sqrt(hd), dtype=torch.float64).float()
    scale = torch.tensor(1.0 / math.sqrt(hd), dtype=torch.float64).float()
    kr = A.clamp_ranges(ranges, n, s)
    x = qkv.float().reshape(n, s, 3, h, hd).permute(2, 0, 3, 1, 4)
    og = out_given.float().reshape(n, s, h, hd).permute(0, 2, 1, 3)
    do = dout.float().reshape(n, s, h, hd).permute(0, 2, 1, 3)
    lse = lse_given.float().reshape(n, h, s)
    dqkv = torch.empty(n * s, 3 * d, dtype=torch.bfloat16)
    dvec = torch.empty(n * s, h, dtype=torch.float32)
    for b in range(n):
        q, k, v = x[0, b], x[1, b], x[2, b]
        k0, k1 = int(kr[b, 0]), int(kr[b, 1])
        pos = torch.arange(s)
        dead = ~((pos >= k0) & (pos < k1))[None, None, :]
        sc = q @ k.transpose(-1, -2)
        p = torch.exp2(fma32(sc, c, -lse[b][..., None])).masked_fill(dead, 0.0)
        dp = do[b] @ v.transpose(-1, -2)
        dsum = (do[b] * og[b]).sum(-1)
        ds = (p * (dp - dsum[..., None]) * scale).masked_fill(dead, 0.0)
        if defect == "ds_last_key":
            ds[..., k1 - 1] *= 0.9
        p_dv = p.clone()
        if defect == "dv_second_block":
            p_dv[:, 128:256, :] *= 0.98
        dv = bf16(p_dv).transpose(-1, -2) @ do[b]
        dq = bf16(ds) @ k
        dk = bf16(ds).transpose(-1, -2) @ q
        r = slice(b * s, (b + 1) * s)
        for i, t in enumerate((dq, dk, dv)):
            dqkv[r, i * d:(i + 1) * d] = t.permute(1, 0, 2).reshape(s, d).bfloat16()
        dvec[r] = dsum.t()
    return dqkv, dvec


@functools.lru_cache(maxsize=None)
def case(i):
    """Inputs, the f64 reference with its bounds, and the clean model's outputs of one case, computed once and shared (read-only)."""
    hd, n, s, h, ranges = CASES[i]
    qkv, dout = A.inputs(hd, n, s, h, ranges)
    fwd, fwd_b = A.forward(qkv, n, s, h, hd, ranges)
    out_m, lse_m = model_forward(qkv, n, s, h, hd, ranges)
    out_g, lse_g = fwd["out"].bfloat16(), fwd["lse2"].float()     # the host-rounded reference values: what the GPU test hands the backward first
    bwd, bwd_b = A.backward(qkv, out_g, dout, lse_g, n, s, h, hd, ranges)
    dqkv_m, dvec_m = model_backward(qkv, out_g, dout, lse_g, n, s, h, hd, ranges)
    return dict(qkv=qkv, dout=dout, fwd=fwd, fwd_b=fwd_b, out_m=out_m, lse_m=lse_m, out_g=out_g, lse_g=lse_g, bwd=bwd, bwd_b=bwd_b, dqkv_m=dqkv_m, dvec_m=dvec_m)


def grads(dqkv, d):
    return {"dq": dqkv[:, :d], "dk": dqkv[:, d:2 * d], "dv": dqkv[:, 2 * d:]}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_forward_restatement_is_the_oracle(i):
    hd, n, s, h, ranges = CASES[i]
    c = case(i)
    x = c["qkv"].double()
    # rtol 1e-12 of the element, or of the largest |v| where the sum cancels (an output element is a convex combination of v's)
    atol = 1e-12 * float(x[:, 2 * h * hd:].abs().max())
    if ranges is None:
        want, want_l = O.attention(x, n, s, h), KR.lse2(x, [(0, s)] * n, n, s, h)
    else:
        want, want_l = KR.attention(x, ranges, n, s, h), KR.lse2(x, ranges, n, s, h)
        # a full range is the oracle's attention too
        if all(tuple(r) == (0, s) for r in ranges):
            torch.testing.assert_close(c["fwd"]["out"], O.attention(x, n, s, h), rtol=1e-12, atol=atol)
    torch.testing.assert_close(c["fwd"]["out"], want, rtol=1e-12, atol=atol)
    torch.testing.assert_close(c["fwd"]["lse2"], want_l.reshape(n * h, s), rtol=1e-12, atol=1e-12)
    for b in c["fwd_b"].values():
        assert bool(torch.isfinite(b).all()) and bool((b > 0).all())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_backward_restatement_is_autograd_of_the_forward_when_handed_its_exact_outputs(i):
    hd, n, s, h, ranges = CASES[i]
    c = case(i)
    d = h * hd
    x = c["qkv"].double().requires_grad_(True)
    ref = O.attention(x, n, s, h) if ranges is None else KR.attention(x, ranges, n, s, h)
    ref.backward(c["dout"].double())
    got, _ = A.backward(c["qkv"], c["fwd"]["out"], c["dout"], c["fwd"]["lse2"], n, s, h, hd, ranges)
    tol = 1e-10 * max(1.0, float(x.grad.abs().max()))
    for name, g in grads(x.grad, d).items():
        assert float((got[name] - g).abs().max()) <= tol, name
    want_d = (c["dout"].double() * c["fwd"]["out"]).reshape(n * s, h, hd).sum(-1)
    assert float((got["dvec"] - want_d).abs().max()) <= 1e-10 * max(1.0, float(want_d.abs().max()))
    # D handed in is used as it stands
    got2, _ = A.backward(c["qkv"], c["fwd"]["out"], c["dout"], c["fwd"]["lse2"], n, s, h, hd, ranges, dvec_given=want_d + 1.0)
    assert torch.equal(got2["dvec"], want_d + 1.0)
    # rows outside a range: exact zeros of the reference
    dead = ~A.live_keys(ranges, n, s).reshape(n * s)
    assert float(got["dk"][dead].abs().max() if bool(dead.any()) else 0.0) == 0.0
    assert float(got["dv"][dead].abs().max() if bool(dead.any()) else 0.0) == 0.0


def test_ranges_are_clamped_as_the_header_says():
    got = A.clamp_ranges([(50, 50), (90, 10), (-7, 300), (500, 600)], 4, 132).tolist()
    assert got == [[50, 51], [90, 91], [0, 132], [131, 132]]
    assert A.clamp_ranges(None, 2, 5).tolist() == [[0, 5], [0, 5]]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_model_of_the_kernels_stays_inside_the_bound(i):
    hd, n, s, h, ranges = CASES[i]
    c = case(i)
    d = h * hd
    r = {"out": A.worst_ratio(c["out_m"], c["fwd"]["out"], c["fwd_b"]["out"])[0],
         "lse2": A.worst_ratio(c["lse_m"], c["fwd"]["lse2"], c["fwd_b"]["lse2"])[0],
         "dvec": A.worst_ratio(c["dvec_m"], c["bwd"]["dvec"], c["bwd_b"]["dvec"])[0]}
    for name, g in grads(c["dqkv_m"], d).items():
        r[name] = A.worst_ratio(g, c["bwd"][name], c["bwd_b"][name])[0]
    # second form: the model's own out and lse handed to the backward, the reference re-evaluated on them
    bwd2, bnd2 = A.backward(c["qkv"], c["out_m"], c["dout"], c["lse_m"], n, s, h, hd, ranges)
    dqkv2, _ = model_backward(c["qkv"], c["out_m"], c["dout"], c["lse_m"], n, s, h, hd, ranges)
    for name, g in grads(dqkv2, d).items():
        r[name + "'"] = A.worst_ratio(g, bwd2[name], bnd2[name])[0]
    print("\nMODEL " + IDS[i] + ": " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()), end="")
    for k, v in r.items():
        assert v <= 1.0, (k, v)


def old_metrics(got, ref):
    """The norm-wise pair of the earlier attention tests: max|got - ref| / max|ref| and the cosine."""
    a, b = got.double().flatten(), ref.double().flatten()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)), float(a @ b / (a.norm() * b.norm()))


TEETH = [i for i, cs in enumerate(CASES) if cs[2] > 128]   # (more than one 128-query block)


@pytest.mark.parametrize("i", TEETH, ids=[IDS[i] for i in TEETH])
def test_bound_rejects_the_planted_defects(i):
    hd, n, s, h, ranges = CASES[i]
    c = case(i)
    d = h * hd
    bad_dv = grads(model_backward(c["qkv"], c["out_g"], c["dout"], c["lse_g"], n, s, h, hd, ranges, defect="dv_second_block")[0], d)
    bad_ds = grads(model_backward(c["qkv"], c["out_g"], c["dout"], c["lse_g"], n, s, h, hd, ranges, defect="ds_last_key")[0], d)
    bad_out, _ = model_forward(c["qkv"], n, s, h, hd, ranges, defect="drop_last_key")
    r_dv = A.worst_ratio(bad_dv["dv"], c["bwd"]["dv"], c["bwd_b"]["dv"])[0]
    r_dq = A.worst_ratio(bad_ds["dq"], c["bwd"]["dq"], c["bwd_b"]["dq"])[0]
    r_dk = A.worst_ratio(bad_ds["dk"], c["bwd"]["dk"], c["bwd_b"]["dk"])[0]
    r_out = A.worst_ratio(bad_out, c["fwd"]["out"], c["fwd_b"]["out"])[0]
    print(f"\nTEETH {IDS[i]}: dv(2 % in block 2) {r_dv:.2f}  dq / dk (last key 10 %) {r_dq:.2f} / {r_dk:.2f}  out(last key dropped) {r_out:.2f}", end="")
    if ranges is None and s >= 256:   # a whole second query block on every key (at S = 132 the block has 4 queries: 2 % of them is below P's bf16 rounding)
        assert r_dv > 1.0
    assert r_dq > 1.0 and r_dk > 1.0
    assert r_out > 1.0


def test_the_normwise_metrics_accept_the_first_two_defects_at_s_260():
    """(3, 260, 4) at head_dim 128, no ranges: the shape of the issue's table.  The earlier tests' reference for the gradients is autograd of the f64
    forward; against it the defective model passes rel < 3e-2 and cosine > 0.9995 on every gradient, and fails the per-element bound."""
    i = CASES.index((128, 3, 260, 4, None))
    hd, n, s, h, ranges = CASES[i]
    c = case(i)
    d = h * hd
    x = c["qkv"].double().requires_grad_(True)
    O.attention(x, n, s, h).backward(c["dout"].double())
    ref = grads(x.grad, d)
    for defect, names in (("dv_second_block", ("dv",)), ("ds_last_key", ("dq", "dk"))):
        out_m, lse_m = c["out_m"], c["lse_m"]          # as in the earlier tests: the backward gets the forward's own outputs
        bad = grads(model_backward(c["qkv"], out_m, c["dout"], lse_m, n, s, h, hd, ranges, defect=defect)[0], d)
        bwd2, bnd2 = A.backward(c["qkv"], out_m, c["dout"], lse_m, n, s, h, hd, ranges)
        for name in ("dq", "dk", "dv"):
            rel, cos = old_metrics(bad[name], ref[name])
            print(f"\nOLD METRICS {defect} {name}: rel {rel:.3e} (tolerance 3e-2) cos {cos:.6f} (0.9995)", end="")
            assert rel < 3e-2 and cos > 0.9995, (defect, name, rel, cos)
        for name in names:
            assert A.worst_ratio(bad[name], bwd2[name], bnd2[name])[0] > 1.0, (defect, name)
