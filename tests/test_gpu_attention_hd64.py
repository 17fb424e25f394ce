"""Fused attention at head_dim 64 (csrc/attention_hd64.hip), forward and backward, against the oracle's attention in f64 on the same bf16
inputs, at the smallest shapes that reach each mechanism: one key, the XCD block map (16 units) and the plain one (6), one partial tile, exactly
one full tile, a full tile plus a 4-row tail, an odd tail, the loader's real width (d = 512, 8 heads, S = 260), four tiles for the online-softmax
rescale.  At these shapes a forward workgroup takes one head; test_hd64_several_heads_per_workgroup runs the smallest shapes at which the
launcher picks two.

As in tests/test_gpu_attention_ragged.py every tensor a kernel touches is a view into a larger allocation whose rows behind the view are
guards: NaN behind the inputs, a bit pattern (itself a NaN) behind the outputs, a whole tile of them.  An unclamped read of the last line's
tail shows as a non-finite output, an unguarded store as a changed guard.  Bounds: those of tests/test_gpu_ops.py::test_fused_attention_fwd_bwd
and the ragged test.  Measured on an MI355X over the eight shapes: see test_hd64_attention_matches_the_oracle_and_stays_inside_the_line."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pero_oracle as O  # noqa: E402

GUARD_ROWS = 128            # a whole tile: nothing runs out of bounds even without a clamp
PAT16, PAT32 = 0x7FC5, 0x7FC12345   # bf16 / f32 NaN patterns
SHAPES = [(1, 1, 1), (2, 4, 8), (3, 100, 2), (2, 128, 4), (2, 132, 4), (1, 191, 1), (3, 260, 8), (1, 388, 2)]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


class Guarded:
    """A (rows, cols) view at the start of an allocation of rows + guard rows."""

    def __init__(self, rows, cols, dtype, guard_rows=GUARD_ROWS, data=None):
        self.buf = torch.empty((rows + guard_rows, cols), device="cuda", dtype=dtype)
        self.ints = self.buf.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)
        self.pattern = PAT16 if dtype == torch.bfloat16 else PAT32
        self.rows = rows
        self.ints.fill_(self.pattern)
        self.t = self.buf[:rows]
        if data is not None:
            self.t.copy_(data)
            self.buf[rows:] = float("nan")
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.ints[self.rows:] == self.pattern).all())


def inputs(n, s, h, hd):
    """The recipe of test_fused_attention_fwd_bwd: randn * 0.7, a spiked query row, a spiked key row inside the line, and a spiked key in the
    last partial tile where the line has more than one tile."""
    d = h * hd
    g = torch.Generator().manual_seed(n * 1000 + s + h)
    qkv = (torch.randn(n * s, 3 * d, generator=g) * 0.7).bfloat16()
    qkv[min(5, n * s - 1), :d] *= 6.0
    qkv[min(s // 2 + 3, s - 1), d:2 * d] *= 6.0
    nb = (s + 127) // 128
    if nb > 1 and s % 128:
        qkv[128 * (nb - 1) + (s - 128 * (nb - 1)) // 2, d:2 * d] *= 6.0
    dout = torch.randn(n * s, d, generator=g).bfloat16()
    return qkv, dout


def fwd(qkv, n, s, h, hd=64):
    from pero_pretraining_amd import ops
    out = Guarded(n * s, h * hd, torch.bfloat16)
    lse = Guarded(n * h, s, torch.float32, guard_rows=128 // s + 2)
    ops.call("pero_attention_fwd", qkv.t.data_ptr(), out.t.data_ptr(), lse.t.data_ptr(), n, s, h, hd, ops.PERO_BF16, ops.stream())
    return out, lse


def bwd(qkv, out, dout, lse, n, s, h, dvec=None, dbias=None, hd=64):
    """out given: D is computed and stored; out None and dvec given: D handed in.  The workspace has the size ops.attention_bwd_fused allocates."""
    from pero_pretraining_amd import ops
    dqkv = Guarded(n * s, 3 * h * hd, torch.bfloat16)
    if dvec is None:
        dvec = Guarded(n * s, h, torch.float32)
    work = torch.empty(3 * n * h * ((s + 127) // 128) * 128, device="cuda") if dbias is not None else None
    ops.call("pero_attention_bwd", qkv.t.data_ptr(), None if out is None else out.t.data_ptr(), dout.t.data_ptr(), lse.t.data_ptr(), dvec.t.data_ptr(),
             dqkv.t.data_ptr(), ops.ptr(dbias), ops.ptr(work), n, s, h, hd, ops.PERO_BF16, ops.stream())
    return dqkv, dvec


@functools.lru_cache(maxsize=None)
def case(n, s, h, hd=64):
    """Inputs, the f64 reference and the kernels' results of one shape, computed once and shared (read-only) by the tests."""
    d = h * hd
    qkv_c, dout_c = inputs(n, s, h, hd)
    ref_in = qkv_c.double().requires_grad_(True)
    ref = O.attention(ref_in, n, s, h)
    ref.backward(dout_c.double())
    q, k, _ = qkv_c.double().reshape(n, s, 3, h, hd).permute(2, 0, 3, 1, 4)
    lse_ref = torch.logsumexp((q @ k.transpose(-1, -2)) / math.sqrt(hd), -1) / math.log(2.0)
    qkv = Guarded(n * s, 3 * d, torch.bfloat16, data=qkv_c.cuda())
    dout = Guarded(n * s, d, torch.bfloat16, data=dout_c.cuda())
    out, lse = fwd(qkv, n, s, h, hd)
    dqkv, dvec = bwd(qkv, out, dout, lse, n, s, h, hd=hd)
    torch.cuda.synchronize()
    return dict(qkv=qkv, dout=dout, out=out, lse=lse, dqkv=dqkv, dvec=dvec, ref=ref.detach(), gref=ref_in.grad, lse_ref=lse_ref)


def check_against_the_oracle(c, n, s, h, hd, tag):
    d = h * hd
    out, lse, dqkv, dvec = c["out"], c["lse"], c["dqkv"], c["dvec"]
    for name in ("out", "lse", "dqkv", "dvec"):
        assert bool(torch.isfinite(c[name].t.float()).all()), name + ": not finite (a read behind the line's last row)"
        assert c[name].intact(), name + ": guard rows changed (a store behind the line's last row)"
    err = rel_err(out.t, c["ref"])
    lerr = float((lse.t.cpu().double().reshape(n, h, s) - c["lse_ref"]).abs().max())
    print(f"\n{tag} n={n} S={s} h={h}: out rel {err:.3e}  lse abs {lerr:.3e}", end="")
    assert err < 2 ** -7
    assert lerr < 2e-3
    want_d = (out.t.float() * c["dout"].t.float()).reshape(n * s, h, hd).sum(-1)
    assert float((dvec.t - want_d).abs().max()) <= 1e-3 * max(1.0, float(want_d.abs().max()))
    for name, sl in (("dq", slice(0, d)), ("dk", slice(d, 2 * d)), ("dv", slice(2 * d, 3 * d))):
        if s == 1 and name != "dv":
            # One key: P = 1 whatever q and k are, so dq = dk = 0 exactly and a relative error or a cosine against them does not exist.  The
            # kernels form dS = P (dP - D) / sqrt(hd) with dP = dO . v and D = dO . O, and O = v exactly here (P = 1, l = 1): two f32 sums of the
            # same hd products in different orders.  Each is within hd x 2^-24 of the sum of the products' magnitudes, so
            # |dq| <= 2 x hd x 2^-24 x max |k| x sum_d |dO_d v_d| / sqrt(hd), and the same with q for dk.
            assert float(c["gref"][:, sl].abs().max()) < 1e-12
            qkv_d, dout_d = c["qkv"].t.double().cpu(), c["dout"].t.double().cpu()
            unc = float((dout_d.abs() * qkv_d[:, 2 * d:].abs()).reshape(n * s, h, hd).sum(-1).max()) / math.sqrt(hd)
            other = float(qkv_d[:, d:2 * d].abs().max()) if name == "dq" else float(qkv_d[:, :d].abs().max())
            got = float(dqkv.t[:, sl].double().abs().max())
            print(f"  {name} abs {got:.3e} (uncancelled {unc * other:.3e})", end="")
            assert got <= 2 * hd * 2.0 ** -24 * unc * other, (name, got)
            continue
        e = rel_err(dqkv.t[:, sl], c["gref"][:, sl])
        a, b = dqkv.t[:, sl].double().cpu().flatten(), c["gref"][:, sl].flatten()
        cos = float(a @ b / (a.norm() * b.norm()))
        print(f"  {name} rel {e:.3e} cos {cos:.6f}", end="")
        assert e < 3e-2, (name, e)
        assert cos > 0.9995, (name, cos)
    # in_proj's bias gradient, accumulated into a pre-filled vector: the column sums of the stored dqkv (rows behind S add exact zeros)
    dbias = torch.full((3 * d,), 2.0, device="cuda")
    dqkv2, dvec2 = bwd(c["qkv"], out, c["dout"], lse, n, s, h, dbias=dbias, hd=hd)
    assert torch.equal(dqkv2.t, dqkv.t) and dqkv2.intact() and dvec2.intact()
    want = 2.0 + dqkv.t.float().sum(0)
    assert float((dbias - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("n,s,h", SHAPES)
def test_hd64_attention_matches_the_oracle_and_stays_inside_the_line(n, s, h):
    """Every line of every shape against the oracle (at most three lines: the first, a middle and the last one).  Measured on an MI355X over
    the shapes with S > 1: out rel 1.8e-3 ... 2.6e-3, lse abs <= 5.9e-6, dq rel 4.0e-3 ... 6.5e-3, dk rel 2.0e-3 ... 1.6e-2, dv rel 2.1e-3 ... 3.6e-3,
    cosines >= 0.99998; at S = 1 dq = dk = 0 exactly.  No bound had to move."""
    check_against_the_oracle(case(n, s, h), n, s, h, 64, "HD64")


@pytest.mark.parametrize("n,s,h", [(2, 4, 8), (2, 132, 4), (3, 260, 8)])
def test_hd64_handed_in_d_gives_the_bits_of_the_call_that_computed_it(n, s, h):
    """`out` null and the stored dvec handed in: the same two kernels run, the dQ kernel reads D where it otherwise writes it."""
    c = case(n, s, h)
    d = h * 64
    dvec = Guarded(n * s, h, torch.float32, data=c["dvec"].t)
    db = torch.zeros(3 * d, device="cuda")
    got, _ = bwd(c["qkv"], None, c["dout"], c["lse"], n, s, h, dvec=dvec, dbias=db)
    assert got.intact() and torch.equal(dvec.t, c["dvec"].t)   # (D is read, not rewritten)
    assert torch.equal(got.t, c["dqkv"].t)
    want = got.t.float().sum(0)
    assert float((db - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("n,s,h", [(2, 4, 8), (3, 260, 8)])
def test_hd64_second_call_gives_the_same_bits(n, s, h):
    """No atomics go into out, lse, dvec or dqkv: a second identical forward and backward gives the same bits (dbias, reduced by a few f32
    atomics per address, to the 1e-3 form)."""
    c = case(n, s, h)
    d = h * 64
    db1, db2 = torch.zeros(3 * d, device="cuda"), torch.zeros(3 * d, device="cuda")
    out, lse = fwd(c["qkv"], n, s, h)
    dqkv, dvec = bwd(c["qkv"], out, c["dout"], lse, n, s, h, dbias=db1)
    bwd(c["qkv"], c["out"], c["dout"], c["lse"], n, s, h, dbias=db2)
    assert torch.equal(out.t, c["out"].t) and torch.equal(lse.t, c["lse"].t)
    assert torch.equal(dqkv.t, c["dqkv"].t) and torch.equal(dvec.t, c["dvec"].t)
    assert float((db1 - db2).abs().max()) <= 1e-3 * max(1.0, float(db2.abs().max()))


def test_hd64_lines_are_independent():
    """S = 100, three lines: the call on all lines equals the calls on each line alone, bit for bit."""
    n, s, h = 3, 100, 2
    c = case(n, s, h)
    d = h * 64
    for i in range(n):
        rows = slice(i * s, (i + 1) * s)
        qkv = Guarded(s, 3 * d, torch.bfloat16, data=c["qkv"].t[rows])
        dout = Guarded(s, d, torch.bfloat16, data=c["dout"].t[rows])
        out, lse = fwd(qkv, 1, s, h)
        dqkv, dvec = bwd(qkv, out, dout, lse, 1, s, h)
        assert torch.equal(out.t, c["out"].t[rows]), i
        assert torch.equal(lse.t, c["lse"].t[i * h:(i + 1) * h]), i
        assert torch.equal(dqkv.t, c["dqkv"].t[rows]), i
        assert torch.equal(dvec.t, c["dvec"].t[rows]), i
        assert out.intact() and lse.intact() and dqkv.intact() and dvec.intact()


def test_head_dim_128_still_matches_its_oracle_through_the_same_entry_points():
    """The launchers' dispatch on head_dim has not broken the old path: one head_dim-128 call at (2, 132, 4)."""
    n, s, h = 2, 132, 4
    check_against_the_oracle(case(n, s, h, 128), n, s, h, 128, "HD128")


@pytest.mark.parametrize("n,s,h", [(256, 4, 8), (128, 132, 8)])
def test_hd64_several_heads_per_workgroup(n, s, h):
    """The smallest shapes at which the launcher lets a forward workgroup walk two heads of a line as one stream (>= 4 workgroups per CU on a
    256-CU device; asserted, not assumed): one tile per head, and two tiles with a ragged second one, so a head ends and the next begins in
    mid-stream.  Measured on an MI355X: out rel 2.6e-3 ... 3.3e-3, lse abs <= 2.4e-6.  The first, a middle and the last line against the f64 oracle, and bit for bit the call on that line alone, which takes one
    head per workgroup."""
    from pero_pretraining_amd import ops
    assert ops.attention_hd64_heads_per_block(n, s, h) >= 2
    assert ops.attention_hd64_heads_per_block(1, s, h) == 1
    d = h * 64
    qkv_c, dout_c = inputs(n, s, h, 64)
    qkv = Guarded(n * s, 3 * d, torch.bfloat16, data=qkv_c.cuda())
    dout = Guarded(n * s, d, torch.bfloat16, data=dout_c.cuda())
    out, lse = fwd(qkv, n, s, h)
    dqkv, dvec = bwd(qkv, out, dout, lse, n, s, h)
    torch.cuda.synchronize()
    for t in (out, lse, dqkv, dvec):
        assert bool(torch.isfinite(t.t.float()).all()) and t.intact()
    for i in (0, n // 2, n - 1):
        rows = slice(i * s, (i + 1) * s)
        ref = O.attention(qkv_c[rows].double(), 1, s, h)
        q, k, _ = qkv_c[rows].double().reshape(1, s, 3, h, 64).permute(2, 0, 3, 1, 4)
        lse_ref = torch.logsumexp((q @ k.transpose(-1, -2)) / 8.0, -1) / math.log(2.0)
        err = rel_err(out.t[rows], ref)
        lerr = float((lse.t[i * h:(i + 1) * h].cpu().double().reshape(1, h, s) - lse_ref).abs().max())
        print(f"\nHD64 several heads n={n} S={s} line {i}: out rel {err:.3e}  lse abs {lerr:.3e}", end="")
        assert err < 2 ** -7 and lerr < 2e-3
        q1 = Guarded(s, 3 * d, torch.bfloat16, data=qkv.t[rows])
        g1 = Guarded(s, d, torch.bfloat16, data=dout.t[rows])
        o1, l1 = fwd(q1, 1, s, h)
        dq1, dv1 = bwd(q1, o1, g1, l1, 1, s, h)
        assert torch.equal(o1.t, out.t[rows]) and torch.equal(l1.t, lse.t[i * h:(i + 1) * h]), i
        assert torch.equal(dq1.t, dqkv.t[rows]) and torch.equal(dv1.t, dvec.t[rows]), i
