"""Fused attention at line lengths that are no multiple of the 128-row tile (the data loader pads a batch to S = W / 8 = a multiple of 4:
S = 260 for a widest line of 2048 px), forward and backward, against the oracle's attention in f64 on the same bf16 inputs.

Every tensor a kernel touches is a view into a larger allocation whose rows behind the view are guards: NaN behind the inputs, a bit pattern
(itself a NaN) behind the outputs, enough of them that a tile read or written without its row clamp would still land inside the allocation.
An unclamped read of the last line's tail then shows as a non-finite output, an unguarded store as a changed guard.  Tolerances are those of
tests/test_gpu_ops.py::test_fused_attention_fwd_bwd.  The layer-level case runs one step of the 2-layer bf16 model at 2 lines of 40 x 2080
(S = 260) with the fused kernels and with the batched-GEMM path, each against the f32 parity mode; measured on an MI355X: see the test's
docstring."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pero_oracle as O  # noqa: E402

HD = 128
GUARD_ROWS = 128            # a whole tile: nothing runs out of bounds even without a clamp
PAT16, PAT32 = 0x7FC5, 0x7FC12345   # bf16 / f32 NaN patterns
SHAPES = [(1, 1, 1), (2, 4, 4), (3, 100, 4), (2, 132, 4), (1, 191, 1), (2, 200, 2), (3, 260, 4), (1, 388, 1)]


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


def inputs(n, s, h):
    """The recipe of test_fused_attention_fwd_bwd: randn * 0.7, a spiked query row, a spiked key row inside the line, and a spiked key in the
    last partial tile where the line has more than one tile."""
    d = h * HD
    g = torch.Generator().manual_seed(n * 1000 + s + h)
    qkv = (torch.randn(n * s, 3 * d, generator=g) * 0.7).bfloat16()
    qkv[min(5, n * s - 1), :d] *= 6.0
    qkv[min(s // 2 + 3, s - 1), d:2 * d] *= 6.0
    nb = (s + 127) // 128
    if nb > 1 and s % 128:
        qkv[128 * (nb - 1) + (s - 128 * (nb - 1)) // 2, d:2 * d] *= 6.0
    dout = torch.randn(n * s, d, generator=g).bfloat16()
    return qkv, dout


def fwd(qkv, n, s, h):
    from pero_pretraining_amd import ops
    d = h * HD
    out = Guarded(n * s, d, torch.bfloat16)
    lse = Guarded(n * h, s, torch.float32, guard_rows=128 // s + 2)
    ops.call("pero_attention_fwd", qkv.t.data_ptr(), out.t.data_ptr(), lse.t.data_ptr(), n, s, h, HD, ops.PERO_BF16, ops.stream())
    return out, lse


def bwd(qkv, out, dout, lse, n, s, h, dvec=None, dbias=None):
    """out given: D is computed and stored (two launches); dvec given: D handed in (the paired launch unless attn_bwd_pair is 0)."""
    from pero_pretraining_amd import ops
    d = h * HD
    dqkv = Guarded(n * s, 3 * d, torch.bfloat16)
    if dvec is None:
        dvec = Guarded(n * s, h, torch.float32)
    work = torch.empty(3 * n * h * ((s + 127) // 128) * 128, device="cuda") if dbias is not None else None
    ops.call("pero_attention_bwd", qkv.t.data_ptr(), None if out is None else out.t.data_ptr(), dout.t.data_ptr(), lse.t.data_ptr(), dvec.t.data_ptr(),
             dqkv.t.data_ptr(), ops.ptr(dbias), ops.ptr(work), n, s, h, HD, ops.PERO_BF16, ops.stream())
    return dqkv, dvec


@functools.lru_cache(maxsize=None)
def case(n, s, h):
    """Inputs, the f64 reference and the kernels' results of one shape, computed once and shared (read-only) by the tests."""
    d = h * HD
    qkv_c, dout_c = inputs(n, s, h)
    ref_in = qkv_c.double().requires_grad_(True)
    ref = O.attention(ref_in, n, s, h)
    ref.backward(dout_c.double())
    q, k, _ = qkv_c.double().reshape(n, s, 3, h, HD).permute(2, 0, 3, 1, 4)
    lse_ref = torch.logsumexp((q @ k.transpose(-1, -2)) / math.sqrt(HD), -1) / math.log(2.0)
    qkv = Guarded(n * s, 3 * d, torch.bfloat16, data=qkv_c.cuda())
    dout = Guarded(n * s, d, torch.bfloat16, data=dout_c.cuda())
    out, lse = fwd(qkv, n, s, h)
    dqkv, dvec = bwd(qkv, out, dout, lse, n, s, h)
    torch.cuda.synchronize()
    return dict(qkv=qkv, dout=dout, out=out, lse=lse, dqkv=dqkv, dvec=dvec, ref=ref.detach(), gref=ref_in.grad, lse_ref=lse_ref)


@pytest.mark.parametrize("n,s,h", SHAPES)
def test_ragged_attention_matches_the_oracle_and_stays_inside_the_line(n, s, h):
    c = case(n, s, h)
    d = h * HD
    out, lse, dqkv, dvec = c["out"], c["lse"], c["dqkv"], c["dvec"]
    for name in ("out", "lse", "dqkv", "dvec"):
        assert bool(torch.isfinite(c[name].t.float()).all()), name + ": not finite (a read behind the line's last row)"
        assert c[name].intact(), name + ": guard rows changed (a store behind the line's last row)"
    err = rel_err(out.t, c["ref"])
    lerr = float((lse.t.cpu().double().reshape(n, h, s) - c["lse_ref"]).abs().max())
    print(f"\nRAGGED n={n} S={s} h={h}: out rel {err:.3e}  lse abs {lerr:.3e}", end="")
    assert err < 2 ** -7
    assert lerr < 2e-3
    want_d = (out.t.float() * c["dout"].t.float()).reshape(n * s, h, HD).sum(-1)
    assert float((dvec.t - want_d).abs().max()) <= 1e-3 * max(1.0, float(want_d.abs().max()))
    for name, sl in (("dq", slice(0, d)), ("dk", slice(d, 2 * d)), ("dv", slice(2 * d, 3 * d))):
        if s == 1 and name != "dv":
            # One key: P = 1 whatever q and k are, so dq = dk = 0 exactly and a relative error or a cosine against them does not exist.  The
            # kernels form dS = P (dP - D) / sqrt(hd) with dP = dO . v and D = dO . O, and O = v exactly here (P = 1, l = 1): two f32 sums of the
            # same 128 products in different orders.  Each is within 128 x 2^-24 of the sum of the products' magnitudes, so
            # |dq| <= 2 x 128 x 2^-24 x max |k| x sum_d |dO_d v_d| / sqrt(hd) (1.5e-5 of what cancels), and the same with q for dk.
            assert float(c["gref"][:, sl].abs().max()) < 1e-12
            qkv_d, dout_d = c["qkv"].t.double().cpu(), c["dout"].t.double().cpu()
            unc = float((dout_d.abs() * qkv_d[:, 2 * d:].abs()).reshape(n * s, h, HD).sum(-1).max()) / math.sqrt(HD)
            other = float(qkv_d[:, d:2 * d].abs().max()) if name == "dq" else float(qkv_d[:, :d].abs().max())
            got = float(dqkv.t[:, sl].double().abs().max())
            print(f"  {name} abs {got:.3e} (uncancelled {unc * other:.3e})", end="")
            assert got <= 2 * 128 * 2.0 ** -24 * unc * other, (name, got)
            continue
        e = rel_err(dqkv.t[:, sl], c["gref"][:, sl])
        a, b = dqkv.t[:, sl].double().cpu().flatten(), c["gref"][:, sl].flatten()
        cos = float(a @ b / (a.norm() * b.norm()))
        print(f"  {name} rel {e:.3e} cos {cos:.6f}", end="")
        assert e < 3e-2, (name, e)
        assert cos > 0.9995, (name, cos)
    # in_proj's bias gradient, accumulated into a pre-filled vector: the column sums of the stored dqkv (rows behind S add exact zeros)
    dbias = torch.full((3 * d,), 2.0, device="cuda")
    dqkv2, dvec2 = bwd(c["qkv"], out, c["dout"], lse, n, s, h, dbias=dbias)
    assert torch.equal(dqkv2.t, dqkv.t) and dqkv2.intact() and dvec2.intact()
    want = 2.0 + dqkv.t.float().sum(0)
    assert float((dbias - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("n,s,h", [(2, 4, 4), (2, 132, 4), (3, 260, 4)])
def test_ragged_paired_launch_equals_the_two_launch_form(n, s, h):
    """D handed in: both backward kernels as one launch (8 units: the XCD block map and the chunked dispatch order; 12: the plain map) and as
    two (attn_bwd_pair 0) give the same dqkv bit for bit, and the dqkv of the call that computed D itself."""
    from pero_pretraining_amd._lib import call
    c = case(n, s, h)
    d = h * HD
    dvec = Guarded(n * s, h, torch.float32, data=c["dvec"].t)
    db_pair, db_two = torch.zeros(3 * d, device="cuda"), torch.zeros(3 * d, device="cuda")
    pair, _ = bwd(c["qkv"], None, c["dout"], c["lse"], n, s, h, dvec=dvec, dbias=db_pair)
    call("pero_set_option", b"attn_bwd_pair", 0)
    try:
        two, _ = bwd(c["qkv"], None, c["dout"], c["lse"], n, s, h, dvec=dvec, dbias=db_two)
    finally:
        call("pero_set_option", b"attn_bwd_pair", 1)
    assert pair.intact() and two.intact()
    assert bool(torch.isfinite(pair.t.float()).all())
    assert torch.equal(pair.t, two.t)
    assert torch.equal(pair.t, c["dqkv"].t)
    assert float((db_pair - db_two).abs().max()) <= 1e-3 * max(1.0, float(db_two.abs().max()))
    want = pair.t.float().sum(0)
    assert float((db_pair - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))


def test_ragged_lines_are_independent():
    """S = 100, three lines (one head per workgroup at this size): the call on all lines equals the calls on each line alone, bit for bit."""
    n, s, h = 3, 100, 4
    c = case(n, s, h)
    d = h * HD
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


def test_layer_step_at_the_real_width_fused_against_unfused(monkeypatch):
    """One forward and backward of the 2-layer bf16 model of tests/test_gpu_bf16_trajectory.py on 2 lines of 40 x 2080 (S = 260): loss and the
    concatenated parameter gradient against the same step in f32 parity mode, with the fused attention kernels (as built) and with
    functional.FUSED_ATTENTION = False (batched GEMM + softmax, what this shape ran before).  Both are bf16 roundings of the same quantities in
    a different order: the fused step's relative errors must be at most 1.5 x the unfused step's.  Measured on an MI355X: loss 1.5e-5 fused,
    5.2e-5 unfused; gradient 1.50e-2 fused, 1.48e-2 unfused."""
    from pero_pretraining_amd import functional as F
    from pero_pretraining_amd import ops
    from pero_pretraining_amd.masked_pretraining import model as M
    from pero_pretraining_amd.masked_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.masked_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    from test_gpu_bf16_trajectory import BB, HD as HEAD
    n, s, h = 2, 260, BB["num_heads"]
    assert ops.attention_fused_ok(torch.empty((n * s, 3 * BB["model_dim"]), dtype=torch.bfloat16), s, h)
    rng = np.random.default_rng(2080)
    images = torch.from_numpy(rng.integers(0, 256, (n, 40, 8 * s, 3), dtype=np.uint8)).cuda()
    labels = torch.from_numpy(rng.integers(0, 4096, (n, s)).astype(np.int64)).cuda()
    mask = (rng.random((n, s)) < 0.15).astype(int)
    fused_calls = []
    real_fwd = ops.attention_fwd_fused
    monkeypatch.setattr(ops, "attention_fwd_fused", lambda *a, **k: (fused_calls.append(1), real_fwd(*a, **k))[1])

    def step(bf16):
        torch.manual_seed(0)
        model = M.MaskedTransformerEncoder(M.init_backbone(dict(BB)), M.init_head(dict(HEAD))).cuda().train()
        model.backbone.set_offsets(np.array([11, 500]))   # the positional shifts of the two lines, the same in every step
        trainer = Trainer(BatchOperator(torch.device("cuda", 0), 0.15), model, None, FusedAdam(model.parameters(), lr=1e-3), None, bfloat16=bf16)
        loss = float(trainer._forward_backward(images, labels, mask))
        torch.cuda.synchronize()
        return loss, torch.cat([p.grad.double().flatten() for p in model.parameters() if p.grad is not None]).cpu()

    loss32, grad32 = step(False)
    assert not fused_calls                      # f32 parity mode: batched GEMM + softmax
    loss_f, grad_f = step(True)
    assert len(fused_calls) == BB["num_blocks"]  # the fused kernels ran in every layer
    monkeypatch.setattr(F, "FUSED_ATTENTION", False)
    loss_u, grad_u = step(True)
    assert len(fused_calls) == BB["num_blocks"]
    assert grad_f.shape == grad32.shape == grad_u.shape and math.isfinite(loss_f) and bool(torch.isfinite(grad_f).all())
    gn = float(grad32.norm())
    e_loss_f, e_loss_u = abs(loss_f - loss32) / abs(loss32), abs(loss_u - loss32) / abs(loss32)
    e_grad_f, e_grad_u = float((grad_f - grad32).norm()) / gn, float((grad_u - grad32).norm()) / gn
    print(f"\nLAYER S=260: loss rel err fused {e_loss_f:.3e} unfused {e_loss_u:.3e}; gradient rel err fused {e_grad_f:.3e} unfused {e_grad_u:.3e}")
    assert e_grad_f <= 1.5 * e_grad_u, (e_grad_f, e_grad_u)
    assert e_loss_f <= 1.5 * e_loss_u, (e_loss_f, e_loss_u)
