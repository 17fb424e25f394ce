"""GPU: pero_conv3x3 (csrc/conv.hip) against the f64 restatement of tests/vgg_ref.py, f32 and bf16 each.

Bound: parity_ref.assert_within with n_terms = 9 Cin + 1 against mag = |b| + sum |x| |w| (bf16: inputs and weights are rounded once on
the host, the reference is evaluated on the rounded values, and the one output rounding adds 2^-8 |ref|).  The integer cases are exact:
every product and partial sum is an integer below 2^24, so the f32 accumulation is exact in any order, and the result must equal the f64
reference rounded once to the output type, bit for bit.  Every case prints its worst error / bound ratio (parity_ref.RATIOS)."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_ref as P  # noqa: E402
import vgg_ref as V  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
INTEGER_SHAPES = [(1, 4, 8, 3, 16), (2, 6, 10, 16, 32)]
RANDOM_SHAPES = [(1, 8, 8, 3, 16), (3, 10, 24, 16, 32), (2, 40, 72, 64, 64), (2, 5, 40, 96, 48), (1, 20, 136, 128, 256)]
ACTIVATIONS = ["none", "relu", "leaky_relu"]


def ops():
    from pero_pretraining_amd import ops as O
    return O


@functools.lru_cache(maxsize=None)
def integer_case(shape):
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-4, 5, (n, cin, h, w), generator=g).float()
    wt = torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).float()
    wt[0, 0] = torch.tensor([[3., -2., 1.], [2., -3., 0.], [-1., 1., -2.]])      # asymmetric in (ky, kx) ...
    wt[1, 0], wt[0, cin - 1] = -wt[0, 0].t(), wt[0, 0].flip(0)                   # ... and in (co, ci)
    b = torch.randint(-5, 6, (cout,), generator=g).float()
    return x, wt, b, V.conv(x, wt, b)[0]


@functools.lru_cache(maxsize=None)
def random_case(shape, bf16):
    """(x, w, b) f32 (bf16-rounded values when bf16) and per activation the f64 (ref, mag).  Computed once and shared, never modified."""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn((n, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.rand((cout,), generator=g) - 0.5
    if bf16:
        x, wt = x.bfloat16().float(), wt.bfloat16().float()
    return x, wt, b, {a: V.conv(x, wt, b, a, 0.01) for a in ACTIVATIONS}


def run(x, wt, b, dtype, activation="none", slope=0.01):
    O = ops()
    xh = V.to_halo(x, dtype).cuda()
    y = O.conv3x3(xh, O.conv3x3_pack_weight(wt.cuda(), dtype), None if b is None else b.cuda(), activation=activation, slope=slope)
    torch.cuda.synchronize()
    return xh, y


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("shape", INTEGER_SHAPES, ids=str)
def test_exact_integers(shape, mode):
    x, wt, b, ref = integer_case(shape)
    _, y = run(x, wt, b, DTYPES[mode])
    assert y.dtype == DTYPES[mode] and tuple(y.shape) == (shape[0], shape[1] + 2, shape[2] + 2, shape[4])
    got, border = V.from_halo(y)
    want = ref.to(DTYPES[mode]).double()              # integers: exact in f32; one rounding to bf16
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} elements differ, first at {torch.nonzero(got != want)[0].tolist()}"
    assert not bool(border.any())


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("activation", ACTIVATIONS)
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=str)
def test_random_parity(shape, activation, mode):
    x, wt, b, refs = random_case(shape, mode == "bf16")
    ref, mag = refs[activation]
    _, y = run(x, wt, b, DTYPES[mode], activation)
    got, border = V.from_halo(y)
    worst = P.assert_within(got, ref, mag, 9 * shape[3] + 1, DTYPES[mode], what="conv3x3 " + activation)
    print(f"conv3x3 {shape} {activation} {mode}: worst error / bound {worst:.3f}")
    assert not bool(border.any()), "halo rows of the output must be exact zeros"
    assert bool(torch.equal(border, torch.zeros_like(border)))


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("shape", [(3, 10, 24, 16, 32), (2, 5, 40, 96, 48)], ids=str)
def test_line_isolation_and_rerun(shape, mode):
    """Line 0's output keeps its bits when the other lines are replaced by 1e4: the halo separates neighbours.  And a second run of the
    same call gives the same bits."""
    O = ops()
    x, wt, b, _ = random_case(shape, mode == "bf16")
    xh, y = run(x, wt, b, DTYPES[mode], "relu")
    y2 = O.conv3x3(xh, O.conv3x3_pack_weight(wt.cuda(), DTYPES[mode]), b.cuda(), activation="relu")
    assert torch.equal(y, y2)
    loud = x.clone()
    loud[1:] = 1.0e4
    _, y3 = run(loud, wt, b, DTYPES[mode], "relu")
    assert torch.equal(y3[0], y[0])
    assert not torch.equal(y3[1], y[1])


def test_bias_is_optional():
    x, wt, b, _ = random_case((1, 8, 8, 3, 16), False)
    ref, mag = V.conv(x, wt, None)
    got, _ = V.from_halo(run(x, wt, None, torch.float32)[1])
    P.assert_within(got, ref, mag, 27, torch.float32)


def test_bad_arguments_are_refused_without_a_launch():
    from pero_pretraining_amd import _lib
    O = ops()
    h = _lib.lib()
    x = torch.zeros((1, 6, 6, 8), device="cuda")
    w = torch.zeros((16, 3, 3, 8), device="cuda")
    y = torch.full((1, 6, 6, 16), 7.0, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def raw(xp, wp, yp, n=1, hh=4, ww=4, cin=8, cout=16, act=1, dtype=_lib.PERO_F32):
        return h.pero_conv3x3(xp, wp, None, yp, n, hh, ww, cin, cout, act, 0.01, dtype, s)

    invalid = _lib.DEFINES["PERO_E_INVALID"]
    assert raw(None, w.data_ptr(), y.data_ptr()) == invalid and b"null" in h.pero_last_error()
    assert raw(x.data_ptr(), None, y.data_ptr()) == invalid
    assert raw(x.data_ptr(), w.data_ptr(), None) == invalid
    assert raw(x.data_ptr(), w.data_ptr(), y.data_ptr(), cin=0) == invalid
    assert raw(x.data_ptr(), w.data_ptr(), y.data_ptr(), cout=0) == invalid
    assert raw(x.data_ptr(), w.data_ptr(), y.data_ptr(), hh=0) == invalid
    assert raw(x.data_ptr() + 4, w.data_ptr(), y.data_ptr()) == invalid and b"aligned" in h.pero_last_error()
    assert raw(x.data_ptr(), w.data_ptr(), y.data_ptr() + 8) == invalid
    assert raw(x.data_ptr(), w.data_ptr(), y.data_ptr(), act=3) == invalid
    assert raw(x.data_ptr(), w.data_ptr(), y.data_ptr(), dtype=5) == invalid
    assert raw(x.data_ptr(), w.data_ptr(), x.data_ptr()) == invalid
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), "a refused call must not launch"
    assert O.CONV_SLACK_ROWS == 0      # the header guards its loads: no slack rows to miss
    with pytest.raises(ValueError, match="halo"):
        O.conv3x3(x[0], w)
    with pytest.raises(ValueError, match="packed weight"):
        O.conv3x3(x, w.bfloat16())
    with pytest.raises(ValueError, match="activation"):
        O.conv3x3(x, w, activation="gelu")
    with pytest.raises(ValueError, match="bias"):
        O.conv3x3(x, w, torch.zeros(3, device="cuda"))
