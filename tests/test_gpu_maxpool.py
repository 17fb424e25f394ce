"""GPU: pero_maxpool_nhwc and pero_image_to_halo (csrc/conv.hip) against tests/vgg_ref.py.  The bare maximum is exact (bit for bit, f32
and bf16); with the affine y = max * a[c] + b[c] the bound is parity_ref.assert_within(n_terms=2) against |max a| + |b|."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_ref as P  # noqa: E402
import vgg_ref as V  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
POOLS = [(2, 2), (2, 1), (1, 2), (1, 1)]
SHAPES = [(2, 40, 72, 16), (1, 10, 24, 96), (2, 6, 10, 12)]      # the last: C % 8 != 0, the element-by-element path


def ops():
    from pero_pretraining_amd import ops as O
    return O


@functools.lru_cache(maxsize=None)
def case(shape, bf16):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(9)
    x = torch.randn((n, c, h, w), generator=g)
    a = 0.5 + torch.rand((c,), generator=g)
    a[::3] = -a[::3]                                  # negative scales: the affine cannot move in front of the maximum
    b = torch.randn((c,), generator=g)
    return (x.bfloat16().float() if bf16 else x), a, b


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("tokens", [False, True], ids=["halo", "token_rows"])
@pytest.mark.parametrize("affine", [False, True], ids=["max", "affine"])
@pytest.mark.parametrize("pool", POOLS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_maxpool(shape, pool, affine, tokens, mode):
    O = ops()
    dtype = DTYPES[mode]
    x, a, b = case(shape, mode == "bf16")
    ref, mag = V.maxpool(x.double(), pool, a.double() if affine else None, b.double() if affine else None)
    xh = V.to_halo(x, dtype).cuda()
    y = O.maxpool_nhwc(xh, pool, a.cuda() if affine else None, b.cuda() if affine else None, token_rows=tokens)
    y2 = O.maxpool_nhwc(xh, pool, a.cuda() if affine else None, b.cuda() if affine else None, token_rows=tokens)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and y.dtype == dtype
    n, c = shape[0], shape[3]
    if tokens:
        assert tuple(y.shape) == (n * (shape[2] // pool[1]), (shape[1] // pool[0]) * c)
        got = V.from_token_rows(y, n, c)
        assert torch.equal(V.token_rows(got), y.double().cpu())
    else:
        got, border = V.from_halo(y)
        assert tuple(y.shape) == (n, shape[1] // pool[0] + 2, shape[2] // pool[1] + 2, c)
        assert bool(torch.equal(border, torch.zeros_like(border))), "halo pixels of the output must be exact zeros"
    if affine:
        worst = P.assert_within(got, ref, mag, 2, dtype, what="maxpool affine")
        print(f"maxpool {shape} {pool} {mode}: worst error / bound {worst:.3f}")
    else:
        assert torch.equal(got, ref), "the maximum is exact"


@pytest.mark.parametrize("mode", list(DTYPES))
def test_image_ingestion(mode):
    O = ops()
    dtype = DTYPES[mode]
    rng = np.random.default_rng(2)
    u8 = torch.from_numpy(rng.integers(0, 256, (3, 40, 72, 3), dtype=np.uint8))
    u8.reshape(-1)[:256] = torch.arange(256, dtype=torch.uint8)          # every byte value occurs
    ref = V.ingest(u8)                                         # (N, C, H, W) f64 of the f32 quotients
    y = O.image_to_halo(u8.cuda(), dtype)
    got, border = V.from_halo(y)
    assert torch.equal(got, ref.float().to(dtype).double()) and not bool(border.any())
    nchw = (u8.double() / 255.0).float().permute(0, 3, 1, 2).contiguous()          # autoencoders/batch_operator.py:14-16
    y2 = O.image_to_halo(nchw.cuda(), dtype)
    assert torch.equal(y, y2)
    odd = torch.from_numpy(rng.standard_normal((2, 5, 7, 9)).astype(np.float32))   # C = 5, H = 7, W = 9
    got, border = V.from_halo(O.image_to_halo(odd.cuda(), dtype))
    assert torch.equal(got, odd.to(dtype).double()) and not bool(border.any())
    # zero channels behind C: 16 bytes per pixel (one store), and a width that is not
    for channels in (O.conv_channel_pad(3, dtype), 11):
        yp = O.image_to_halo(u8.cuda(), dtype, channels=channels)
        assert tuple(yp.shape) == (3, 42, 74, channels) and torch.equal(yp[..., :3], y) and not bool(yp[..., 3:].any())
        assert torch.equal(O.image_to_halo(nchw.cuda(), dtype, channels=channels), yp)


def test_bad_arguments():
    from pero_pretraining_amd import _lib
    O = ops()
    h = _lib.lib()
    x = torch.zeros((1, 6, 8, 8), device="cuda")
    y = torch.full((1, 4, 5, 8), 7.0, device="cuda")
    a = torch.ones(8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    invalid = _lib.DEFINES["PERO_E_INVALID"]
    assert h.pero_maxpool_nhwc(None, y.data_ptr(), None, None, 1, 4, 6, 8, 2, 2, 0, 0, s) == invalid
    assert h.pero_maxpool_nhwc(x.data_ptr(), y.data_ptr(), a.data_ptr(), None, 1, 4, 6, 8, 2, 2, 0, 0, s) == invalid
    assert h.pero_maxpool_nhwc(x.data_ptr(), y.data_ptr(), None, None, 1, 4, 6, 8, 3, 2, 0, 0, s) == invalid
    assert h.pero_maxpool_nhwc(x.data_ptr(), y.data_ptr(), None, None, 1, 5, 6, 8, 2, 2, 0, 0, s) == invalid
    assert h.pero_maxpool_nhwc(x.data_ptr(), y.data_ptr(), None, None, 1, 4, 6, 0, 2, 2, 0, 0, s) == invalid
    assert h.pero_image_to_halo(None, y.data_ptr(), 1, 2, 3, 8, 8, 0, 0, s) == invalid
    assert h.pero_image_to_halo(x.data_ptr(), y.data_ptr(), 1, 2, 3, 8, 8, 2, 0, s) == invalid
    assert h.pero_image_to_halo(x.data_ptr(), y.data_ptr(), 1, 2, 3, 8, 4, 0, 0, s) == invalid      # C_pad below C
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), "a refused call must not launch"
    with pytest.raises(ValueError, match="pool"):
        O.maxpool_nhwc(x, (3, 1))
    with pytest.raises(ValueError, match="divisible"):
        O.maxpool_nhwc(torch.zeros((1, 5, 8, 8), device="cuda"), (2, 2))
    with pytest.raises(ValueError, match="both"):
        O.maxpool_nhwc(x, (2, 2), a=a)
    with pytest.raises(ValueError, match="uint8"):
        O.image_to_halo(torch.zeros((1, 4, 4, 3), device="cuda", dtype=torch.float64), torch.float32)
