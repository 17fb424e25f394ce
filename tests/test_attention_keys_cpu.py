"""CPU: the host side of attention with per-line key ranges - the yardstick of the GPU tests (tests/attention_keys_ref.py) against torch's
scaled_dot_product_attention, ops.key_ranges_from_masks on collated masks, the host-side argument checks of the new C entry points, and the
defaults: the option is off on both model classes and no constructor changed (tests/test_gpu_attention_keys*.py run the kernels)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import attention_keys_ref as KR


@pytest.mark.parametrize("n,s,h,hd,ranges", [(2, 4, 4, 16, [(0, 4), (1, 3)]), (3, 37, 2, 8, [(3, 30), (36, 37), (0, 37)]), (1, 1, 1, 4, [(0, 1)])])
def test_reference_attention_is_sdpa_with_a_key_mask(n, s, h, hd, ranges):
    g = torch.Generator().manual_seed(s)
    d = h * hd
    qkv = torch.randn(n * s, 3 * d, generator=g, dtype=torch.float64)
    q, k, v = KR.split_heads(qkv, n, s, h)
    keep = ~KR.key_padding_mask(ranges, s)
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=keep[:, None, None, :])
    got = KR.attention(qkv, ranges, n, s, h)
    assert float((got - want.permute(0, 2, 1, 3).reshape(n * s, d)).abs().max()) < 1e-12
    # the log-sum-exp over the same keys, by hand
    sc = (q @ k.transpose(-1, -2)) / hd ** 0.5
    for b, (k0, k1) in enumerate(ranges):
        want_l = torch.log2(torch.exp(sc[b, :, :, k0:k1]).sum(-1))
        assert float((KR.lse2(qkv, ranges, n, s, h)[b] - want_l).abs().max()) < 1e-12


def collated_masks(widths, seed=7, sub=8, pad=32):
    """The image masks BatchCreator makes for lines of these widths: random left paddings (in label positions), [lp, lp + ceil(w / 8))."""
    from pero_pretraining_amd.common.dataloader import BatchCreator
    rng = np.random.default_rng(seed)
    target = int(np.ceil(max(widths) / pad) * pad) + pad
    left = [int(rng.integers(0, target - w)) // sub for w in widths]
    return BatchCreator._host_masks(list(widths), left, None, None, [0] * len(widths), target // sub, sub)[0], left


def test_key_ranges_from_masks_on_collated_masks():
    from pero_pretraining_amd import ops
    widths = (480, 512, 400, 512)
    masks, left = collated_masks(widths)
    assert masks.shape == (4, 68) and len(set(left)) > 1
    want = np.array([[lp, lp + -(-w // 8)] for lp, w in zip(left, widths)], dtype=np.int32)
    got = ops.key_ranges_from_masks(masks, device="cpu")
    assert got.dtype == torch.int32 and got.shape == (4, 2) and got.is_contiguous()
    assert np.array_equal(got.numpy(), want)
    # a CPU tensor takes the host path as well; the device path's arithmetic (argmax of the mask and of its flip) agrees, for every mask dtype, and
    # treats the shift masks' value 2 as not valid
    assert torch.equal(ops.key_ranges_from_masks(torch.from_numpy(masks), device="cpu"), got)
    for dtype in (torch.uint8, torch.int32, torch.int64):
        assert torch.equal(ops._hull_argmax(torch.from_numpy(masks).to(dtype)), got)
    three = masks.copy()
    three[0, :left[0]] = 2
    assert torch.equal(ops._hull_argmax(torch.from_numpy(three)), got) and torch.equal(ops.key_ranges_from_masks(three, device="cpu"), got)
    assert torch.equal(ops.key_ranges_from_masks(masks.tolist(), device="cpu"), got)


def test_key_ranges_from_masks_rejects_empty_and_holed_lines_on_the_host():
    from pero_pretraining_amd import ops
    masks, _ = collated_masks((480, 512, 400, 512))
    empty = masks.copy()
    empty[2] = 0
    with pytest.raises(ValueError, match="line 2 has no valid position"):
        ops.key_ranges_from_masks(empty, device="cpu")
    holed = masks.copy()
    k0 = int(np.argmax(holed[1]))
    holed[1, k0 + 3] = 0
    with pytest.raises(ValueError, match="line 1 has a hole"):
        ops.key_ranges_from_masks(holed, device="cpu")
    with pytest.raises(ValueError):
        ops.key_ranges_from_masks(masks[0], device="cpu")   # not (N, S)


def test_backbone_rejects_bad_host_ranges_before_any_launch():
    from pero_pretraining_amd.models.transformers import VisionTransformerEncoder
    bb = VisionTransformerEncoder(model_dim=64, num_heads=1, num_blocks=1, feedforward_dim=64)
    for bad in ([[0, 4], [3, 3]], [[0, 4], [5, 2]], [[-1, 4], [0, 2]]):
        with pytest.raises(ValueError, match="k0 < k1"):
            bb._key_ranges(np.array(bad), 2, torch.device("cpu"))
    with pytest.raises(ValueError, match="shape"):
        bb._key_ranges(np.array([[0, 4]]), 2, torch.device("cpu"))
    kr = bb._key_ranges(np.array([[0, 4], [1, 2]]), 2, torch.device("cpu"))
    assert kr.dtype == torch.int32 and kr.tolist() == [[0, 4], [1, 2]]
    assert bb._key_ranges(None, 2, torch.device("cpu")) is None


def test_new_entry_points_check_their_arguments_on_the_host():
    """Null pointers, head_dim 32 and empty shapes are refused before any launch (non-null dummies where a pointer must pass the null check)."""
    from pero_pretraining_amd import _lib, ops
    L = _lib.lib()
    buf = (ctypes.c_uint16 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    B = ops.PERO_BF16
    fwd = lambda *a: L.pero_attention_fwd_keys(*a)     # noqa: E731
    bwd = lambda *a: L.pero_attention_bwd_keys(*a)     # noqa: E731
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert fwd(*args, 1, 4, 1, 128, B, None) < 0 and b"pero_attention_fwd_keys: null pointer" in L.pero_last_error()
    for i in (0, 1, 3, 4, 5, 6):   # qkv, key_ranges, dout, lse, dvec, dqkv; `out` (2), dbias and work may be null
        args = [p, p, p, p, p, p, p, None, None]
        args[i] = None
        assert bwd(*args, 1, 4, 1, 128, B, None) < 0 and b"pero_attention_bwd_keys: null pointer" in L.pero_last_error()
    assert bwd(p, p, p, p, p, p, p, p, None, 1, 4, 1, 128, B, None) < 0 and b"workspace" in L.pero_last_error()
    for hd in (32, 256):
        assert fwd(p, p, p, p, 1, 4, 1, hd, B, None) < 0
        assert b"pero_attention_fwd_keys" in L.pero_last_error() and b"64 or 128" in L.pero_last_error()
        assert bwd(p, p, p, p, p, p, p, None, None, 1, 4, 1, hd, B, None) < 0
        assert b"pero_attention_bwd_keys" in L.pero_last_error() and b"64 or 128" in L.pero_last_error()
    for hd in (64, 128):
        assert fwd(p, p, p, p, 1, 4, 1, hd, ops.PERO_F32, None) < 0            # f32
        assert fwd(p, p, p, p, 0, 4, 1, hd, B, None) < 0 and fwd(p, p, p, p, 1, 0, 1, hd, B, None) < 0
        assert bwd(p, p, p, p, p, p, p, None, None, 0, 4, 1, hd, B, None) < 0 and bwd(p, p, p, p, p, p, p, None, None, 1, 0, 1, hd, B, None) < 0
    sm = lambda *a: L.pero_softmax_fwd_keys(*a)        # noqa: E731
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert sm(*args, 4, 4, 4, 1.0, ops.PERO_F32, None) < 0 and b"pero_softmax_fwd_keys" in L.pero_last_error()
    assert sm(p, p, p, 0, 4, 4, 1.0, ops.PERO_F32, None) < 0 and sm(p, p, p, 4, 0, 4, 1.0, ops.PERO_F32, None) < 0
    assert sm(p, p, p, 4, 4, 0, 1.0, ops.PERO_F32, None) < 0


def test_ops_refuse_key_ranges_that_are_not_int32_device_tensors():
    from pero_pretraining_amd import ops
    qkv = torch.zeros((8, 3 * 128), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="int32 device tensor"):
        ops.attention_fwd_fused(qkv, 2, 4, 1, key_ranges=torch.tensor([[0, 4], [0, 4]], dtype=torch.int32))   # on the host


def test_the_option_is_off_by_default_and_no_constructor_changed():
    from pero_pretraining_amd.joint_embedding_pretraining.model import JointEmbeddingTransformerEncoder
    from pero_pretraining_amd.masked_pretraining.model import MaskedTransformerEncoder
    from pero_pretraining_amd.models.transformers import TransformerEncoder, VisionTransformerEncoder
    assert MaskedTransformerEncoder.attend_valid_only is False and JointEmbeddingTransformerEncoder.attend_valid_only is False
    sig = lambda c: str(inspect.signature(c.__init__))   # noqa: E731
    assert sig(MaskedTransformerEncoder) == "(self, backbone, head, loss=None)"
    assert sig(JointEmbeddingTransformerEncoder) == "(self, backbone, head, loss)"
    assert sig(TransformerEncoder) == ("(self, height=40, patch_size=(40, 8), in_channels=3, model_dim=512, num_heads=4, num_blocks=6, "
                                       "feedforward_dim=2048, dropout=0.0, max_len=4096, *args, **kwargs)")
    assert sig(VisionTransformerEncoder) == ("(self, height=40, patch_size=(40, 8), in_channels=3, model_dim=512, num_heads=4, num_blocks=6, "
                                             "feedforward_dim=2048, dropout=0.0, *args, **kwargs)")
    # the new arguments are optional and last
    for fn, names in ((TransformerEncoder.forward, ["self", "x", "mask", "key_ranges"]), (TransformerEncoder.encode_tokens, ["self", "x", "mask", "key_ranges"]),
                      (TransformerEncoder.encode_tokens_views, ["self", "views", "key_ranges"]),
                      (MaskedTransformerEncoder.forward, ["self", "x", "labels", "mask", "rows", "key_ranges"]),
                      (MaskedTransformerEncoder.encode, ["self", "images", "mask", "key_ranges"])):
        ps = inspect.signature(fn).parameters
        assert list(ps) == names and ps["key_ranges"].default is None
