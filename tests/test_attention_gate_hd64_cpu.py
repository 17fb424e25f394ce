"""CPU: the gate that sends a layer's attention to the head_dim-64 fused kernels (ops.attention_fused_hd64_ok, csrc/attention_hd64.hip) takes
bf16 at head_dim 64 and every line length and refuses f32 and every other head width; ops.attention_fused_ok answers as before; the C entry
points refuse other head widths on the host, before any launch (tests/test_gpu_attention_hd64.py runs the kernels)."""
import ctypes

import pytest
import torch


@pytest.mark.parametrize("s", [4, 100, 260])
def test_attention_fused_hd64_ok_takes_head_dim_64_at_any_line_length(s):
    from pero_pretraining_amd import ops
    n = 2
    for d, h in ((512, 8), (256, 4)):
        qkv = torch.zeros((n * s, 3 * d), dtype=torch.bfloat16)
        assert ops.attention_fused_hd64_ok(qkv, s, h)
        assert not ops.attention_fused_ok(qkv, s, h)                                                    # the head_dim-128 gate still refuses it
        assert not ops.attention_fused_hd64_ok(torch.zeros((n * s, 3 * d), dtype=torch.float32), s, h)  # f32 parity mode
    bf = lambda d: torch.zeros((n * s, 3 * d), dtype=torch.bfloat16)   # noqa: E731
    assert not ops.attention_fused_hd64_ok(bf(512), s, 16)   # head_dim 32
    assert not ops.attention_fused_hd64_ok(bf(512), s, 4)    # head_dim 128
    assert not ops.attention_fused_hd64_ok(bf(512), s, 2)    # head_dim 256
    assert not ops.attention_fused_hd64_ok(bf(512), 0, 8)    # no rows
    assert not ops.attention_fused_hd64_ok(bf(192), s, 2)    # d % h != 0 is never head_dim 64 (96), and 200 / 3 is refused as well
    assert not ops.attention_fused_hd64_ok(bf(200), s, 3)
    assert ops.attention_fused_ok(bf(512), s, 4) and ops.attention_fused_ok(bf(128), s, 1)
    assert not ops.attention_fused_ok(bf(256), s, 1)


@pytest.mark.parametrize("hd", [32, 256])
def test_c_entry_points_refuse_other_head_widths_before_any_launch(hd):
    """Non-null dummy pointers: the check runs on the host, nothing is launched; the message names the accepted widths."""
    from pero_pretraining_amd import _lib, ops
    L = _lib.lib()
    buf = (ctypes.c_uint16 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert L.pero_attention_fwd(p, p, p, 1, 4, 1, hd, ops.PERO_BF16, None) < 0
    msg = L.pero_last_error()
    assert b"pero_attention_fwd" in msg and b"64 or 128" in msg, msg
    assert L.pero_attention_bwd(p, p, p, p, p, p, None, None, 1, 4, 1, hd, ops.PERO_BF16, None) < 0
    msg = L.pero_last_error()
    assert b"pero_attention_bwd" in msg and b"64 or 128" in msg, msg


def test_c_entry_points_still_refuse_f32_at_head_dim_64():
    from pero_pretraining_amd import _lib, ops
    L = _lib.lib()
    buf = (ctypes.c_uint16 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert L.pero_attention_fwd(p, p, p, 1, 4, 1, 64, ops.PERO_F32, None) < 0
    assert L.pero_attention_bwd(p, p, p, p, p, p, None, None, 1, 4, 1, 64, ops.PERO_F32, None) < 0
