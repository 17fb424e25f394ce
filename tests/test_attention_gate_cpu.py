"""CPU: the gate that sends a layer's attention to the fused HIP kernels (ops.attention_fused_ok) takes every line length - the kernels
handle a ragged last tile - and still refuses f32 and head dims other than 128 (tests/test_gpu_attention_ragged.py runs the kernels)."""
import pytest
import torch


@pytest.mark.parametrize("s", [4, 100, 260])
def test_attention_fused_ok_takes_any_line_length(s):
    from pero_pretraining_amd import ops
    n, h, d = 2, 4, 512
    assert ops.attention_fused_ok(torch.zeros((n * s, 3 * d), dtype=torch.bfloat16), s, h)
    assert ops.attention_fused_ok(torch.zeros((n * s, 3 * 128), dtype=torch.bfloat16), s, 1)
    assert not ops.attention_fused_ok(torch.zeros((n * s, 3 * d), dtype=torch.float32), s, h)      # f32 parity mode
    assert not ops.attention_fused_ok(torch.zeros((n * s, 3 * d), dtype=torch.bfloat16), s, 8)     # head_dim 64
    assert not ops.attention_fused_ok(torch.zeros((n * s, 3 * 256), dtype=torch.bfloat16), s, 1)   # head_dim 256
