"""CPU: the SGPR hazard lint of tools/check_async_loads.py on the ISA of csrc/attention_hd64.hip (hipcc cross-compiles without a GPU), as
tests/test_cabi_and_host.py runs it on the other two attention files: no vector-memory instruction - the LDS-DMA loads among them - reads an
SGPR that a v_readlane_b32 / v_readfirstlane_b32 wrote fewer than five wait states earlier."""
import os
import shutil
import subprocess
import sys

import pytest


def test_head_dim_64_attention_kernels_pass_the_sgpr_lint(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "pero_pretraining_amd", "csrc", "attention_hd64.hip")
    asm = str(tmp_path / "attention_hd64.s")
    # the flags of csrc/Makefile
    c = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-Wno-unused-result", "-Wno-unused-value",
                        "-ffp-contract=off", "-S", "--cuda-device-only", src, "-o", asm], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-3000:]
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_async_loads.py"), asm, "attn", "--sgpr-only"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    for kernel in ("attn64_fwd_k", "attn64_bwd_dq_k", "attn64_bwd_dkv_k", "attn_bias_reduce_k"):   # the last one: attention_common.hpp's template at 64 columns
        assert kernel in r.stdout, kernel
