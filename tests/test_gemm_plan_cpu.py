"""pero_gemm's kernel choice, seen through pero_gemm_plan (csrc/gemm.hip: gemm_plan): the family that takes a product, the k-slices it runs with and the
extra pass over C where the family has no fused side output.  The plan is pure host arithmetic - no launch, no GPU, the operands are made-up addresses
(4096: aligned, 4104: misaligned) - so these tests pin the dispatch table on any machine; tests/test_gpu_gemm_plan.py checks on a GPU that the launch
follows the plan.  Unless a case says otherwise: bf16 in, bf16 out, batch 1, leading dimensions equal to the row length, policy 0."""
import contextlib

import pytest

from pero_pretraining_amd import _lib, ops
from pero_pretraining_amd._lib import (GEMM_ATOMIC, GEMM_COLSUM, GEMM_FORCE_GENERIC, GEMM_MASK_TILED, GEMM_RELU, GEMM_RELU_BITS, GEMM_ROWDOT, GEMM_TILE128,
                                       GEMM_TILE256, GEMM_TRANS_A, GEMM_TRANS_B, PERO_BF16, PERO_F32, PeroHipError)

OK, ODD = 4096, 4104
DEFAULTS = {"gemm_policy": 0, "gemm_e_splitk_min": 4, "gemm_nw": 0}


@contextlib.contextmanager
def option(name, value):
    _lib.call("pero_set_option", name.encode(), value)
    try:
        yield
    finally:
        _lib.call("pero_set_option", name.encode(), DEFAULTS[name])


def plan(M, N, K, flags=0, *, batch=1, A=OK, B=OK, C=OK, f32_in=False, f32_out=False, bias=None, residual=None, gate=None, ldg=None, alpha=1.0, k_split=1):
    """ops.gemm_plan of the product with dense operands; gate: rows of N elements (the bit mask: N / 8 bytes) unless ldg is given."""
    lda = M if flags & GEMM_TRANS_A else K
    ldb = N if flags & GEMM_TRANS_B else K
    if ldg is None:
        ldg = 0 if gate is None else N // 8 if flags & GEMM_RELU_BITS else N
    return ops.gemm_plan(A, B, C, M, N, K, lda, ldb, N, bias=bias, residual=residual, gate=gate, ldr=N if residual is not None else 0, ldg=ldg,
                         batch=batch, sA=(M * K, 0), sB=(N * K, 0), sC=(M * N, 0), alpha=alpha, flags=flags, k_split=k_split,
                         in_dtype=PERO_F32 if f32_in else PERO_BF16, out_dtype=PERO_F32 if f32_out else PERO_BF16)


def family(*a, **kw):
    return plan(*a, **kw)[0]


def test_products_outside_the_tile_kernels_take_the_generic_kernel():
    assert plan(128, 128, 64, f32_in=True, f32_out=True) == ("generic", 1, None)      # 1: f32 operands
    assert family(100, 128, 64) == "generic"                                          # 2: ragged M
    assert family(256, 256, 128, GEMM_FORCE_GENERIC) == "generic"                     # 3
    assert family(256, 256, 128, A=ODD) == "generic"                                  # 4: misaligned A
    assert plan(256, 256, 128, GEMM_COLSUM, A=ODD, bias=OK) == ("generic", 1, "colsum")


def test_stored_products_under_the_automatic_policy():
    assert plan(128, 128, 64) == ("t128", 1, None)                                    # 5: M is no multiple of 256
    assert plan(256, 128, 64) == ("r256", 1, None)                                    # 6
    assert family(256, 128, 64, batch=4) == "r256"                                    # 7
    assert family(128, 128, 64, batch=4) == "t128"                                    # 8
    assert family(256, 256, 128) == "r256"                                            # 9: one 256x256 tile < gemm_e256_min
    assert plan(256, 256, 128, GEMM_TILE256) == ("e256", 1, None)                     # 10
    assert family(49152, 256, 128) == "e256"                                          # 13: 192 tiles
    assert family(48896, 256, 128) == "r256"                                          # 14: 191 tiles
    assert plan(256, 256, 128, GEMM_ROWDOT, bias=OK, gate=OK) == ("r256", 1, None)    # 21: r256 fuses the row dots
    assert family(256, 256, 128, GEMM_TILE128) == "t128"


def test_policy_20_takes_the_eight_phase_kernel_only_for_what_its_epilogues_cover():
    with option("gemm_policy", 20):
        assert family(256, 256, 128) == "e256"                                                        # 11
        assert family(256, 256, 64) == "r256"                                                         # 12: K < 128
        assert family(256, 256, 128, gate=OK) == "r256"                                               # 15: bf16 gate rows
        assert family(256, 256, 128, GEMM_RELU_BITS, gate=OK, bias=OK) == "r256"                      # 16: gate-in with an input bias
        assert plan(256, 256, 128, GEMM_RELU_BITS | GEMM_COLSUM, gate=OK, bias=OK) == ("e256", 1, None)   # (the same with column sums: fused)
        assert family(256, 256, 128, GEMM_RELU_BITS, gate=OK) == "e256"
        assert family(256, 256, 128, GEMM_RELU_BITS | GEMM_RELU, gate=OK, bias=OK) == "e256"
        assert family(256, 256, 128, GEMM_TRANS_A | GEMM_RELU) == "r256"                              # 17
        assert family(256, 256, 128, GEMM_TRANS_A) == "e256"
        assert family(256, 256, 128, alpha=0.5) == "r256"                                             # 18
        assert family(256, 256, 128, f32_out=True) == "r256"                                          # 19
        assert plan(256, 256, 128, GEMM_ROWDOT, bias=OK, gate=OK) == ("e256", 1, None)                # 20
        assert family(256, 256, 128, residual=OK) == "e256"
        assert family(256, 256, 128, GEMM_RELU, residual=OK) == "r256"
        assert family(256, 256, 128, GEMM_COLSUM, bias=OK) == "r256"                                  # column sums without the bit mask


def test_policies_1_4_and_7_force_their_family():
    with option("gemm_policy", 1):
        assert plan(256, 256, 128, GEMM_ROWDOT, bias=OK, gate=OK) == ("t128", 1, "rowdot")            # 22
        for kw in (dict(), dict(flags=GEMM_TILE256), dict(batch=4), dict(flags=GEMM_RELU, bias=OK), dict(flags=GEMM_TRANS_A | GEMM_TRANS_B),
                   dict(flags=GEMM_ATOMIC, f32_out=True, k_split=0), dict(flags=GEMM_ATOMIC, f32_out=True, k_split=2)):
            assert family(512, 512, 32768, **kw) == "t128", kw                                        # 25
    with option("gemm_policy", 4):
        assert plan(256, 256, 128, GEMM_COLSUM, bias=OK) == ("t128", 1, "colsum")                     # 23
        assert plan(256, 256, 128) == ("o128", 1, None)                                               # 24
    with option("gemm_policy", 7):
        assert family(256, 256, 128) == "r256"
        assert family(512, 512, 32768, GEMM_ATOMIC, f32_out=True, k_split=0) == "t128"                # 30


SPLITK_CASES = [  # (M, N, K, k_split, gemm_e_splitk_min) -> plan
    ((512, 512, 32768, 0, 4), ("e256_splitk", 64, None)),   # 26: four tiles, one round of 256 workgroups
    ((512, 512, 32704, 0, 4), ("o128", 32, None)),          # 27: reduction < 32768
    ((256, 256, 65536, 0, 4), ("o128", 128, None)),         # 28: one 256x256 tile < gemm_e_splitk_min
    ((256, 256, 65536, 0, 1), ("e256_splitk", 256, None)),  # 29
    ((512, 512, 32768, 8, 4), ("e256_splitk", 8, None)),
    ((512, 512, 32704, 7, 4), ("o128", 7, None)),           # 511 K-steps in chunks of 73
    ((512, 512, 512, 6, 4), ("o128", 4, None)),             # 8 K-steps in chunks of 2: four slices, not six
    ((4096, 4096, 32768, 0, 4), ("e256_splitk", 1, None)),  # 256 tiles fill the round: one slice, no workspace
    ((128, 128, 32768, 0, 4), ("o128", 64, None)),
]


@pytest.mark.parametrize("case,expected", SPLITK_CASES)
def test_split_k_products_and_their_workspace(case, expected):
    """... and pero_gemm_workspace_bytes is non-zero exactly where the plan says e256 split-K with more than one slice (a 256 x 256 f32 tile per work item)."""
    M, N, K, k_split, smin = case
    with option("gemm_e_splitk_min", smin):
        got = plan(M, N, K, GEMM_ATOMIC, f32_out=True, k_split=k_split)
        ws = _lib.lib().pero_gemm_workspace_bytes(M, N, K, 1, GEMM_ATOMIC, k_split, PERO_BF16, PERO_F32)
    assert got == expected
    if got[0] == "e256_splitk" and got[1] > 1:
        assert ws == (M // 256) * (N // 256) * got[1] * 256 * 256 * 4
    else:
        assert ws == 0


def test_forced_small_tile_and_workspace_of_other_products():
    assert family(512, 512, 32768, GEMM_ATOMIC | GEMM_TILE128, f32_out=True, k_split=0) == "t128"     # 31
    h = _lib.lib()
    assert h.pero_gemm_workspace_bytes(512, 512, 32768, 1, GEMM_ATOMIC | GEMM_TILE128, 0, PERO_BF16, PERO_F32) == 0
    assert h.pero_gemm_workspace_bytes(512, 512, 32768, 1, 0, 1, PERO_BF16, PERO_BF16) == 0            # a stored product
    assert h.pero_gemm_workspace_bytes(512, 512, 32768, 2, GEMM_ATOMIC, 0, PERO_BF16, PERO_F32) == 0   # batched
    assert h.pero_gemm_workspace_bytes(512, 512, 32768, 1, GEMM_ATOMIC, 0, PERO_F32, PERO_F32) == 0    # f32 operands


def test_row_complete_tile_is_opt_in_and_plain_or_residual_only():
    assert family(128, 512, 192) == "t128"
    with option("gemm_nw", 1):
        assert plan(128, 512, 192) == ("n512", 1, None)                                               # 32
        assert family(128, 512, 192, bias=OK, residual=OK) == "n512"
        assert family(128, 512, 128) == "t128"                                                        # 33: K < 192
        assert family(128, 512, 192, GEMM_RELU) == "t128"
        assert family(256, 512, 192, GEMM_RELU) == "r256"
        assert family(128, 512, 192, GEMM_TRANS_B) == "t128"


def test_refusals_are_pero_gemms_refusals():
    def refused(match, *a, **kw):
        with pytest.raises(PeroHipError, match=match):
            plan(*a, **kw)
    with option("gemm_policy", 1):
        refused("PERO_GEMM_RELU_BITS", 256, 256, 128, GEMM_RELU_BITS, gate=OK)                        # 34
    refused("PERO_GEMM_RELU_BITS", 128, 256, 128, GEMM_RELU_BITS, gate=OK)                            # 35
    refused("PERO_GEMM_RELU_BITS", 256, 256, 128, GEMM_RELU_BITS, gate=OK, B=ODD)                     # 36
    refused("PERO_GEMM_MASK_TILED", 256, 256, 128, GEMM_MASK_TILED)                                   # 37
    refused("k_split", 256, 256, 128, k_split=2)                                                      # 38
    refused("null operand", 256, 256, 128, A=None)
    refused("ATOMIC/ACCUM need f32 C", 256, 256, 128, GEMM_ATOMIC)
    refused("PERO_GEMM_COLSUM", 256, 256, 128, GEMM_COLSUM)
    # the null outputs are allowed, and a refusal is a negative status with the text in pero_last_error()
    h = _lib.lib()
    args = (OK, OK, OK, None, None, None, 256, 256, 128, 128, 128, 256, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1.0, 0)
    assert h.pero_gemm_plan(*args, 1, PERO_BF16, PERO_BF16, None, 0, None, None, None) == 4   # PERO_GEMM_KERNEL_R256
    assert h.pero_gemm_plan(*args, 2, PERO_BF16, PERO_BF16, None, 0, None, None, None) == -1
    assert b"k_split" in h.pero_last_error()
