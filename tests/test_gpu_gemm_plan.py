"""Plan and launch agree: for one product per kernel family, pero_gemm_plan names the family that tests/test_gemm_plan_cpu.py expects and the real
product of the same call - small integers in [-3, 3], every partial sum exact in f32 - equals the integer reference exactly (through the one
rounding of a bf16 output), whatever k-slices and work-item order the launch derives from the plan."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [  # id, M, N, K, option, flags, f32 C, k_split -> (family, k-slices)
    ("t128", 128, 128, 64, None, 0, False, 1, ("t128", 1)),
    ("r256", 256, 128, 64, None, 0, False, 1, ("r256", 1)),
    ("r256_one_256_tile", 256, 256, 128, None, 0, False, 1, ("r256", 1)),
    ("e256_flagged", 256, 256, 128, None, 128, False, 1, ("e256", 1)),              # PERO_GEMM_TILE256
    ("o128_policy4", 256, 256, 128, ("gemm_policy", 4, 0), 0, False, 1, ("o128", 1)),
    ("o128_splitk", 512, 512, 32704, None, 2, True, 0, ("o128", 32)),               # PERO_GEMM_ATOMIC, the library chooses the slices
    ("n512", 128, 512, 192, ("gemm_nw", 1, 0), 0, False, 1, ("n512", 1)),
]


@pytest.mark.parametrize("M,N,K,option,flags,f32_out,k_split,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_the_launch_follows_the_plan(M, N, K, option, flags, f32_out, k_split, expected):
    from pero_pretraining_amd import _lib, ops
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    b = torch.randint(-3, 4, (N, K), generator=g).float()
    ref = a @ b.t()                                     # |sum| <= 9 K < 2^24: exact in f32 in any order
    ad, bd = a.cuda().bfloat16(), b.cuda().bfloat16()
    c = torch.ones(M, N, device="cuda") if f32_out else torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    if option:
        _lib.call("pero_set_option", option[0].encode(), option[1])
    try:
        plan = ops.gemm_plan(ad, bd, c, M, N, K, K, K, N, flags=flags, k_split=k_split)
        ops.gemm_raw(ad, bd, c, M, N, K, K, K, N, flags=flags, k_split=k_split)
    finally:
        if option:
            _lib.call("pero_set_option", option[0].encode(), option[2])
    assert plan == expected + (None,)
    want = ref + 1 if f32_out else ref.bfloat16().float()   # the split-K product is ADDED to what C held
    assert torch.equal(c.float().cpu(), want)
