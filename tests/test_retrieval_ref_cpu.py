"""tests/retrieval_ref.py against brute force, the conditions on the INPUTS of tests/test_gpu_retrieval.py that can be checked without a
GPU (the near-tie cap, where the planted copies fall), the host-side rules of pero_sim_topk (argument validation, the key-split choice)
and the host arithmetic of the retrieval metrics."""
import ctypes
import math

import numpy as np
import pytest
import torch

import retrieval_ref as R

DTYPES = [torch.float32, torch.bfloat16]


def lib():
    from pero_pretraining_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("M,N,D,k", [(3, 5, 8, 2), (4, 3, 8, 5), (6, 9, 16, 9), (2, 1, 8, 1)])
def test_reference_ranking_is_the_brute_force_loop(M, N, D, k):
    rng = np.random.default_rng(M + 10 * N)
    q, keys = rng.standard_normal((M, D)).astype(np.float32), rng.standard_normal((N, D)).astype(np.float32)
    if N > 2:
        keys[2] = keys[0]                                  # an exact tie for every query
    if N > 4:
        keys[4, 0] = np.nan
    qs, ks = R.inv_norm_f32(q), R.inv_norm_f32(np.nan_to_num(keys))
    valid = np.ones(N, dtype=np.uint8)
    if N > 3:
        valid[3] = 0
    skip = np.full(M, -1, dtype=np.int32)
    skip[0] = 1 % N
    ref = R.reference(q, keys, k, qs, ks, valid, skip)
    for m in range(M):
        cand = []
        for n in range(N):
            s = float(np.dot(q[m].astype(np.float64), keys[n].astype(np.float64))) * float(qs[m]) * float(ks[n])
            if valid[n] and n != skip[m] and not math.isnan(s):
                cand.append((-s, n))
        cand.sort()
        want_i = [n for _, n in cand[:k]] + [-1] * (k - len(cand[:k]))
        want_v = [-s for s, _ in cand[:k]] + [-math.inf] * (k - len(cand[:k]))
        assert ref["idx"][m].tolist() == want_i
        assert ref["val"][m].tolist() == pytest.approx(want_v, rel=1e-13, abs=1e-15)     # two f64 summation orders of D <= 16 terms
        assert ref["nq"][m] == len(cand)


def test_sure_positions_on_a_hand_made_ranking():
    # scores 10, 9, 9 - 1e-9, 5, 5 (a bitwise copy), 1; bound 1e-6 everywhere
    s = np.array([[10.0, 9.0, 9.0 - 1e-9, 5.0, 5.0, 1.0]])
    b = np.full_like(s, 1e-6)
    idx, val, nq, order = R.rank(s, 5)
    classes = np.array([0, 1, 2, 3, 3, 4])
    sure = R.sure_positions(s, b, order, nq, 5, classes)
    assert sure.tolist() == [[True, False, False, True, True]]       # the near tie is unsure, the copy pair is decided by the tie rule
    sure = R.sure_positions(s, b, order, nq, 4, classes)
    assert sure.tolist() == [[True, False, False, True]]             # rank 3's lower neighbour is the first key left out: its copy
    sure = R.sure_positions(s[:, :3], b[:, :3], *R.rank(s[:, :3], 5)[3:1:-1], 5, classes[:3])
    assert sure.tolist() == [[True, False, False]]                   # N < k: no neighbour below the last key


def test_hist_loop_and_metrics():
    from pero_pretraining_amd.joint_embedding_pretraining.retrieval import metrics_from_hist
    idx = [[4, 2, 9], [1, 0, 3], [5, 6, 7], [8, 8, 8]]
    h = R.hist_loop(idx, [4, 3, -1, 2], 3)
    assert h == [3, 1, 0, 1, 1]
    m = metrics_from_hist(h, (1, 3))
    assert m == {"recall@1": 1 / 3, "recall@3": 2 / 3, "mrr@3": (1 + 1 / 3) / 3, "retrieval_queries": 3}
    assert math.isnan(metrics_from_hist([0, 0, 0], (1,))["recall@1"])


# ------------------------------------------------------------------------------------------------ inputs of the GPU test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_near_ties_stay_under_the_cap(shape, dtype):
    """Rank positions that are not sure: at most NEAR_TIE_CAP of M * min(k, N), with the larger of the two bounds (computed scales).
    With this generator and (3 D + 9) 2^-24: worst 1.6 % at (64, 257, 136, 10) bf16, 0.8 % at (33, 1100, 16, 16) f32."""
    M, N, D, k = shape
    q, keys, plants = R.case(M, N, D, dtype)
    qs, ks = R.inv_norm_f32(q), R.inv_norm_f32(keys)
    ref = R.reference(q, keys, k, qs, ks, scales="computed")
    unsure = int((~ref["sure"]).sum())
    print(f"NEAR_TIES {shape} {dtype}: {unsure} of {M * min(k, N)}")
    assert unsure <= R.NEAR_TIE_CAP * M * min(k, N), (shape, unsure)
    # the planted query finds its two copies in front, lower index first, and that is sure
    for row, lo, hi in plants:
        assert ref["idx"][row, 0] == lo and (k < 2 or N < 2 or ref["idx"][row, 1] == hi)
        assert ref["sure"][row, 0]


def test_plants_fall_where_the_table_says():
    def place(n):
        t = n % 128
        return n // 128, t // 32, (t >> 2) & 1, (t & 3) + 4 * ((t % 32) >> 3)     # tile, wave, lane half, register

    def split_of(n, N, S):
        T = (N + 127) // 128
        return next(s for s in range(S) if T * s // S <= n // 128 < T * (s + 1) // S)

    p = {n: (place(n), place(n + d)) for n, d in R.PLANTS}
    assert p[20][0][:3] == p[20][1][:3] and p[20][0][3] != p[20][1][3]
    assert p[1][0][2] == 0 and p[1][1][2] == 1 and p[12][0][2] == 1 and p[12][1][2] == 0
    assert p[3][0][:2] == (0, 0) and p[3][1][:2] == (0, 1)
    assert p[100][0][:2] == (0, 3) and p[100][1][:2] == (1, 1)
    assert p[8][0][1:] == p[8][1][1:] and p[8][1][0] == 1
    for S in (2, 3, 7):
        assert split_of(8, 300, S) != split_of(136, 300, S)
    assert split_of(380, 1100, 3) != split_of(388, 1100, 3) and split_of(380, 1100, 7) != split_of(388, 1100, 7)
    assert split_of(500, 1100, 2) != split_of(524, 1100, 2)
    keys = [n for n, d in R.PLANTS] + [n + d for n, d in R.PLANTS]
    assert len(set(keys)) == len(keys)


def test_alignment_loop_on_collated_masks():
    """The expected values of alignment_targets: the plain loop against the project's host twin of pero_ntxent_slots, on masks made by
    BatchCreator's own host rule with real left paddings and crop shifts."""
    from pero_pretraining_amd.common.dataloader import BatchCreator
    from pero_pretraining_amd.joint_embedding_pretraining.losses import ntxent_slots_host
    S, sub = 24, 8
    widths1, left1 = [100, 64, 150, 8], [3, 0, 2, 20]
    widths2, left2 = [100, 70, 150, 8], [1, 5, 2, 0]
    im1, im2, sm1, sm2 = BatchCreator._host_masks(widths1, left1, widths2, left2, [0, 2, -1, 0], S, sub)
    want = R.alignment_targets_loop(im1, im2, sm1, sm2)
    slot1, slot2, count = ntxent_slots_host(im1, im2, sm1, sm2)
    for l in range(len(widths1)):
        for p in range(S):
            if slot1[l, p] >= 0 and count[l] >= 0:
                assert want[l, p] == l * S + int(np.nonzero(slot2[l] == slot1[l, p])[0][0])
            else:
                assert want[l, p] == -1
    assert (want >= 0).any() and (want < 0).any()


# ------------------------------------------------------------------------------------------------ host-side rules of the library
def test_sim_topk_validates_arguments_without_gpu():
    h = lib()
    raw = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(raw) + 15) // 16 * 16
    buf = ctypes.c_void_p(base)

    def topk(q=buf, ldq=8, keys=buf, ldk=8, idx=buf, val=buf, work=buf, M=4, N=4, D=8, k=2, splits=1, dtype=0):
        return h.pero_sim_topk(q, ldq, keys, ldk, None, None, None, None, idx, val, work, M, N, D, k, splits, dtype, None)

    assert topk(k=0) == -1 and b"k = 0" in h.pero_last_error()
    assert topk(k=17) == -1
    assert topk(D=12) == -1 and b"multiple of 8" in h.pero_last_error()          # odd D
    assert topk(D=4) == -1
    assert topk(q=ctypes.c_void_p(base + 4)) == -1 and b"aligned" in h.pero_last_error()     # misaligned base
    assert topk(ldk=10) == -1                                                      # f32 pitch of 40 bytes
    assert topk(dtype=1, ldq=12) == -1                                             # bf16 pitch of 24 bytes
    assert topk(ldq=4) == -1                                                       # pitch below D
    assert topk(idx=None) == -1 and b"null" in h.pero_last_error()
    assert topk(val=None) == -1
    assert topk(M=0) == -1 and topk(N=0) == -1
    assert topk(dtype=2) == -1
    assert topk(splits=129) == -1 and topk(splits=-1) == -1
    assert topk(splits=2, work=None) == -1 and b"work" in h.pero_last_error()
    assert h.pero_retrieval_hist(buf, buf, None, 4, 2, None) == -1
    assert h.pero_retrieval_hist(buf, buf, buf, 4, 17, None) == -1
    assert h.pero_retrieval_hist(buf, buf, buf, 0, 2, None) == 0                    # M = 0: nothing to launch
    assert h.pero_inv_rownorm(buf, 8, buf, 4, 12, 0, None) == -1
    assert h.pero_inv_rownorm(ctypes.c_void_p(base + 8), 8, buf, 4, 8, 0, None) == -1


def test_key_split_rule():
    """pero_sim_topk_key_splits = max(1, min(ceil(512 / ceil(M / 64)), ceil(N / 128), 128)), as the header states it."""
    from pero_pretraining_amd import ops
    for M, N in [(1, 1), (64, 16384), (65, 16384), (16384, 16384), (33, 1100), (130, 300), (4096, 100000), (64 * 511, 300), (64 * 512, 300)]:
        want = max(1, min(-(-512 // -(-M // 64)), -(-N // 128), 128))
        assert ops.sim_topk_key_splits(M, N) == want, (M, N)
    assert ops.sim_topk_key_splits(64, 16384) == 128 and ops.sim_topk_key_splits(16384, 16384) == 2 and ops.sim_topk_key_splits(64 * 512, 300) == 1


def test_tester_refuses_k_above_the_kernel_limit():
    from pero_pretraining_amd.joint_embedding_pretraining.tester import Tester
    with pytest.raises(ValueError):
        Tester(None, None, None, retrieval_ks=(1, 17))
    assert Tester(None, None, None).retrieval_ks is None
    assert Tester(None, None, None, retrieval_ks=[1, 5, 16]).retrieval_ks == (1, 5, 16)
