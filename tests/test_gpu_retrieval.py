"""pero_sim_topk, pero_retrieval_hist and pero_inv_rownorm (csrc/retrieval.hip) against the f64 reference of tests/retrieval_ref.py, and the
joint Tester's retrieval metrics end to end.  The specification quoted here is the header's (include/pero_hip.h "Retrieval"):
  score = ((q . key) q_scale) key_scale; higher score first, equal f32 scores: lower key index first; a key with key_valid == 0, the key
  skip[m] and NaN scores never enter; unused slots are idx = -1, val = -inf; every output element is written; the result does not depend
  on the number of key splits.
Outputs sit in `Guarded` buffers as in tests/test_gpu_datapath_parity.py: 0xA5 bytes around them must survive, and the output starts as
0x5C bytes, so that an element the kernel skipped fails the comparison.  No tolerance here is a measured number: the bound is
retrieval_ref.rounding_bound."""
import functools

import numpy as np
import pytest
import torch

import retrieval_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def call(name, *args):
    from pero_pretraining_amd._lib import call as _call
    return _call(name, *args)


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).cuda()


class Guarded:
    """`t`: a tensor of `shape` / `dtype` that starts `guard` bytes into its allocation and ends `guard` bytes before its end."""

    def __init__(self, shape, dtype, guard, init=None):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        assert guard % 16 == 0 and guard >= 16
        self.raw = torch.full((2 * guard + nbytes,), 0xA5, device="cuda", dtype=torch.uint8)
        body = self.raw[guard:guard + nbytes]
        body.fill_(0x5C)
        self.t = body.view(dtype).view(shape)
        self.guard = guard
        if init is not None:
            self.t.copy_(torch.as_tensor(init).to(dtype))

    def check(self):
        g = self.guard
        assert int(self.raw[:g].min()) == 0xA5 and int(self.raw[:g].max()) == 0xA5, "bytes in front of the output were written"
        assert int(self.raw[-g:].min()) == 0xA5 and int(self.raw[-g:].max()) == 0xA5, "bytes behind the output were written"
        return self.t


def topk(ops, q, keys, k, q_scale=None, key_scale=None, key_valid=None, skip=None, key_splits=0):
    """pero_sim_topk on device tensors (q, keys may be views with a row pitch) into guarded outputs -> (idx, val) on the host."""
    M, D = q.shape
    N = keys.shape[0]
    guard = (4 * k + 16 + 15) // 16 * 16                                   # one output row plus one 16-byte piece
    idx, val = Guarded((M, k), torch.int32, guard), Guarded((M, k), torch.float32, guard)
    splits = key_splits if key_splits else ops.sim_topk_key_splits(M, N)
    work = Guarded((8 * splits * M * k,), torch.uint8, 64) if splits > 1 else None     # exactly the header's formula
    call("pero_sim_topk", ops.ptr(q), q.stride(0), ops.ptr(keys), keys.stride(0), ops.ptr(q_scale), ops.ptr(key_scale), ops.ptr(key_valid),
         ops.ptr(skip), ops.ptr(idx.t), ops.ptr(val.t), None if work is None else ops.ptr(work.t), M, N, D, k, key_splits, ops.dt(q), ops.stream())
    if work is not None:
        work.check()
    return idx.check().cpu().numpy(), val.check().cpu().numpy()


@functools.lru_cache(maxsize=None)
def cosine_case(shape, dtype):
    """inputs and reference of one (shape, dtype), computed once and shared: cosine scores with the scales as f32 inputs"""
    M, N, D, k = shape
    q, keys, plants = R.case(M, N, D, dtype)
    qs, ks = R.inv_norm_f32(q), R.inv_norm_f32(keys)
    return q, keys, plants, qs, ks, R.reference(q, keys, k, qs, ks)


def check_lists(idx, val, ref, k, key_valid=None, skip=None):
    """the parity conditions of one call against reference `ref`"""
    s, b = ref["scores"], ref["bound"]
    M, N = s.shape
    out = np.isnan(s)
    if key_valid is not None:
        out |= (key_valid == 0)[None, :]
    if skip is not None:
        out |= np.arange(N)[None, :] == skip[:, None]
    for m in range(M):
        n_live = min(k, int(ref["nq"][m]))
        got = idx[m, :n_live]
        # distinct, in range, valid, not skipped, not NaN; exact filling behind them
        assert len(set(got.tolist())) == n_live and got.min(initial=0) >= 0 and got.max(initial=0) < N, (m, idx[m])
        assert not out[m, got].any(), (m, idx[m])
        assert (idx[m, n_live:] == -1).all() and np.isneginf(val[m, n_live:]).all(), (m, idx[m], val[m])
        # every value within the bound of the f64 score of the index it stands beside
        assert np.all(np.abs(val[m, :n_live].astype(np.float64) - s[m, got]) <= b[m, got]), (m, val[m], s[m, got])
        # sorted under the strict order on the returned f32 values
        v = val[m, :n_live]
        assert np.all((v[:-1] > v[1:]) | ((v[:-1] == v[1:]) & (got[:-1] < got[1:]))), (m, idx[m], val[m])
        # no key left out beats the list's last entry by more than the two bounds
        if n_live == k:
            rest = ~out[m]
            rest[got] = False
            last = got[-1]
            assert np.all(s[m, rest] - s[m, last] <= b[m, rest] + b[m, last]), m
    sure = ref["sure"]
    kk = sure.shape[1]
    assert np.array_equal(idx[:, :kk][sure], ref["idx"][:, :kk][sure])


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_parity(ops, shape, dtype):
    M, N, D, k = shape
    q, keys, plants, qs, ks, ref = cosine_case(shape, dtype)
    idx, val = topk(ops, dev(q, dtype), dev(keys, dtype), k, dev(qs), dev(ks))
    check_lists(idx, val, ref, k)
    for row, lo, hi in plants:                      # the planted copies: the same f32 bits, lower index first, the other directly behind
        assert idx[row, 0] == lo
        if min(k, N) > 1:
            assert idx[row, 1] == hi and val[row, 0] == val[row, 1]
    assert len(plants) == min(M, sum(n + d < N for n, d in R.PLANTS))


# ------------------------------------------------------------------------------------------------ 2. masks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(5, 3, 8, 16), (70, 200, 40, 16), (33, 1100, 16, 16), (66, 127, 56, 4)])
def test_masks(ops, shape, dtype):
    M, N, D, k = shape
    q, keys, _ = R.case(M, N, D, dtype)
    rng = np.random.default_rng(N)
    valid = (rng.random(N) >= 1 / 3).astype(np.uint8)
    nan_key = N - 1
    valid[[0, nan_key]], valid[1] = 1, 0                              # at the smallest N too: one key on, one off, and the NaN key on
    qs, ks = R.inv_norm_f32(q), R.inv_norm_f32(keys)
    keys[nan_key, D // 2] = np.nan                                    # ks[nan_key] stays finite: the NaN comes from the dot
    first = R.rank(R.scores64(q, keys, qs, ks), 1, valid)[0][:, 0]    # the key that would be rank 0 without `skip`
    skip = first.astype(np.int32)
    skip[::5] = -1                                                    # and some queries without one
    ref = R.reference(q, keys, k, qs, ks, valid, skip)
    idx, val = topk(ops, dev(q, dtype), dev(keys, dtype), k, dev(qs), dev(ks), dev(valid), dev(skip))
    assert not np.isin(idx, np.nonzero(valid == 0)[0]).any() and not (idx == nan_key).any()
    has = skip >= 0
    assert has.any() and not (idx[has] == skip[has, None]).any()
    check_lists(idx, val, ref, k, valid, skip)
    if N < k:
        assert (ref["nq"] < k).all() and (idx[:, N:] == -1).all()
    # nothing qualifies at all: every slot is the filling
    idx, val = topk(ops, dev(q, dtype), dev(keys, dtype), k, key_valid=dev(np.zeros(N, dtype=np.uint8)))
    assert (idx == -1).all() and np.isneginf(val).all()


# ------------------------------------------------------------------------------------------------ 3. scales
@pytest.mark.parametrize("dtype", DTYPES)
def test_null_scales_are_scales_of_one(ops, dtype):
    shape = (70, 200, 40, 16)
    M, N, D, k = shape
    q, keys, _ = R.case(M, N, D, dtype)
    qd, kd = dev(q, dtype), dev(keys, dtype)
    a = topk(ops, qd, kd, k)
    b = topk(ops, qd, kd, k, dev(np.ones(M, dtype=np.float32)), dev(np.ones(N, dtype=np.float32)))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    check_lists(a[0], a[1], R.reference(q, keys, k), k)              # plain dot products against f64


@pytest.mark.parametrize("dtype", DTYPES)
def test_retrieve_normalises_the_row_scale_away(ops, dtype):
    """retrieve(normalize=True) on rows multiplied by arbitrary positive factors returns the indices of the unscaled rows at every sure
    position.  The factors are powers of two, 2^-20 ... 2^20, one per row: the scaled rows are then exact in both dtypes and the exact
    cosine does not move (any other factor rounds the rows - in bf16 that alone moves a cosine by 2^-8).  The scales are computed on the
    device here, so sure-ness uses the bound for computed scales."""
    from pero_pretraining_amd.joint_embedding_pretraining.retrieval import retrieve
    shape = (70, 200, 40, 16)
    M, N, D, k = shape
    q, keys, plants = R.case(M, N, D, dtype)
    rng = np.random.default_rng(7)
    fq, fk = np.exp2(rng.integers(-20, 21, M)).astype(np.float32), np.exp2(rng.integers(-20, 21, N)).astype(np.float32)
    ref = R.reference(q, keys, k, R.inv_norm_f32(q), R.inv_norm_f32(keys), scales="computed")
    sure = ref["sure"]
    plain = retrieve(dev(q, dtype).view(7, 10, D), dev(keys, dtype).view(2, 100, D), k)
    scaled = retrieve(dev(q * fq[:, None], dtype).view(7, 10, D), dev(keys * fk[:, None], dtype).view(2, 100, D), k)
    assert plain.indices.shape == plain.scores.shape == (7, 10, k) and plain.indices.dtype == torch.int32
    pi, si = plain.indices.view(M, k).cpu().numpy(), scaled.indices.view(M, k).cpu().numpy()
    assert np.array_equal(pi[sure], ref["idx"][sure]) and np.array_equal(si[sure], ref["idx"][sure])
    assert np.all(np.abs(scaled.scores.view(M, k).cpu().numpy().astype(np.float64) - np.take_along_axis(ref["scores"], si.astype(np.int64), 1))
                  <= np.take_along_axis(ref["bound"], si.astype(np.int64), 1))
    for row, lo, hi in plants:
        assert pi[row, 0] == lo and pi[row, 1] == hi
    # inv_rownorm alone: 1 / |x| within (D + 1) / 2 + 2 units of f32 roundoff (retrieval_ref.rounding_bound, "computed")
    inv = ops.inv_rownorm(dev(keys, dtype)).cpu().numpy().astype(np.float64)
    want = 1.0 / np.sqrt((keys.astype(np.float64) ** 2).sum(1))
    assert np.all(np.abs(inv - want) <= ((D + 1) / 2 + 2) * R.U * want)
    # key_mask and skip reach the kernel: self-retrieval never returns the query itself
    me = retrieve(dev(keys, dtype), dev(keys, dtype), 3, key_mask=torch.ones(N), skip=torch.arange(N))
    assert not (me.indices.cpu() == torch.arange(N)[:, None]).any()


# ------------------------------------------------------------------------------------------------ 4. key splits
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(33, 1100, 16, 16), (130, 300, 72, 16)])
def test_key_splits_do_not_change_a_bit(ops, shape, dtype):
    M, N, D, k = shape
    q, keys, plants, qs, ks, ref = cosine_case(shape, dtype)
    args = (dev(q, dtype), dev(keys, dtype), k, dev(qs), dev(ks))
    base = topk(ops, *args, key_splits=1)
    check_lists(base[0], base[1], ref, k)
    for splits in (2, 3, 7, 0, 2):                                     # 0: the library's own choice; 2 again: two runs, the same bits
        got = topk(ops, *args, key_splits=splits)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1].view(np.int32), base[1].view(np.int32)), splits
    assert len(plants) == (8 if N > 524 else 6)                       # the copies across a split boundary are among them
    for row, lo, hi in plants:
        assert base[0][row, 0] == lo and base[0][row, 1] == hi


# ------------------------------------------------------------------------------------------------ 5. pitch and base offset
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_pitch_and_offset_base(ops, dtype):
    shape = (70, 200, 40, 16)
    M, N, D, k = shape
    q, keys, plants, qs, ks, ref = cosine_case(shape, dtype)
    es = torch.empty((), dtype=dtype).element_size()
    views = []
    for a in (q, keys):
        pitch = D + 8                                                  # 32 more bytes (f32) / 16 more bytes (bf16) per row
        raw = torch.full((16 // es + a.shape[0] * pitch,), float("nan"), device="cuda", dtype=dtype)   # NaN wherever no row element lives
        v = raw[16 // es:].view(a.shape[0], pitch)[:, :D]              # the base pointer 16 bytes into its allocation
        v.copy_(dev(a, dtype))
        assert v.data_ptr() % 16 == 0 and v.data_ptr() - raw.data_ptr() == 16 and v.stride(0) == pitch
        views.append(v)
    got = topk(ops, views[0], views[1], k, dev(qs), dev(ks))
    want = topk(ops, dev(q, dtype), dev(keys, dtype), k, dev(qs), dev(ks))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
    check_lists(got[0], got[1], ref, k)
    inv = ops.inv_rownorm(views[1])
    assert torch.equal(inv, ops.inv_rownorm(dev(keys, dtype)))


# ------------------------------------------------------------------------------------------------ 6. the histogram
@pytest.mark.parametrize("k", [1, 5, 16])
def test_retrieval_hist_accumulates(ops, k):
    M = 300                                                             # two workgroups
    rng = np.random.default_rng(k)
    total = [0] * (k + 2)
    hist = Guarded((k + 2,), torch.int64, 32, init=torch.zeros(k + 2, dtype=torch.int64))
    for call_no in range(2):
        idx = np.stack([rng.permutation(1000)[:k] for _ in range(M)]).astype(np.int32)
        idx[5, k - 1:] = -1                                             # a list with an unused slot
        target = np.full(M, -1, dtype=np.int32)                         # a quarter each: none, rank 0, rank k - 1, absent
        target[1::4] = idx[1::4, 0]
        target[2::4] = idx[2::4, k - 1]
        target[3::4] = 1000 + call_no
        some = np.arange(M) % 8 == 4
        target[some] = idx[some, rng.integers(0, k, int(some.sum()))]   # and ranks in between
        want = R.hist_loop(idx, target, k)
        total = [a + b for a, b in zip(total, want)]
        ops.retrieval_hist(dev(idx), dev(target), hist.t)
        assert hist.check().cpu().tolist() == total
    assert total[0] > 0 and total[1] > 0 and total[k] > 0 and total[k + 1] > 0 and sum(total[1:]) == total[0]


# ------------------------------------------------------------------------------------------------ 7. the Tester
def _batches(same_views):
    from pero_pretraining_amd.common.dataloader import BatchCreator
    rng = np.random.default_rng(21)
    out = []
    for b, widths in enumerate(((200, 256, 130, 96), (256, 180, 64))):
        data = []
        for i, w in enumerate(widths):
            a = rng.integers(0, 256, (40, w, 3), dtype=np.uint8)
            data.append({"image": a, "image2": a if same_views else rng.integers(0, 256, (40, w, 3), dtype=np.uint8), "labels": None,
                         "image_id": f"{b}.{i}"})
        np.random.seed(3 + b)                                           # real, different left paddings per view
        out.append(BatchCreator(same_left_paddings=same_views).create_batch(data))
    return out


def _tiny_model():
    from pero_pretraining_amd.joint_embedding_pretraining.train import init_model
    torch.manual_seed(0)
    return init_model(torch.device("cuda", 0), {"type": "vit", "num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128},
                      {"type": "linear", "in_features": 64, "out_features": 80})


@pytest.mark.parametrize("bf16", [False, True])
def test_tester_reports_what_the_lists_say(ops, bf16):
    from pero_pretraining_amd.joint_embedding_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.joint_embedding_pretraining.retrieval import alignment_targets
    from pero_pretraining_amd.joint_embedding_pretraining.tester import Tester
    batches, model, bop = _batches(False), _tiny_model(), BatchOperator(torch.device("cuda", 0))
    seen = []
    forward = model.forward

    def recording(*prepared):
        res = forward(*prepared)
        seen.append((res, prepared[2:]))
        return res

    model.forward = recording
    plain = Tester(bop, model, batches, bfloat16=bf16).test()
    assert set(plain) == {"loss"}
    # today's Tester, restated: the mean of the batch losses in eval mode
    today = sum(r["loss"] for r, _ in seen) / len(seen)
    assert torch.equal(plain["loss"], today) and model.training
    seen.clear()
    res = Tester(bop, model, batches, bfloat16=bf16, retrieval_ks=(1, 5)).test()
    assert set(res) == {"loss", "recall@1", "recall@5", "mrr@5", "retrieval_queries"} and torch.equal(res["loss"], plain["loss"])
    hist, queries = [0] * 7, 0
    for out, masks in seen:
        assert out["output1"].dtype in (torch.float32, torch.bfloat16) and (bf16 or out["output1"].dtype == torch.float32)
        host = [m.cpu().numpy() for m in masks]
        want_t = R.alignment_targets_loop(*host)
        targets = alignment_targets(*masks)
        assert targets.dtype == torch.int32 and np.array_equal(targets.cpu().numpy(), want_t)
        assert (want_t >= 0).any() and (want_t < 0).any() and not (host[0] == 1).all()      # real paddings: some positions have no twin
        rows = np.nonzero(want_t.reshape(-1) >= 0)[0]
        queries += len(rows)
        d = out["output1"].shape[-1]
        x, y = out["output1"].reshape(-1, d), out["output2"].reshape(-1, d).contiguous()
        qrows = x[dev(rows)].contiguous()
        idx, _ = ops.sim_topk(qrows, y, 5, q_scale=ops.inv_rownorm(qrows), key_scale=ops.inv_rownorm(y), key_valid=dev((host[1] == 1).reshape(-1).astype(np.uint8)))
        hist = [a + b for a, b in zip(hist, R.hist_loop(idx.cpu().numpy(), want_t.reshape(-1)[rows], 5))]
    assert res["retrieval_queries"] == queries == hist[0]
    assert res["recall@1"] == hist[1] / queries and res["recall@5"] == sum(hist[1:6]) / queries
    assert res["mrr@5"] == sum(hist[1 + r] / (r + 1) for r in range(5)) / queries


def test_tester_finds_every_twin_of_identical_views(ops):
    """The two views are the same image at shift 0: every query's twin carries its own embedding, so recall@1 is 1."""
    from pero_pretraining_amd.joint_embedding_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.joint_embedding_pretraining.tester import Tester
    batches = _batches(True)
    assert all(s == 0 for b in batches for s in b["shifts"])
    res = Tester(BatchOperator(torch.device("cuda", 0)), _tiny_model(), batches, retrieval_ks=(1, 3)).test()
    assert res["retrieval_queries"] == sum(int(((b["image_masks"] == 1) & (b["shift_masks"] == 1)).sum()) for b in batches) > 0
    assert res["recall@1"] == 1.0 and res["recall@3"] == 1.0 and res["mrr@3"] == 1.0
