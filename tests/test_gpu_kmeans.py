"""GPU: mini-batch k-means fit (scripts/kmeans.py over csrc/kmeans.hip) against the sklearn references of
tests/golden/g23_kmeans.npz (tools/make_golden_kmeans.py) and against f64 restatements computed here."""
import math

import numpy as np
import pytest
import torch

import kmeans_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of f32


@pytest.fixture(scope="module")
def g23():
    g = R.load_g23()
    g["x_dev"] = torch.from_numpy(g["x"]).cuda()
    return g


def _model(**kw):
    from pero_pretraining_amd.scripts.kmeans import MiniBatchKMeans
    return MiniBatchKMeans(**kw)


def _sigma_bound(samples):
    """mean + 4 sigma of the fixture's sklearn samples."""
    return float(samples.mean() + 4.0 * samples.std())


# ---- 1. partial_fit against sklearn / f64, step by step ------------------------------------------------------------
def test_partial_fit_matches_g23_step_by_step(g23):
    from pero_pretraining_amd import ops
    x = g23["x_dev"]
    m = _model(n_clusters=R.K, init=g23["x"][g23["init_rows"]], n_init=1, batch_size=R.B, reassignment_ratio=0.0)
    tol = 8.0 * float(g23["sk_vs_f64"])   # sklearn's own f32 rounding distance to f64, times 8: from the reference data
    prev_counts = np.zeros(R.K)
    centers = torch.from_numpy(g23["x"][g23["init_rows"]]).cuda()
    for s in range(R.STEPS):
        xb = x[s * R.B:(s + 1) * R.B].contiguous()
        before = (m.cluster_centers_ if s else centers).clone()
        labels = ops.vq_argmin(xb, before)   # the labels the step is about to use
        m.partial_fit(xb)
        assert np.array_equal(labels.cpu().numpy(), g23["labels"][s]), f"step {s}: pre-update labels"   # all rows
        counts = m._counts.cpu().numpy()
        assert np.array_equal(counts, g23["counts"][s].astype(np.float64)), f"step {s}: _counts"
        got = m.cluster_centers_.cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - g23["centers64"][s]).max())
        print(f"step {s}: max |centres - f64| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol
        empty = counts == prev_counts
        assert np.array_equal(got[empty].view(np.uint32), before.cpu().numpy()[empty].view(np.uint32)), f"step {s}: empty centres moved"
        prev_counts = counts
    assert m.n_steps_ == R.STEPS and m.labels_.shape == (R.B,)


# ---- 2. the update kernel alone ------------------------------------------------------------------------------------
def _row_groups(d):
    """Row groups G of csrc/kmeans.hip km_update_k: 256 / (column slots, a power of two <= 256)."""
    cols = d // 4 if d % 4 == 0 else d
    cw = 1
    while cw < 256 and cw < cols:
        cw *= 2
    return 256 // cw


def _check_update(x, labels, centers, weights):
    """One ops.kmeans_update against f64 with the kernel's own input labels and the worst-case bound of its summation order.

    Thread (g, column) adds the member rows g, g+G, ... of a centre one after the other, then the G partial sums are
    added in the order g = 0..G-1: a term passes through at most depth = ceil(n/G) + G - 2 f32 additions (the first
    addition of a chain is to 0, exact), so |fl(S) - S| <= gamma_depth * sum|x|, gamma_d = d u / (1 - d u), u = 2^-24.
    The quotient (c w + S) / (w + n) is formed in f64 and rounded once: one more u |c_new|.  The f64 operations add
    at most 3 * 2^-53 relative to |c| w + sum|x|, covered by the 2^-20 head-room factor."""
    from pero_pretraining_amd import ops
    K, D = centers.shape
    c0, w0 = centers.clone(), weights.clone()
    shift = ops.kmeans_update(x, labels, centers, weights)
    xd = x.double()
    n = torch.bincount(labels, minlength=K).double()
    sums = torch.zeros(K, D, device=x.device, dtype=torch.float64).index_add_(0, labels, xd)
    sabs = torch.zeros(K, D, device=x.device, dtype=torch.float64).index_add_(0, labels, xd.abs())
    hit = n > 0
    wn = w0 + n
    ref = torch.where(hit[:, None], (c0.double() * w0[:, None] + sums) / wn.clamp(min=1)[:, None], c0.double())
    G = _row_groups(D)
    depth = torch.ceil(n / G) + G - 2
    gamma = depth * U / (1 - depth * U)
    bound = (gamma[:, None] * sabs / wn.clamp(min=1)[:, None] + U * ref.abs()) * (1 + 2.0 ** -20)
    err = (centers.double() - ref).abs()
    worst = float((err - bound).max())
    print(f"K={K} D={D} B={x.shape[0]}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, max n_k {int(n.max())}")
    assert worst <= 0.0, worst
    assert torch.equal(weights, wn)
    assert torch.equal(centers[~hit].view(torch.int32), c0[~hit].view(torch.int32))   # untouched centres keep their bits
    sref = float(((centers.double() - c0.double()) ** 2).sum())
    assert abs(float(shift) - sref) <= 1e-4 * sref + 1e-30
    return int((~hit).sum())


@pytest.mark.parametrize("K,D,B", [(100, 20, 777), (7, 3, 50), (1, 1, 1)])
def test_update_awkward_shapes(K, D, B):
    from pero_pretraining_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(K * 1000 + D)
    x = torch.randn(B, D, device="cuda", generator=gen) * 3
    centers = x[torch.randperm(B, device="cuda", generator=gen)[:K]].clone()
    centers[K // 2:] += 40.0   # the upper half gets no member: the empty branch
    weights = torch.randint(0, 5, (K,), device="cuda", generator=gen).double()
    weights[0] = 2.0 ** 24 + 1   # a count f32 cannot hold
    labels = ops.vq_argmin(x, centers)
    empties = _check_update(x, labels, centers, weights)
    assert empties > 0 or K == 1


def test_update_real_shape_three_steps():
    from pero_pretraining_amd import ops
    from pero_pretraining_amd.models.autoencoders import kmeans_labels
    K, D, B = 4096, 512, 16384
    gen = torch.Generator(device="cuda").manual_seed(5)
    blobs = torch.randn(K, D, device="cuda", generator=gen)
    popular = torch.randint(0, 64, (B // 2,), device="cuda", generator=gen)   # heavy centres: hundreds of rows each
    centers = (blobs + 0.05 * torch.randn(K, D, device="cuda", generator=gen)).contiguous()
    weights = torch.zeros(K, device="cuda", dtype=torch.float64)
    for step in range(3):
        which = torch.cat([popular, torch.randint(0, K, (B - B // 2,), device="cuda", generator=gen)])
        x = (blobs[which] + 0.3 * torch.randn(B, D, device="cuda", generator=gen)).contiguous()
        labels = ops.vq_argmin(x, centers)
        feats = x.view(16, B // 16, D).permute(0, 2, 1)   # (N, F, T) as the label pipeline sees the same rows
        assert torch.equal(labels, kmeans_labels(feats, centers).reshape(-1))
        _check_update(x, labels, centers, weights)
    assert float(weights.sum()) == 3 * B


# ---- 3. determinism ------------------------------------------------------------------------------------------------
def test_update_is_bit_identical_from_run_to_run():
    from pero_pretraining_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(11)
    K, D, B = 512, 96, 8192
    x = torch.randn(B, D, device="cuda", generator=gen)
    c = torch.randn(K, D, device="cuda", generator=gen)
    w = torch.randint(0, 100, (K,), device="cuda", generator=gen).double()
    labels = torch.randint(0, 8, (B,), device="cuda", generator=gen) ** 3   # skewed: label 0 and 1 are heavy, most centres empty
    out = []
    for _ in range(2):
        ci, wi = c.clone(), w.clone()
        s = ops.kmeans_update(x, labels, ci, wi)
        out.append((ci, wi, s.clone()))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
    assert torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][2].view(torch.int32), out[1][2].view(torch.int32))


def test_fit_is_bit_identical_for_one_random_state(g23):
    runs = [_model(n_clusters=R.K, batch_size=R.B, max_iter=3, n_init=2, random_state=3).fit(g23["x_dev"]) for _ in range(2)]
    assert torch.equal(runs[0].cluster_centers_.view(torch.int32), runs[1].cluster_centers_.view(torch.int32))
    assert torch.equal(runs[0]._counts, runs[1]._counts)
    assert runs[0].inertia_ == runs[1].inertia_ and runs[0].n_steps_ == runs[1].n_steps_


# ---- 4. seeding ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_kmeans_plusplus_seeding_quality(g23, seed):
    x = g23["x_dev"]
    m = _model(n_clusters=R.K, init="k-means++", init_size=x.shape[0], random_state=seed)
    m._check_params(x)
    centers = m._init_centroids(x).cpu().numpy()
    idx = m._init_indices.cpu().numpy()
    assert idx.shape == (R.K,) and idx.min() >= 0 and idx.max() < x.shape[0]
    assert len(np.unique(idx)) == R.K
    assert np.array_equal(centers, g23["x"][idx])   # every centre is a row of X
    pot = R.potential(g23["x"], centers)
    bound = _sigma_bound(g23["pp_potential"])
    print(f"seed {seed}: potential {pot:.0f}, sklearn {g23['pp_potential'].mean():.0f} +- {g23['pp_potential'].std():.0f}, bound {bound:.0f}, "
          f"uniform {g23['uniform_potential'].mean():.0f}")
    assert pot <= bound


@pytest.mark.parametrize("d", [32, 7])
def test_pp_step_commits_the_best_candidate(g23, d):
    """One pero_kmeans_pp_step against f64 (16-byte path and generic path): potentials of 5 candidates, the minimum is
    committed.  Distances are the expanded form in f32: a (d + 3)-term chain over |x|^2 + |c|^2 + 2|x||c| <= 4 max|x|^2."""
    from pero_pretraining_amd import ops
    xh = np.ascontiguousarray(g23["x"][:1000, :d])   # 1000 rows: the last workgroup is partial
    x = torch.from_numpy(xh).cuda()
    closest = torch.from_numpy(R.sqdist(xh, xh[[17]]).min(1).astype(np.float32)).cuda()
    cand = torch.tensor([3, 500, 999, 17, 640], device="cuda")
    dist = np.minimum(R.sqdist(xh, xh[cand.cpu().numpy()]), closest.cpu().numpy().astype(np.float64)[:, None])
    pots = dist.sum(0)
    best = int(pots.argmin())
    atol = (d + 3) * U * 4.0 * float((xh.astype(np.float64) ** 2).sum(1).max())
    chosen = torch.empty(1, device="cuda", dtype=torch.int64)
    pot = torch.empty(1, device="cuda", dtype=torch.float64)
    ops.kmeans_pp_step(x, ops.kmeans_sqnorm(x), closest, cand, chosen, pot)
    assert int(chosen) == int(cand[best])
    assert abs(float(pot) - pots[best]) <= len(xh) * atol
    np.testing.assert_allclose(closest.cpu().numpy(), dist[:, best], rtol=0, atol=atol)
    assert float(closest[int(chosen)]) == 0.0


# ---- 5. fit end to end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_fit_inertia_matches_sklearn_quality(g23, seed):
    """`fit` (batch 1024, max_iter=100, n_init=10) on the g23 rows: the inertia, computed here in f64, is at most mean + 4 sigma of the
    fixture's 8 sklearn fits (102 144 + 4 * 1 835 = 109 484)."""
    x = g23["x_dev"]
    m = _model(n_clusters=R.K, init="k-means++", batch_size=R.B, max_iter=100, n_init=10, random_state=seed).fit(x)
    inertia = R.potential(g23["x"], m.cluster_centers_.cpu().numpy())
    bound = _sigma_bound(g23["fit_inertia"])
    print(f"seed {seed}: inertia {inertia:.0f} (model {m.inertia_:.0f}), sklearn {g23['fit_inertia'].mean():.0f} +- "
          f"{g23['fit_inertia'].std():.0f}, bound {bound:.0f}, steps {m.n_steps_}")
    assert inertia <= bound
    assert abs(m.inertia_ - inertia) <= 1e-4 * inertia
    assert 1 <= m.n_steps_ <= 100 * x.shape[0] // R.B
    assert m.n_iter_ == math.ceil(m.n_steps_ * R.B / x.shape[0])
    assert torch.equal(m.labels_, m.predict(x)) and m.labels_.shape == (x.shape[0],)


def test_convergence_state_follows_sklearn_rule():
    """pero_kmeans_converge against a host restatement of MiniBatchKMeans._mini_batch_convergence."""
    from pero_pretraining_amd import ops
    n, b, mni = 300, 100, 3   # alpha = 200 / 301
    inertias = [900.0, 800.0, 700.0, 650.0, 660.0, 670.0, 680.0, 690.0, 640.0]   # the EWA rises at steps 6, 7 and 8
    state = torch.zeros(6, device="cuda", dtype=torch.float64)
    shift = torch.ones(1, device="cuda")
    ewa = ewa_min = None
    no_imp, stop_at = 0, None
    alpha = min(1.0, b * 2.0 / (n + 1))
    for step, v in enumerate(inertias, 1):
        ops.kmeans_converge(torch.tensor([v], device="cuda"), shift, state, n, b, 0.0, mni)
        if step == 1:
            continue
        bi = float(np.float32(v)) / b
        ewa = bi if ewa is None else ewa * (1 - alpha) + bi * alpha
        if ewa_min is None or ewa < ewa_min:
            no_imp, ewa_min = 0, ewa
        else:
            no_imp += 1
        if no_imp >= mni and stop_at is None:
            stop_at = step
    s = state.cpu().numpy()
    assert stop_at == 8
    assert s[3] == 1.0 and s[5] == stop_at and s[4] == len(inertias)
    assert abs(s[0] - ewa) <= 1e-12 * ewa and abs(s[1] - ewa_min) <= 1e-12 * ewa_min
    # tol rule: a shift at or below tol stops at once
    state.zero_()
    for _ in range(2):
        ops.kmeans_converge(torch.tensor([5.0], device="cuda"), torch.full((1,), 1e-3, device="cuda"), state, n, b, 1e-2, None)
    assert state[3].item() == 1.0 and state[5].item() == 2.0


# ---- 6. reassignment -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,expect", [(64, 4), (4, 2)])
def test_forced_reassignment(B, expect):
    from pero_pretraining_amd import ops
    K, D = 16, 8
    gen = torch.Generator(device="cuda").manual_seed(B)
    near = torch.randn(12, D, device="cuda", generator=gen) * 4
    centers = torch.cat([near, near[:4] + 500.0]).contiguous()                    # centres 12..15 are far from all data: starved
    xb = (near[torch.randint(0, 12, (B,), device="cuda", generator=gen)] + 0.1 * torch.randn(B, D, device="cuda", generator=gen)).contiguous()
    weights = torch.cat([torch.full((12,), 1000.0), torch.tensor([4.0, 3.0, 1.0, 2.0])]).double().cuda()
    m = _model(n_clusters=K, init=centers, reassignment_ratio=0.01, random_state=1)
    m._reset(centers.clone())   # a fitted model that has seen ~12000 rows
    m._check_params(xb)
    m._counts.copy_(weights)
    # the plain update of the same batch
    pc, pw = centers.clone(), weights.clone()
    ops.kmeans_update(xb, ops.vq_argmin(xb, pc), pc, pw)
    m._mini_batch_step(xb, random_reassign=True)
    got_c, got_w = m.cluster_centers_, m._counts
    starved = pw < 0.01 * pw.max()
    assert int(starved.sum()) == 4
    moved = (got_c != pc).any(1)
    assert int(moved.sum()) == expect and expect <= B // 2 and bool((moved <= starved).all())
    if expect < 4:   # more starved centres than B / 2: the lightest go first
        assert moved.nonzero().reshape(-1).tolist() == [14, 15]
    rows = []
    for k in moved.nonzero().reshape(-1).tolist():
        match = (xb == got_c[k]).all(1).nonzero().reshape(-1)
        assert match.numel() >= 1, f"centre {k} is not a batch row"
        rows.append(int(match[0]))
    assert len(set(rows)) == len(rows)
    assert torch.equal(got_w[moved], pw[~moved].min().expand(int(moved.sum())))
    assert torch.equal(got_c[~moved].view(torch.int32), pc[~moved].view(torch.int32))
    assert torch.equal(got_w[~moved], pw[~moved])


# ---- 7. pipeline: features -> fit -> labels --------------------------------------------------------------------------
def test_pipeline_features_fit_labels(tmp_path):
    import pickle

    from pero_pretraining_amd.scripts import kmeans as S
    from pero_pretraining_amd.scripts.labels import compute_features, compute_kmeans_labels
    rng = np.random.default_rng(3)
    n, d, t = 3, 12, 10
    dataset = []
    for b in range(4):
        masks = (rng.random((n, t)) < 0.7).astype(np.int64)
        masks[0, 0] = 1
        dataset.append({"ids": [f"line_{b}_{i}" for i in range(n)], "image_masks": masks,
                        "images": torch.from_numpy(rng.standard_normal((n, d, t)).astype(np.float32)).cuda()})

    def encode(images):   # stands for the VGG stack: (N, D, 1, T)
        return (images * 2.0).unsqueeze(2)

    feats = compute_features(encode, dataset)
    expect = np.vstack([(b["images"] * 2.0).permute(0, 2, 1).cpu().numpy()[b["image_masks"] == 1] for b in dataset])   # produce_features.py
    assert feats.is_cuda and feats.dtype == torch.float32
    assert np.array_equal(feats.cpu().numpy(), expect)

    data, out, labels_path = tmp_path / "features.pkl", tmp_path / "centroids.npy", tmp_path / "labels.txt"
    data.write_bytes(pickle.dumps(expect.copy()))
    model = S.fit(str(data), 8, batch_size=32, epochs=2)
    S.save_centroids(model, str(out))
    centroids = torch.from_numpy(np.load(out)).cuda()
    assert centroids.shape == (8, d) and torch.equal(centroids, model.cluster_centers_)
    assert compute_kmeans_labels(encode, centroids, dataset, str(labels_path)) == 4 * n
    predicted = model.predict(feats).cpu().numpy().tolist()
    written = [int(v) for line in open(labels_path) for v in line.split()[1:]]
    assert written == predicted
