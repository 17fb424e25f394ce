"""CPU: the k-means entry points of the C ABI resolve, the g23 fixture is what its generator says it is, the
script-level interface (argument parsing, .npy output, parameter surface) behaves like scripts/fit_kmeans.py."""
import inspect
import pickle

import numpy as np
import pytest

import kmeans_ref as R

KMEANS_SYMBOLS = ("pero_kmeans_update", "pero_kmeans_sqnorm", "pero_kmeans_pp_step", "pero_kmeans_converge")

# sklearn 1.7 MiniBatchKMeans.__init__
SKLEARN_DEFAULTS = dict(n_clusters=8, init="k-means++", max_iter=100, batch_size=1024, verbose=0, compute_labels=True, random_state=None,
                        tol=0.0, max_no_improvement=10, init_size=None, n_init="auto", reassignment_ratio=0.01)


def test_library_exports_kmeans_symbols():
    from pero_pretraining_amd import _lib
    h = _lib.lib()
    for name in KMEANS_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(h, name), name
    assert h.pero_abi_version() == _lib.ABI_VERSION == 2


def test_g23_restatement_matches_fixture():
    g = R.load_g23()
    rows = g["x"]
    assert rows.dtype == np.float32 and rows.shape == (R.STEPS * R.B, R.D)
    init_rows = g["init_rows"]
    assert len(np.unique(init_rows)) == R.K
    labels, inertia, centers, counts, margin = R.restate_steps(rows, rows[init_rows])
    assert np.array_equal(labels, g["labels"])
    assert np.array_equal(counts, g["counts"])
    assert np.array_equal(g["sk_counts"], g["counts"])
    np.testing.assert_allclose(centers, g["centers64"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(inertia, g["inertia"], rtol=1e-12)
    # what the generator asserted: no near-ties, sklearn's f32 within 1e-5 of f64; the empty-centre branch is covered
    assert margin >= 2e-5 and abs(margin - float(g["margin"])) <= 1e-9
    sk = float(np.abs(g["sk_centers"].astype(np.float64) - centers).max())
    assert sk <= 1e-5 and abs(sk - float(g["sk_vs_f64"])) <= 1e-12
    prev = np.vstack([np.zeros((1, R.K)), counts[:-1]])
    assert int((counts == prev).sum()) > 0
    assert len(g["pp_potential"]) == 16 and len(g["fit_inertia"]) == 8
    # the regime the seeding test must tell apart
    assert g["uniform_potential"].mean() > g["pp_potential"].mean() + 10 * g["pp_potential"].std()


def test_parameter_and_method_surface():
    from pero_pretraining_amd.scripts.kmeans import MiniBatchKMeans
    sig = inspect.signature(MiniBatchKMeans.__init__).parameters
    for name, default in SKLEARN_DEFAULTS.items():
        assert name in sig, name
        assert sig[name].default == default, (name, sig[name].default)
    assert sig["poll_every"].default == 64
    m = MiniBatchKMeans(n_clusters=4096, init="k-means++", batch_size=2 ** 14, max_iter=100, n_init=10)
    assert m.get_params()["n_clusters"] == 4096 and m.get_params()["n_init"] == 10
    for meth in ("fit", "partial_fit", "predict"):
        assert callable(getattr(m, meth))
    assert "poll_every" in MiniBatchKMeans.__doc__


def test_defaults_equal_sklearn():
    cluster = pytest.importorskip("sklearn.cluster")
    sig = inspect.signature(cluster.MiniBatchKMeans.__init__).parameters
    for name, default in SKLEARN_DEFAULTS.items():
        assert sig[name].default == default, name


def test_unsupported_inputs_raise():
    from pero_pretraining_amd.scripts.kmeans import MiniBatchKMeans

    class Sparse:
        def tocsr(self):
            return self

    x = np.zeros((8, 4), dtype=np.float32)
    m = MiniBatchKMeans(n_clusters=2)
    with pytest.raises(ValueError):
        m.fit(x, sample_weight=np.ones(8))
    with pytest.raises(ValueError):
        m.partial_fit(x, sample_weight=np.ones(8))
    with pytest.raises(ValueError):
        m.fit(Sparse())
    with pytest.raises(ValueError):
        m._check_X(np.zeros(8, dtype=np.float32))


def test_fit_script_arguments_and_npy_output(tmp_path, monkeypatch, capsys):
    from pero_pretraining_amd.scripts import kmeans as S
    seen = {}

    class Stub:
        def __init__(self, **kw):
            seen["kw"] = kw

        def fit(self, vectors):
            seen["vectors"] = np.array(vectors)
            self.inertia_ = 12.5
            self.cluster_centers_ = np.arange(seen["kw"]["n_clusters"] * vectors.shape[1], dtype=np.float64).reshape(-1, vectors.shape[1])
            return self

    monkeypatch.setattr(S, "MiniBatchKMeans", Stub)
    vectors = np.random.default_rng(0).standard_normal((50, 6)).astype(np.float32)
    data = tmp_path / "features.pkl"
    data.write_bytes(pickle.dumps(vectors.copy()))
    out = tmp_path / "centroids.npy"

    assert S.main(["--dataset", str(data), "--k", "16", "--batch-size", "64", "--iters", "3", "--output", str(out)]) == 0
    assert seen["kw"] == dict(n_clusters=16, init="k-means++", batch_size=64, max_iter=3, n_init=10)   # --iters reaches max_iter
    assert seen["vectors"].shape == vectors.shape                                                        # shuffled, not changed
    assert np.array_equal(np.sort(seen["vectors"], 0), np.sort(vectors, 0))
    got = np.load(out)   # what produce_kmeans_labels.py does
    assert got.dtype == np.float32 and got.shape == (16, 6)
    assert np.array_equal(got, np.arange(96, dtype=np.float32).reshape(16, 6))
    assert "Inertia:12.5" in capsys.readouterr().out

    a = S.parse_arguments([])
    assert (a.k, a.batch_size, a.iters) == (4096, 2 ** 14, 100)
    assert inspect.signature(S.fit).parameters["batch_size"].default == 2 ** 14
    assert inspect.signature(S.fit).parameters["epochs"].default == 100
