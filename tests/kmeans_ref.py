"""f64 restatements shared by test_kmeans_cpu.py and test_gpu_kmeans.py (not a test module)."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_kmeans.npz")
K, D, B, STEPS = 128, 32, 1024, 6


def make_data():
    """The g23 rows (tools/make_golden_kmeans.py make_data): (6144, 32) f32 rows and the 128 init row numbers."""
    rng = np.random.default_rng(7)
    blob = 2.0 * rng.standard_normal((K, D))
    rows = blob[rng.integers(0, K, STEPS * B)] + 0.7 * rng.standard_normal((STEPS * B, D))
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    return rows, np.sort(rng.choice(STEPS * B, K, replace=False))


def load_g23():
    """The fixture plus `x`: the rows, regenerated from the recipe and checked against the stored SHA-256."""
    z = np.load(GOLDEN, allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["x"], init_rows = make_data()
    digest = np.frombuffer(hashlib.sha256(g["x"].tobytes()).digest(), dtype=np.uint8)
    assert np.array_equal(digest, g["rows_sha256"]) and np.array_equal(init_rows, g["init_rows"]), \
        "numpy no longer regenerates the g23 rows: rerun tools/make_golden_kmeans.py"
    return g


def sqdist(x, c):
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def potential(x, c):
    """sum over the rows of the squared distance to the nearest centre, f64."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    d = (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)   # f64: the expansion costs ~1e-13 here
    return float(np.maximum(d, 0.0).min(1).sum())


def update_f64(x, labels, centers, counts):
    """sklearn _minibatch_update_dense in f64: -> (centers, counts, member mask)."""
    x, centers, counts = np.asarray(x, dtype=np.float64), np.asarray(centers, dtype=np.float64).copy(), np.asarray(counts, dtype=np.float64)
    k = centers.shape[0]
    n = np.bincount(labels, minlength=k).astype(np.float64)
    sums = np.zeros_like(centers)
    np.add.at(sums, labels, x)
    hit = n > 0
    centers[hit] = (centers[hit] * counts[hit, None] + sums[hit]) / (counts[hit] + n[hit])[:, None]
    return centers, counts + n, hit


def restate_steps(rows, init):
    """The six mini-batch steps of g23 in f64: labels, batch inertia, centres, counts per step and the smallest
    relative best / runner-up margin."""
    centers, counts = np.asarray(init, dtype=np.float64).copy(), np.zeros(K)
    labels, inertia, cs, ns, margin = [], [], [], [], np.inf
    for s in range(STEPS):
        x = rows[s * B:(s + 1) * B]
        d = sqdist(x, centers)
        lab = d.argmin(1)
        two = np.partition(d, 1, axis=1)[:, :2]
        with np.errstate(divide="ignore"):
            margin = min(margin, float(((two[:, 1] - two[:, 0]) / two[:, 0]).min()))
        centers, counts, _ = update_f64(x, lab, centers, counts)
        labels.append(lab)
        inertia.append(d.min(1).sum())
        cs.append(centers.copy())
        ns.append(counts.copy())
    return np.array(labels), np.array(inertia), np.array(cs), np.array(ns), margin
