#!/usr/bin/env python3
"""Writes tests/golden/g23_kmeans.npz: sklearn references for the GPU mini-batch k-means (scripts/kmeans.py).
Needs scikit-learn (written with 1.7.2); the tests that read the file do not.

(a) step parity.  default_rng(7); K = 128, D = 32, six batches of 1024 rows, rows = blob[randint] + 0.7 N(0,1) with
    blob = 2 N(0,1), as f32; init = 128 distinct rows.  The rows are not stored: the tests regenerate them with the
    same recipe (`tests/kmeans_ref.py make_data`) and compare their SHA-256 with the one stored here.
    sklearn `MiniBatchKMeans(init=init, n_init=1, batch_size=1024, reassignment_ratio=0.0)`: centres and `_counts`
    after each `partial_fit`, next to an f64 restatement of the same steps (labels, batch inertia, centres).
    Asserted here, so that a regenerated file cannot silently hold near-ties: the smallest relative margin between
    the best and the second-best centre of a row is >= 2e-5, and sklearn's f32 centres are within 1e-5 of the f64 ones.
(b) quality references on the same 6144 rows: the `kmeans_plusplus` potential over 16 seeds, the potential of uniform
    seeding over 16 seeds, and the inertia of the full `fit` (batch 1024, max_iter=100, n_init=10) over 8 seeds -
    the samples, not only their moments."""
import hashlib
import os

import numpy as np

K, D, B, STEPS = 128, 32, 1024, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g23_kmeans.npz")


def make_data():
    rng = np.random.default_rng(7)
    blob = 2.0 * rng.standard_normal((K, D))
    rows = blob[rng.integers(0, K, STEPS * B)] + 0.7 * rng.standard_normal((STEPS * B, D))
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    init_rows = np.sort(rng.choice(STEPS * B, K, replace=False))
    return rows, init_rows


def sqdist(x, c):
    """(n, K) squared distances in f64, difference form."""
    x, c = x.astype(np.float64), c.astype(np.float64)
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def restate_steps(rows, init):
    """The mini-batch steps in f64: per step the pre-update labels, the batch inertia, the centres and the counts, and
    the smallest relative best / runner-up margin met."""
    centers, counts = init.astype(np.float64).copy(), np.zeros(K)
    labels, inertia, cs, ns, margin, empty = [], [], [], [], np.inf, 0
    for s in range(STEPS):
        x = rows[s * B:(s + 1) * B].astype(np.float64)
        d = sqdist(x, centers)
        lab = d.argmin(1)
        two = np.partition(d, 1, axis=1)[:, :2]
        with np.errstate(divide="ignore"):   # a row that still is its own centre: distance 0, margin inf
            margin = min(margin, float(((two[:, 1] - two[:, 0]) / two[:, 0]).min()))
        n = np.bincount(lab, minlength=K).astype(np.float64)
        sums = np.zeros((K, D))
        np.add.at(sums, lab, x)
        hit = n > 0
        empty += int((~hit).sum())
        centers[hit] = (centers[hit] * counts[hit, None] + sums[hit]) / (counts[hit] + n[hit])[:, None]
        counts = counts + n
        labels.append(lab)
        inertia.append(d.min(1).sum())
        cs.append(centers.copy())
        ns.append(counts.copy())
    return np.array(labels), np.array(inertia), np.array(cs), np.array(ns), margin, empty


def potential(x, c):
    return float(sqdist(x, c).min(1).sum())


def main():
    from sklearn.cluster import MiniBatchKMeans, kmeans_plusplus

    rows, init_rows = make_data()
    init = rows[init_rows]
    labels, inertia, centers64, counts64, margin, empty = restate_steps(rows, init)

    model = MiniBatchKMeans(n_clusters=K, init=init, n_init=1, batch_size=B, reassignment_ratio=0.0)
    sk_centers, sk_counts = [], []
    for s in range(STEPS):
        model.partial_fit(rows[s * B:(s + 1) * B])
        sk_centers.append(model.cluster_centers_.copy())
        sk_counts.append(model._counts.copy())
    sk_centers, sk_counts = np.array(sk_centers, dtype=np.float32), np.array(sk_counts, dtype=np.float64)
    sk_dist = float(np.abs(sk_centers.astype(np.float64) - centers64).max())
    print(f"margin {margin:.3e}  sklearn-vs-f64 {sk_dist:.3e}  empty-centre events {empty}")
    assert margin >= 2e-5, margin
    assert sk_dist <= 1e-5, sk_dist
    assert np.array_equal(sk_counts, counts64)
    assert empty > 0

    pp = np.array([potential(rows, kmeans_plusplus(rows, K, random_state=s)[0]) for s in range(16)])
    uni = np.array([potential(rows, rows[np.random.default_rng(100 + s).choice(len(rows), K, replace=False)]) for s in range(16)])
    fit = np.array([MiniBatchKMeans(n_clusters=K, init="k-means++", batch_size=B, max_iter=100, n_init=10, random_state=s).fit(rows).inertia_
                    for s in range(8)])
    print(f"k-means++ potential {pp.mean():.0f} +- {pp.std():.0f}   uniform {uni.mean():.0f}   fit inertia {fit.mean():.0f} +- {fit.std():.0f}")
    assert uni.mean() > pp.mean() + 10 * pp.std()

    np.savez_compressed(OUT, rows_sha256=np.frombuffer(hashlib.sha256(rows.tobytes()).digest(), dtype=np.uint8), init_rows=init_rows.astype(np.int32), labels=labels.astype(np.int16), inertia=inertia,
                        centers64=centers64, counts=counts64.astype(np.int32), sk_centers=sk_centers, sk_counts=sk_counts.astype(np.int32),
                        sk_vs_f64=np.float64(sk_dist), margin=np.float64(margin), pp_potential=pp, uniform_potential=uni, fit_inertia=fit)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
