"""Feature-Quantization centroids on the device - the step between feature production and label production
(scripts/fit_kmeans.py, which calls sklearn `MiniBatchKMeans(n_clusters=4096, init="k-means++", batch_size=2**14,
max_iter=100, n_init=10)` on the host).

`MiniBatchKMeans` keeps sklearn's constructor arguments, defaults, fitted attributes and algorithm; the feature
matrix stays resident on the GPU and every step runs in the HIP kernels:

    mini-batch      `torch.randint` indices (with replacement) -> `ops.gather_rows`
    labels/inertia  `ops.vq_argmin` (exact f32, the kernel that later produces the labels) + `ops.sum_scale`
    centre update   `ops.kmeans_update`   (stable sort of the labels + fixed-order segmented sums, no float atomics)
    seeding         `ops.kmeans_pp_step`  (greedy k-means++, 2 + int(ln K) trials per centre, no device->host copy)
    early stopping  `ops.kmeans_converge` (sklearn's EWA-inertia rule, state on the device)

Draw-for-draw equality with sklearn's `RandomState` is not a goal (the draws come from a `torch.Generator` on the
device); the arithmetic of a step is sklearn's.  The same `random_state` gives the same bits from run to run.

Fitted arrays (`cluster_centers_` (K, D) f32, `labels_` int64, `_counts` (K) f64) are device tensors, so that
features -> fit -> labels (`scripts.labels.compute_features` / `compute_kmeans_labels`) never leaves the GPU.
`sample_weight` and sparse input are not supported (ValueError)."""
import argparse
import math
import pickle

import numpy as np
import torch

from .. import ops

_LABEL_CHUNK = 1 << 18   # rows per call of the final labelling pass


def _is_sparse(X):
    return hasattr(X, "tocsr") or (isinstance(X, torch.Tensor) and X.layout != torch.strided)


class MiniBatchKMeans:
    """sklearn.cluster.MiniBatchKMeans on the GPU (dense f32 input, no sample weights).

    Early stopping: the EWA of the batch inertia, its minimum, the no-improvement counter and the stop flag live on
    the device; the host reads the flag every `poll_every` steps (default 64) instead of synchronising every step.
    Stopping can therefore come up to `poll_every - 1` steps later than sklearn's rule would stop, and `n_steps_`
    counts the steps actually taken."""

    def __init__(self, n_clusters=8, *, init="k-means++", max_iter=100, batch_size=1024, verbose=0, compute_labels=True,
                 random_state=None, tol=0.0, max_no_improvement=10, init_size=None, n_init="auto", reassignment_ratio=0.01,
                 poll_every=64, device=None):
        self.n_clusters = n_clusters
        self.init = init
        self.max_iter = max_iter
        self.batch_size = batch_size
        self.verbose = verbose
        self.compute_labels = compute_labels
        self.random_state = random_state
        self.tol = tol
        self.max_no_improvement = max_no_improvement
        self.init_size = init_size
        self.n_init = n_init
        self.reassignment_ratio = reassignment_ratio
        self.poll_every = poll_every
        self.device = device

    def get_params(self, deep=True):
        names = ("n_clusters", "init", "max_iter", "batch_size", "verbose", "compute_labels", "random_state", "tol",
                 "max_no_improvement", "init_size", "n_init", "reassignment_ratio")
        return {n: getattr(self, n) for n in names}

    # ---- input / parameter checks ---------------------------------------------------------------------------------
    def _device(self):
        return torch.device(self.device if self.device is not None else "cuda")

    def _check_X(self, X, sample_weight=None):
        if sample_weight is not None:
            raise ValueError("MiniBatchKMeans (GPU): sample_weight is not supported")
        if _is_sparse(X):
            raise ValueError("MiniBatchKMeans (GPU): sparse input is not supported")
        if not isinstance(X, torch.Tensor):
            X = torch.from_numpy(np.ascontiguousarray(np.asarray(X), dtype=np.float32))
        if X.dim() != 2:
            raise ValueError(f"expected a 2-D array, got {tuple(X.shape)}")
        if not X.is_cuda:
            X = X.to(self._device())   # uploaded once
        return X.float().contiguous()

    def _check_params(self, X):
        n = X.shape[0]
        if self.n_clusters < 1 or (n < self.n_clusters and not hasattr(self, "cluster_centers_")):
            raise ValueError(f"n_samples={n} should be >= n_clusters={self.n_clusters}")
        if self.max_iter < 1 or self.batch_size < 1 or self.poll_every < 1:
            raise ValueError("max_iter, batch_size and poll_every must be >= 1")
        if isinstance(self.init, str) and self.init not in ("k-means++", "random"):
            raise ValueError(f"init should be 'k-means++', 'random' or an array, got {self.init!r}")
        self._batch_size = min(self.batch_size, n)
        init_size = self.init_size if self.init_size is not None else 3 * self._batch_size
        if init_size < self.n_clusters:
            init_size = 3 * self.n_clusters
        self._init_size = min(init_size, n)
        if isinstance(self.init, str):
            self._n_init = (3 if self.init == "random" else 1) if self.n_init == "auto" else int(self.n_init)
        else:
            self._n_init = 1
        if not hasattr(self, "_gen"):
            self._gen = torch.Generator(device=X.device)
            if self.random_state is None:
                self._gen.seed()
            else:
                self._gen.manual_seed(int(self.random_state))

    # ---- seeding ---------------------------------------------------------------------------------------------------
    def _kmeans_plusplus(self, X):
        """Greedy k-means++ over the rows of X: (K) int64 row indices on the device, no device->host copy."""
        n, K, dev = X.shape[0], self.n_clusters, X.device
        t = 2 + int(math.log(K))
        sqn = ops.kmeans_sqnorm(X)
        closest = torch.full((n,), float("inf"), device=dev, dtype=torch.float32)
        indices = torch.empty(K, device=dev, dtype=torch.int64)
        pot = torch.empty(1, device=dev, dtype=torch.float64)
        work = ops.kmeans_pp_workspace(n, t, dev)
        first = torch.randint(0, n, (1,), device=dev, generator=self._gen)
        ops.kmeans_pp_step(X, sqn, closest, first, indices[0:1], pot, work)
        for c in range(1, K):
            # candidates with probability proportional to closest_dist_sq (rows already chosen have distance 0)
            cum = torch.cumsum(closest, 0, dtype=torch.float64)
            r = torch.rand(t, device=dev, dtype=torch.float64, generator=self._gen) * cum[-1]
            cand = torch.searchsorted(cum, r, right=True).clamp_(max=n - 1)
            ops.kmeans_pp_step(X, sqn, closest, cand, indices[c:c + 1], pot, work)
        return indices

    def _init_centroids(self, X):
        n, K = X.shape[0], self.n_clusters
        if not isinstance(self.init, str):
            init = self.init
            if not isinstance(init, torch.Tensor):
                init = torch.from_numpy(np.ascontiguousarray(np.asarray(init), dtype=np.float32))
            if tuple(init.shape) != (K, X.shape[1]):
                raise ValueError(f"init has shape {tuple(init.shape)}, expected {(K, X.shape[1])}")
            return init.to(X.device).float().contiguous().clone()
        if self._init_size < n:
            X = ops.gather_rows(X, torch.randint(0, n, (self._init_size,), device=X.device, generator=self._gen))
            n = self._init_size
        if self.init == "k-means++":
            self._init_indices = self._kmeans_plusplus(X)
        else:
            self._init_indices = torch.randperm(n, device=X.device, generator=self._gen)[:K].contiguous()
        return ops.gather_rows(X, self._init_indices)

    def _reset(self, centers):
        dev = centers.device
        self.cluster_centers_ = centers
        self._counts = torch.zeros(self.n_clusters, device=dev, dtype=torch.float64)
        self._n_since_last_reassign = torch.zeros((), device=dev, dtype=torch.int64)
        self._shift = torch.zeros(1, device=dev, dtype=torch.float32)
        self._state = torch.zeros(6, device=dev, dtype=torch.float64)
        self.n_steps_ = 0

    # ---- one step --------------------------------------------------------------------------------------------------
    def _random_reassign(self):
        """sklearn's rule, as a device flag: a count is 0, or 10 * n_clusters samples have passed since the last one."""
        self._n_since_last_reassign = self._n_since_last_reassign + self._batch_size
        do = (self._counts == 0).any() | (self._n_since_last_reassign >= 10 * self.n_clusters)
        self._n_since_last_reassign = torch.where(do, torch.zeros_like(self._n_since_last_reassign), self._n_since_last_reassign)
        return do

    def _reassign(self, xb, do):
        """Replace the centres with weight_sums < ratio * max by distinct rows of the batch - at most B / 2 of them, the
        lightest first - and set their weights to the minimum of the untouched ones.  Fixed shapes, no host sync."""
        B, K = xb.shape[0], self.n_clusters
        W, C = self._counts, self.cluster_centers_
        to = W < self.reassignment_ratio * W.max()
        if do is not True:
            to = to & do
        rank = torch.empty(K, device=W.device, dtype=torch.int64)
        rank[torch.argsort(W, stable=True)] = torch.arange(K, device=W.device)
        to = to & (rank < int(0.5 * B))
        slot = (torch.cumsum(to, 0) - 1).clamp_(min=0, max=B - 1)
        perm = torch.randperm(B, device=W.device, generator=self._gen)
        rows = ops.gather_rows(xb, perm[slot].contiguous())
        C.copy_(torch.where(to[:, None], rows, C))
        min_untouched = torch.where(to, torch.full_like(W, float("inf")), W).min()
        W.copy_(torch.where(to, min_untouched, W))
        self._reassigned = to

    def _mini_batch_step(self, xb, random_reassign=False):
        """labels + inertia against the current centres, centre update, optional reassignment.  `random_reassign` is
        False, True (forced) or a device bool scalar.  Returns the (1,) f32 batch inertia (a device tensor)."""
        C = self.cluster_centers_
        labels, best = ops.vq_argmin(xb, C, want_dist=True)
        inertia = ops.sum_scale(best)
        reassign = random_reassign is not False and self.reassignment_ratio > 0
        old = C.clone() if (reassign and self.tol > 0.0) else None
        ops.kmeans_update(xb, labels, C, self._counts, self._shift)
        if reassign:
            self._reassign(xb, random_reassign)
            if old is not None:   # sklearn's tol sees the reassignment jumps too
                self._shift.copy_(((C - old) ** 2).sum().reshape(1))
        return inertia

    def _labels_inertia(self, X):
        C = self.cluster_centers_
        labels = torch.empty(X.shape[0], device=X.device, dtype=torch.int64)
        total = torch.zeros(1, device=X.device, dtype=torch.float64)
        for s in range(0, X.shape[0], _LABEL_CHUNK):
            idx, best = ops.vq_argmin(X[s:s + _LABEL_CHUNK], C, want_dist=True)
            labels[s:s + _LABEL_CHUNK] = idx
            total += ops.sum_scale(best).double()
        return labels, total

    # ---- public interface ------------------------------------------------------------------------------------------
    def fit(self, X, y=None, sample_weight=None):
        X = self._check_X(X, sample_weight)
        self._check_params(X)
        N, B, dev = X.shape[0], self._batch_size, X.device
        tol = float(self.tol) * float(X.var(dim=0, unbiased=False).mean()) if self.tol > 0.0 else 0.0

        best_centers, best_inertia = None, None
        if self._n_init > 1:
            X_valid = ops.gather_rows(X, torch.randint(0, N, (self._init_size,), device=dev, generator=self._gen))
        for _ in range(self._n_init):
            centers = self._init_centroids(X)
            if self._n_init == 1:
                best_centers = centers
                break
            _, dist = ops.vq_argmin(X_valid, centers, want_dist=True)
            inertia = float(ops.sum_scale(dist))
            if self.verbose:
                print(f"Inertia for init: {inertia}")
            if best_inertia is None or inertia < best_inertia:
                best_centers, best_inertia = centers, inertia
        self._reset(best_centers)

        n_steps = (self.max_iter * N) // B
        steps = 0
        for i in range(n_steps):
            xb = ops.gather_rows(X, torch.randint(0, N, (B,), device=dev, generator=self._gen))
            inertia = self._mini_batch_step(xb, self._random_reassign() if self.reassignment_ratio > 0 else False)
            ops.kmeans_converge(inertia, self._shift, self._state, N, B, tol, self.max_no_improvement)
            steps = i + 1
            if steps % self.poll_every == 0 and float(self._state[3]) != 0.0:
                if self.verbose:
                    print(f"Converged at step {int(self._state[5])}/{n_steps}, stopped at step {steps}")
                break
        self.n_steps_ = steps
        self.n_iter_ = int(math.ceil(steps * B / N))
        if self.compute_labels:
            self.labels_, total = self._labels_inertia(X)
            self.inertia_ = float(total)
        else:
            self.inertia_ = float(self._state[0]) * N
        return self

    def partial_fit(self, X, y=None, sample_weight=None):
        X = self._check_X(X, sample_weight)
        has_centers = hasattr(self, "cluster_centers_")
        self._check_params(X)
        if not has_centers:
            self._reset(self._init_centroids(X))
        self._mini_batch_step(X, self._random_reassign() if self.reassignment_ratio > 0 else False)
        self.n_steps_ += 1
        if self.compute_labels:
            self.labels_, total = self._labels_inertia(X)
            self.inertia_ = float(total)
        return self

    def predict(self, X):
        if not hasattr(self, "cluster_centers_"):
            raise RuntimeError("this MiniBatchKMeans instance is not fitted yet")
        return self._labels_inertia(self._check_X(X))[0]


# ---- scripts/fit_kmeans.py ----------------------------------------------------------------------------------------
def load_pickle(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--dataset", help="Path to a file with the pickled features")
    parser.add_argument("--k", help="Number of clusters ('K'-means).", default=4096, required=False, type=int)
    parser.add_argument("--batch-size", help="Batch size.", default=2 ** 14, required=False, type=int)
    parser.add_argument("--iters", help="Number of iterations over dataset (epochs).", default=100, required=False, type=int)
    parser.add_argument("--output", help="Path to the output file (.npy of the (K, D) centroids).")
    return parser.parse_args(argv)


def fit(dataset_file, k, batch_size=2 ** 14, epochs=100):
    kmeans = MiniBatchKMeans(n_clusters=k, init="k-means++", batch_size=batch_size, max_iter=epochs, n_init=10)

    vectors = load_pickle(dataset_file)
    print(f"Loaded '{dataset_file}' ({len(vectors)})")

    np.random.shuffle(vectors)
    print("Shuffled")

    kmeans = kmeans.fit(vectors)
    print(f"Inertia:{kmeans.inertia_}")

    return kmeans


def save_centroids(kmeans, path):
    """The (K, D) f32 array that produce_kmeans_labels.py reads with `np.load` and `compute_kmeans_labels` takes."""
    centers = kmeans.cluster_centers_
    centers = centers.detach().cpu().numpy() if isinstance(centers, torch.Tensor) else np.asarray(centers)
    with open(path, "wb") as f:   # an open file: np.save must not append ".npy" to the name the user gave
        np.save(f, np.ascontiguousarray(centers, dtype=np.float32))


def main(argv=None):
    args = parse_arguments(argv)

    k_means = fit(args.dataset, args.k, batch_size=args.batch_size, epochs=args.iters)
    print("K-means trained")

    save_centroids(k_means, args.output)
    print(f"K-means centroids saved to '{args.output}'")

    return 0


if __name__ == "__main__":
    exit(main())
