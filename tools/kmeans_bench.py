#!/usr/bin/env python3
"""Times the GPU mini-batch k-means (scripts/kmeans.py); prints one JSON line per measurement.

  step   one mini-batch step at K = 4096, D = 512, B = 16384 on a resident feature matrix: gather + argmin + update
         (+ the sort of the labels), each part timed with events around `--iters` back-to-back repeats
  fit    a whole `fit` on 2^21 synthetic rows (K = 4096, D = 512, batch 2^14, n_init and max_iter from the command line)
  sklearn  the same fit with scikit-learn on the host CPUs (needs scikit-learn; reduce --max-iter and say so)

A kernel-level split of `step` comes from `rocprofv3 --kernel-trace --stats -- python tools/kmeans_bench.py step`."""
import argparse
import json
import time

import numpy as np
import torch


def synthetic(n, d, k, seed=0, device="cuda"):
    """n rows around k blobs (blob = N(0,1), noise 0.3 N(0,1)), generated on the device in chunks."""
    gen = torch.Generator(device=device).manual_seed(seed)
    blobs = torch.randn(k, d, device=device, generator=gen)
    x = torch.empty(n, d, device=device)
    for s in range(0, n, 1 << 18):
        e = min(n, s + (1 << 18))
        x[s:e] = blobs[torch.randint(0, k, (e - s,), device=device, generator=gen)]
        x[s:e] += 0.3 * torch.randn(e - s, d, device=device, generator=gen)
    return x


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def bench_step(args):
    from pero_pretraining_amd import ops
    K, D, B, N = args.k, args.d, args.batch_size, args.rows
    x = synthetic(N, D, K)
    gen = torch.Generator(device="cuda").manual_seed(1)
    centers = ops.gather_rows(x, torch.randint(0, N, (K,), device="cuda", generator=gen))
    weights = torch.zeros(K, device="cuda", dtype=torch.float64)
    idx = torch.randint(0, N, (B,), device="cuda", generator=gen)
    xb = ops.gather_rows(x, idx)
    labels = ops.vq_argmin(xb, centers)

    def step():
        b = ops.gather_rows(x, idx)
        lab, best = ops.vq_argmin(b, centers, want_dist=True)
        ops.sum_scale(best)
        ops.kmeans_update(b, lab, centers, weights)

    res = {"bench": "kmeans_step", "K": K, "D": D, "B": B, "rows": N,
           "gather_ms": timed(lambda: ops.gather_rows(x, idx), args.iters),
           "argmin_ms": timed(lambda: ops.vq_argmin(xb, centers, want_dist=True), args.iters),
           "sort_ms": timed(lambda: torch.sort(labels, stable=True), args.iters),
           "update_ms": timed(lambda: ops.kmeans_update(xb, labels, centers.clone(), weights.clone()), args.iters),
           "clone_ms": timed(lambda: (centers.clone(), weights.clone()), args.iters),
           "step_ms": timed(step, args.iters)}
    print(json.dumps(res))


def bench_fit(args):
    from pero_pretraining_amd.scripts.kmeans import MiniBatchKMeans
    x = synthetic(args.rows, args.d, args.k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = MiniBatchKMeans(n_clusters=args.k, init="k-means++", batch_size=args.batch_size, max_iter=args.max_iter, n_init=args.n_init,
                        random_state=0).fit(x)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"bench": "kmeans_fit", "K": args.k, "D": args.d, "B": args.batch_size, "rows": args.rows, "max_iter": args.max_iter,
                      "n_init": args.n_init, "seconds": dt, "n_steps": m.n_steps_, "inertia": m.inertia_}))


def bench_sklearn(args):
    from sklearn.cluster import MiniBatchKMeans
    x = synthetic(args.rows, args.d, args.k, device="cpu").numpy()
    t0 = time.perf_counter()
    m = MiniBatchKMeans(n_clusters=args.k, init="k-means++", batch_size=args.batch_size, max_iter=args.max_iter, n_init=args.n_init,
                        random_state=0).fit(x)
    dt = time.perf_counter() - t0
    print(json.dumps({"bench": "sklearn_fit", "K": args.k, "D": args.d, "B": args.batch_size, "rows": args.rows, "max_iter": args.max_iter,
                      "n_init": args.n_init, "seconds": dt, "n_steps": int(m.n_steps_), "inertia": float(m.inertia_),
                      "threads": torch.get_num_threads()}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=["step", "fit", "sklearn"])
    p.add_argument("--k", type=int, default=4096)
    p.add_argument("--d", type=int, default=512)
    p.add_argument("--batch-size", type=int, default=2 ** 14)
    p.add_argument("--rows", type=int, default=2 ** 21)
    p.add_argument("--max-iter", type=int, default=100)
    p.add_argument("--n-init", type=int, default=10)
    p.add_argument("--iters", type=int, default=20)
    args = p.parse_args()
    {"step": bench_step, "fit": bench_fit, "sklearn": bench_sklearn}[args.what](args)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
