#!/usr/bin/env python3
"""Times NT-Xent forward + backward in bf16 at n lines, D features, S positions per line; prints one JSON line per S.

  a  NTXentLoss() on all-ones masks: every position, products of S x S x D per line (the tile kernel only when S % 128 == 0)
  b  NTXentLoss(apply_masks=True) on all-ones masks: the same arithmetic through the compact blocks of Sp = ceil(S / 128) 128 rows
  c  NTXentLoss(apply_masks=True) on masks as the collator draws them (widths uniform in [max / 3, max], random left paddings)
  rows  pero_ntxent_rows_fwd + pero_ntxent_rows_bwd alone (both views stacked), next to pero_rownorm_fwd + pero_rownorm_bwd

Every configuration: HIP events around `--iters` calls after `--warmup` calls; `--rounds` rounds that alternate the configurations;
median with min ... max over the rounds, and the allocator's peak during one call."""
import argparse
import json
import statistics

import numpy as np
import torch


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def with_twins(masks):
    out = []
    for m in masks:
        t = torch.from_numpy(m).cuda()
        t._pero_host = m
        out.append(t)
    return out


def collated_masks(n, S, seed, sub=8, pad=32):
    from pero_pretraining_amd.common.dataloader import BatchCreator
    rng = np.random.default_rng(seed)
    target = S * sub
    wmax = target - pad
    widths = rng.integers(wmax // 3, wmax + 1, n)
    widths[0] = wmax
    left1 = [int(rng.integers(0, target - w)) // sub for w in widths]
    left2 = [int(rng.integers(0, target - w)) // sub for w in widths]
    return BatchCreator._host_masks(widths.tolist(), left1, widths.tolist(), left2, [0] * n, S, sub)


def summary(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def bench(args, S):
    import pero_pretraining_amd as P
    from pero_pretraining_amd import ops
    from pero_pretraining_amd.joint_embedding_pretraining.losses import NTXentLoss, ntxent_slots_host, ragged_block_rows
    n, D = args.lines, args.dim
    gen = torch.Generator(device="cuda").manual_seed(S)
    xy = torch.randn(2 * n, S, D, device="cuda", generator=gen).bfloat16().requires_grad_(True)
    ones = with_twins([np.ones((n, S), np.uint8)] * 4)
    coll_host = collated_masks(n, S, S)
    coll = with_twins(coll_host)
    plain, ragged = NTXentLoss(), NTXentLoss(apply_masks=True)

    def step(module, masks):
        def fn():
            xy.grad = None
            with P.autocast(True):
                module.forward_stacked(xy, *masks)["loss"].backward()
        return fn

    Sp = ragged_block_rows(S, torch.bfloat16)
    x2 = xy.detach().view(2 * n * S, D)
    slot, count = ops.ntxent_slots(*ones)
    xn_r, inv_r = ops.ntxent_rows_fwd(x2, slot, count, Sp)
    dxn_r = torch.randn_like(xn_r)
    xn_d, inv_d = ops.rownorm_fwd(x2)
    dxn_d = torch.randn_like(xn_d)
    one = torch.ones(1, device="cuda")
    configs = {
        "a": step(plain, ones), "b": step(ragged, ones), "c": step(ragged, coll),
        "rows_ragged": lambda: (ops.ntxent_rows_fwd(x2, slot, count, Sp, out=(xn_r, inv_r)), ops.ntxent_rows_bwd(xn_r, dxn_r, inv_r, slot, count, Sp, one)),
        "rows_dense": lambda: (ops.rownorm_fwd(x2, out=(xn_d, inv_d)), ops.rownorm_bwd(xn_d, dxn_d, inv_d, one)),
    }
    times = {k: [] for k in configs}
    for _ in range(args.rounds):
        for k, fn in configs.items():
            times[k].append(timed(fn, args.iters, args.warmup))
    res = {"bench": "ntxent", "dtype": "bf16", "lines": n, "D": D, "S": S, "Sp": Sp, "iters": args.iters, "rounds": args.rounds,
           "selected_fraction_c": round(float((ntxent_slots_host(*coll_host)[2].sum()) / (n * S)), 3)}
    for k in configs:
        res[k] = summary(times[k])
    for k in ("a", "b", "c"):
        res[k]["peak_mib"] = round(peak_mib(configs[k]), 1)
    res["a_over_b"] = round(res["a"]["median_ms"] / res["b"]["median_ms"], 3)
    res["b_minus_a_ms"] = round(res["b"]["median_ms"] - res["a"]["median_ms"], 3)
    res["allowance_ms"] = round(max(res["a"]["max_ms"] - res["a"]["min_ms"], res["rows_ragged"]["median_ms"]), 3)
    print(json.dumps(res), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lines", type=int, default=512)
    p.add_argument("--dim", type=int, default=4096)
    p.add_argument("--positions", type=int, nargs="+", default=[256, 260])
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args()
    for S in args.positions:
        bench(args, S)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
