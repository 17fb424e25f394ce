"""Times BarlowTwinsLoss forward + backward in bf16 at the pre-training shape (2048 lines x 256 positions, D = 4096, all-ones masks):
each kernel of csrc/barlow.hip alone with the bytes it moves (from the shapes) and TB/s beside the 6.3 TB/s copy ceiling, the three
products, and VICRegLoss forward + backward on the same tensors in the same process.  Everything is warmed up; three alternating rounds of
device-event windows of about 0.3 s each; one JSON line.  --lines / --positions / --dim shrink it for a rehearsal."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pero_pretraining_amd as P  # noqa: E402
from pero_pretraining_amd import ops  # noqa: E402
from pero_pretraining_amd.joint_embedding_pretraining.losses import BarlowTwinsLoss, VICRegLoss  # noqa: E402

COPY_CEILING = 6.3e12   # bytes / s: what a device copy reaches on an MI355X


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds(fns, window_ms=300.0, n_rounds=3):
    """name -> [ms per call] over n_rounds alternating rounds; every function is warmed up and sized to a window first."""
    reps = {}
    for name, fn in fns.items():
        fn()
        reps[name] = max(3, min(500, int(window_ms / max(timed(fn, 2), 0.01))))
    out = {name: [] for name in fns}
    for _ in range(n_rounds):
        for name, fn in fns.items():
            out[name].append(timed(fn, reps[name]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=2048)
    ap.add_argument("--positions", type=int, default=256)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "barlow_time.py measures on the GPU; there is nothing to time without one"
    N, S, D = a.lines, a.positions, a.dim
    dt, es = torch.bfloat16, 2
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((N, S, D), device="cuda", dtype=dt, generator=g)
    y = (x + 0.3 * torch.randn((N, S, D), device="cuda", dtype=dt, generator=g)).requires_grad_(True)
    x.requires_grad_(True)
    ones = np.ones((N, S), np.uint8)
    n = N * S
    n_pad = ((n + 63) // 64) * 64
    x2, y2 = x.detach().view(n, D), y.detach().view(n, D)
    ix = torch.arange(n, device="cuda")
    iy = ix.clone()

    # ---- the kernels of the family, one at a time, on the tensors the loss would hand them
    mean, rstd = ops.barlow_stats(x2, ix, y2, iy, 1e-5)
    zh = ops.barlow_standardize(x2, ix, y2, iy, mean, rstd, n_pad)
    c = ops.zeros((D, D), x.device, torch.float32)

    def corr_gemm():
        cz = ops.zeros((D, D), x.device, torch.float32)
        ops.gemm(zh[0], zh[1], out=cz, trans_a=True, trans_b=True, alpha=1.0 / n, atomic=True, k_split=0)

    c.zero_()
    ops.gemm(zh[0], zh[1], out=c, trans_a=True, trans_b=True, alpha=1.0 / n, atomic=True, k_split=0)
    out, G = ops.barlow_corr(c, n, 0.0051, dt)
    dzh = torch.empty_like(zh)
    ops.gemm(zh[1], G, out=dzh[0])
    ops.gemm(zh[0], G, out=dzh[1], trans_b=True)
    ab = ops.barlow_bwd_stats(dzh, zh, n)
    dxy = ops.zeros((2 * n, D), x.device, dt)
    gdev = torch.ones(1, device="cuda")
    tiles = -(-n // ops.BARLOW_TILE_ROWS)
    part_bytes = 4 * tiles * D * 4
    kernels = {
        "barlow_stats": (lambda: ops.barlow_stats(x2, ix, y2, iy, 1e-5), 2 * n * D * es + 2 * n * 8 + 2 * part_bytes + 4 * D * 4),
        "barlow_standardize": (lambda: ops.barlow_standardize(x2, ix, y2, iy, mean, rstd, n_pad), 2 * n * D * es + 2 * n_pad * D * es + 2 * n * 8),
        "barlow_corr": (lambda: ops.barlow_corr(c, n, 0.0051, dt), D * D * 4 + D * D * es + 4 * D * 4),
        "barlow_bwd_stats": (lambda: ops.barlow_bwd_stats(dzh, zh, n), 4 * n * D * es + 2 * part_bytes + 4 * D * 4),
        "barlow_standardize_bwd": (lambda: ops.barlow_standardize_bwd(dzh, zh, rstd, ab[0], ab[1], ix, iy, dxy[:n], dxy[n:], gdev),
                                   4 * n * D * es + 2 * n * D * es + 2 * n * 8),
        "zero_fill_of_the_gradients": (lambda: ops.zeros((2 * n, D), x.device, dt), 2 * n * D * es),
    }
    products = {
        "c = zh1^T zh2 / n (with the zero fill of c)": (corr_gemm, 2.0 * D * D * n_pad),
        "d zh1 = zh2 G^T": (lambda: ops.gemm(zh[1], G, out=dzh[0]), 2.0 * n_pad * D * D),
        "d zh2 = zh1 G": (lambda: ops.gemm(zh[0], G, out=dzh[1], trans_b=True), 2.0 * n_pad * D * D),
    }
    kt = rounds({k: f for k, (f, _) in kernels.items()})
    pt = rounds({k: f for k, (f, _) in products.items()})
    del zh, dzh, dxy, c, G
    torch.cuda.empty_cache()

    # ---- the two losses, forward + backward, on the same tensors
    def step(loss):
        def run():
            x.grad = y.grad = None
            with P.autocast(True):
                res = loss(x, y, ones, ones, ones, ones)
            res["loss"].backward()
        return run

    lt = rounds({"BarlowTwinsLoss": step(BarlowTwinsLoss()), "VICRegLoss": step(VICRegLoss())}, window_ms=600.0)
    rec = {"lines": N, "positions": S, "D": D, "dtype": str(dt), "pairs": n, "row_tiles": tiles, "copy_ceiling_TBps": COPY_CEILING / 1e12,
           "kernels": {k: {"ms": kt[k], "bytes": b, "TBps": b / min(kt[k]) / 1e9, "share_of_copy_ceiling": b / (min(kt[k]) * 1e-3) / COPY_CEILING}
                       for k, (_, b) in kernels.items()},
           "products": {k: {"ms": pt[k], "flop": f, "TFLOPs": f / min(pt[k]) / 1e9} for k, (_, f) in products.items()},
           "loss_fwd_bwd_ms": lt,
           "sum_of_barlow_kernels_ms": sum(min(v) for v in kt.values()), "sum_of_products_ms": sum(min(v) for v in pt.values())}
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
