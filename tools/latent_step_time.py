"""Time the latent-target step beside the masked step on one GPU, in ONE process, in bf16 at the shapes of BASELINE.json configs[1]
(12 layers, d 512, 40 x 2048 lines; the masked model with head_rows = "masked"), and the three kernel families of csrc/latent.hip alone
at the step's shapes.  Everything is warmed up, then the two steps are timed in alternating windows with a device synchronise behind
each (DESIGN.md section 19 quotes the result).  The expectation to check, not asserted: latent step = masked step + one no-grad forward
+ under 1 ms for the three kernel families.

    python tools/latent_step_time.py [--lines 2048 --steps 20 --warmup 5 --rounds 2 --top-k 8 --masking-prob 0.15]

Prints one JSON line: step times in milliseconds (median and range over the windows), the kernels' times, their bytes and bytes per second."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(num_blocks=12, model_dim=512, num_heads=4, feedforward_dim=2048, vocab=4096, width=2048, height=40, patch=8, channels=3)


def summary(v):
    return {"median_ms": round(statistics.median(v), 3), "range_ms": [round(min(v), 3), round(max(v), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per model, split over the rounds")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--top-k", type=int, default=8)
    ap.add_argument("--masking-prob", type=float, default=0.15)
    ap.add_argument("--kernel-iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latent_step_time.py needs a GPU: a timing taken anywhere else says nothing")
    from pero_pretraining_amd import ops
    from pero_pretraining_amd.latent_pretraining import model as LM
    from pero_pretraining_amd.latent_pretraining.trainer import Trainer as LatentTrainer
    from pero_pretraining_amd.masked_pretraining import model as MM
    from pero_pretraining_amd.masked_pretraining.trainer import Trainer as MaskedTrainer
    from pero_pretraining_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    bdef = {"type": "vit", "num_blocks": CFG["num_blocks"], "model_dim": CFG["model_dim"], "num_heads": CFG["num_heads"],
            "feedforward_dim": CFG["feedforward_dim"]}
    d, B, S = CFG["model_dim"], a.lines, CFG["width"] // CFG["patch"]
    torch.manual_seed(0)
    masked = MM.MaskedTransformerEncoder(MM.init_backbone(dict(bdef)), MM.init_head({"in_features": d, "out_features": CFG["vocab"]})).to(dev).train()
    masked.head_rows = "masked"
    torch.manual_seed(0)
    latent = LM.LatentTargetTransformerEncoder(LM.init_backbone(dict(bdef)), LM.init_head({"in_features": d, "out_features": d}),
                                               top_k=a.top_k).to(dev).train()
    mtrainer = MaskedTrainer(None, masked, None, FusedAdam(masked.parameters(), lr=2e-4), None, bfloat16=True)
    ltrainer = LatentTrainer(None, latent, None, FusedAdam(latent.parameters(), lr=2e-4), None, bfloat16=True)
    rng = np.random.default_rng(1234)
    images = torch.from_numpy(rng.integers(0, 256, (B, CFG["height"], CFG["width"], CFG["channels"]), dtype=np.uint8)).to(dev)
    labels = torch.from_numpy(rng.integers(0, CFG["vocab"], (B, S)).astype(np.int64)).to(dev)
    mask = (rng.random((B, S)) < a.masking_prob).astype(np.int64)      # a host array: the row list costs no sync in either model

    steps = {"masked_step": lambda: mtrainer.train_step_prepared(images, labels, mask),
             "latent_step": lambda: ltrainer.train_step_prepared(images, None, mask)}

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for fn in steps.values():
        window(fn, a.warmup)
    per = max(1, a.steps // a.rounds)
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for name, fn in steps.items():
            times[name].append(window(fn, per))
    out = {"lines": B, "positions": S, "dtype": "bf16", "top_k": min(a.top_k, CFG["num_blocks"]), "masked_rows": int(mask.sum()),
           "timed_steps_per_model": per * a.rounds}
    out.update({k: summary(v) for k, v in times.items()})

    # the teacher's no-grad forward alone (what the latent step adds beside the three kernels)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        fwd = lambda: latent.teacher.encode_layers(images, latent.tap_layers())   # noqa: E731
        window(fwd, 2)
        out["teacher_forward"] = summary([window(fwd, 5) for _ in range(a.rounds)])

    # the three kernel families alone, at the step's shapes, with device events
    def kernel_ms(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.kernel_iters

    ema = latent.ema
    ema.update()
    n_params = sum(p.numel() for p in ema.module.parameters())
    k = out["top_k"]
    index = torch.from_numpy(np.flatnonzero(mask.reshape(-1) == 1)).to(dev)
    n = index.numel()
    n_pad = ((n + 255) // 256) * 256
    taps = [torch.randn(B * S, d, device=dev).bfloat16() for _ in range(k)]
    y = ops.latent_targets(taps, index, n_pad)
    pred = torch.randn(n_pad, d, device=dev).bfloat16()
    one = torch.ones(1, device=dev)
    kernels = {
        # reads p and a, writes a and its bf16 copy
        "ema_update": (lambda: ops.ema_update(ema._flat, ema._table, ema._tiles, 1e-3, ema._flat_bf16), n_params * (4 + 4 + 4 + 2)),
        # reads K bf16 rows per listed position, writes one f32 row per padded position
        "latent_targets": (lambda: ops.latent_targets(taps, index, n_pad), n * d * 2 * k + n_pad * d * 4),
        # reads bf16 predictions and f32 targets of the listed rows
        "latent_loss_fwd": (lambda: ops.latent_loss_fwd(pred, y, n, 2.0), n * d * (2 + 4)),
        # the same reads, writes bf16 gradients of every padded row
        "latent_loss_bwd": (lambda: ops.latent_loss_bwd(pred, y, n, 2.0, one), n * d * (2 + 4) + n_pad * d * 2),
    }
    total = 0.0
    for name, (fn, nbytes) in kernels.items():
        ms = kernel_ms(fn)
        total += ms
        out[name] = {"ms": round(ms, 4), "bytes": int(nbytes), "TB_per_s": round(nbytes / ms / 1e9, 3)}
    out["latent_kernels_ms"] = round(total, 4)
    out["latent_minus_masked_ms"] = round(out["latent_step"]["median_ms"] - out["masked_step"]["median_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
