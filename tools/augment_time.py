"""Time the augmenting collation kernel on one GPU, in ONE process: pero_augment_stack_lines with a LineAugmenter's default draw, and
with the neutral values, beside pero_stack_lines on the same ragged upload - the yardstick: the same bytes in and out, a copy where the
augmenting form samples, recolours and hashes.  Everything is warmed up, then timed with device events in alternating windows
(DESIGN.md section 14 quotes the result).  The neutral run is also compared with pero_stack_lines bit for bit.

    python tools/augment_time.py [--lines 2048 --height 40 --width 2048 --channels 3 --iters 10 --rounds 5]
                                 [--only augment|augment_neutral|stack_lines]    (one kernel alone, for a profiler's kernel trace)

Prints one JSON line: milliseconds (median and range over the rounds) and the bytes written per second."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v, nbytes):
    med = statistics.median(v)
    return {"median_ms": round(med, 4), "range_ms": [round(min(v), 4), round(max(v), 4)], "written_TB_per_s": round(nbytes / med / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=2048)
    ap.add_argument("--height", type=int, default=40)
    ap.add_argument("--width", type=int, default=2048, help="padded width; line widths are drawn in [width / 2, width]")
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-ms", type=float, default=136.0, help="the training step the share is quoted against")
    ap.add_argument("--only", choices=["augment", "augment_neutral", "stack_lines"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_time.py needs a GPU: a timing taken anywhere else says nothing")
    from pero_pretraining_amd import ops
    from pero_pretraining_amd.common.augment import LineAugmenter, neutral
    B, H, Wt, C = a.lines, a.height, a.width, a.channels
    rng = np.random.default_rng(0)
    widths = rng.integers(Wt // 2, Wt + 1, B)
    left = np.array([rng.integers(0, Wt - w + 1) for w in widths])
    sizes = widths * H * C
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    packed = torch.from_numpy(rng.integers(0, 256, int(sizes.sum()) + 8, dtype=np.uint8)).cuda()
    off_d, w_d, left_d = torch.from_numpy(offsets).cuda(), torch.from_numpy(widths).int().cuda(), torch.from_numpy(left).int().cuda()
    aug = LineAugmenter(seed=0, p=1.0)
    drawn = [t.cuda() for t in aug.draw(widths.tolist(), H, Wt, C)]
    plain = [t.cuda() for t in neutral(B, Wt, C, aug.knot_shift)]

    kernels = {"augment": lambda: ops.augment_stack_lines(packed, off_d, w_d, left_d, *drawn, B, H, Wt, C, aug.knot_shift),
               "augment_neutral": lambda: ops.augment_stack_lines(packed, off_d, w_d, left_d, *plain, B, H, Wt, C, aug.knot_shift),
               "stack_lines": lambda: ops.stack_lines(packed, off_d, w_d, left_d, B, H, Wt, C)}
    if a.only is not None:
        kernels = {a.only: kernels[a.only]}

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for fn in kernels.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in kernels}
    for _ in range(a.rounds):
        for name, fn in kernels.items():
            times[name].append(window(fn))
    nbytes = B * H * Wt * C
    out = {"lines": B, "height": H, "width": Wt, "channels": C, "ragged_bytes": int(sizes.sum()), "batch_bytes": nbytes}
    out.update({name: summary(v, nbytes) for name, v in times.items()})
    if "augment" in times:
        out["augment_share_of_step"] = round(statistics.median(times["augment"]) / a.step_ms, 4)
    if "augment_neutral" in kernels and "stack_lines" in kernels:
        out["neutral_bit_equal"] = bool(torch.equal(kernels["augment_neutral"](), kernels["stack_lines"]()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
