"""Time CTC forced alignment on one GPU, in ONE process: pero_ctc_align with the backpointers in LDS (where the shape allows it) and
forced into the global workspace, beside pero_ctc_fwd on the same logits and strings - the nearest yardstick: the same recursion
shape with expf / logf where the alignment has a max.  Everything is warmed up, then timed with device events in alternating windows
(DESIGN.md "CTC forced alignment" quotes the result).  The two backpointer paths are also compared bit for bit.

    python tools/ctc_align_time.py [--lines 256 --seq 256 --classes 512 --labels 60 --dtype bf16 --iters 20 --rounds 5]
                                   [--only align_lds|align_global|ctc_fwd]    (one kernel family alone, for a profiler's kernel trace)

Prints one JSON line: milliseconds (median and range over the rounds)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "range_ms": [round(min(v), 4), round(max(v), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=256)
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--classes", type=int, default=512)
    ap.add_argument("--labels", type=int, default=60)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=4.0, help="logits = scale * randn")
    ap.add_argument("--only", choices=["align_lds", "align_global", "ctc_fwd"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_time.py needs a GPU: a timing taken anywhere else says nothing")
    from pero_pretraining_amd import ops
    N, S, C = a.lines, a.seq, a.classes
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    gen = torch.Generator().manual_seed(0)
    logits = (a.scale * torch.randn(N * S, C, generator=gen)).to(dtype).cuda()
    input_lengths = torch.randint(S - S // 8, S + 1, (N,), generator=gen).cuda()
    lengths = torch.randint(max(a.labels - 10, 0), a.labels + 11, (N,), generator=gen)
    Lmax = int(lengths.max())
    targets = torch.randint(1, C, (N, Lmax), generator=gen).cuda()
    target_lengths = lengths.cuda()
    fits_lds = S * (2 * Lmax + 1) <= ops.CTC_ALIGN_LDS_BACK_BYTES

    kernels = {"align_global": lambda: ops.ctc_align(logits, targets, input_lengths, target_lengths, 0, global_back=True),
               "ctc_fwd": lambda: ops.ctc_fwd(logits, targets, input_lengths, target_lengths, 0)}
    if fits_lds:
        kernels["align_lds"] = lambda: ops.ctc_align(logits, targets, input_lengths, target_lengths, 0)
    if a.only is not None:
        if a.only not in kernels:
            raise SystemExit(f"--only {a.only}: S (2 Lmax + 1) = {S * (2 * Lmax + 1)} bytes of backpointers do not fit LDS at this shape")
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
    out = {"lines": N, "seq": S, "classes": C, "labels": a.labels, "Lmax": Lmax, "dtype": a.dtype, "logit_scale": a.scale,
           "backpointer_bytes_per_line": S * (2 * Lmax + 1), "fits_lds": fits_lds}
    out.update({name: summary(v) for name, v in times.items()})
    if "align_lds" in kernels and "align_global" in kernels:
        x, y = kernels["align_lds"](), kernels["align_global"]()
        out["paths_bit_equal"] = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x, y))
        out["feasible_lines"] = int(torch.isfinite(x[3]).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
