"""Time CTC beam search with an n-gram language model (pero_ctc_beam_lm) against the plain search (pero_ctc_beam) on one GPU, in ONE
process, the sibling of tools/ctc_decode_time.py: the same logits (N = S = 256, C = 512, bf16, 4 randn), an order-3 model fitted on 20 000
random strings (so that most look-ups back off), and an order-1 model (one state: a look-up is one binary search, no back-off) to tell the
cost of the walks from the cost of ranking more candidates.  Everything is warmed up, then timed with device events in alternating windows
(DESIGN.md section 15 quotes the result).

    python tools/ctc_beam_lm_time.py [--lines 256 --seq 256 --classes 512 --dtype bf16 --iters 10 --rounds 5 --strings 20000
                                      --parent-lib FILE]

--parent-lib: the parent commit's libpero_hip.so; its pero_ctc_beam is then timed in the same windows as this tree's (the A/B of "the plain
search is no slower than before").  Prints one JSON line: milliseconds (median and range over the rounds) and microseconds per frame."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = [(16, 17), (16, 40), (4, 40)]   # (W, K)


def summary(v, frames):
    return {"median_ms": round(statistics.median(v), 4), "range_ms": [round(min(v), 4), round(max(v), 4)],
            "us_per_frame": round(1e3 * statistics.median(v) / frames, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=256)
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--classes", type=int, default=512)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--strings", type=int, default=20000)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_lm_time.py needs a GPU: a timing taken anywhere else says nothing")
    from pero_pretraining_amd import _lib, ops
    from pero_pretraining_amd.recognition import NGramLM
    N, S, C = a.lines, a.seq, a.classes
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    gen = torch.Generator().manual_seed(0)
    logits = (a.scale * torch.randn(N * S, C, generator=gen)).to(dtype).cuda()
    input_lengths = torch.randint(S - S // 8, S + 1, (N,), generator=gen).cuda()
    rng = np.random.default_rng(0)
    strings = [rng.integers(1, C, int(rng.integers(40, 81))).tolist() for _ in range(a.strings)]
    lm3 = NGramLM.fit(strings, C, 0, order=3)
    lm1 = NGramLM.fit(strings, C, 0, order=1)

    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.pero_ctc_beam.restype = ctypes.c_int
        parent.pero_ctc_beam.argtypes = _lib.SIGNATURES["pero_ctc_beam"]

    def parent_beam(W):
        """ops.ctc_beam's call through the parent's library (the same buffers, allocated the same way)."""
        K, H = ops.ctc_beam_workspace(S, C, W)
        dev, i32, i64, f32 = logits.device, torch.int32, torch.int64, torch.float32
        bufs = [torch.empty((N, W, S), device=dev, dtype=i64), torch.empty((N, W), device=dev, dtype=i64), torch.empty((N, W), device=dev, dtype=f32),
                torch.empty(N, device=dev, dtype=i64), torch.empty((N, S * W + 1), device=dev, dtype=i32), torch.empty((N, S * W + 1), device=dev, dtype=i32),
                torch.empty(N, device=dev, dtype=i32), torch.empty((N, S, W), device=dev, dtype=i32), torch.empty((N, S, W, 2), device=dev, dtype=f32),
                torch.empty(N * S, device=dev, dtype=f32), torch.empty((N * S, K), device=dev, dtype=f32), torch.empty((N * S, K), device=dev, dtype=i32),
                torch.empty((N, H), device=dev, dtype=i64)]
        rc = parent.pero_ctc_beam(ops.ptr(logits), ops.ptr(input_lengths), *[ops.ptr(t) for t in bufs], N, S, C, 0, W, ops.dt(logits), ops.stream())
        if rc != 0:
            raise SystemExit(f"the parent's pero_ctc_beam failed ({rc})")
        return bufs

    fns = {}
    for W in sorted({w for w, _ in ROWS}):
        fns[f"plain_W{W}"] = lambda W=W: ops.ctc_beam(logits, input_lengths, W, 0)
        if parent is not None:
            fns[f"parent_plain_W{W}"] = lambda W=W: parent_beam(W)
    for W, K in ROWS:
        fns[f"lm3_W{W}_K{K}"] = lambda W=W, K=K: ops.ctc_beam_lm(logits, input_lengths, W, lm3, 0.5, 0.0, K)
        fns[f"lm1_W{W}_K{K}"] = lambda W=W, K=K: ops.ctc_beam_lm(logits, input_lengths, W, lm1, 0.5, 0.0, K)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for name, fn in fns.items():
            times[name].append(window(fn))
    frames = float(input_lengths.max())
    out = {"lines": N, "seq": S, "classes": C, "dtype": a.dtype, "logit_scale": a.scale, "iters": a.iters, "rounds": a.rounds,
           "lm3": {"states": lm3.num_states, "arcs": lm3.num_arcs, "bytes": int(sum(v.nbytes for v in lm3.arrays().values()))},
           "lm1": {"states": lm1.num_states, "arcs": lm1.num_arcs}}
    out.update({name: summary(v, frames) for name, v in times.items()})
    if parent is not None:   # the same bits from both libraries
        W = ROWS[0][0]
        mine, theirs = ops.ctc_beam(logits, input_lengths, W, 0), parent_beam(W)
        out["plain_equals_parent"] = bool(torch.equal(mine[0], theirs[0]) and torch.equal(mine[2].view(torch.int32), theirs[2].view(torch.int32)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
