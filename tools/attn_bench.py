#!/usr/bin/env python3
"""Fused attention kernels: TFLOP/s vs sequence length (prologue / epilogue share).
usage: python tools/attn_bench.py [--head-dim 128|64] [--table | --keys]
--head-dim: the head width at d = 512 (128: 4 heads, the default; 64: 8 heads, csrc/attention_hd64.hip).
--table: the fused-against-unfused table of DESIGN 8.000 / 8.0000 instead: N = 2048 lines, d = 512, forward + backward in the step's form (`out`
given, in_proj's bias gradient wanted) with the fused kernels and with functional.attention_fwd / attention_bwd (batched GEMM + softmax), HIP
events around 20 calls after 3 warm-up calls, five rounds alternating the configurations, median (min ... max) in us, and the allocator peak of
one call above the resident inputs (the fused side also produces in_proj's bias gradient, the unfused side leaves it to a later column-sum
launch that is not timed: the comparison favours the unfused side by that much); at --head-dim 64 the head_dim-128 / 4-head fused time (the same FLOPs) is printed beside it.
--keys: per-line key ranges (DESIGN "Attention with per-line key ranges"): N = --lines, S = 256, d = 512, forward + backward in the same form and with the same timing
scheme, without ranges, with the full range [0, 256) on every line and with ranges of half the line ([lp, lp + 128), lp drawn per line like the collator's left padding)."""
import argparse, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pero_pretraining_amd import ops
ap = argparse.ArgumentParser()
ap.add_argument("--head-dim", type=int, default=128, choices=(64, 128))
ap.add_argument("--table", action="store_true")
ap.add_argument("--keys", action="store_true")
ap.add_argument("--lines", type=int, default=2048)
args = ap.parse_args()
def bench(fn, iters=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3
def table():
    from pero_pretraining_amd import functional as F
    n, d = args.lines, 512
    def peak_mib(fn):
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    def fmt(v): return f"{statistics.median(v):9.0f} ({min(v):.0f} ... {max(v):.0f})"
    for s in (256, 260, 128, 132, 100, 36, 4):
        torch.manual_seed(s)
        qkv = (torch.randn(n * s, 3 * d, device="cuda") * 0.7).bfloat16()
        dout = torch.randn(n * s, d, device="cuda").bfloat16()
        db = torch.zeros(3 * d, device="cuda")
        def fused(h):
            out, lse = ops.attention_fwd_fused(qkv, n, s, h)
            return ops.attention_bwd_fused(qkv, out, dout, lse, n, s, h, dbias=db)
        def unfused(h):
            a, p = F.attention_fwd(qkv, n, s, h)
            return F.attention_bwd(qkv, p, dout, n, s, h)
        h = d // args.head_dim
        configs = {"fused": lambda: fused(h), "unfused": lambda: unfused(h)}
        if args.head_dim != 128: configs["fused hd128"] = lambda: fused(d // 128)
        times = {k: [] for k in configs}
        for _ in range(5):
            for k, fn in configs.items(): times[k].append(bench(fn, 20))
        peaks = {k: peak_mib(fn) for k, fn in configs.items()}
        ratio = statistics.median(times["unfused"]) / statistics.median(times["fused"])
        print(f"S={s:4d} hd={args.head_dim}: " + " | ".join(f"{k} {fmt(v)} us, peak {peaks[k]:6.0f} MiB" for k, v in times.items()) + f" | unfused / fused {ratio:.2f}", flush=True)
def keys():
    n, d, s, h = args.lines, 512, 256, 512 // args.head_dim
    torch.manual_seed(s)
    qkv = (torch.randn(n * s, 3 * d, device="cuda") * 0.7).bfloat16()
    dout = torch.randn(n * s, d, device="cuda").bfloat16()
    db = torch.zeros(3 * d, device="cuda")
    lp = torch.randint(0, s // 2 + 1, (n,), device="cuda", dtype=torch.int32)
    full = torch.stack((torch.zeros_like(lp), torch.full_like(lp, s)), 1).contiguous()
    half = torch.stack((lp, lp + s // 2), 1).contiguous()
    def run(kr):
        out, lse = ops.attention_fwd_fused(qkv, n, s, h, key_ranges=kr)
        return ops.attention_bwd_fused(qkv, out, dout, lse, n, s, h, dbias=db, key_ranges=kr)
    configs = {"no ranges": lambda: run(None), "full ranges": lambda: run(full), "half-line ranges": lambda: run(half)}
    times = {k: [] for k in configs}
    for _ in range(5):
        for k, fn in configs.items(): times[k].append(bench(fn, 20))
    print(f"N={n} S={s} hd={args.head_dim} fwd + bwd: " + " | ".join(f"{k} {statistics.median(v):.0f} ({min(v):.0f} ... {max(v):.0f}) us" for k, v in times.items()), flush=True)
if args.table:
    table()
    sys.exit(0)
if args.keys:
    keys()
    sys.exit(0)
hd = args.head_dim
h = 512 // hd
for n, s in [(256, 256), (128, 512), (64, 1024), (32, 2048)]:
    d = h * hd
    qkv = (torch.randn(n * s, 3 * d, device="cuda") * 0.7).bfloat16()
    dout = torch.randn(n * s, d, device="cuda").bfloat16()
    out, lse = ops.attention_fwd_fused(qkv, n, s, h)
    tf = bench(lambda: ops.attention_fwd_fused(qkv, n, s, h))
    tb = bench(lambda: ops.attention_bwd_fused(qkv, out, dout, lse, n, s, h))
    db = torch.zeros(3 * h * hd, device="cuda")
    tbb = bench(lambda: ops.attention_bwd_fused(qkv, out, dout, lse, n, s, h, dbias=db))
    fl = 4.0 * s * s * hd * n * h
    print(f"N={n:4d} S={s:5d}: fwd {tf:7.1f} us {fl/tf/1e6:6.1f} TF | bwd {tb:7.1f} us {2.5*fl/tb/1e6:6.1f} TF useful ({3.0*fl/tb/1e6:6.1f} executed) | with in_proj bias gradient {tbb:7.1f} us")
