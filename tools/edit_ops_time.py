"""Time the edit operations of a recogniser's evaluation on one GPU, in ONE process, on the workload of tools/ctc_decode_time.py (256 pairs of
about 60 labels, C = 512): pero_edit_distance; pero_edit_ops with counts only, with counts, script and confusion matrix, and at word level;
the recogniser's forward pass on the same batch for scale; and Tester.test() on that tool's four fixed batches - the default (pero_edit_distance,
{'loss', 'cer'}) against details=True with word_separators (pero_edit_ops twice per batch).  Everything is warmed up, then timed in
alternating windows (DESIGN.md "Edit operations" quotes the result): device events around the kernels, the wall clock around Tester.test(),
which ends in a host read either way.

    python tools/edit_ops_time.py [--lines 256 --seq 256 --classes 512 --labels 60 --separators 16 --dtype bf16 --iters 20 --rounds 5
                                   --batches 4 --limit]

--separators: the classes 1 .. separators separate words; the strings draw one of them with probability 1 / 6, so a word has about five
labels.  --limit: also time pero_edit_distance and pero_edit_ops (counts; with script; with script and confusion) on 256 pairs at la = lb = 512 over
two symbols, the largest table and the longest walk back.  Prints one JSON line: milliseconds (median and range over the rounds)."""
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


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "range_ms": [round(min(v), 4), round(max(v), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=256)
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--classes", type=int, default=512)
    ap.add_argument("--labels", type=int, default=60)
    ap.add_argument("--separators", type=int, default=16)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--limit", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edit_ops_time.py needs a GPU: a timing taken anywhere else says nothing")
    from pero_pretraining_amd import ops
    from pero_pretraining_amd.precision import autocast
    from pero_pretraining_amd.recognition import BatchOperator, Tester, init_model
    N, S, C = a.lines, a.seq, a.classes
    bf16 = a.dtype == "bf16"
    gen = torch.Generator().manual_seed(0)
    lengths = torch.randint(max(a.labels - 10, 0), a.labels + 11, (N,), generator=gen)
    Lmax = int(lengths.max())
    # strings to compare (ctc_decode_time.py's): the targets against copies with about one label in ten changed and a few dropped at the end;
    # one label in six is a separator, so the same strings serve the word level
    seps = list(range(1, a.separators + 1))
    targets = torch.randint(a.separators + 1, C, (N, Lmax), generator=gen)
    targets = torch.where(torch.rand(N, Lmax, generator=gen) < 1 / 6, torch.randint(1, a.separators + 1, (N, Lmax), generator=gen), targets).cuda()
    target_lengths = lengths.cuda()
    noisy = torch.where(torch.rand(N, Lmax, generator=gen).cuda() < 0.1, torch.randint(1, C, (N, Lmax), generator=gen).cuda(), targets)
    noisy_lengths = (target_lengths - torch.randint(0, 4, (N,), generator=gen).cuda()).clamp_min(0)
    is_sep = ops.edit_separator_table(seps, C, targets.device)
    totals = torch.zeros(6, dtype=torch.int64).cuda()
    confusion = torch.zeros((C + 1, C + 1), dtype=torch.int64).cuda()
    pair = (noisy, noisy_lengths, targets, target_lengths)

    # the recogniser and the Tester's batches: lines of `seq` positions, 8 pixel columns each (ctc_decode_time.py's)
    torch.manual_seed(0)
    model = init_model(torch.device("cuda"), {"type": "vit", "num_blocks": 6, "model_dim": 512, "num_heads": 8, "feedforward_dim": 2048},
                       {"type": "linear", "in_features": 512, "out_features": C}, blank=0)
    rng = np.random.default_rng(0)
    batches = []
    for _ in range(a.batches):
        tl = rng.integers(max(a.labels - 10, 0), a.labels + 11, N)
        batches.append({"images": rng.integers(0, 256, (N, 40, 8 * S, 3), dtype=np.uint8), "targets": rng.integers(1, C, (N, int(tl.max()))),
                        "target_lengths": tl, "widths": rng.integers(8 * (S - S // 8), 8 * S + 1, N)})
    operator = BatchOperator(torch.device("cuda"))
    images, _, _, il0 = operator.prepare_batch(batches[0])

    def forward():
        with torch.no_grad(), autocast(bf16):
            model(images, input_lengths=il0)

    kernels = {"edit_distance": lambda: ops.edit_distance(*pair),
               "edit_ops_counts": lambda: ops.edit_ops(*pair, totals=totals, want_script=False),
               "edit_ops_script_confusion": lambda: ops.edit_ops(*pair, num_classes=C, totals=totals, confusion=confusion),
               "edit_ops_words": lambda: ops.edit_ops(*pair, num_classes=C, separators=is_sep, totals=totals, want_spans=True),
               "forward": forward}
    if a.limit:
        long_a, long_b = torch.randint(0, 2, (N, 512), generator=gen).cuda(), torch.randint(0, 2, (N, 512), generator=gen).cuda()
        full = torch.full((N,), 512).cuda()
        long_pair = (long_a, full, long_b, full)
        kernels["edit_distance_512"] = lambda: ops.edit_distance(*long_pair)
        kernels["edit_ops_counts_512"] = lambda: ops.edit_ops(*long_pair, totals=totals, want_script=False)
        kernels["edit_ops_script_512"] = lambda: ops.edit_ops(*long_pair, totals=totals)
        # two symbols: every confusion count of the call lands on one of eight entries of the matrix, the worst case for its atomics
        kernels["edit_ops_script_confusion_512"] = lambda: ops.edit_ops(*long_pair, num_classes=C, totals=totals, confusion=confusion)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, result

    testers = {"tester": Tester(operator, model, batches, bfloat16=bf16),
               "tester_details_words": Tester(operator, model, batches, bfloat16=bf16, details=True, word_separators=seps)}
    for fn in kernels.values():
        for _ in range(3):
            fn()
    results = {}
    for name, t in testers.items():
        r = t.test()
        results[name] = {k: v for k, v in r.items() if k != "confusion"}
    torch.cuda.synchronize()
    times = {k: [] for k in list(kernels) + list(testers)}
    for _ in range(a.rounds):
        for name, fn in kernels.items():
            times[name].append(window(fn))
        for name, t in testers.items():
            times[name].append(wall(t.test)[0])
    out = {"lines": N, "seq": S, "classes": C, "labels": a.labels, "separators": a.separators, "dtype": a.dtype, "tester_batches": a.batches}
    out.update({name: summary(v) for name, v in times.items()})
    out["tester_results"] = results
    out["tester_cer_equal"] = results["tester"]["cer"] == results["tester_details_words"]["cer"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
