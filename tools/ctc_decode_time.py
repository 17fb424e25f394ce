"""Time the evaluation of a recogniser on one GPU, in ONE process: greedy decoding, beam search at W = 4, 16, 32, the batched edit
distance, the recogniser's forward pass on the same batch, and Tester.test() on a fixed list of batches - this tree's Tester (error
counting on the device) against the parent commit's (labels read back per batch, a Python edit distance per line).  Everything is warmed
up, then timed in alternating windows (DESIGN.md "CTC decoding" quotes the result): device events around the kernels, the wall clock
around Tester.test(), which ends in a host read either way.

    python tools/ctc_decode_time.py [--lines 256 --seq 256 --classes 512 --labels 60 --dtype bf16 --iters 20 --rounds 5
                                     --batches 4 --parent-tester FILE]

--parent-tester: the parent commit's pero_pretraining_amd/recognition/tester.py (default: `git show HEAD~1:...` of this checkout; without
either, that comparison is left out and the output says so).  Prints one JSON line: milliseconds (median and range over the rounds)."""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TESTER = "pero_pretraining_amd/recognition/tester.py"


def parent_tester_class(path):
    """The Tester of the parent commit, loaded beside this tree's as a module of the same package (its relative imports resolve here)."""
    if path is None:
        try:
            src = subprocess.run(["git", "-C", ROOT, "show", "HEAD~1:" + TESTER], check=True, capture_output=True, text=True).stdout
        except (OSError, subprocess.CalledProcessError):
            return None
        f = tempfile.NamedTemporaryFile("w", suffix="_parent_tester.py", delete=False)
        f.write(src)
        f.close()
        path = f.name
    spec = importlib.util.spec_from_file_location("pero_pretraining_amd.recognition._parent_tester", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Tester


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
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--scale", type=float, default=4.0, help="logits = scale * randn for the kernel timings")
    ap.add_argument("--parent-tester", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_decode_time.py needs a GPU: a timing taken anywhere else says nothing")
    from pero_pretraining_amd import ops
    from pero_pretraining_amd.precision import autocast
    from pero_pretraining_amd.recognition import BatchOperator, Tester, init_model
    N, S, C = a.lines, a.seq, a.classes
    bf16 = a.dtype == "bf16"
    dtype = torch.bfloat16 if bf16 else torch.float32
    gen = torch.Generator().manual_seed(0)
    logits = (a.scale * torch.randn(N * S, C, generator=gen)).to(dtype).cuda()
    input_lengths = torch.randint(S - S // 8, S + 1, (N,), generator=gen).cuda()
    lengths = torch.randint(max(a.labels - 10, 0), a.labels + 11, (N,), generator=gen)
    Lmax = int(lengths.max())
    targets = torch.randint(1, C, (N, Lmax), generator=gen).cuda()
    target_lengths = lengths.cuda()
    # strings to compare: the targets against copies with about one label in ten changed and a few dropped at the end
    noisy = torch.where(torch.rand(N, Lmax, generator=gen).cuda() < 0.1, torch.randint(1, C, (N, Lmax), generator=gen).cuda(), targets)
    noisy_lengths = (target_lengths - torch.randint(0, 4, (N,), generator=gen).cuda()).clamp_min(0)

    # the recogniser and the Tester's batches: lines of `seq` positions, 8 pixel columns each
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

    kernels = {"greedy": lambda: ops.ctc_greedy(logits, input_lengths, 0),
               "beam4": lambda: ops.ctc_beam(logits, input_lengths, 4, 0),
               "beam16": lambda: ops.ctc_beam(logits, input_lengths, 16, 0),
               "beam32": lambda: ops.ctc_beam(logits, input_lengths, 32, 0),
               "edit_distance": lambda: ops.edit_distance(noisy, noisy_lengths, targets, target_lengths),
               "forward": forward}

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

    testers = {"tester": Tester(operator, model, batches, bfloat16=bf16), "tester_beam16": Tester(operator, model, batches, bfloat16=bf16, beam_width=16)}
    parent = parent_tester_class(a.parent_tester)
    if parent is not None:
        testers["tester_parent"] = parent(operator, model, batches, bfloat16=bf16)

    for fn in kernels.values():
        for _ in range(3):
            fn()
    results = {}
    for name, t in testers.items():
        results[name] = t.test()
    torch.cuda.synchronize()
    times = {k: [] for k in list(kernels) + list(testers)}
    for _ in range(a.rounds):
        for name, fn in kernels.items():
            times[name].append(window(fn))
        for name, t in testers.items():
            times[name].append(wall(t.test)[0])
    out = {"lines": N, "seq": S, "classes": C, "labels": a.labels, "dtype": a.dtype, "logit_scale": a.scale, "tester_batches": a.batches}
    out.update({name: summary(v) for name, v in times.items()})
    out["tester_results"] = results
    if parent is None:
        out["tester_parent"] = "left out: no parent tester given and no git history here"
    else:
        out["tester_cer_equal_to_parent"] = results["tester"]["cer"] == results["tester_parent"]["cer"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
