"""Time the CTC loss (forward + backward) of recognition.CTCLoss against what a user runs without it,
torch.nn.functional.ctc_loss(log_softmax(logits.float()).transpose(0, 1), ...) + its backward, in ONE process on one GPU:
both sides warmed up, then timed in alternating windows with device events (DESIGN.md "CTC" quotes the result).

    python tools/ctc_time.py [--lines 256 --seq 256 --classes 512 --labels 60 --dtype bf16 --iters 50 --rounds 5]

Prints one JSON line: milliseconds per forward + backward of each side (median and range over the rounds), the workspace bytes
of ours, and the worst difference of the two gradients (a sanity check at the timed size, not a parity test)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=256)
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--classes", type=int, default=512)
    ap.add_argument("--labels", type=int, default=60)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_time.py needs a GPU: a timing taken anywhere else says nothing")
    from pero_pretraining_amd.recognition import CTCLoss
    N, S, C = a.lines, a.seq, a.classes
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    gen = torch.Generator().manual_seed(0)
    logits = (4 * torch.randn(N, S, C, generator=gen)).to(dtype).cuda().requires_grad_(True)
    lengths = torch.randint(max(a.labels - 10, 0), a.labels + 11, (N,), generator=gen)
    Lmax = int(lengths.max())
    targets = torch.randint(1, C, (N, Lmax), generator=gen).cuda()
    target_lengths = lengths.cuda()
    input_lengths = torch.randint(S - S // 8, S + 1, (N,), generator=gen).cuda()
    ours_fn = CTCLoss(blank=0, reduction="mean")

    def ours():
        logits.grad = None
        ours_fn(logits, targets, input_lengths, target_lengths).backward()

    def theirs():
        logits.grad = None
        lp = torch.log_softmax(logits.float(), -1).transpose(0, 1)
        torch.nn.functional.ctc_loss(lp, targets, input_lengths, target_lengths, blank=0, reduction="mean").backward()

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for fn in (ours, theirs):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ours()
    g_ours = logits.grad.float().clone()
    theirs()
    g_theirs = logits.grad.float().clone()
    t = {"ours": [], "torch": []}
    for _ in range(a.rounds):
        t["ours"].append(window(ours))
        t["torch"].append(window(theirs))
    W = 2 * Lmax + 1
    out = {"lines": N, "seq": S, "classes": C, "labels": a.labels, "dtype": a.dtype,
           "ours_ms": round(statistics.median(t["ours"]), 4), "ours_range_ms": [round(min(t["ours"]), 4), round(max(t["ours"]), 4)],
           "torch_ms": round(statistics.median(t["torch"]), 4), "torch_range_ms": [round(min(t["torch"]), 4), round(max(t["torch"]), 4)],
           "workspace_bytes": {"alpha": 4 * N * S * W, "beta": 4 * N * S * W, "row_lse": 4 * N * S, "chain": 4 * N * Lmax, "nll": 4 * N},
           "torch_log_softmax_bytes": 4 * N * S * C,
           "max_abs_grad_difference": float((g_ours - g_theirs).abs().max()), "max_abs_grad": float(g_theirs.abs().max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
