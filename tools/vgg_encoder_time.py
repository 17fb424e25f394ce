"""Times the tokenizer's VGG encoder (models.autoencoders.VGGEncoder, csrc/conv.hip) at the default definition on 40 x 2048 lines:
the whole stack in bf16 and f32 at 64 lines and at the largest chunk max_workspace_bytes allows; in bf16 every convolution on its own with
the TFLOP/s it reaches (useful FLOP: 2 * 9 * Cin * Cout per interior pixel), and the pools and the ingestion with the bytes they move
and TB/s beside a device copy of as many bytes.  In the same process: torch.nn.functional.conv2d / max_pool2d with the same weights in
bf16 channels_last - the way a user runs this stack without the package; skipped when torch's convolution backend is missing.
Everything is warmed up; alternating rounds of device-event windows; one JSON line.  --lines / --width shrink it
for a rehearsal."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pero_pretraining_amd as P  # noqa: E402
from pero_pretraining_amd import ops  # noqa: E402
from pero_pretraining_amd.models.autoencoders import VGGEncoder  # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds(fns, window_ms=200.0, n_rounds=3):
    """name -> [ms per call] over n_rounds alternating rounds; every function is warmed up and sized to a window first."""
    reps = {}
    for name, fn in fns.items():
        fn()
        reps[name] = max(1, min(200, int(window_ms / max(timed(fn, 1), 0.01))))
    out = {name: [] for name in fns}
    for _ in range(n_rounds):
        for name, fn in fns.items():
            out[name].append(timed(fn, reps[name]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "vgg_encoder_time.py measures on the GPU; there is nothing to time without one"
    torch.manual_seed(0)
    enc = VGGEncoder().cuda().eval()
    H, W, N = enc.height, a.width, a.lines
    g = torch.Generator(device="cuda").manual_seed(0)
    images = torch.randint(0, 256, (N, H, W, 3), device="cuda", dtype=torch.uint8, generator=g)
    es = {torch.bfloat16: 2, torch.float32: 4}
    steps = enc.steps()
    flop_line = 0.0
    h, w, c = H, W, 3
    for s in steps:
        if s[0] == "conv":
            flop_line += 2.0 * 9 * c * s[2].out_channels * h * w
            c = s[2].out_channels
        else:
            h, w = h // s[2][0], w // s[2][1]
    flop_line += 2.0 * h * c * enc.out_channels * w
    rec = {"height": H, "width": W, "lines": N, "GFLOP_per_line": flop_line / 1e9, "stack": {}, "layers_bf16": {}, "memory_bound_bf16": {}}

    # ---- the whole stack
    def stack_run(dtype, imgs):
        def run():
            with torch.no_grad(), P.autocast(dtype == torch.bfloat16):
                enc(imgs)
        return run

    legs = {}
    for dtype in (torch.bfloat16, torch.float32):
        chunk = enc.lines_per_chunk(H, W, dtype)
        big = torch.randint(0, 256, (chunk, H, W, 3), device="cuda", dtype=torch.uint8, generator=g)
        legs[f"{dtype} {N} lines"] = (stack_run(dtype, images), N)
        legs[f"{dtype} {chunk} lines (largest chunk)"] = (stack_run(dtype, big), chunk)
    st = rounds({k: f for k, (f, _) in legs.items()}, window_ms=400.0, n_rounds=2)
    for k, (_, n) in legs.items():
        ms = min(st[k])
        rec["stack"][k] = {"ms": st[k], "ms_per_line": ms / n, "TFLOPs": flop_line * n / ms / 1e9}
    del legs
    torch.cuda.empty_cache()

    # ---- bf16: every layer on its own, on the activations the stack hands it
    dt = torch.bfloat16
    trace = []
    with torch.no_grad(), P.autocast(True):
        enc(images, trace=trace)
    conv_fns, mem_fns, mem_bytes, conv_flop = {}, {}, {}, {}
    x_in = trace[0][2]
    mem_fns["ingest uint8"] = lambda c=x_in.shape[3]: ops.image_to_halo(images, dt, channels=c)
    mem_bytes["ingest uint8"] = images.numel() + x_in.numel() * 2
    for s, (kind, index, y) in zip(steps, trace[1:-1]):
        if kind == "conv":
            wk, bk = enc._conv_operands(index, s[2], dt)
            name = f"conv {s[2].in_channels}->{s[2].out_channels} at {x_in.shape[1] - 2}x{x_in.shape[2] - 2}"
            name = name if name not in conv_fns else name + " (2)"
            conv_fns[name] = (lambda xi=x_in, wk=wk, bk=bk, yo=y: ops.conv3x3(xi, wk, bk, activation="relu", out=yo))
            conv_flop[name] = 2.0 * 9 * s[2].in_channels * s[2].out_channels * (x_in.shape[1] - 2) * (x_in.shape[2] - 2) * N
        else:
            ab = (None, None) if s[3] is None else enc._bn_affine(index, s[3])
            name = f"pool {s[2]} C={x_in.shape[3]}" + (" + affine, token rows" if y.dim() == 2 else "")
            mem_fns[name] = (lambda xi=x_in, ab=ab, yo=y, s=s: ops.maxpool_nhwc(xi, s[2], ab[0], ab[1], token_rows=yo.dim() == 2, out=yo))
            mem_bytes[name] = (x_in.numel() + y.numel()) * 2
        x_in = y
    tokens = trace[-2][2]
    wk, bk = enc._aggregation_operands(dt)
    conv_fns["aggregation gemm"] = lambda: ops.gemm(tokens, wk, bias=bk, out_dtype=torch.float32)
    conv_flop["aggregation gemm"] = 2.0 * tokens.shape[0] * tokens.shape[1] * wk.shape[0]
    ct = rounds(conv_fns)
    for k in conv_fns:
        rec["layers_bf16"][k] = {"ms": ct[k], "GFLOP": conv_flop[k] / 1e9, "TFLOPs": conv_flop[k] / min(ct[k]) / 1e9}
    copies = {}
    for k, b in mem_bytes.items():
        src = torch.empty(b // 2, device="cuda", dtype=torch.uint8)
        dst = torch.empty_like(src)
        copies["copy for " + k] = (lambda s=src, d=dst: d.copy_(s))
    mt = rounds({**mem_fns, **copies})
    for k, b in mem_bytes.items():
        rec["memory_bound_bf16"][k] = {"ms": mt[k], "bytes": b, "TBps": b / min(mt[k]) / 1e9, "device_copy_TBps": b / min(mt["copy for " + k]) / 1e9}
    rec["sum_of_layers_bf16_ms"] = sum(min(v) for v in ct.values()) + sum(min(mt[k]) for k in mem_fns)
    del trace, conv_fns, mem_fns, copies
    torch.cuda.empty_cache()

    # ---- torch's own path: bf16 channels_last, the same weights
    try:
        mods = [(s, (s[2].weight.detach().to(dt).contiguous(memory_format=torch.channels_last), s[2].bias.detach().to(dt)) if s[0] == "conv" else None)
                for s in steps]
        agg_w, agg_b = enc.aggregation_layer.weight.detach().to(dt), enc.aggregation_layer.bias.detach().to(dt)
        bn = steps[-1][3]

        def torch_run():
            with torch.no_grad():
                x = (images.permute(0, 3, 1, 2).to(dt) / 255).contiguous(memory_format=torch.channels_last)
                for s, wb in mods:
                    if s[0] == "conv":
                        x = F.relu(F.conv2d(x, wb[0], wb[1], padding=1))
                    else:
                        x = F.max_pool2d(x, s[2], s[2])
                        if s[3] is not None:
                            x = F.batch_norm(x, bn.running_mean.to(dt), bn.running_var.to(dt), bn.weight.to(dt), bn.bias.to(dt), False, 0.0, bn.eps)
                return F.conv2d(x, agg_w, agg_b)

        torch_run()
        tt = rounds({"torch": torch_run, "pero": stack_run(dt, images)}, window_ms=400.0)
        rec["torch_bf16_channels_last"] = {"ms": tt["torch"], "pero_ms_same_rounds": tt["pero"], "TFLOPs": flop_line * N / min(tt["torch"]) / 1e9,
                                           "pero_time_over_torch_time": min(tt["pero"]) / min(tt["torch"])}
    except RuntimeError as e:       # no convolution backend in this torch build
        rec["torch_bf16_channels_last"] = {"skipped": str(e).splitlines()[0][:200]}
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
