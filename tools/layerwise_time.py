"""Times one step() of FusedAdamW, FusedLAMB and FusedLARS in the same process on the real tensor lists of the config-2 model (12-layer
d = 512 ViT + linear head 4096, 40.4 M parameters) and of the joint-embedding model with the reference's default MLP head (138.4 M
in the head, 176.8 M in all):
the same two groups (layerwise_groups / decay_groups), the same gradients, no clip.  Everything warmed up, then ROUNDS alternating
rounds of device-event windows of REPS steps each; one JSON line per model with every window's ms/step, min / median / max, the ratios
of the medians to FusedAdamW's and the spread (max - min) / median seen in this run.  The byte model per parameter
(Adam 30 B, LAMB 24 + 18 = 42 B, LARS 8 + 22 = 30 B; the transposed bf16 copies, 4 B per matrix element, come on top of all three) gives
the GB/s column.
usage: python tools/layerwise_time.py [out.json]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pero_pretraining_amd.optim import FusedAdamW, FusedLAMB, FusedLARS, decay_groups, layerwise_groups  # noqa: E402

ROUNDS, REPS = 5, 20
BYTES = {"adamw": 30, "lamb": 42, "lars": 30}


class Tensors:
    """A stand-in for a model: the groups helpers only ask for parameters()."""

    def __init__(self, params):
        self.params = params

    def parameters(self):
        return iter(self.params)


def models(dev):
    from pero_pretraining_amd.joint_embedding_pretraining import model as J
    from pero_pretraining_amd.masked_pretraining import model as M
    bb_def = {"type": "vit", "num_blocks": 12, "model_dim": 512, "num_heads": 4, "feedforward_dim": 2048}
    torch.manual_seed(0)
    masked = M.MaskedTransformerEncoder(M.init_backbone(dict(bb_def)), M.init_head({"in_features": 512, "out_features": 4096}))
    yield "config-2 masked model", [p.detach().to(dev) for p in masked.parameters()]
    del masked
    bb_def.pop("type")
    joint = torch.nn.ModuleList([J.init_backbone(bb_def), J.init_head({"type": "mlp"})])
    yield "joint-embedding model with the MLP head", [p.detach().to(dev) for p in joint.parameters()]


def timed(opt, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        opt.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    dev = torch.device("cuda", 0)
    out = []
    for name, tensors in models(dev):
        gen = torch.Generator(device=dev).manual_seed(1)
        opts = {}
        for kind in ("adamw", "lamb", "lars"):
            holder = Tensors([torch.nn.Parameter(t.clone()) for t in tensors])
            if kind == "adamw":
                opts[kind] = FusedAdamW(decay_groups(holder, 0.01), lr=1e-4, weight_decay=0.01)
            elif kind == "lamb":
                opts[kind] = FusedLAMB(layerwise_groups(holder, 0.01), lr=1e-4, weight_decay=0.01)
            else:
                opts[kind] = FusedLARS(layerwise_groups(holder, 1e-4), lr=0.1, momentum=0.9, weight_decay=1e-4)
        for opt in opts.values():      # the same gradients in all three
            gen.manual_seed(1)
            for flat in opt.flat_grads().values():
                flat.copy_(torch.randn(flat.shape, device=dev, generator=gen) * 1e-3)
        for opt in opts.values():
            timed(opt, 5)
        windows = {k: [] for k in opts}
        for _ in range(ROUNDS):
            for kind, opt in opts.items():
                windows[kind].append(timed(opt, REPS))
        n = sum(t.numel() for t in tensors)
        n_mat = sum(t.numel() for t in tensors if t.dim() >= 2)
        rec = {"model": name, "parameters": n, "tensors": len(tensors), "matrix_elements": n_mat, "rounds": ROUNDS, "reps": REPS}
        med = {}
        for kind, w in windows.items():
            s = sorted(w)
            med[kind] = s[len(s) // 2]
            rec[kind] = {"ms_per_step": [round(x, 4) for x in w], "min": round(s[0], 4), "median": round(med[kind], 4), "max": round(s[-1], 4),
                         "spread": round((s[-1] - s[0]) / med[kind], 4), "bytes_per_parameter": BYTES[kind],
                         "model_gb_per_s": round((BYTES[kind] * n + 4 * n_mat) / med[kind] / 1e6, 1)}
        rec["lamb_over_adamw"] = round(med["lamb"] / med["adamw"], 4)
        rec["lars_over_adamw"] = round(med["lars"] / med["adamw"], 4)
        rec["byte_ratio_lamb"] = round((42 * n + 4 * n_mat) / (30 * n + 4 * n_mat), 4)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del opts
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
