#!/usr/bin/env python3
"""Round-5 golden vectors, produced by the reference itself.  TEST INFRASTRUCTURE.

Runs ONLY in the build container (imports /root/reference read-only on CPU); writes under tests/golden/:

  g22_bf16_trajectory.npz   three `Trainer.train_step` calls (Adam + warm-up, masks and offsets drawn as in g5) of a config-2-width model
                            with 2 layers (d = 512, 4 heads of 128, FF 2048, head 512 -> 4096) on 2 lines of 40 x 2048 (S = 256, 512 rows:
                            the shapes at which the bf16 mode takes the fused attention, the n512 LayerNorm epilogues, the ReLU bit masks and
                            the row-sparse last layer).  Two variants: "fresh" (the seed recipe's weights) and "trained" (the same with the
                            norm1 / norm2 gamma and beta of both layers overwritten by pero_oracle.trained_layernorm_columns; those vectors
                            are stored).  Per step: loss, lr, mask, offsets, labels and a checksum of the images (they are regenerated from
                            a seeded numpy Generator).  At the end: every tensor with <= 4096 entries in full, the others at 4096 seeded
                            positions (`index.<name>`), and the f64 norm of (sd3 - sd0) of every tensor.

usage:  python oracle/make_golden_r5.py [--out tests/golden]
"""
import argparse
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REFERENCE_ROOT, cuda_to_is_noop, np_sd  # noqa: E402

BB = {"type": "vit", "num_blocks": 2, "model_dim": 512, "num_heads": 4, "feedforward_dim": 2048}
HD = {"type": "linear", "in_features": 512, "out_features": 4096}
LINES, WIDTH, LR = 2, 2048, 1e-3
SAMPLES = 4096


def batches():
    """The three steps' images and labels (tests/test_gpu_bf16_trajectory.py draws the same)."""
    rng = np.random.default_rng(2205)
    return [(rng.integers(0, 256, (LINES, 40, WIDTH, 3), dtype=np.uint8), rng.integers(0, 4096, (LINES, WIDTH // 8)).astype(np.int64))
            for _ in range(3)]


def trained_norms(layers=2):
    """{state-dict key: vector} of the "trained" variant's LayerNorm weights."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from oracle import pero_oracle as O
    out = {}
    for i in range(layers):
        for k, norm in enumerate(("norm1", "norm2")):
            gamma, beta = O.trained_layernorm_columns(512, 100 + 2 * i + k)
            out[f"backbone.encoder_layers.layers.{i}.{norm}.weight"] = gamma.numpy()
            out[f"backbone.encoder_layers.layers.{i}.{norm}.bias"] = beta.numpy()
    return out


def sample_index(name, numel):
    return np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(numel, SAMPLES, replace=False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "tests", "golden"))
    out = os.path.abspath(ap.parse_args().out)
    os.makedirs(out, exist_ok=True)
    sys.path.insert(0, REFERENCE_ROOT)
    torch.set_num_threads(8)
    from pero_pretraining.masked_pretraining import model as R_mm
    from pero_pretraining.masked_pretraining import trainer as R_mt
    from pero_pretraining.masked_pretraining import batch_operator as R_mb
    from pero_pretraining.common import lr_scheduler as R_lr

    data = batches()
    fix = {"image_sums": np.array([int(im.astype(np.int64).sum()) for im, _ in data]), "labels": np.stack([lab for _, lab in data])}
    norms = trained_norms()
    for k, v in norms.items():
        fix["norms." + k] = v
    for variant in ("fresh", "trained"):
        torch.manual_seed(0)
        with cuda_to_is_noop():
            backbone = R_mm.init_backbone(dict(BB))
        model = R_mm.MaskedTransformerEncoder(backbone, R_mm.init_head(dict(HD)))
        if variant == "trained":
            sd = model.state_dict()
            with torch.no_grad():
                for k, v in norms.items():
                    sd[k].copy_(torch.from_numpy(v))
        sd0 = np_sd(model)
        bop = R_mb.BatchOperator(torch.device("cpu"), 0.15)
        opt = torch.optim.Adam(model.parameters(), lr=LR)
        sched = R_lr.WarmupSchleduler(opt, LR, 2, 1)
        trainer = R_mt.Trainer(bop, model, None, opt, sched, bfloat16=False)
        model.train()
        traj = {"lr": [], "loss": [], "offsets": [], "mask": []}
        np.random.seed(5)
        torch.manual_seed(11)
        for it, (images, labels) in enumerate(data, start=1):
            batch = {"images": images, "labels": labels}
            sched.update_learning_rate(it)
            np_state = np.random.get_state()
            m = bop._create_mask(batch)
            np.random.set_state(np_state)
            st = torch.get_rng_state()
            offs = torch.randint(0, 4096 - WIDTH // 8, (LINES,))
            torch.set_rng_state(st)
            loss = trainer.train_step(batch)
            traj["lr"].append(sched.current_lr); traj["loss"].append(loss.item()); traj["offsets"].append(offs.numpy()); traj["mask"].append(m)
        for k, v in traj.items():
            fix[f"{variant}.{k}"] = np.stack(v)
        for k, v in np_sd(model).items():
            flat = v.reshape(-1)
            if flat.size > SAMPLES:
                idx = sample_index(k, flat.size)
                fix["index." + k] = idx.astype(np.int32)
                flat = flat[idx]
            fix[f"{variant}.sd3.{k}"] = flat
            fix[f"{variant}.dnorm.{k}"] = np.float64(np.linalg.norm(v.astype(np.float64) - sd0[k].astype(np.float64)))
            fix[f"{variant}.sd0sum.{k}"] = np.float64(sd0[k].astype(np.float64).sum())
    np.savez_compressed(os.path.join(out, "g22_bf16_trajectory.npz"), **fix)


if __name__ == "__main__":
    main()
