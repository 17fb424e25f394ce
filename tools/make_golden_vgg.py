#!/usr/bin/env python3
"""Writes tests/golden/g30_vgg_encoder.npz: the reference's own VGGEncoder(pretrained_vgg_layers=0, base_channels=8) on CPU.
Usage: make_golden_vgg.py REFERENCE_CHECKOUT.  The reference is imported only when this script runs; the tests that read the file do
not need it.

Stored: the state-dict names in order (`names`) and every entry as `param.<name>` (so names and shapes are the reference's), a uint8
(3, 40, 72, 3) input (`images`), the f32 output on `images / 255.` prepared as autoencoders/batch_operator.py:14 does (`output`), the
output shape of every module of `encoder` and of the aggregation layer (`layer_names`, `layer_shapes`), and the constructor's
attributes (`out_channels`, `base_channels`).  The weights are seeded (tests/vgg_ref.py seeded_state, seed 30): He-scaled convolution
weights, biases in +-0.5, non-trivial BatchNorm weight (some negative), bias, running mean and variance - the default initialisation
gives features of 0.06 and tests nothing.  Asserted here: the f64 restatement of tests/vgg_ref.py agrees within 1e-5 of the feature
scale (the reference is f32).  About 33 k parameters; data only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g30_vgg_encoder.npz")
SEED, BASE, SHAPE = 30, 8, (3, 40, 72, 3)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vgg_ref as V
    from pero_pretraining.models.autoencoders import VGGEncoder

    enc = VGGEncoder(pretrained_vgg_layers=0, base_channels=BASE).eval()
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert shapes == V.encoder_shapes(BASE), "tests/vgg_ref.py encoder_shapes disagrees with the reference's state dict"
    state = V.seeded_state(shapes, SEED)
    enc.load_state_dict(state, strict=True)
    images = V.smooth_images(SHAPE, SEED)
    x = torch.from_numpy(images / 255.).float().permute(0, 3, 1, 2)
    layer_names, layer_shapes = [], []
    with torch.no_grad():
        y = x
        for i, m in enumerate(enc.encoder):
            y = m(y)
            layer_names.append(f"encoder.{i}")
            layer_shapes.append(tuple(y.shape))
        y = enc.aggregation_layer(y)
        layer_names.append("aggregation_layer")
        layer_shapes.append(tuple(y.shape))
        out = enc(x)
    assert torch.equal(out, y)
    ref64 = V.encoder_forward(state, torch.from_numpy(images))[0]
    scale = float(ref64.abs().max())
    diff = float((out.double() - ref64).abs().max())
    print(f"reference output {tuple(out.shape)}, feature scale {scale:.3f}, |reference - f64 restatement| max {diff:.3e} ({diff / scale:.2e} relative)")
    assert diff < 1e-5 * scale
    params = {"param." + k: v.numpy() for k, v in state.items()}
    np.savez_compressed(OUT, names=np.array(list(state)), images=images, output=out.numpy(), layer_names=np.array(layer_names),
                        layer_shapes=np.array(layer_shapes, np.int64), out_channels=np.int64(enc.out_channels), base_channels=np.int64(BASE),
                        **params)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {sum(v.numel() for v in state.values())} parameters)")


if __name__ == "__main__":
    main()
