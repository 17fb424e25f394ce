#!/usr/bin/env python3
"""Writes tests/golden/g24_ntxent_image_masks.npz: the reference's own NTXentLoss on the one kind of non-trivial masks it accepts.
Usage: make_golden_ntxent_masked.py REFERENCE_CHECKOUT.  The reference is imported only when this script runs; the tests that read the
file do not need it.

The reference indexes the shift-reduced similarity matrix with the full-length image masks (joint_embedding_pretraining/losses.py:78),
so it runs only when every shift mask is all ones; the image masks may then be anything with equal counts per line.  On such masks its
value is the definition NTXentLoss(apply_masks=True) implements (positions with shift mask == 1 and image mask == 1, k-th with k-th).

Shapes as g9: n = 3, S = 24, D = 40, f32, default_rng(24).  Image masks: line 0 selects 17 positions in both views at the same
places, line 1 selects 9 positions at DIFFERENT places in the two views, line 2 selects all 24.  Stored: x, y, the four masks, and the
reference's loss, grad_x, grad_y; asserted here: the f64 restatement of the definition agrees within 1e-5 (the reference is f32).
Also stored: whether the reference raises IndexError on masks of its own BatchCreator (widths 480, 512, 400, 130, 512), the masks
themselves and the per-line selected counts of the two views."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g24_ntxent_image_masks.npz")
WIDTHS = (480, 512, 400, 130, 512)


def definition_f64(x, y, im1, im2, sm1, sm2, temperature=0.1):
    x, y = torch.from_numpy(x).double(), torch.from_numpy(y).double()
    xn = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    yn = y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    losses = []
    for l in range(x.shape[0]):
        a = xn[l][torch.from_numpy((sm1[l] == 1) & (im1[l] == 1))]
        b = yn[l][torch.from_numpy((sm2[l] == 1) & (im2[l] == 1))]
        sim = a @ b.t() / temperature
        losses.append((torch.logsumexp(sim, dim=0) - torch.diag(sim)).mean())
    return float(torch.stack(losses).mean())


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from pero_pretraining.common import dataloader as R_dl
    from pero_pretraining.joint_embedding_pretraining import losses as R_jl

    rng = np.random.default_rng(24)
    n, S, D = 3, 24, 40
    x = rng.standard_normal((n, S, D)).astype(np.float32)
    y = (x + 1.5 * rng.standard_normal((n, S, D))).astype(np.float32)
    im1, im2 = np.zeros((n, S), np.uint8), np.zeros((n, S), np.uint8)
    im1[0, 3:20] = 1; im2[0, 3:20] = 1            # 17 pairs, same places
    im1[1, 2:11] = 1; im2[1, 12:21] = 1           # 9 pairs, view 2 ten positions further right
    im1[2, :] = 1; im2[2, :] = 1                  # all 24
    y[1, 12:21] = x[1, 2:11] + (y[1, 2:11] - x[1, 2:11])   # line 1: the k-th selected row of view 2 is the noisy copy of the k-th of view 1
    sm1, sm2 = np.ones((n, S), np.uint8), np.ones((n, S), np.uint8)

    xv, yv = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(y).requires_grad_(True)
    res = R_jl.NTXentLoss()(xv, yv, *(torch.from_numpy(m) for m in (im1, im2, sm1, sm2)))
    res["loss"].backward()
    loss = float(res["loss"].detach())
    ref64 = definition_f64(x, y, im1, im2, sm1, sm2)
    print(f"reference {loss:.7f}   definition (f64) {ref64:.7f}")
    assert abs(loss - ref64) < 1e-5 * ref64
    np.random.seed(5)
    data = [{"image": rng.integers(0, 256, (40, w, 3), dtype=np.uint8), "image2": rng.integers(0, 256, (40, w, 3), dtype=np.uint8),
             "labels": None, "image_id": str(i)} for i, w in enumerate(WIDTHS)]
    batch = R_dl.BatchCreator().create_batch(data)
    masks = [np.asarray(batch[k]).astype(np.uint8) for k in ("image_masks", "image_masks2", "shift_masks", "shift_masks2")]
    B, Sc = masks[0].shape
    xc = torch.from_numpy(rng.standard_normal((B, Sc, 8)).astype(np.float32))
    raised = False
    try:
        R_jl.NTXentLoss()(xc, xc.clone(), *(torch.from_numpy(m) for m in masks))
    except IndexError:
        raised = True
    c1 = ((masks[2] == 1) & (masks[0] == 1)).sum(1)
    c2 = ((masks[3] == 1) & (masks[1] == 1)).sum(1)
    print(f"collated masks: S = {Sc}, selected {c1.tolist()} / {c2.tolist()}, reference raises IndexError: {raised}")
    assert raised and np.array_equal(c1, c2)
    assert bool(((masks[2] != 1) | (masks[0] == 1)).all()) and bool(((masks[3] != 1) | (masks[1] == 1)).all())   # shift == 1 implies image == 1

    np.savez_compressed(OUT, x=x, y=y, image_masks1=im1, image_masks2=im2, shift_masks1=sm1, shift_masks2=sm2, loss=np.float64(loss),
                        loss_definition_f64=np.float64(ref64), grad_x=xv.grad.numpy(), grad_y=yv.grad.numpy(),
                        collated_masks_raise_indexerror=np.bool_(raised), collated_widths=np.array(WIDTHS, np.int32),
                        collated_image_masks1=masks[0], collated_image_masks2=masks[1], collated_shift_masks1=masks[2],
                        collated_shift_masks2=masks[3], collated_counts=c1.astype(np.int32))
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
