"""Plain f64 restatements of the entry points of csrc/ntxent_ragged.hip (NT-Xent on collated batches), one per entry point, written
from the formulas of include/pero_hip.h in the style of tests/parity_ref.py (each returns the result and `mag`, the sum of the absolute
values of the terms its formula adds), and the literal loss they serve: boolean indexing per line, with and without the pooled
negatives, on the concatenated batch.  Not a test module; it never calls the library."""
import math

import numpy as np
import torch

import parity_ref as R
from parity_ref import f64


def selected(image_mask, shift_mask):
    return (np.asarray(shift_mask) == 1) & (np.asarray(image_mask) == 1)


def slots(im1, im2, sm1, sm2):
    """pero_ntxent_slots by boolean indexing: slot_v[l][positions selected in view v] = 0, 1, 2, ...; count[l] = their number, -1 when the
    views differ."""
    lines, S = np.asarray(im1).shape
    slot1, slot2 = np.full((lines, S), -1, np.int32), np.full((lines, S), -1, np.int32)
    count = np.zeros(lines, np.int32)
    for l in range(lines):
        p1, p2 = np.flatnonzero(selected(im1[l], sm1[l])), np.flatnonzero(selected(im2[l], sm2[l]))
        slot1[l, p1] = np.arange(p1.size)
        slot2[l, p2] = np.arange(p2.size)
        count[l] = p1.size if p1.size == p2.size else -1
    return slot1, slot2, count


def rows_fwd(x, slot, count, Sp):
    """xn[l][k] = x[l][p] / max(|x[l][p]|, 1e-12), inv[l][k] the reciprocal norm, for slot[l][p] = k < max(count, 0); zeros behind.
    x (lines, S, d); count has lines or lines / 2 entries (line l uses count[l % len(count)])."""
    x = f64(x)
    lines, S, d = x.shape
    (full, finv), _ = R.rownorm(x.reshape(lines * S, d))
    full, finv = full.reshape(lines, S, d), finv.reshape(lines, S)
    xn, inv = torch.zeros(lines, Sp, d, dtype=torch.float64), torch.zeros(lines, Sp, dtype=torch.float64)
    for l in range(lines):
        m = max(int(count[l % len(count)]), 0)
        for p in range(S):
            k = int(slot[l][p])
            if 0 <= k < m:
                xn[l, k], inv[l, k] = full[l, p], finv[l, p]
    return (xn, inv), (xn.abs(), inv.abs())


def rows_bwd(xn, dxn, inv, slot, count, g):
    """dx[l][p] = (dxn[l][k] - xn[l][k] <xn[l][k], dxn[l][k]>) inv[l][k] g for slot[l][p] = k in [0, count); zero elsewhere."""
    xn, dxn, inv = f64(xn), f64(dxn), f64(inv)
    lines, Sp, d = xn.shape
    S = np.asarray(slot).shape[1]
    full, fmag = R.rownorm_bwd(xn.reshape(-1, d), dxn.reshape(-1, d), inv.reshape(-1), g)
    full, fmag = full.reshape(lines, Sp, d), fmag.reshape(lines, Sp, d)
    dx, mag = torch.zeros(lines, S, d, dtype=torch.float64), torch.zeros(lines, S, d, dtype=torch.float64)
    for l in range(lines):
        m = int(count[l % len(count)])
        for p in range(S):
            k = int(slot[l][p])
            if 0 <= k < m:
                dx[l, p], mag[l, p] = full[l, k], fmag[l, k]
    return dx, mag


def cols_ragged(sim, count, cross=None, own0=0):
    """pero_ntxent_cols_ragged: per line parity_ref.ntxent_cols / ntxent_cols_cross on the leading m x m block (and the first m rows of the
    line's part of cross), the gradients weighted 1 / (m lines) and embedded in zeros; m <= 0: NaN line loss, zero gradients.
    `ulps` as there (the worst over the lines)."""
    sim = f64(sim)
    lines, Sp, _ = sim.shape
    L = 0 if cross is None else cross.shape[1]
    cr = None if cross is None else f64(cross).reshape(lines, Sp, L)
    line_loss, mag_line = torch.full((lines,), math.nan, dtype=torch.float64), torch.zeros(lines, dtype=torch.float64)
    dsim, mag_dsim = torch.zeros_like(sim), torch.zeros_like(sim)
    dcross = mag_dcross = None
    if cr is not None:
        dcross, mag_dcross = torch.zeros_like(cr), torch.zeros_like(cr)
    ulps = 0
    for l in range(lines):
        m = int(count[l])
        if m <= 0:
            continue
        if cr is None:
            res, mag = R.ntxent_cols(sim[l:l + 1, :m, :m])
        else:
            res, mag = R.ntxent_cols_cross(sim[l:l + 1, :m, :m], cr[l, :m], own0 + l)
            dcross[l, :m] = res["dcross"] / lines
            mag_dcross[l, :m] = mag["dcross"] / lines
        line_loss[l], mag_line[l] = res["line_loss"][0], mag["line_loss"][0]
        dsim[l, :m, :m] = res["dsim"][0] / lines
        mag_dsim[l, :m, :m] = mag["dsim"][0] / lines
        ulps = max(ulps, mag["ulps"])
    out = {"loss": line_loss.mean().reshape(1), "line_loss": line_loss, "dsim": dsim}
    mags = {"loss": mag_line.mean().reshape(1), "line_loss": mag_line, "dsim": mag_dsim, "ulps": ulps}
    if cr is not None:
        out["dcross"], mags["dcross"] = dcross.reshape(lines * Sp, L), mag_dcross.reshape(lines * Sp, L)
    return out, mags


def line_mean_ragged(x, count, Sp):
    """out[l] = mean over the first count[l] rows of the line's block of Sp rows (0 for count <= 0)"""
    x = f64(x).reshape(len(count), Sp, -1)
    out, mag = torch.zeros(len(count), x.shape[2], dtype=torch.float64), torch.zeros(len(count), x.shape[2], dtype=torch.float64)
    for l, m in enumerate(int(c) for c in count):
        if m > 0:
            out[l], mag[l] = x[l, :m].mean(0), x[l, :m].abs().mean(0)
    return out, mag


def add_line_rows_ragged(dst0, src, count, Sp):
    """dst[l Sp + s] += src[l] / count[l] for s < count[l]"""
    dst, src = f64(dst0).clone().reshape(len(count), Sp, -1), f64(src)
    mag = dst.abs()
    for l, m in enumerate(int(c) for c in count):
        if m > 0:
            dst[l, :m] += src[l] / m
            mag[l, :m] += src[l].abs() / m
    return dst.reshape(len(count) * Sp, -1), mag.reshape(len(count) * Sp, -1)


def normalize(t):
    return t / torch.sqrt((t * t).sum(dim=-1, keepdim=True)).clamp_min(1e-12)


def loss(x, y, im1, im2, sm1, sm2, temperature=0.1, cross=False):
    """The loss of NTXentLoss(apply_masks=True) by boolean indexing, differentiable torch (f64 when x, y are): per line the normalised rows
    at the positions with shift mask == 1 and image mask == 1, the k-th of view 1 paired with the k-th of view 2; column-normalised
    softmax cross-entropy of their similarities / T, mean over the pairs, mean over all lines.  cross=True: every column's normaliser
    also holds normalize(mean of the selected view-1 rows) of every OTHER line of the (concatenated) batch."""
    xn, yn = normalize(x), normalize(y)
    n = x.shape[0]
    X = [xn[l][torch.from_numpy(selected(im1[l], sm1[l]))] for l in range(n)]
    Y = [yn[l][torch.from_numpy(selected(im2[l], sm2[l]))] for l in range(n)]
    p = normalize(torch.stack([a.mean(dim=0) for a in X])) if cross else None
    losses = []
    for l in range(n):
        sim = X[l] @ Y[l].t() / temperature
        cols = sim
        if cross:
            keep = torch.ones(n, dtype=torch.bool)
            keep[l] = False
            cols = torch.cat([sim, p[keep] @ Y[l].t() / temperature], dim=0)
        losses.append((torch.logsumexp(cols, dim=0) - torch.diag(sim)).mean())
    return torch.stack(losses).mean()


def collated_masks(widths=(480, 512, 400, 130, 512), seed=5, sub=8, pad=32):
    """Masks as BatchCreator draws them for paired lines of these widths (both views of a line have its width): random left paddings,
    image masks, three-valued shift masks.  Returns (im1, im2, sm1, sm2) uint8 (lines, S), S = (ceil(max / pad) pad + pad) / sub."""
    from pero_pretraining_amd.common.dataloader import BatchCreator
    rng = np.random.default_rng(seed)
    target = int(np.ceil(max(widths) / pad) * pad) + pad
    left1 = [int(rng.integers(0, target - w)) // sub for w in widths]
    left2 = [int(rng.integers(0, target - w)) // sub for w in widths]
    return BatchCreator._host_masks(list(widths), left1, list(widths), left2, [0] * len(widths), target // sub, sub)
