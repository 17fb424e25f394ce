"""Barlow Twins in torch, dtype-generic (the tests run it in f64): the loss as BarlowTwinsLoss defines it, differentiable by autograd, and
a second, hand-written backward in exactly the stages of the kernels (G, d zh, a, b, dz)."""
import numpy as np
import torch


def pairs(shift_masks1, shift_masks2):
    """Flat row indices of the paired positions: the k-th position with shift mask 1 == 1 and the k-th with shift mask 2 == 1."""
    ix = np.flatnonzero(np.asarray(shift_masks1).reshape(-1) == 1)
    iy = np.flatnonzero(np.asarray(shift_masks2).reshape(-1) == 1)
    return ix, iy


def standardize(z, eps):
    mu = z.mean(dim=0)
    var = ((z - mu) ** 2).mean(dim=0)   # biased, as BatchNorm1d normalises
    rstd = 1.0 / torch.sqrt(var + eps)
    return (z - mu) * rstd, mu, rstd


def loss_from_rows(z1, z2, lam=0.0051, eps=1e-5):
    """(loss, on, off, (zh1, zh2, rstd1, rstd2, c)) of the paired rows z1, z2 (n, D)."""
    n = z1.shape[0]
    zh1, _, rstd1 = standardize(z1, eps)
    zh2, _, rstd2 = standardize(z2, eps)
    c = zh1.T @ zh2 / n
    diag = torch.diagonal(c)
    on = ((diag - 1.0) ** 2).sum()
    off = (c ** 2).sum() - (diag ** 2).sum()
    return on + lam * off, on, off, (zh1, zh2, rstd1, rstd2, c)


def barlow_loss(x, y, shift_masks1, shift_masks2, lam=0.0051, eps=1e-5):
    """The loss on (N, S, D) inputs and (N, S) shift masks: {"loss", "loss.on_diagonal", "loss.off_diagonal"}."""
    ix, iy = pairs(shift_masks1, shift_masks2)
    assert ix.size == iy.size and ix.size > 0
    D = x.shape[-1]
    z1 = x.reshape(-1, D)[torch.from_numpy(ix)]
    z2 = y.reshape(-1, D)[torch.from_numpy(iy)]
    loss, on, off, _ = loss_from_rows(z1, z2, lam, eps)
    return {"loss": loss, "loss.on_diagonal": on.detach(), "loss.off_diagonal": off.detach()}


def staged_backward(z1, z2, lam=0.0051, eps=1e-5, g=1.0):
    """(dz1, dz2) by the kernels' stages, no autograd."""
    n = z1.shape[0]
    with torch.no_grad():
        _, _, _, (zh1, zh2, rstd1, rstd2, c) = loss_from_rows(z1, z2, lam, eps)
        G = 2.0 * lam * c / n
        G.diagonal().copy_(2.0 * (torch.diagonal(c) - 1.0) / n)
        dzh1 = zh2 @ G.T
        dzh2 = zh1 @ G
        out = []
        for dzh, zh, rstd in ((dzh1, zh1, rstd1), (dzh2, zh2, rstd2)):
            a = dzh.sum(dim=0)
            b = (dzh * zh).sum(dim=0)
            out.append(g * rstd * (dzh - a / n - zh * b / n))
    return out[0], out[1]
