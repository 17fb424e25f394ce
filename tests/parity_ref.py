"""Plain torch f64 restatements of the C-ABI entry points of include/pero_hip.h, one per entry point, written from the
header's formula (not a test module; it never imports the library).  Shared by test_parity_ref_cpu.py (which pins these
restatements to the oracle and to torch autograd) and by the GPU parity tests.

Every function returns the result and, beside it, `mag`: the sum of the ABSOLUTE values of the terms the formula adds,
in f64.  An error bound is taken against `mag`, never against the result, so a sum that cancels gets no free pass.

The one comparison, `assert_within(got, ref, mag, n_terms, out_dtype, extra_ulps)`, holds per element

    |got - ref| <= (n_terms + 4 + extra_ulps) * 2^-24 * mag  (+ 2^-8 * |ref| for a bf16 output)  + 2^-126

2^-24 is the unit roundoff of f32: an f32 sum of n terms, added in ANY order, is within (n - 1) * 2^-24 * sum|terms| of
the exact sum (first order); the 4 covers the roundings of forming a term (a product, a difference, a division by a
count).  `extra_ulps` counts, in the same unit, what the library functions add: expf and logf are 1 ulp = 2 units
each, a correctly rounded sqrtf or division 1 unit, and an ABSOLUTE error e of the argument of expf is a RELATIVE error
e of its value (`exp_arg_units` turns the magnitudes an argument is formed from into units).  2^-8 is the figure the
suite already uses for one bf16 output rounding (tests/test_gpu_ops.py).  2^-126, the smallest normal f32 (and bf16), is
the underflow step: exp(-180) has no f32 value, and a result below the normal range may be flushed to zero.  bf16 inputs
are rounded once on the host and the reference is evaluated in f64 on the rounded values."""
import math

import torch

U32 = 2.0 ** -24
BF16_OUT = 2.0 ** -8
UNDERFLOW = 2.0 ** -126
EXPF, LOGF, SQRTF, DIVF = 2, 2, 1, 1   # error of one call, in units of 2^-24 relative


def f64(t):
    return torch.as_tensor(t).detach().cpu().double()


def bound(ref, mag, n_terms, out_dtype, extra_ulps=0):
    b = (n_terms + 4 + extra_ulps) * U32 * f64(mag) + UNDERFLOW
    if out_dtype == torch.bfloat16:
        b = b + BF16_OUT * f64(ref).abs()
    return b


def worst_ratio(got, ref, mag, n_terms, out_dtype, extra_ulps=0):
    """max over the elements of error / bound (0 / 0 counts as 0); NaN or inf where the reference is finite -> inf."""
    got, ref = f64(got), f64(ref)
    b = bound(ref, mag, n_terms, out_dtype, extra_ulps).expand_as(ref)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got) | ~torch.isfinite(ref), err, torch.full_like(err, math.inf))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    return ratio


RATIOS = {}   # "what [output type]" -> worst error / bound seen in this process (the GPU tests print it; DESIGN.md section 5 quotes it)


def assert_within(got, ref, mag, n_terms, out_dtype, extra_ulps=0, what=""):
    got_, ref_ = f64(got), f64(ref)
    assert got_.shape == ref_.shape, (what, tuple(got_.shape), tuple(ref_.shape))
    if ref_.numel() == 0:
        return 0.0
    ratio = worst_ratio(got_, ref_, mag, n_terms, out_dtype, extra_ulps)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    worst = float(ratio.max())
    if what:
        key = what + (" [bf16]" if out_dtype == torch.bfloat16 else " [f32]")
        RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    if worst > 1.0:
        flat = int(ratio.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref_.shape)) if ref_.dim() else ()
        b = bound(ref_, mag, n_terms, out_dtype, extra_ulps).expand_as(ref_)
        raise AssertionError(f"{what}: element {idx}: got {float(got_.reshape(-1)[flat])!r}, ref {float(ref_.reshape(-1)[flat])!r}, "
                             f"bound {float(b.reshape(-1)[flat])!r} (error / bound = {worst:.3g}; n_terms {n_terms}, extra_ulps {extra_ulps})")
    return worst


def exp_arg_units(*magnitudes):
    """Units of 2^-24 by which expf's value moves when its argument is formed in f32 from values of these magnitudes (each
    rounding of a value of magnitude a is an absolute error a * 2^-24 of the argument = a relative error of the value)."""
    return int(math.ceil(sum(float(m) for m in magnitudes)))


# ---------------------------------------------------------------------------------------------- VICReg pieces
def sqdiff(x, ix, y, iy, scale):
    """out = scale * sum_r |x[ix[r]] - y[iy[r]]|^2.  Terms: the squares (all of one sign)."""
    d = f64(x)[ix] - f64(y)[iy]
    out = scale * (d * d).sum().reshape(1)
    return out, out.abs()


def sqdiff_bwd(x, ix, y, iy, dx0, dy0, g, coef):
    """dx[ix[r]] += g coef (x - y), dy[iy[r]] -= g coef (x - y); rows outside ix / iy keep dx0 / dy0.  Terms per element: the
    old value, c x, c y."""
    x, y, dx, dy = f64(x), f64(y), f64(dx0).clone(), f64(dy0).clone()
    c = coef * (1.0 if g is None else float(g))
    t = c * (x[ix] - y[iy])
    tm = abs(c) * (x[ix].abs() + y[iy].abs())
    mx, my = dx.abs(), dy.abs()
    dx[ix] += t
    dy[iy] -= t
    mx[ix] += tm
    my[iy] += tm
    return (dx, dy), (mx, my)


def sum_scale(partial, scale):
    p = f64(partial)
    return (scale * p.sum()).reshape(1), (abs(scale) * p.abs().sum()).reshape(1)


def colsum(x, out0):
    """out[n] = out0[n] + sum_m x[m][n]"""
    x, o = f64(x), f64(out0)
    return o + x.sum(0), o.abs() + x.abs().sum(0)


def center_cols(z, colsum_, m, sumsq0):
    """zc = z - colsum / m for rows < m, 0 behind; sumsq[c] = sumsq0[c] + sum_r zc[r][c]^2.  The squares are those of the
    unrounded differences: their magnitude is taken from |z| + |mean|, so that the rounding of the difference (relative to
    |z| + |mean|, not to zc) is inside the bound - 2 zc dzc <= 2 * 3 units of (|z| + |mean|)^2: extra_ulps 6 at the call."""
    z, mu = f64(z), f64(colsum_) / m
    zc = torch.zeros_like(z)
    zc[:m] = z[:m] - mu
    mag_zc = torch.zeros_like(z)
    mag_zc[:m] = z[:m].abs() + mu.abs()
    sumsq = f64(sumsq0) + (zc * zc).sum(0)
    return (zc, sumsq), (mag_zc, f64(sumsq0).abs() + (mag_zc * mag_zc).sum(0))


def vicreg_std(sumsq, m, eps):
    return torch.sqrt(f64(sumsq) / (m - 1) + eps)


def vicreg_var(sumsq, m, threshold, eps):
    """loss_var = mean_j relu(thr - std_j), cvar_j = std_j < thr ? -1 / (d std_j (m - 1)) : 0.  Terms of the loss: thr / d and
    std_j / d of the active columns."""
    sd = vicreg_std(sumsq, m, eps)
    d = sd.numel()
    h = threshold - sd
    act = h > 0
    loss = torch.where(act, h, torch.zeros_like(h)).sum().reshape(1) / d
    cvar = torch.where(act, -1.0 / (d * sd * (m - 1)), torch.zeros_like(sd))
    mag_loss = torch.where(act, abs(threshold) + sd, torch.zeros_like(sd)).sum().reshape(1) / d
    return (cvar, loss), (cvar.abs(), mag_loss)


def vicreg_cov(cov, cvar, m, wv, wc):
    """loss_cov = sum_{i != j} cov_ij^2 / d; G_ij = wc 4 cov_ij / (d (m - 1)) (i != j), G_jj = wv cvar_j."""
    cov, cvar = f64(cov), f64(cvar)
    d = cov.shape[0]
    off = cov - torch.diag(torch.diag(cov))
    loss = ((off * off).sum() / d).reshape(1)
    G = wc * 4.0 * off / (d * (m - 1)) + torch.diag(wv * cvar)
    return (G, loss), (G.abs(), loss.abs())


def scatter_add_scaled(src, index, dst0, g):
    """dst[index[i]] += g src[i]"""
    gs = 1.0 if g is None else float(g)
    dst, mag = f64(dst0).clone(), f64(dst0).abs()
    dst[index] += gs * f64(src)
    mag[index] += abs(gs) * f64(src).abs()
    return dst, mag


# ---------------------------------------------------------------------------------------------- NT-Xent pieces
def rownorm(x):
    """inv[r] = 1 / max(|x_r|_2, 1e-12), xn = x inv.  (1e-12 as the f32 constant the header names.)  A relative error of the
    sum of d squares reaches inv halved and xn halved: n_terms d is on the safe side."""
    x = f64(x)
    floor = float(torch.tensor(1e-12, dtype=torch.float32))
    inv = 1.0 / torch.sqrt((x * x).sum(1)).clamp_min(floor)
    xn = x * inv[:, None]
    return (xn, inv), (xn.abs(), inv.abs())


def rownorm_bwd(xn, dxn, inv, g):
    """dx = (dxn - xn <xn, dxn>) inv g"""
    xn, dxn, inv = f64(xn), f64(dxn), f64(inv)
    gs = 1.0 if g is None else float(g)
    r = (inv * gs)[:, None]
    dot = (xn * dxn).sum(1, keepdim=True)
    dx = (dxn - xn * dot) * r
    mag = (dxn.abs() + xn.abs() * (xn * dxn).abs().sum(1, keepdim=True)) * r.abs()
    return dx, mag


def _lse_units(cols, lse):
    """Units of 2^-24 of the relative error of p = exp(s - lse) over a set of columns `cols` ([terms][S], the values one log-sum-exp
    normalises): the argument s - max is rounded (range), logf's own error on log(sum) and the rounding of `+ max` reach lse (2 |lse - max|
    + |lse|), and s - lse is rounded once more (|s - lse| <= range + |lse - max|)."""
    mx = cols.max(0).values
    rng = float((mx - cols.min(0).values).max())
    lm = float((lse - mx).abs().max())
    return exp_arg_units(rng, LOGF * lm, float(lse.abs().max()), rng + lm)


def ntxent_cols(sim):
    """sim (lines, S, S): lse_j = log sum_r exp(sim[l][r][j]); line_loss[l] = mean_j (lse_j - sim[l][j][j]); loss = mean_l;
    dsim[l][r][j] = (exp(sim[l][r][j] - lse_j) - [r == j]) / (S lines).
    Terms of line_loss: |lse_j| / S, |sim_jj| / S and 1 / S per column (the relative error of the sum of exponentials is an
    absolute error of its logarithm); of dsim: p / (S lines) and [r == j] / (S lines).  `ulps`: see _lse_units."""
    sim = f64(sim)
    lines, S, _ = sim.shape
    lse = torch.logsumexp(sim, dim=1)                       # (lines, S): over the rows r
    diag = torch.diagonal(sim, dim1=1, dim2=2)
    line_loss = (lse - diag).mean(1)
    loss = line_loss.mean().reshape(1)
    eye = torch.eye(S, dtype=torch.float64)
    p = torch.exp(sim - lse[:, None, :])
    dsim = (p - eye) / (S * lines)
    mag_line = (lse.abs() + diag.abs() + 1.0).mean(1)
    ulps = max(_lse_units(sim[l], lse[l]) for l in range(lines))
    res = {"loss": loss, "line_loss": line_loss, "dsim": dsim, "lse": lse}
    mag = {"loss": mag_line.mean().reshape(1), "line_loss": mag_line, "dsim": (p + eye) / (S * lines), "ulps": ulps}
    return res, mag


def ntxent_cols_cross(sim, cross, own0):
    """Column j of line l is normalised over its S own rows and the L - 1 pooled negatives cross[l S + j][l'], l' != own0 + l:
    lse_j = log(sum_i exp(sim[l][i][j]) + sum_{l' != own} exp(cross[l S + j][l'])), line_loss, loss, dsim as in ntxent_cols,
    dcross[l S + j][l'] = exp(cross - lse_j) / (S lines), 0 for the own line."""
    sim, cross = f64(sim), f64(cross)
    lines, S, _ = sim.shape
    L = cross.shape[1]
    cr = cross.reshape(lines, S, L)
    keep = torch.ones(lines, L, dtype=torch.bool)
    keep[torch.arange(lines), own0 + torch.arange(lines)] = False
    neg = torch.where(keep[:, None, :], cr, torch.full_like(cr, -math.inf))     # (lines, S = j, L)
    both = torch.cat([sim, neg.transpose(1, 2)], dim=1)                              # (lines, S + L, S = j)
    lse = torch.logsumexp(both, dim=1)
    diag = torch.diagonal(sim, dim1=1, dim2=2)
    line_loss = (lse - diag).mean(1)
    eye = torch.eye(S, dtype=torch.float64)
    w = 1.0 / (S * lines)
    p = torch.exp(sim - lse[:, None, :])
    q = torch.exp(neg - lse[:, :, None])                                              # exp(-inf) = 0 for the own line
    mag_line = (lse.abs() + diag.abs() + 1.0).mean(1)
    ulps = 0
    for l in range(lines):
        k = keep[l]
        cols = torch.cat([sim[l], cr[l][:, k].t()], dim=0)
        ulps = max(ulps, _lse_units(cols, lse[l]))
    res = {"loss": line_loss.mean().reshape(1), "line_loss": line_loss, "dsim": (p - eye) * w, "dcross": (q * w).reshape(lines * S, L), "lse": lse}
    mag = {"loss": mag_line.mean().reshape(1), "line_loss": mag_line, "dsim": (p + eye) * w, "dcross": (q * w).reshape(lines * S, L), "ulps": ulps}
    return res, mag


def line_mean(x, lines, S):
    x = f64(x).reshape(lines, S, -1)
    return x.mean(1), x.abs().mean(1)


def add_line_rows(dst0, src, lines, S, scale):
    """dst[l S + s][c] += scale src[l][c]"""
    dst, src = f64(dst0), f64(src)
    add = (scale * src)[:, None, :].expand(lines, S, src.shape[1]).reshape(lines * S, -1)
    return dst + add, dst.abs() + add.abs()


# ---------------------------------------------------------------------------------------------- BatchNorm1d (+ ReLU)
def bn_fwd(x, weight, bias, running_mean, running_var, eps, momentum, training, relu, running_mag=None):
    """training: mean, BIASED variance over the rows; rstd = 1 / sqrt(var + eps); running <- (1 - mom) running + mom batch, the running
    variance from the UNBIASED batch variance.  evaluation: the running statistics.  y = (x - mean) rstd w + b, then ReLU.
    Returns {y, mean, rstd, running_mean, running_var} and the same keys of magnitudes.  rstd's magnitude carries the factor
    (sum of |terms| of var + eps) / (var + eps) by which the rounding of the variance's terms is amplified; y's magnitude that of
    rstd times |w| (|x| + sum|x| / rows), plus |b|.  `running_mag`: magnitudes of the running buffers handed in (a second step)."""
    x, w, b = f64(x), f64(weight), f64(bias)
    rows = x.shape[0]
    res, mag = {}, {}
    if training:
        mean = x.sum(0) / rows
        mag_mean = x.abs().sum(0) / rows
        cen = x - mean
        mag_cen = x.abs() + mag_mean
        var = (cen * cen).sum(0) / rows
        mag_var = (mag_cen * mag_cen).sum(0) / rows
        if running_mean is not None:
            rm0, rv0 = f64(running_mean), f64(running_var)
            rmm, rvm = (rm0.abs(), rv0.abs()) if running_mag is None else running_mag
            unb = var * rows / (rows - 1) if rows > 1 else var
            res["running_mean"] = (1 - momentum) * rm0 + momentum * mean
            res["running_var"] = (1 - momentum) * rv0 + momentum * unb
            mag["running_mean"] = (1 - momentum) * rmm + momentum * mag_mean
            mag["running_var"] = (1 - momentum) * rvm + momentum * (mag_var * rows / max(rows - 1, 1))
    else:
        mean, var = f64(running_mean), f64(running_var)
        mag_mean, mag_var = mean.abs(), var.abs()
        mag_cen = x.abs() + mag_mean
    rstd = 1.0 / torch.sqrt(var + eps)
    amp = (mag_var + eps) / (var + eps)
    v = (x - mean) * rstd * w + b
    res.update(y=torch.clamp_min(v, 0.0) if relu else v, mean=mean, rstd=rstd)
    mag.update(y=mag_cen * (rstd * amp * w.abs()) + b.abs(), mean=mag_mean, rstd=rstd * amp)
    return res, mag


def bn_bwd(dy, x, y, weight, mean, rstd, dweight0, dbias0, relu):
    """g = dy (zeroed where the stored y <= 0 under relu); sg = sum_r g, sgx = sum_r g (x - mean);
    dx = w rstd (g - sg / rows - xhat sgx rstd / rows), xhat = (x - mean) rstd; dweight += sgx rstd; dbias += sg.
    mean, rstd: the saved f32 statistics (inputs)."""
    dy, x, w, mean, rstd = f64(dy), f64(x), f64(weight), f64(mean), f64(rstd)
    rows = x.shape[0]
    g = torch.where(f64(y) > 0, dy, torch.zeros_like(dy)) if relu else dy
    cen, mag_cen = x - mean, x.abs() + mean.abs()
    sg, sgx = g.sum(0), (g * cen).sum(0)
    msg, msgx = g.abs().sum(0), (g.abs() * mag_cen).sum(0)
    dx = w * rstd * (g - sg / rows - cen * rstd * sgx * rstd / rows)
    mag_dx = (w * rstd).abs() * (g.abs() + msg / rows + mag_cen * rstd * msgx * rstd / rows)
    res = {"dx": dx, "dweight": None if dweight0 is None else f64(dweight0) + sgx * rstd, "dbias": None if dbias0 is None else f64(dbias0) + sg}
    mag = {"dx": mag_dx, "dweight": None if dweight0 is None else f64(dweight0).abs() + msgx * rstd, "dbias": None if dbias0 is None else f64(dbias0).abs() + msg}
    return res, mag


# ---------------------------------------------------------------------------------------------- row kernels
def softmax(s, scale):
    """p = softmax(scale s) over the last dim.  `ulps`: the argument scale s - max is formed from scale s (one rounding of magnitude
    |scale s|) and a difference of magnitude up to the row's range."""
    a = f64(s) * scale
    p = torch.softmax(a, -1)
    rng = float((a.max(-1).values - a.min(-1).values).max())
    return p, {"p": p, "ulps": exp_arg_units(float(a.abs().max()), rng) + EXPF + DIVF}


def softmax_bwd(p, dp, scale):
    """ds = scale p (dp - sum_j p dp)"""
    p, dp = f64(p), f64(dp)
    dot = (p * dp).sum(-1, keepdim=True)
    return scale * p * (dp - dot), abs(scale) * p * (dp.abs() + (p * dp).abs().sum(-1, keepdim=True))


def masked_ce(logits, labels, mask, unmasked_weight, dloss=None):
    """loss = mean CE over mask == 1 (+ uw mean CE over mask == 0 & label >= 0) - the oracle's restatement, evaluated in f64 - and
    dlogits = dloss d loss / d logits = (softmax - onehot) weight(row) dloss.  Magnitude of a gradient element: (p + onehot) |weight dloss|;
    `ulps`: the relative error of p = exp(s - lse), as in _lse_units, over the rows that take part."""
    from oracle import pero_oracle as O
    lg, labels, mask = f64(logits), torch.as_tensor(labels).cpu(), torch.as_tensor(mask).cpu()
    loss = O.masked_cross_entropy(lg[None], labels[None], mask[None], unmasked_weight).reshape(1)
    rows, V = lg.shape
    m1 = mask == 1
    m0 = (mask == 0) & (labels >= 0) if unmasked_weight is not None else torch.zeros_like(m1)
    wrow = torch.zeros(rows, dtype=torch.float64)
    wrow[m1] = 1.0 / float(m1.sum())
    if unmasked_weight is not None:
        wrow[m0] = unmasked_weight / float(m0.sum())
    wrow = wrow * (1.0 if dloss is None else float(dloss))
    act = m1 | m0
    lse = torch.logsumexp(lg, -1)
    p = torch.exp(lg - lse[:, None])
    onehot = torch.zeros_like(lg)
    onehot[act, labels[act]] = 1.0
    grad = (p - onehot) * wrow[:, None]
    mag = (p + onehot) * wrow.abs()[:, None]
    ulps = _lse_units(lg[act].t(), lse[act]) if bool(act.any()) else 0
    return (loss, grad), {"loss": loss.abs(), "grad": mag, "ulps": ulps + EXPF + DIVF}


def rowdot_blocks(x, y):
    """out[m][b] = sum over columns 128 b .. 128 b + 127 of x[m][c] y[m][c]"""
    pr = f64(x) * f64(y)
    rows, cols = pr.shape
    return pr.reshape(rows, cols // 128, 128).sum(-1), pr.abs().reshape(rows, cols // 128, 128).sum(-1)
