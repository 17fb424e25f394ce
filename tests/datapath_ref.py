"""Plain numpy / f64 restatements of the data-path entry points of include/pero_hip.h - the front end (csrc/misc.hip), the collator
(csrc/collate.hip), the quantizer (csrc/vq.hip), the evaluation rank kernel (csrc/eval.hip) and LayerNorm (csrc/rowops.hip) - written
from the header's text and parameterised by every size the C ABI takes (not a test module; it never imports the library).  Shared by
test_datapath_ref_cpu.py, which ties each restatement to the oracle, and by test_gpu_datapath_parity.py.

Byte, integer and copy results are exact (numpy arrays compared with array_equal).  Float results follow tests/parity_ref.py: every
function returns the f64 result and, beside it, `mag` - the sum of the absolute values of the terms the formula adds - for
parity_ref.assert_within.  The second half of the file builds the INPUTS of the GPU cases that carry a coverage condition (the collation
lines, the planted codebooks), so that the CPU test can assert those conditions on the very inputs the GPU test runs."""
import numpy as np
import torch

F32 = np.float32


def f64(t):
    return torch.as_tensor(t).detach().cpu().double()


# ---------------------------------------------------------------------------------------------- front end
def _tile_rows(tile, C, H, P):
    return np.asarray(tile, dtype=F32).reshape(C * H * P)


def patches_u8(images, mask, tile, P, ld_out):
    """images u8 (N, H, W, C) -> f32 (N * S, ld_out), S = W / P: column (c * H + h) * P + p of row n * S + s is
    f32(images[n][h][s * P + p][c]) / f32(255) (one IEEE division), the whole row is the (C, H, P) tile where mask[n][s] == 1, and the
    columns from C * H * P up to ld_out are zero.  mask (N, S) or None."""
    images = np.asarray(images)
    N, H, W, C = images.shape
    S = W // P
    x = images.astype(F32) / F32(255)
    rows = x.reshape(N, H, S, P, C).transpose(0, 2, 4, 1, 3).reshape(N * S, C * H * P)
    return _finish_rows(rows, mask, tile, C, H, P, ld_out)


def patches_f32(images_nchw, mask, tile, P, ld_out):
    """The same rows from f32 (N, C, H, W) images, copied as they are."""
    x = np.asarray(images_nchw, dtype=F32)
    N, C, H, W = x.shape
    S = W // P
    rows = x.reshape(N, C, H, S, P).transpose(0, 3, 1, 2, 4).reshape(N * S, C * H * P)
    return _finish_rows(rows, mask, tile, C, H, P, ld_out)


def _finish_rows(rows, mask, tile, C, H, P, ld_out):
    out = np.zeros((rows.shape[0], ld_out), dtype=F32)
    out[:, :C * H * P] = rows
    if mask is not None:
        out[np.asarray(mask).reshape(-1) == 1, :C * H * P] = _tile_rows(tile, C, H, P)
    return out


def apply_mask(images_nchw, mask, tile, P):
    """f32 (N, C, H, W): pixel (n, c, h, w) becomes tile[c][h][w % P] where mask[n][w / P] == 1.  Returns a new array."""
    x = np.array(images_nchw, dtype=F32)
    N, C, H, W = x.shape
    t = np.asarray(tile, dtype=F32).reshape(C, H, P)
    m = np.asarray(mask).reshape(N, W // P)
    for n in range(N):
        for s in np.nonzero(m[n] == 1)[0]:
            x[n, :, :, s * P:(s + 1) * P] = t
    return x


# ---------------------------------------------------------------------------------------------- collation
def stack_lines(packed, offsets, widths, left_px, B, H, Wt, C):
    """A zero (B, H, Wt, C) u8 batch plus one slice copy per line: line b is (H, widths[b], C) row-major at byte offsets[b] of `packed`
    and lands at columns [left_px[b], left_px[b] + widths[b])."""
    packed = np.asarray(packed, dtype=np.uint8)
    out = np.zeros((B, H, Wt, C), dtype=np.uint8)
    for b in range(B):
        w, lp, o = int(widths[b]), int(left_px[b]), int(offsets[b])
        out[b, :, lp:lp + w, :] = packed[o:o + H * w * C].reshape(H, w, C)
    return out


def line_masks(widths1, left1, S, sub, widths2=None, left2=None, crop_shifts=None):
    """image mask: 1 on the ceil(width / sub) label positions from left (in label positions) on.  With a second view: shift =
    crop_shift + left1 - left2; the first shift mask is 1 on row[shift:] (shift >= 0) or row[:shift] (shift < 0) - Python slices, which
    clamp -, the second is its reverse; a 1 outside the view's own image mask becomes 2.  Returns (im1, im2, sm1, sm2, shifts); the last
    four are None without a second view."""
    def image_mask(widths, left):
        m = np.zeros((len(widths), S), dtype=np.uint8)
        for b, (w, a) in enumerate(zip(widths, left)):
            m[b, int(a):int(a) + (int(w) + sub - 1) // sub] = 1
        return m
    im1 = image_mask(widths1, left1)
    if widths2 is None:
        return im1, None, None, None, None
    im2 = image_mask(widths2, left2)
    cs = np.zeros(len(widths1), dtype=np.int64) if crop_shifts is None else np.asarray(crop_shifts, dtype=np.int64)
    shifts = (cs + np.asarray(left1, dtype=np.int64) - np.asarray(left2, dtype=np.int64)).astype(np.int32)
    sm1 = np.zeros_like(im1)
    for row, shift in zip(sm1, shifts.tolist()):
        if shift < 0:
            row[:shift] = 1
        else:
            row[shift:] = 1
    sm2 = np.copy(sm1[:, ::-1])
    sm1[(sm1 == 1) & (im1 == 0)] = 2
    sm2[(sm2 == 1) & (im2 == 0)] = 2
    return im1, im2, sm1, sm2, shifts


# ---------------------------------------------------------------------------------------------- quantizer
def vq_distances(x, e, copies=()):
    """dist[m][k] = |x_m|^2 + |e_k|^2 - 2 x_m . e_k in f64.  Returns a dict: dist, index (first minimum), best, margin (second best
    minus best; inf with one code), mag[m] = |x_m|^2 + max_k |e_k|^2 (the magnitude the f32 evaluation's rounding is relative to).
    `copies`: codes that are bit-for-bit copies of a code with a lower index - they can never be the first minimum and are left out of
    the margin (the margin of a row is to the nearest code that DIFFERS from its best)."""
    x, e = np.asarray(x, dtype=np.float64), np.asarray(e, dtype=np.float64)
    sx, se = (x * x).sum(1), (e * e).sum(1)
    dist = (sx[:, None] + se[None, :]) - 2.0 * (x @ e.T)
    index = np.argmin(dist, axis=1)
    srt = np.sort(np.delete(dist, list(copies), axis=1), axis=1)
    margin = srt[:, 1] - srt[:, 0] if dist.shape[1] > 1 else np.full(x.shape[0], np.inf)
    return {"dist": dist, "index": index.astype(np.int64), "best": srt[:, 0], "margin": margin, "mag": sx + se.max()}


def vq_gather(x, e, idx):
    """quantized = x + (e[idx] - x), two f32 roundings in this order"""
    x, e = np.asarray(x, dtype=F32), np.asarray(e, dtype=F32)
    return x + (e[np.asarray(idx)] - x)


def vq_ema_update(x, idx, cluster0, ema_w0, decay, epsilon):
    """The header's EMA update in f64 with its scalar rules: decay, 1 - decay, epsilon and K * epsilon are formed in double and rounded
    to f32 before use.  counts[k] = #{m : idx[m] = k}, dw[k] = sum of the rows on code k (dw_abs: of their absolute values),
    pre = cluster0 decay + (1 - decay) counts, n = sum(pre), cluster = (pre + eps) / (n + K eps) n,
    ema_w = ema_w0 decay + (1 - decay) dw, codebook = ema_w / cluster[k].  Returns (results, magnitudes)."""
    x, w0, c0 = np.asarray(x, dtype=np.float64), np.asarray(ema_w0, dtype=np.float64), np.asarray(cluster0, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    K, D = w0.shape
    fd, omd, eps, keps = float(F32(decay)), float(F32(1.0 - decay)), float(F32(epsilon)), float(F32(K * epsilon))
    counts = np.bincount(idx, minlength=K).astype(np.float64)
    dw, dw_abs = np.zeros((K, D)), np.zeros((K, D))
    np.add.at(dw, idx, x)
    np.add.at(dw_abs, idx, np.abs(x))
    pre = c0 * fd + omd * counts
    n = pre.sum()
    cluster = (pre + eps) / (n + keps) * n
    ema_w = w0 * fd + omd * dw
    mag_w = np.abs(w0) * fd + omd * dw_abs
    res = {"counts": counts, "dw": dw, "cluster": cluster, "ema_w": ema_w, "codebook": ema_w / cluster[:, None]}
    mag = {"dw": dw_abs, "cluster": np.abs(c0) * fd + omd * counts + eps, "ema_w": mag_w, "codebook": mag_w / np.abs(cluster)[:, None]}
    return res, mag


# ---------------------------------------------------------------------------------------------- evaluation
def label_ranks(logits, labels, mask):
    """int32 (rows, 3): gt = #{j : logit[j] > x}, eq_lo / eq_hi = #{j : logit[j] == x, j < label / j > label}, x = logit[label], for
    the rows with mask == 1; (V, 0, 0) where the label is outside [0, V); -1 where mask != 1.  Comparisons are IEEE (-inf == -inf)."""
    lg = np.asarray(logits, dtype=np.float64)
    rows, V = lg.shape
    out = np.full((rows, 3), -1, dtype=np.int32)
    for r in range(rows):
        if int(mask[r]) != 1:
            continue
        lab = int(labels[r])
        if lab < 0 or lab >= V:
            out[r] = (V, 0, 0)
            continue
        gt = lo = hi = 0
        x = lg[r, lab]
        for j in range(V):
            v = lg[r, j]
            gt += v > x
            lo += (v == x) and j < lab
            hi += (v == x) and j > lab
        out[r] = (gt, lo, hi)
    return out


def rank_counters(ranks, ks):
    """The header's counters for one call: [rows with mask == 1] + [rows whose label is not in the top k, for k in ks]
    (k == 1: gt + eq_lo >= 1, the first maximum; k > 1: gt + eq_hi >= k, the stable-argsort order)."""
    act = ranks[ranks[:, 0] >= 0]
    out = [len(act)]
    for k in ks:
        out.append(int(np.sum((act[:, 0] + act[:, 1]) >= 1)) if k == 1 else int(np.sum((act[:, 0] + act[:, 2]) >= k)))
    return np.asarray(out, dtype=np.int64)


# ---------------------------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x, gamma, beta, eps, pe=None, offsets=None, S=1):
    """mean and biased variance over the row, rstd = 1 / sqrt(var + eps), y = (x - mean) rstd gamma + beta (+ pe[offsets[row / S] + row % S]).
    Magnitudes as parity_ref.bn_fwd: rstd's carries the factor amp = (sum of |terms| of var + eps) / (var + eps) by which the rounding of
    the variance's terms is amplified; y's is rstd |gamma| (sum|x| / d + (|x| + sum|x| / d) amp) + |beta| + |pe|, i.e. the share of the
    mean's d-term sum plus the share of the variance's d-term sum (a relative error of var is half that of rstd: on the safe side)."""
    x, g, b = f64(x), f64(gamma), f64(beta)
    rows, d = x.shape
    mean = x.sum(1) / d
    mag_mean = x.abs().sum(1) / d
    cen = x - mean[:, None]
    mag_cen = x.abs() + mag_mean[:, None]
    var = (cen * cen).sum(1) / d
    mag_var = (mag_cen * mag_cen).sum(1) / d
    rstd = 1.0 / torch.sqrt(var + eps)
    amp = (mag_var + eps) / (var + eps)
    y = cen * rstd[:, None] * g + b
    mag_y = (mag_mean[:, None] + mag_cen * amp[:, None]) * rstd[:, None] * g.abs() + b.abs()
    if pe is not None:
        r = torch.arange(rows)
        off = torch.zeros(rows, dtype=torch.int64) if offsets is None else torch.as_tensor(offsets).cpu().long()[r // S]
        add = f64(pe)[off + r % S]
        y, mag_y = y + add, mag_y + add.abs()
    return {"y": y, "mean": mean, "rstd": rstd}, {"y": mag_y, "mean": mag_mean, "rstd": rstd * amp}


def _ln_bwd(dy, xh, mag_xh, rstd, gamma, dgamma0, dbeta0, dxsum0):
    dy, g, rs = f64(dy), f64(gamma), f64(rstd)[:, None]
    d = dy.shape[1]
    gy = dy * g
    c1, c2 = gy.sum(1, keepdim=True) / d, (gy * xh).sum(1, keepdim=True) / d
    m1, m2 = gy.abs().sum(1, keepdim=True) / d, (gy.abs() * mag_xh).sum(1, keepdim=True) / d
    dx = rs * (gy - c1 - xh * c2)
    mag_dx = rs.abs() * (gy.abs() + m1 + mag_xh * m2)
    res = {"dx": dx, "dgamma": f64(dgamma0) + (dy * xh).sum(0), "dbeta": f64(dbeta0) + dy.sum(0)}
    mag = {"dx": mag_dx, "dgamma": f64(dgamma0).abs() + (dy.abs() * mag_xh).sum(0), "dbeta": f64(dbeta0).abs() + dy.abs().sum(0)}
    if dxsum0 is not None:
        res["dxsum"], mag["dxsum"] = f64(dxsum0) + dx.sum(0), f64(dxsum0).abs() + mag_dx.sum(0)
    return res, mag


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma0, dbeta0, dxsum0=None):
    """From the input rows and the SAVED f32 statistics (inputs): xhat = (x - mean) rstd, g = dy gamma,
    dx = rstd (g - mean_j g - xhat mean_j (g xhat)); dgamma += sum_rows dy xhat, dbeta += sum_rows dy, dxsum += sum_rows dx.
    xhat's magnitude is (|x| + |mean|) rstd - the difference is rounded relative to its operands, not to its value."""
    x, mu, rs = f64(x), f64(mean)[:, None], f64(rstd)[:, None]
    return _ln_bwd(dy, (x - mu) * rs, (x.abs() + mu.abs()) * rs, rstd, gamma, dgamma0, dbeta0, dxsum0)


def layernorm_bwd_out(dy, t, rstd, gamma, beta, dgamma0, dbeta0, dxsum0=None):
    """The same from the layer's output t = xhat gamma + beta: xhat = (t - beta) / gamma (gamma != 0), magnitude (|t| + |beta|) / |gamma|."""
    t, g, b = f64(t), f64(gamma), f64(beta)
    return _ln_bwd(dy, (t - b) / g, (t.abs() + b.abs()) / g.abs(), rstd, gamma, dgamma0, dbeta0, dxsum0)


# ---------------------------------------------------------------------------------------------- inputs of the GPU cases
# (H, C, P, W, pitch beyond C H P or None for the default pitch, bytes by which the u8 images are shifted inside their allocation)
PATCH_CASES = [
    (40, 3, 8, 256, None, 0),   # 16-byte staging, two blocks of 16 tokens: the second has s0 != 0
    (40, 3, 8, 200, None, 0),   # 4-byte staging (the shape the suite already runs)
    (7, 1, 3, 51, None, 0),     # byte staging: row pitch 51; 17 tokens, the second block holds one
    (40, 3, 8, 128, None, 1),   # byte staging at the production shape: the images start 1 byte into their allocation
    (90, 3, 2, 40, None, 0),    # C H = 270 > 256: the tall-patch branch
    (32, 2, 8, 64, None, 0),    # C H a power of two, four tokens per pass
    (1, 1, 8, 16, None, 0),     # C H = 1
    (40, 3, 8, 128, 4, 0),      # bf16: a pitch that is no multiple of 8 - scalar stores, scalar padding
    (5, 3, 4, 16, 8, 0),        # bf16: P = 4 - scalar stores; C H P = 60 is no multiple of 8 either: scalar padding
    (6, 3, 4, 16, 8, 0),        # bf16: P = 4 - scalar stores; C H P = 72, pitch 80: 16-byte padding
    (40, 3, 8, 128, 0, 0),      # pitch exactly C H P: no padding
]
PT_TOK = 16   # tokens per workgroup of patches_u8_k


def patch_branches(H, C, P, W, pitch, shift, itemsize, out_addr=0):
    """The code paths of patches_u8_k for one launch, restated from its conditions: the set of staging forms over its blocks
    ("stage16" / "stage4" / "stage1"), the index scheme ("tall" or "pow2"), the store form ("store16" / "store1") and the padding form
    ("pad16" / "pad1" / "nopad").  `shift`: the images' address modulo 16; `itemsize`: 4 (f32) or 2 (bf16)."""
    S, pd = W // P, C * H * P
    ld = pd if pitch is None else pd + pitch
    out = set()
    for s0 in range(0, S, PT_TOK):
        rowbytes = min(PT_TOK, S - s0) * P * C
        al = [rowbytes, W * C, s0 * P * C, shift]
        out.add("stage16" if all(v % 16 == 0 for v in al) else "stage4" if all(v % 4 == 0 for v in al) else "stage1")
        if s0:
            out.add("block>0:" + ("stage16" if all(v % 16 == 0 for v in al) else "stage4" if all(v % 4 == 0 for v in al) else "stage1"))
    chp = 1
    while chp < C * H:
        chp *= 2
    out.add("tall" if chp > 256 else "pow2")
    vec = itemsize == 2 and ld % 8 == 0 and out_addr % 16 == 0
    out.add("store16" if vec and P == 8 and chp <= 256 else "store1")
    out.add("nopad" if ld == pd else "pad16" if vec and (ld - pd) % 8 == 0 and pd % 8 == 0 else "pad1")
    return out


def patch_mask(N, S):
    """Both values in every block of 16 tokens (a one-token block differs between the two lines), and a 2, which is not a set bit."""
    s, n = np.meshgrid(np.arange(S), np.arange(N))
    m = ((s + n) % 2).astype(np.int64)
    m[(s + n) % 6 == 2] = 2
    return m


# (width, left_px) of the lines of one collation case at Wt = 32: widths 1, 2 and 5, a line that ends exactly at the row end (3 + 29), a
# full-width line, and left paddings / widths of every residue modulo 4
STACK_LINES_WT = 32
STACK_LINES = [(1, 0), (2, 1), (5, 2), (7, 3), (3, 29), (32, 0), (6, 5), (4, 11), (1, 25)]


def stack_lines_case(C, H, Wt=STACK_LINES_WT, lines=None, seed=0):
    """packed (the lines back to back, pixel values 1..254 so that neither a zero nor a slack byte passes for one, then the 8 documented
    slack bytes, 0xFF), offsets, widths, left_px."""
    lines = STACK_LINES if lines is None else lines
    rng = np.random.default_rng(1000 * C + 10 * H + seed)
    widths = np.asarray([w for w, _ in lines], dtype=np.int32)
    left = np.asarray([l for _, l in lines], dtype=np.int32)
    assert int((widths + left).max()) <= Wt and int(widths.min()) >= 1 and int(left.min()) >= 0
    sizes = widths.astype(np.int64) * H * C
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    packed = np.concatenate([rng.integers(1, 255, int(sizes.sum()), dtype=np.uint8), np.full(8, 0xFF, dtype=np.uint8)])
    return packed, offsets, widths, left


def stack_lines_residues(offsets, widths, left_px, H, C):
    """The three address residues modulo 4 that select stack_lines_k's paths: of lo = left_px C, of hi = lo + width C, and of the source
    address offsets[b] + h width C - lo, the last over all (b, h)."""
    lo = left_px.astype(np.int64) * C
    hi = lo + widths.astype(np.int64) * C
    src = {int((offsets[b] + h * int(widths[b]) * C - lo[b]) % 4) for b in range(len(widths)) for h in range(H)}
    return {int(v % 4) for v in lo}, {int(v % 4) for v in hi}, src


VQ_SHAPES = [(1, 1, 1), (65, 33, 5), (70, 200, 40), (64, 128, 16), (64, 128, 32), (128, 256, 64)]
# duplicate codes (c, c + delta): + 4 is the other lane half (both orders: code 1 sits in lanes 0-31, code 12 in lanes 32-63), + 32 the
# other accumulator of the generic kernel / the next wave of the fast one, + 64 the other wave column / wave, + 128 the next code tile
VQ_PLANTS = [(1, 4), (12, 4), (0, 32), (3, 64), (8, 128)]
NEAR_TIE_CAP = 0.02


def vq_case(M, K, D):
    """x (M, D), codebook (K, D) f32, and the planted rows: a list of (row, lower code, higher code) - codebook[higher] is a copy of
    codebook[lower] and x[row] equals both, for every pair of VQ_PLANTS that K (and M) has room for."""
    rng = np.random.default_rng(100000 * M + 100 * K + D)
    x = rng.standard_normal((M, D)).astype(F32)
    e = rng.standard_normal((K, D)).astype(F32)
    plants = []
    for c, delta in VQ_PLANTS:
        if c + delta < K and len(plants) < M:
            e[c + delta] = e[c]
            row = (7 * len(plants) + 3) % M
            assert row not in [p[0] for p in plants]
            x[row] = e[c]
            plants.append((row, c, c + delta))
    return x, e, plants


def vq_rounding_bound(mag, D):
    """Bound on |f32 evaluation - exact| of one distance, as parity_ref.bound with n_terms = 2 D (the 4 is bound()'s own):
    sx and se are D squares each, added in f32: D 2^-24 |x|^2 and D 2^-24 |e|^2; their sum: one rounding of |x|^2 + |e|^2; the dot is a
    D-term fmaf chain, (D + 1) 2^-24 |x||e| <= (D + 1) 2^-24 (|x|^2 + |e|^2) / 2, doubled by the factor 2; the last subtraction rounds
    a value of at most 2 (|x|^2 + |e|^2).  In all (2 D + 4) 2^-24 (|x|^2 + |e|^2)."""
    return (2 * D + 4) * 2.0 ** -24 * np.asarray(mag, dtype=np.float64) + 2.0 ** -126


def vq_sure_rows(ref, D, plants):
    """Rows whose f64 argmin the f32 evaluation must return: the margin to the second best exceeds the rounding bounds of both
    distances (`ref`: vq_distances with the planted copies left out of the margin - a row whose best code has a copy must still come
    back with the lower index).  The planted rows are reported apart: the tie rule is what they are there for."""
    sure = ref["margin"] > 2.0 * vq_rounding_bound(ref["mag"], D)
    planted = np.zeros(len(sure), dtype=bool)
    planted[[p[0] for p in plants]] = True
    return sure & ~planted, planted
