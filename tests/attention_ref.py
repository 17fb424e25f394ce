"""Plain torch f64 restatement of the fused attention entry points of include/pero_hip.h (pero_attention_fwd / _bwd and their _keys forms),
written from the header's formulas on the packed bf16 qkv rows, head_dim 128 and 64 (not a test module; it never imports the library).  Like
parity_ref.py every result comes with a per-element bound; unlike there the bound is not one `mag` times a count, because a bf16 rounding sits
in the MIDDLE of each kernel (P and dS are rounded to bf16 in front of their MFMAs), so each sum carries its own weights.

`forward` returns out, lse2 (the base-2 log-sum-exp of the scaled scores); `backward` evaluates the header's backward formula on WHAT THE KERNEL
IS HANDED - the bf16 `out`, the f32 `lse` (and, where the caller supplies it, D) - not autograd of the forward: the rounding of the forward's
outputs is an input of the backward, not an error charged to it, and a forward defect can neither cause nor mask a backward failure.

Key ranges: line b attends to the keys [k0_b, k1_b), clamped as the header says (k0 into [0, S - 1], then k1 into [k0 + 1, S]); P is an exact 0
outside, every query of the line is computed.

The bound.  Nothing in it is measured.  U = 2^-24 (parity_ref.U32: f32 unit roundoff), u = 2^-8 (parity_ref.BF16_OUT: one bf16 round-to-nearest),
c = log2(e) / sqrt(hd), a_qk = sum_d |q_d| |k_d|.  What the kernels do (csrc/attention_fwd.hip, attention_bwd.hip, attention_hd64.hip): scores
by bf16 MFMAs with f32 accumulation (the products of two bf16 values are exact in f32), p = exp2(fma(s, c, -m c)) in the forward and
exp2(fma(s, c, -lse)) in the backward, l summed from the unrounded p, P and dS rounded to bf16 (pack8: v_cvt_pk_bf16_f32, round to nearest even)
in front of the MFMAs that consume them, f32 accumulators, outputs rounded to bf16 once.

  eps_qk, the relative error of one f32 p = the ABSOLUTE error of exp2's argument x times ln 2, plus exp2's own:
      x = fma(s~, c, -lse)      s~: an f32 sum of hd exact products, in any order: (hd - 1) U a_qk      -> c (hd - 1) U a
                                c rounded to f32: U c |s| <= U c a                                          -> c U a
                                the fma's one rounding: U |x| <= U (c a + |lse2|)                           -> c U a + U |lse2|
                                (forward: the constant is m c, rounded once: U |m c|, and |m c| <= |lse2| + log2 S; the 4 absorbs it)
      together <= U ((hd + 4) c a + |lse2| + 4); v_exp_f32 is 1 ulp = 2 U (parity_ref.EXPF)
      eps_qk = ln2 U ((hd + 4) c a_qk + |lse2_q| + 4) + 2 U
  forward normalisation, the relative error of l = sum_k p~:  max_k eps_qk (over the line's live keys) + (S + 4) U (S terms in any order, the
      per-tile `l * alpha + ps`, `inv = 1 / l`, `o * inv`).  One term added to the form of the issue, named from the code: attention_fwd.hip forms
      alpha = exp2((m - mn) * c) from the unrounded maxima and p from the ROUNDED product mc = mn * c (lines `const float alpha`, `const float mc`;
      the same two lines in attention_hd64.hip), so the share of an earlier key tile is off by the two roundings of m c: 2 ln2 U |m c| relative.
      It is ~1e-6 at these inputs, 1000 x below u.
  out   = bf16(sum_k bf16(p~_qk) v_kd / l~):   sum_k (u + eps_qk + [S + 4] U + norm_q) P_qk |v_kd| + u |ref| + S 2^-126
              u: P's bf16 rounding; eps: p itself; (S + 4) U: the f32 accumulation of S terms and the per-tile rescale of O (o *= alpha: one
              rounding per tile; alpha's own error is common to o and l); norm_q: the denominator; u |ref|: the output's rounding;
              S 2^-126: p's that underflow (exp2 of less than -126 has no normal f32 value).
  lse2  = m c + log2(l~):   norm_q / ln2 (a relative error of l is an absolute one of its logarithm) + 4 U (|m c| + |log2 l|) (the product m c,
              v_log_f32's 1 ulp = 2 U of |log2 l|, the sum)
  D     = sum_d dO out in f32:   (hd + 4) U sum_d |dO out|
  dV    = bf16(sum_q bf16(p~_qk) dO_qd):   sum_q (u + eps_qk + [S + 4] U) P_qk |dO_qd| + u |ref|
  dS~   = p~ (dP~ - D~) scale:  delta_qk = (eps_qk + 4 U) |dS_qk|  (p; the difference, two products, scale rounded to f32)
                                         + P_qk / sqrt(hd) (hd + 4) U (sum_d |dO_qd v_kd| + sum_d |dO_qd out_qd|)   (dP~ and D~: f32 sums of hd terms;
                                           what cancels in dP - D gets no free pass)
  dQ    = bf16(sum_k bf16(dS~_qk) k_kd):   sum_k (u |dS_qk| + delta_qk + [S + 4] U |dS_qk|) |k_kd| + u |ref|
  dK    : the same with q for k, summed over the queries.
  (dV, dQ, dK carry the same underflow step as out, S 2^-126 times the largest operand: a p below the normal range may be flushed.)
The (S + 4) U and (hd + 4) U terms are 100 x below the u terms; no safety factor anywhere."""
import math

import torch

import parity_ref as R

U, u = R.U32, R.BF16_OUT
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
EXP2 = R.EXPF   # v_exp_f32: 1 ulp = 2 units of 2^-24 relative


def clamp_ranges(key_ranges, n, s):
    """(N, 2) int64, clamped as the header says: k0 into [0, S - 1], then k1 into [k0 + 1, S]; None = [0, S) on every line."""
    if key_ranges is None:
        return torch.tensor([[0, s]] * n, dtype=torch.int64)
    kr = torch.as_tensor(key_ranges).to(torch.int64).reshape(n, 2).clone()
    kr[:, 0] = kr[:, 0].clamp(0, s - 1)
    kr[:, 1] = torch.minimum(torch.maximum(kr[:, 1], kr[:, 0] + 1), torch.tensor(s))
    return kr


def live_keys(key_ranges, n, s):
    """(N, S) bool: True where the key is inside the line's (clamped) range."""
    kr = clamp_ranges(key_ranges, n, s)
    pos = torch.arange(s)[None, :]
    return (pos >= kr[:, :1]) & (pos < kr[:, 1:2])


def heads(x, n, s, h, hd):
    """(N*S, h*hd) -> (N, h, S, hd) f64"""
    return R.f64(x).reshape(n, s, h, hd).permute(0, 2, 1, 3)


def rows(x):
    """(N, h, S, hd) -> (N*S, h*hd)"""
    n, h, s, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(n * s, h * hd)


def split(qkv, n, s, h, hd):
    d = h * hd
    x = R.f64(qkv)
    assert x.shape == (n * s, 3 * d)
    return heads(x[:, :d], n, s, h, hd), heads(x[:, d:2 * d], n, s, h, hd), heads(x[:, 2 * d:], n, s, h, hd)


def _scores(q, k, hd, live):
    """t = c q.k (base-2 scaled, -inf outside the range), a = sum_d |q_d| |k_d|, c."""
    c = LOG2E / math.sqrt(hd)
    t = c * (q @ k.transpose(-1, -2))
    a = q.abs() @ k.abs().transpose(-1, -2)
    return t.masked_fill(~live[:, None, None, :], -math.inf), a, c


def _eps(a, lse2, c, hd):
    """eps_qk of the module docstring: (N, h, S, S)"""
    return LN2 * U * ((hd + 4) * c * a + lse2.abs()[..., None] + 4.0) + EXP2 * U


def forward(qkv, n, s, h, hd, key_ranges=None):
    """out (N*S, h*hd), lse2 (N*h, S): ({"out", "lse2"}, the same keys of bounds)."""
    q, k, v = split(qkv, n, s, h, hd)
    live = live_keys(key_ranges, n, s)
    t, a, c = _scores(q, k, hd, live)
    m = t.max(-1).values                                    # m c of the docstring: the largest scaled score of the line's live keys
    l = torch.exp2(t - m[..., None]).sum(-1)
    lse2 = m + torch.log2(l)
    p = torch.exp2(t - lse2[..., None])                     # exact 0 outside the range
    out = p @ v
    eps = _eps(a, lse2, c, hd)
    eps_max = eps.masked_fill(~live[:, None, None, :], 0.0).max(-1).values
    norm = eps_max + (s + 4) * U + 2.0 * LN2 * U * m.abs()
    w = (u + eps + (s + 4) * U + norm[..., None]) * p
    b_out = w @ v.abs() + u * out.abs() + s * R.UNDERFLOW
    b_lse = norm / LN2 + 4.0 * U * (m.abs() + torch.log2(l).abs())
    res = {"out": rows(out), "lse2": lse2.reshape(n * h, s)}
    bnd = {"out": rows(b_out), "lse2": b_lse.reshape(n * h, s)}
    return res, bnd


def backward(qkv, out_given, dout, lse_given, n, s, h, hd, key_ranges=None, dvec_given=None):
    """The header's backward on the tensors the kernel is handed: out_given (N*S, h*hd) bf16, lse_given (N*h, S) f32, dout (N*S, h*hd) bf16;
    dvec_given (N*S, h) f32: D as supplied by the caller (the `out == null` form) - D is then that tensor, not recomputed.
    Returns ({"dvec" (N*S, h), "dq", "dk", "dv" (N*S, h*hd)}, the same keys of bounds)."""
    q, k, v = split(qkv, n, s, h, hd)
    live = live_keys(key_ranges, n, s)
    t, a, c = _scores(q, k, hd, live)
    og, do = heads(out_given, n, s, h, hd), heads(dout, n, s, h, hd)
    lse = R.f64(lse_given).reshape(n, h, s)
    scale = 1.0 / math.sqrt(hd)
    p = torch.exp2(t - lse[..., None])
    dp = do @ v.transpose(-1, -2)
    mdp = do.abs() @ v.abs().transpose(-1, -2)
    dvec = (do * og).sum(-1)
    md = (do * og).abs().sum(-1)
    b_dvec = (hd + 4) * U * md
    if dvec_given is not None:
        dvec = R.f64(dvec_given).reshape(n, s, h).permute(0, 2, 1)
    ds = p * (dp - dvec[..., None]) * scale
    dv = p.transpose(-1, -2) @ do
    dq = ds @ k
    dk = ds.transpose(-1, -2) @ q
    eps = _eps(a, lse, c, hd)
    under = s * R.UNDERFLOW
    b_dv = ((u + eps + (s + 4) * U) * p).transpose(-1, -2) @ do.abs() + u * dv.abs() + under * max(1.0, float(do.abs().max()))
    delta = (eps + 4.0 * U) * ds.abs() + p * scale * (hd + 4) * U * (mdp + md[..., None])
    w = (u + (s + 4) * U) * ds.abs() + delta
    b_dq = w @ k.abs() + u * dq.abs() + under * max(1.0, float(k.abs().max()))
    b_dk = w.transpose(-1, -2) @ q.abs() + u * dk.abs() + under * max(1.0, float(q.abs().max()))
    res = {"dvec": dvec.permute(0, 2, 1).reshape(n * s, h), "dq": rows(dq), "dk": rows(dk), "dv": rows(dv)}
    bnd = {"dvec": b_dvec.permute(0, 2, 1).reshape(n * s, h), "dq": rows(b_dq), "dk": rows(b_dk), "dv": rows(b_dv)}
    return res, bnd


def worst_ratio(got, ref, bnd):
    """max over the elements of error / bound (0 / 0 counts as 0; a non-finite value where the reference is finite, or a NaN ratio, counts as inf)."""
    got, ref, bnd = R.f64(got), R.f64(ref), R.f64(bnd)
    assert got.shape == ref.shape == bnd.shape, (tuple(got.shape), tuple(ref.shape), tuple(bnd.shape))
    if ref.numel() == 0:
        return 0.0, 0
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got) | ~torch.isfinite(ref), err, torch.full_like(err, math.inf))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    flat = int(ratio.reshape(-1).argmax())
    return float(ratio.reshape(-1)[flat]), flat


def assert_inside(got, ref, bnd, what, out_dtype):
    """Per element |got - ref| <= bnd; the worst error / bound goes into parity_ref.RATIOS under `what`, as assert_within records it."""
    worst, flat = worst_ratio(got, ref, bnd)
    key = what + (" [bf16]" if out_dtype == torch.bfloat16 else " [f32]")
    R.RATIOS[key] = max(R.RATIOS.get(key, 0.0), worst)
    if worst > 1.0:
        got_, ref_, bnd_ = R.f64(got), R.f64(ref), R.f64(bnd)
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref_.shape))
        raise AssertionError(f"{what}: element {idx}: got {float(got_.reshape(-1)[flat])!r}, ref {float(ref_.reshape(-1)[flat])!r}, "
                             f"bound {float(bnd_.reshape(-1)[flat])!r} (error / bound = {worst:.3g})")
    return worst


# ---------------------------------------------------------------------------------------------- the cases of the GPU parity test
# (n, S, h): the smallest shapes that reach each instantiation.  (1, 1, 1), (2, 4, 4): one ragged tile; (1, 128, 2), (2, 256, 2): S % 128 = 0, the
# non-ragged head_dim-128 instantiations with one and two key tiles; (2, 132, .), (3, 260, .): a 4-key last tile; (1, 388, 1): four tiles.
PLAIN = {128: [(1, 1, 1), (2, 4, 4), (1, 128, 2), (2, 256, 2), (2, 132, 4), (3, 260, 4), (1, 388, 1)],
         64: [(1, 1, 1), (2, 4, 4), (1, 128, 2), (2, 256, 2), (2, 132, 2), (3, 260, 8), (1, 388, 1)]}


def all_cases():
    """[(hd, n, S, h, ranges or None)]: PLAIN through the entry points without ranges, then the six CASES of test_gpu_attention_keys.py."""
    from test_gpu_attention_keys import CASES
    out = []
    for hd in (128, 64):
        out += [(hd, n, s, h, None) for n, s, h in PLAIN[hd]]
        out += [(hd, n, s, h, ranges) for n, s, h, ranges in CASES]
    return out


def case_id(case):
    hd, n, s, h, ranges = case
    return f"hd{hd}-n{n}-s{s}-h{h}" + ("-keys" if ranges is not None else "")


def inputs(hd, n, s, h, ranges):
    """bf16 (qkv, dout) on the host.  Without ranges: the recipe of tests/test_gpu_attention_ragged.py (randn * 0.7, a spiked query row, a spiked key
    inside the line and one in the last partial tile); with ranges: that of tests/test_gpu_attention_keys.py (a spiked key inside every range, dead K / V
    rows x 2^10)."""
    if ranges is None:
        from test_gpu_attention_hd64 import inputs as plain_inputs   # the ragged test's recipe, with head_dim as a parameter
        return plain_inputs(n, s, h, hd)
    from test_gpu_attention_keys import inputs as keys_inputs
    return keys_inputs(n, s, h, hd, ranges)
