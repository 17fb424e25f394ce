"""Tensor-level wrappers over the C ABI (libpero_hip.so).  PyTorch supplies device memory and the
current HIP stream; all arithmetic happens in the hand-written kernels.  No CPU fallback."""
import ctypes
import threading

import numpy as np
import torch

from . import _lib
from ._lib import (GEMM_ACCUM, GEMM_ATOMIC, GEMM_COLSUM, GEMM_FORCE_GENERIC, GEMM_MASK_TILED, GEMM_ROWDOT, GEMM_RELU, GEMM_RELU_BITS, GEMM_TRANS_A, GEMM_TRANS_B,
                   PERO_BF16, PERO_F32, call)


def dt(t_or_dtype):
    d = t_or_dtype.dtype if isinstance(t_or_dtype, torch.Tensor) else t_or_dtype
    if d == torch.float32:
        return PERO_F32
    if d == torch.bfloat16:
        return PERO_BF16
    raise TypeError(f"unsupported dtype {d}")


def ptr(t):
    return t.data_ptr() if isinstance(t, torch.Tensor) else t   # None, or a raw address


def stream():
    return torch.cuda.current_stream().cuda_stream


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.PeroHipError("pero_pretraining_amd ops need CUDA/HIP tensors: the HIP kernels are the only "
                                    "implementation (no CPU fallback)")


# optional launch timeline for bench.py's roofline leg: list of (start_event, end_event, flops, kernel tag)
gemm_timeline = None


def _timeline(e0=None, flops=None, tag=None):
    """Called while the timeline is on: before a launch -> its recorded start event; behind it, with that event -> records the end and appends the entry."""
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e if e0 is None else gemm_timeline.append((e0, e, flops, tag))


# Split-K workspaces (partial tiles of the weight-gradient products, pero_gemm's `workspace`): the C ABI never allocates, so the
# caller - this module - keeps one buffer per (device, stream) from PyTorch's caching allocator, grown on demand.  Products on one
# stream run one after the other and may share it; the weight-gradient side stream and the autograd threads' streams get their own.
_ws_lock = threading.Lock()
_ws_cache = {}


def gemm_workspace(nbytes, device):
    """uint8 device buffer of at least `nbytes` for the current stream (None for 0)."""
    if nbytes <= 0:
        return None
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    with _ws_lock:
        buf = _ws_cache.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = _ws_cache[key] = torch.empty(max(int(nbytes), 64 << 20), device=device, dtype=torch.uint8)
    return buf


def release_workspaces():
    """Drop the cached split-K workspaces (they return to PyTorch's allocator once the queued work has run)."""
    with _ws_lock:
        _ws_cache.clear()


def gemm_raw(A, B, C, M, N, K, lda, ldb, ldc, *, bias=None, residual=None, gate=None, ldr=0, ldg=0, batch=1,
             batch_inner=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), alpha=1.0, flags=0, k_split=1, in_dtype=None,
             out_dtype=None):
    """Direct pero_gemm call; A/B/C may be tensors (pointer taken at storage offset) or raw ints."""
    _req_cuda(A, B, C)
    idt = dt(A) if in_dtype is None else in_dtype
    odt = dt(C) if out_dtype is None else out_dtype
    ws = None
    if flags & GEMM_ATOMIC:
        need = _lib.lib().pero_gemm_workspace_bytes(M, N, K, batch, int(flags), int(k_split), idt, odt)
        ws = gemm_workspace(need, A.device if isinstance(A, torch.Tensor) else torch.device("cuda", torch.cuda.current_device()))
    e0 = None if gemm_timeline is None else _timeline()
    call("pero_gemm", ptr(A), ptr(B), ptr(C), ptr(bias), ptr(residual), ptr(gate), M, N, K, lda, ldb, ldc, ldr, ldg,
         batch, batch_inner, sA[0], sA[1], sB[0], sB[1], sC[0], sC[1], float(alpha), int(flags), int(k_split),
         idt, odt, ptr(ws), ws.numel() if ws is not None else 0, stream())
    if e0 is not None:
        fast = idt == PERO_BF16 and M % 128 == 0 and N % 128 == 0 and K % 64 == 0 and not (flags & GEMM_FORCE_GENERIC)
        lay = ("T" if flags & GEMM_TRANS_A else "N") + ("T" if flags & GEMM_TRANS_B else "N")
        _timeline(e0, 2.0 * M * N * K * batch, ("gemm_bf16_tile" if fast else "gemm_generic") + ":" + lay)


def gemm_plan(A, B, C, M, N, K, lda, ldb, ldc, *, bias=None, residual=None, gate=None, ldr=0, ldg=0, batch=1,
              batch_inner=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), alpha=1.0, flags=0, k_split=1, in_dtype=None,
              out_dtype=None):
    """What gemm_raw would run for these arguments (pero_gemm_plan; nothing is launched, the operands may be made-up addresses):
    (kernel family - a name of _lib.GEMM_KERNELS, k-slices, extra pass over C - None / "colsum" / "rowdot").  Raises where pero_gemm would refuse."""
    ks, extra = ctypes.c_int(0), ctypes.c_int(0)
    idt = dt(A) if in_dtype is None else in_dtype
    odt = dt(C) if out_dtype is None else out_dtype
    h = _lib.lib()
    rc = h.pero_gemm_plan(ptr(A), ptr(B), ptr(C), ptr(bias), ptr(residual), ptr(gate), M, N, K, lda, ldb, ldc, ldr, ldg,
                          batch, batch_inner, sA[0], sA[1], sB[0], sB[1], sC[0], sC[1], float(alpha), int(flags), int(k_split),
                          idt, odt, None, 0, None, ctypes.byref(ks), ctypes.byref(extra))
    if rc <= 0:
        raise _lib.PeroHipError(f"pero_gemm_plan failed ({rc}): {h.pero_last_error().decode()}")
    return _lib.GEMM_KERNELS[rc], ks.value, _lib.GEMM_PASSES[extra.value]


def gemm(a, b, out=None, *, bias=None, residual=None, gate=None, trans_a=False, trans_b=False, relu=False,
         alpha=1.0, out_dtype=None, atomic=False, accum=False, k_split=1, force_generic=False, extra_flags=0,
         colsum_into=None, rowdot=None, relu_bits=None, bits_tiled=False):
    """out[M,N] = alpha * op(a) @ op(b)^T ...   a: [M,K] ([K,M] if trans_a); b: [N,K] ([K,N] if trans_b).
    Row-strided 2-D views are fine (unit stride in the last dim).  colsum_into (f32 [N]): the column sums of the stored
    result are accumulated into it (PERO_GEMM_COLSUM; no input bias in that mode).  rowdot = (y, out): out (f32 [M][N/128])
    receives, per 128-column block, the row dots of the stored bf16 result with y (bf16 [M][N]) - PERO_GEMM_ROWDOT.
    relu_bits (uint8 [M][N/8]): with relu=True it RECEIVES the bit mask (stored result > 0); otherwise it is applied as the
    ReLU gate in place of a bf16 gate matrix - PERO_GEMM_RELU_BITS.  bits_tiled: the mask is laid out per 256-column block ([N/256][M][32 bytes],
    PERO_GEMM_MASK_TILED; N % 256 == 0, relu_bits contiguous) - producer and consumer must pass the same value."""
    assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    M, K = (a.shape[1], a.shape[0]) if trans_a else a.shape
    N, Kb = (b.shape[1], b.shape[0]) if trans_b else b.shape
    assert K == Kb, (a.shape, b.shape, trans_a, trans_b)
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=out_dtype or a.dtype)
    assert out.shape == (M, N) and out.stride(1) == 1
    flags = (GEMM_RELU if relu else 0) | (GEMM_TRANS_A if trans_a else 0) | (GEMM_TRANS_B if trans_b else 0) | \
        (GEMM_ATOMIC if atomic else 0) | (GEMM_ACCUM if accum else 0) | (GEMM_FORCE_GENERIC if force_generic else 0) | extra_flags
    if colsum_into is not None:
        assert bias is None and colsum_into.dtype == torch.float32 and colsum_into.numel() == N
        bias, flags = colsum_into, flags | GEMM_COLSUM
    if relu_bits is not None:
        assert gate is None and relu_bits.dtype == torch.uint8 and relu_bits.shape == (M, N // 8) and relu_bits.stride(1) == 1
        gate, flags = relu_bits, flags | GEMM_RELU_BITS
        if bits_tiled:
            assert N % 256 == 0 and relu_bits.is_contiguous()
            flags |= GEMM_MASK_TILED
    if rowdot is not None:
        y, dots = rowdot
        assert bias is None and gate is None and N % 128 == 0 and y.shape == (M, N) and y.stride(1) == 1
        assert dots.dtype == torch.float32 and dots.numel() == M * (N // 128) and dots.is_contiguous()
        bias, gate, flags = dots, y, flags | GEMM_ROWDOT
    gemm_raw(a, b, out, M, N, K, a.stride(0), b.stride(0), out.stride(0), bias=bias, residual=residual, gate=gate,
             ldr=residual.stride(0) if residual is not None else 0, ldg=gate.stride(0) if gate is not None else 0,
             alpha=alpha, flags=flags, k_split=k_split)
    return out


def layernorm_fwd(x, gamma, beta, eps, pe=None, offsets=None, S=1):
    _req_cuda(x)
    rows, d = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    call("pero_layernorm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(pe), ptr(offsets), ptr(y), ptr(mean), ptr(rstd),
         rows, d, S, float(eps), dt(x), stream())
    return y, mean, rstd


def gemm_resid_layernorm_ok(a, w, residual):
    """Shapes the fused Linear + residual + LayerNorm launch takes (csrc/gemm_n.hip gemm_bf16_n512: bf16, 512 output columns)."""
    return (a.dtype == torch.bfloat16 and a.dim() == 2 and w.dim() == 2 and w.shape[0] == 512 and a.shape[0] % 128 == 0 and a.shape[1] % 64 == 0 and
            a.shape[1] >= 192 and a.shape[1] == w.shape[1] and residual is not None and residual.shape == (a.shape[0], 512) and
            a.stride(1) == 1 and w.stride(1) == 1 and residual.stride(1) == 1 and a.stride(0) % 8 == 0 and w.stride(0) % 8 == 0 and residual.stride(0) % 8 == 0)


def gemm_resid_layernorm(a, w, bias, residual, gamma, beta, eps, store_y=True):
    """y = a @ w^T + bias + residual (bf16, stored unless store_y=False: then None), t = LayerNorm(y) * gamma + beta, mean, rstd - ONE launch
    (pero_gemm_resid_layernorm)."""
    _req_cuda(a)
    M, K = a.shape
    y = torch.empty((M, 512), device=a.device, dtype=torch.bfloat16) if store_y else None
    t = torch.empty((M, 512), device=a.device, dtype=torch.bfloat16)
    mean = torch.empty(M, device=a.device, dtype=torch.float32)
    rstd = torch.empty(M, device=a.device, dtype=torch.float32)
    e0 = None if gemm_timeline is None else _timeline()
    call("pero_gemm_resid_layernorm", ptr(a), ptr(w), ptr(bias), ptr(residual), ptr(gamma), ptr(beta), ptr(y), ptr(t), ptr(mean), ptr(rstd),
         M, 512, K, a.stride(0), w.stride(0), y.stride(0) if y is not None else 0, residual.stride(0), t.stride(0), float(eps), stream())
    if e0 is not None:   # counted with the tile GEMMs of bench.py's roofline: the product's flops over the WHOLE launch (LayerNorm included)
        _timeline(e0, 2.0 * M * 512 * K, "gemm_bf16_tile_ln_fwd:NN")
    return y, t, mean, rstd


def gemm_resid_layernorm_bwd_ok(a, w_t, residual, t):
    """Shapes the fused input-gradient + LayerNorm-backward launch takes (csrc/gemm_n.hip gemm_bf16_n512, EP_RESID_LNB)."""
    return gemm_resid_layernorm_ok(a, w_t, residual) and t is not None and t.shape == (a.shape[0], 512) and t.stride(1) == 1 and t.stride(0) % 8 == 0


def gemm_resid_layernorm_bwd(a, w_t, residual, t, rstd, gamma, beta, dgamma, dbeta, dxsum=None):
    """dx = LayerNorm backward (from the norm's output t and rstd) of dt = a @ w_t^T + residual, dt never stored; dgamma / dbeta / dxsum are
    accumulated into - ONE launch + the small column-sum reduce (pero_gemm_resid_layernorm_bwd)."""
    _req_cuda(a)
    M, K = a.shape
    dx = torch.empty((M, 512), device=a.device, dtype=torch.bfloat16)
    work = torch.empty(3 * _lib.LN_BWD_BLOCKS * 512, device=a.device, dtype=torch.float32)
    e0 = None if gemm_timeline is None else _timeline()
    call("pero_gemm_resid_layernorm_bwd", ptr(a), ptr(w_t), ptr(residual), ptr(t), ptr(rstd), ptr(gamma), ptr(beta), ptr(dx), ptr(dgamma), ptr(dbeta),
         ptr(dxsum), ptr(work), M, 512, K, a.stride(0), w_t.stride(0), residual.stride(0), t.stride(0), dx.stride(0), stream())
    if e0 is not None:   # the product's flops over the WHOLE launch (LayerNorm backward and the reduce included)
        _timeline(e0, 2.0 * M * 512 * K, "gemm_bf16_tile_ln_bwd:NN")
    return dx


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, dxsum=None):
    rows, d = x.shape
    dx = torch.empty_like(x)
    work = torch.empty(3 * _lib.LN_BWD_BLOCKS * d, device=x.device, dtype=torch.float32)
    call("pero_layernorm_bwd", ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(dx), ptr(dgamma), ptr(dbeta),
         ptr(dxsum), ptr(work), rows, d, dt(x), stream())
    return dx


def layernorm_bwd_out(dy, t, rstd, gamma, beta, dgamma, dbeta, dxsum=None):
    """LayerNorm backward from the layer's OUTPUT t (pero_layernorm_bwd_out): the forward kept t and rstd only."""
    rows, d = t.shape
    dx = torch.empty_like(t)
    work = torch.empty(3 * _lib.LN_BWD_BLOCKS * d, device=t.device, dtype=torch.float32)
    call("pero_layernorm_bwd_out", ptr(dy), ptr(t), ptr(rstd), ptr(gamma), ptr(beta), ptr(dx), ptr(dgamma), ptr(dbeta),
         ptr(dxsum), ptr(work), rows, d, dt(t), stream())
    return dx


def bn_fwd(x, weight, bias, running_mean, running_var, eps, momentum, training, relu):
    """BatchNorm1d (+ ReLU) over the rows of x (rows, d): returns (y, save_mean, save_rstd); running statistics updated in place in training."""
    _req_cuda(x)
    rows, d = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(d, device=x.device, dtype=torch.float32)
    rstd = torch.empty(d, device=x.device, dtype=torch.float32)
    work = torch.empty(2 * d, device=x.device, dtype=torch.float32)
    call("pero_bn_fwd", ptr(x), ptr(weight), ptr(bias), ptr(running_mean), ptr(running_var), ptr(y), ptr(mean), ptr(rstd), ptr(work),
         rows, d, float(eps), float(momentum), int(bool(training)), int(bool(relu)), dt(x), stream())
    return y, mean, rstd


def bn_bwd(dy, x, y, weight, mean, rstd, dweight, dbias, relu):
    rows, d = x.shape
    dx = torch.empty_like(x)
    work = torch.empty(2 * d, device=x.device, dtype=torch.float32)
    call("pero_bn_bwd", ptr(dy), ptr(x), ptr(y), ptr(weight), ptr(mean), ptr(rstd), ptr(dx), ptr(dweight), ptr(dbias), ptr(work),
         rows, d, int(bool(relu)), dt(x), stream())
    return dx


def softmax_fwd(scores, scale, out_dtype, key_ranges=None, rows_per_line=None):
    """key_ranges (int32 (lines, 2), device): each row takes the keys [k0, k1) of its line (row // rows_per_line) only; p is exactly 0 outside."""
    rows, cols = scores.numel() // scores.shape[-1], scores.shape[-1]
    p = torch.empty(scores.shape, device=scores.device, dtype=out_dtype)
    if key_ranges is None:
        call("pero_softmax_fwd", ptr(scores), ptr(p), rows, cols, float(scale), dt(out_dtype), stream())
    else:
        if rows_per_line is None:
            raise ValueError("softmax_fwd: key_ranges needs rows_per_line")
        _check_key_ranges(key_ranges, rows // int(rows_per_line))
        call("pero_softmax_fwd_keys", ptr(scores), ptr(key_ranges), ptr(p), rows, cols, int(rows_per_line), float(scale), dt(out_dtype), stream())
    return p


def softmax_bwd(p, dp, scale):
    rows, cols = p.numel() // p.shape[-1], p.shape[-1]
    ds = torch.empty_like(p)
    call("pero_softmax_bwd", ptr(p), ptr(dp), ptr(ds), rows, cols, float(scale), dt(p), stream())
    return ds


def attention_fused_ok(qkv, s, h):
    d = qkv.shape[1] // 3
    return qkv.dtype == torch.bfloat16 and d // h == 128 and d % h == 0 and s >= 1


def attention_fused_hd64_ok(qkv, s, h):
    """The head_dim-64 kernels (csrc/attention_hd64.hip): bf16, d // h == 64, every s >= 1 (faster than the unfused path at every measured s: DESIGN 8.0000)."""
    d = qkv.shape[1] // 3
    return qkv.dtype == torch.bfloat16 and d % h == 0 and d // h == 64 and s >= 1


def attention_hd64_heads_per_block(n, s, h):
    """Heads of a line that one head_dim-64 forward workgroup walks at this shape on the current device (tests assert the choice)."""
    return int(_lib.lib().pero_attention_hd64_heads_per_block(n, s, h))


def key_ranges_kw(key_ranges):
    """The `key_ranges=` keyword of a call, or none at all without ranges: code that wraps or replaces the functions of this package with their signatures of
    before (no such argument) keeps working as long as no ranges are in play."""
    return {} if key_ranges is None else {"key_ranges": key_ranges}


def _check_key_ranges(key_ranges, n):
    if not (isinstance(key_ranges, torch.Tensor) and key_ranges.is_cuda and key_ranges.dtype == torch.int32 and key_ranges.shape == (n, 2) and
            key_ranges.is_contiguous()):
        raise ValueError(f"key_ranges must be a contiguous int32 device tensor of shape ({n}, 2) (ops.key_ranges_from_masks builds one)")


def _hull_argmax(masks):
    """[first, last + 1) of the positions equal to 1 per row of a 2-d tensor, by torch ops on the tensor's device (no host read)."""
    v = (masks == 1).to(torch.uint8)
    k0 = torch.argmax(v, dim=1)                      # argmax: the first of equal maxima
    k1 = v.shape[1] - torch.argmax(v.flip(1), dim=1)
    return torch.stack((k0, k1), dim=1).to(torch.int32).contiguous()


def key_ranges_from_masks(masks, device=None):
    """(N, S) mask, valid where it equals 1 (the collator's image_masks; `labels >= 0` of a masked-pretraining batch) -> int32 (N, 2) device tensor
    [first valid position, last valid position + 1) per line: the `key_ranges` of the attention ops.  A device mask is reduced on the device without a
    synchronisation (a line without a valid position comes out as [0, 1): the kernels' clamp of an empty range).  A mask known on the host (numpy array,
    CPU tensor, list) is reduced there, and a line with no valid position or with a hole inside its hull raises ValueError; `device` says where it goes."""
    if isinstance(masks, torch.Tensor) and masks.is_cuda:
        if masks.dim() != 2:
            raise ValueError("key_ranges_from_masks: the mask must be (N, S)")
        return _hull_argmax(masks)
    m = masks.numpy() if isinstance(masks, torch.Tensor) else np.asarray(masks)
    if m.ndim != 2:
        raise ValueError("key_ranges_from_masks: the mask must be (N, S)")
    v = m == 1
    cnt = v.sum(1)
    if (cnt == 0).any():
        raise ValueError(f"key_ranges_from_masks: line {int(np.argmax(cnt == 0))} has no valid position")
    k0 = v.argmax(1)
    k1 = m.shape[1] - v[:, ::-1].argmax(1)
    if (k1 - k0 != cnt).any():
        raise ValueError(f"key_ranges_from_masks: line {int(np.argmax(k1 - k0 != cnt))} has a hole inside its valid interval: only intervals are supported")
    t = torch.from_numpy(np.stack((k0, k1), axis=1).astype(np.int32))
    return t.to(device if device is not None else "cuda")


def attention_fwd_fused(qkv, n, s, h, key_ranges=None):
    """key_ranges (int32 (n, 2), device): line b attends to the keys [k0, k1) only (pero_attention_fwd_keys; clamped by the kernels)."""
    d = qkv.shape[1] // 3
    out = torch.empty((n * s, d), device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty((n * h, s), device=qkv.device, dtype=torch.float32)
    if key_ranges is None:
        call("pero_attention_fwd", ptr(qkv), ptr(out), ptr(lse), n, s, h, d // h, dt(qkv), stream())
    else:
        _check_key_ranges(key_ranges, n)
        call("pero_attention_fwd_keys", ptr(qkv), ptr(key_ranges), ptr(out), ptr(lse), n, s, h, d // h, dt(qkv), stream())
    return out, lse


def attention_bwd_fused(qkv, out, dout, lse, n, s, h, dbias=None, dvec=None, key_ranges=None):
    """key_ranges: those of the forward (pero_attention_bwd_keys: dK / dV rows outside a line's range are exact zeros).
    dbias (f32 [3d], optional): in_proj's bias gradient (column sums of dqkv) is accumulated into it by the kernels.
    dvec (f32 [n*s][h], optional): D = per-head row sums of dout * out, already computed (then `out` is not read)."""
    d = qkv.shape[1] // 3
    dqkv = torch.empty_like(qkv)
    if dvec is None:
        dvec = torch.empty((n * s, h), device=qkv.device, dtype=torch.float32)
    else:
        out = None
    work = torch.empty(3 * n * h * ((s + 127) // 128) * 128, device=qkv.device, dtype=torch.float32) if dbias is not None else None
    if key_ranges is None:
        call("pero_attention_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(dvec), ptr(dqkv), ptr(dbias), ptr(work), n, s, h, d // h,
             dt(qkv), stream())
    else:
        _check_key_ranges(key_ranges, n)
        call("pero_attention_bwd_keys", ptr(qkv), ptr(key_ranges), ptr(out), ptr(dout), ptr(lse), ptr(dvec), ptr(dqkv), ptr(dbias), ptr(work), n, s, h,
             d // h, dt(qkv), stream())
    return dqkv


def ce_work_elems(rows):
    """f32 elements of the masked cross entropy's workspace: the header's PERO_CE_WORK(rows)."""
    return 2 * rows + 8 + 256


def masked_ce_fwd(logits, labels, mask, unmasked_weight=None):
    """logits (rows,V); labels/mask int64 (rows).  Returns (loss: f32 tensor of 1 element, work buffer)."""
    _req_cuda(logits, labels, mask)
    rows, V = logits.shape
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    work = torch.empty(ce_work_elems(rows), device=logits.device, dtype=torch.float32)
    call("pero_masked_ce_fwd", ptr(logits), ptr(labels), ptr(mask), -1.0 if unmasked_weight is None else float(unmasked_weight),
         ptr(loss), ptr(work), rows, V, dt(logits), stream())
    return loss, work


def masked_ce_fwd_rows(logits, labels, mask, index):
    """masked_ce_fwd with unmasked_weight None for a caller that lists the rows with mask == 1 (int64 device tensor): same bits."""
    rows, V = logits.shape
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    work = torch.empty(ce_work_elems(rows), device=logits.device, dtype=torch.float32)
    call("pero_masked_ce_fwd_rows", ptr(logits), ptr(labels), ptr(mask), ptr(index), index.numel(), ptr(loss), ptr(work), rows, V,
         dt(logits), stream())
    return loss, work


def zeros(shape, device, dtype):
    """A zero tensor filled by the library's linear fill kernel (torch's elementwise fill runs at a third of its rate)."""
    t = torch.empty(shape, device=device, dtype=dtype)
    if t.numel():
        call("pero_zero_fill", ptr(t), t.numel() * t.element_size(), stream())
    return t


def masked_ce_bwd(logits, labels, mask, work, unmasked_weight=None, dloss=None):
    rows, V = logits.shape
    dlogits = torch.empty_like(logits)
    call("pero_masked_ce_bwd", ptr(logits), ptr(labels), ptr(mask), -1.0 if unmasked_weight is None else float(unmasked_weight),
         ptr(dloss), ptr(work), ptr(dlogits), rows, V, dt(logits), stream())
    return dlogits


def masked_ce_bwd_rows(logits, labels, mask, work, index, n_rows_out, unmasked_weight=None, dloss=None):
    """Compact CE gradient: (n_rows_out, V), row i = gradient row of logits row index[i], zero rows behind index.numel()."""
    rows, V = logits.shape
    out = torch.empty((n_rows_out, V), device=logits.device, dtype=logits.dtype)
    call("pero_masked_ce_bwd_rows", ptr(logits), ptr(labels), ptr(mask), -1.0 if unmasked_weight is None else float(unmasked_weight),
         ptr(dloss), ptr(work), ptr(index), index.numel(), n_rows_out, ptr(out), rows, V, dt(logits), stream())
    return out


def host_mask(m):
    """The mask's values on the HOST when they are known there without a device sync: numpy arrays, CPU tensors, and device
    tensors that a batch operator / collator / prefetcher uploaded from host arrays (they carry a private copy of the original as
    `_pero_host`; such a device mask must not be modified in place after the upload).  None: the mask lives on the device only."""
    if isinstance(m, np.ndarray):
        return m
    if isinstance(m, torch.Tensor):
        if not m.is_cuda:
            return m.numpy()
        return getattr(m, "_pero_host", None)
    return np.asarray(m)


def colsum(x, out):
    rows, cols = x.shape
    call("pero_colsum", ptr(x), ptr(out), rows, cols, x.stride(0), dt(x), stream())
    return out


def _tile_table(rows, tiles_of, extent_of, device, refuse=None):
    """The device table of a kernel that walks segments in tiles (csrc/flat_tiles.hpp): `rows` with the running first tile appended as
    the last column -> (int64 table on `device`, total tiles).  tiles_of(row) and extent_of(row) give a row's tile count and the end of the
    elements it addresses; the largest end is the table's `_pero_extent`, a host integer, so that a wrapper can refuse a flat buffer shorter
    than its table without reading the device.  refuse: (function name, noun) of the ValueError for an empty table or one of 2^31 tiles or
    more (None: the launch refuses it)."""
    table, tiles = [], 0
    for row in rows:
        table.append([*row, tiles])
        tiles += tiles_of(row)
    if refuse is not None and (not table or tiles >= 1 << 31):
        raise ValueError(f"{refuse[0]}: {len(table)} {refuse[1]}, {tiles} tiles")
    extent = max((extent_of(row) for row in rows), default=0)
    table = torch.tensor(table, dtype=torch.int64).to(device)
    table._pero_extent = extent
    return table, tiles


def _table_check(name, table, columns, made_by, flat=()):
    """A table of _tile_table with `columns` columns; flat: the buffers it indexes (None allowed).  Returns the extent."""
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != columns or not table.is_contiguous():
        raise TypeError(f"{name}: table is a contiguous int64 [n][{columns}] device tensor (ops.{made_by})")
    extent = getattr(table, "_pero_extent", None)
    if extent is None:
        raise ValueError(f"{name}: the table does not come from ops.{made_by} (its extent is unknown)")
    for t in flat:
        if t is not None and t.numel() < extent:
            raise ValueError(f"{name}: a flat buffer of {t.numel()} elements is shorter than the table's extent {extent}")
    return extent


def transpose_table(entries, device):
    """entries: [(src offset, dst offset, rows, cols)] -> (device table for transpose_multi, total 64x64 tiles)."""
    return _tile_table([list(e) for e in entries], lambda e: ((e[2] + 63) // 64) * ((e[3] + 63) // 64),
                       lambda e: max(e[0], e[1]) + e[2] * e[3], device)


def transpose_multi(src, dst, table, tiles):
    """dst matrix t = src matrix t transposed, for every row of `table` (2-byte elements, one launch)."""
    assert src.element_size() == 2 and dst.element_size() == 2 and table.dtype == torch.int64 and table.is_cuda
    call("pero_transpose_multi", ptr(src), ptr(dst), ptr(table), table.shape[0], tiles, stream())
    return dst


def cast_to_bf16(src, dst):
    call("pero_cast_f32_bf16", ptr(src), ptr(dst), src.numel(), stream())
    return dst


def scale_(x, s):
    call("pero_scale", ptr(x), x.numel(), float(s), dt(x), stream())
    return x


def patches_from_u8(images, mask, tile, P, dtype, pitch=None):
    """(N*S, pitch) buffer whose first C*H*P columns are the patch rows (rest zero)."""
    _req_cuda(images)
    images = images.contiguous()
    N, H, W, C = images.shape
    pitch = pitch or C * H * P
    out = torch.empty((N * (W // P), pitch), device=images.device, dtype=dtype)
    call("pero_patches_from_u8", ptr(images), ptr(mask), ptr(tile), ptr(out), N, H, W, C, P, pitch, dt(dtype), stream())
    return out


def patches_from_f32(images, mask, tile, P, dtype, pitch=None):
    _req_cuda(images)
    images = images.contiguous()
    N, C, H, W = images.shape
    pitch = pitch or C * H * P
    out = torch.empty((N * (W // P), pitch), device=images.device, dtype=dtype)
    call("pero_patches_from_f32", ptr(images), ptr(mask), ptr(tile), ptr(out), N, H, W, C, P, pitch, dt(dtype), stream())
    return out


def cast_pad_to_bf16(src2d, pitch):
    rows, cols = src2d.shape
    dst = torch.empty((rows, pitch), device=src2d.device, dtype=torch.bfloat16)
    call("pero_cast_pad_f32_bf16", ptr(src2d), ptr(dst), rows, cols, pitch, stream())
    return dst


def add_rows2d(dst2d, src2d, cols):
    call("pero_add_rows2d", ptr(dst2d), ptr(src2d), dst2d.shape[0], cols, dst2d.stride(0), src2d.stride(0), stream())
    return dst2d


def apply_mask_(images, mask, tile, P):
    _req_cuda(images)
    N, C, H, W = images.shape
    call("pero_apply_mask_f32", ptr(images), ptr(mask), ptr(tile), N, H, W, C, P, stream())
    return images


def adam_step(p, g, m, v, p_bf16, lr, beta1, beta2, eps, step, grad_scale=1.0):
    call("pero_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), p.numel(), float(lr), float(beta1), float(beta2),
         float(eps), int(step), float(grad_scale), stream())


def adam_step_ex(p, g, m, v, p_bf16, lr, beta1, beta2, eps, step, grad_scale=1.0, weight_decay=0.0, decoupled=False, vmax=None,
                 maximize=False, grad_norm=None, max_norm=0.0):
    """pero_adam_step_ex: vmax (f32, like v) switches amsgrad on; grad_norm (one f32 on the device, see grad_norm_finish) the clip at
    max_norm.  With the defaults it is adam_step, bit for bit."""
    call("pero_adam_step_ex", ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), p.numel(), float(lr), float(beta1), float(beta2),
         float(eps), int(step), float(grad_scale), float(weight_decay), int(bool(decoupled)), ptr(vmax), int(bool(maximize)),
         ptr(grad_norm), float(max_norm), stream())


# layout of the norm's first pass (csrc/optim.hip): 16-byte pieces, 256 lanes per workgroup, one workgroup per 1024 pieces up to a cap
SUMSQ_LANES, SUMSQ_PIECES_PER_BLOCK, SUMSQ_MAX_BLOCKS = 256, 1024, 2048


def sumsq_num_partials(n):
    """Number of partial sums pero_sumsq_partials writes for n elements (a function of n alone)."""
    return int(_lib.lib().pero_sumsq_num_partials(int(n)))


def sumsq_chain(n):
    """Longest chain of f32 additions one partial goes through for n elements: the lane's running sum over its pieces, the fold of the
    piece's four elements (2), the wave butterfly (6), the four waves (3)."""
    nv = (n + 3) // 4
    blocks = max(1, min((nv + SUMSQ_PIECES_PER_BLOCK - 1) // SUMSQ_PIECES_PER_BLOCK, SUMSQ_MAX_BLOCKS))
    return (nv + blocks * SUMSQ_LANES - 1) // (blocks * SUMSQ_LANES) + 2 + 6 + 3


def sumsq_partials(x, partials):
    """partials[b] = sum of squares of workgroup b's share of the flat f32 buffer x; partials: f32 view of sumsq_num_partials(n) elements."""
    _req_cuda(x, partials)
    if x.dtype != torch.float32 or partials.dtype != torch.float32 or not x.is_contiguous() or not partials.is_contiguous():
        raise TypeError("sumsq_partials: contiguous f32 tensors")
    if partials.numel() != sumsq_num_partials(x.numel()):
        raise ValueError(f"sumsq_partials: {x.numel()} elements give {sumsq_num_partials(x.numel())} partials, the view holds {partials.numel()}")
    call("pero_sumsq_partials", ptr(x), x.numel(), ptr(partials), stream())


def grad_norm_finish(partials, scale, out):
    """out[0] = scale * sqrt(sum(partials)) (f64 sum in index order, one f32 result on the device)."""
    _req_cuda(partials, out)
    if partials.dtype != torch.float32 or out.dtype != torch.float32 or not partials.is_contiguous():
        raise TypeError("grad_norm_finish: contiguous f32 tensors")
    call("pero_grad_norm_finish", ptr(partials), partials.numel(), float(scale), ptr(out), stream())


# layer-wise optimizers (csrc/optim_layerwise.hip): every tensor of a flat buffer in tiles of LAYER_TILE elements that start at the tensor
LAYER_TILE = _lib.DEFINES["PERO_LAYER_TILE"]


def layer_tiles(numel):
    """Tiles of one tensor: ceil(numel / LAYER_TILE), the last one possibly short."""
    return (int(numel) + LAYER_TILE - 1) // LAYER_TILE


def layer_chain():
    """Longest chain of f32 additions one tile partial goes through: the lane's running sum over its four pieces (4), the fold of the
    piece's four elements (2), the wave butterfly (6), the four waves (3).  The tile is fixed, so the chain does not depend on the size."""
    return 4 + 2 + 6 + 3


def layer_table(entries, device):
    """entries: [(offset, numel)] of the tensors of a flat buffer -> (table int64 [n][3] = {offset, numel, first tile} on `device`,
    total tiles).  A function of the sizes alone.  The table carries its extent (the largest offset + numel) as `_pero_extent`, a host
    integer, so that the wrappers below can refuse a flat buffer that is shorter than its table without reading the device."""
    rows_ = []
    for off, n in entries:
        if off % 8 or off < 0 or n < 1:
            raise ValueError(f"layer_table: offsets are multiples of 8 elements and tensors are not empty, got offset {off}, numel {n}")
        rows_.append([off, n])
    return _tile_table(rows_, lambda r: layer_tiles(r[1]), lambda r: r[0] + r[1], device, refuse=("layer_table", "tensors"))


def _layer_check(name, table, tiles, f32, flat=(), **sized):
    """f32: every f32 argument (None allowed); flat: those of them, and the bf16 copy, that the table indexes."""
    _req_cuda(table, *f32, *flat)
    _table_check(name, table, 3, "layer_table", flat)
    if any(t is not None and (t.dtype != torch.float32 or not t.is_contiguous()) for t in f32):
        raise TypeError(f"{name}: contiguous f32 tensors")
    for what, (t, need) in sized.items():
        if t.numel() != need:
            raise ValueError(f"{name}: {what} holds {t.numel()} elements, the table needs {need}")
    return table.shape[0], int(tiles)


def lamb_stage1(p, g, m, v, table, tiles, partials, beta1, beta2, step, eps, grad_scale=1.0, weight_decay=0.0, maximize=False,
                grad_norm=None, max_norm=0.0):
    """m, v <- the moments of this step; partials[2 * tile] = sum p^2, [2 * tile + 1] = sum u^2 of LAMB's update u (include/pero_hip.h)."""
    n, tiles = _layer_check("lamb_stage1", table, tiles, (p, g, m, v, partials, grad_norm), (p, g, m, v), partials=(partials, 2 * tiles))
    call("pero_lamb_stage1", ptr(p), ptr(g), ptr(m), ptr(v), ptr(table), n, tiles, ptr(partials), float(beta1), float(beta2), int(step),
         float(eps), float(grad_scale), float(weight_decay), int(bool(maximize)), ptr(grad_norm), float(max_norm), stream())


def lamb_stage2(p, m, v, p_bf16, table, tiles, stats, lr, beta1, beta2, step, eps, weight_decay=0.0):
    """p <- p - (lr * r) * u with u computed again from the stored m, v and r = stats[tensor][2]; p_bf16 (may be None) <- its bf16 copy."""
    n, tiles = _layer_check("lamb_stage2", table, tiles, (p, m, v, stats), (p, m, v, p_bf16), stats=(stats, 3 * table.shape[0]))
    call("pero_lamb_stage2", ptr(p), ptr(m), ptr(v), ptr(p_bf16), ptr(table), n, tiles, ptr(stats), float(lr), float(beta1), float(beta2),
         int(step), float(eps), float(weight_decay), stream())


def lars_stage1(p, g, table, tiles, partials, grad_scale=1.0, weight_decay=0.0, maximize=False, grad_norm=None, max_norm=0.0):
    """partials[2 * tile] = sum p^2, [2 * tile + 1] = sum u^2 of LARS's update u = g' + weight_decay * p; nothing else is written."""
    n, tiles = _layer_check("lars_stage1", table, tiles, (p, g, partials, grad_norm), (p, g), partials=(partials, 2 * tiles))
    call("pero_lars_stage1", ptr(p), ptr(g), ptr(table), n, tiles, ptr(partials), float(grad_scale), float(weight_decay),
         int(bool(maximize)), ptr(grad_norm), float(max_norm), stream())


def lars_stage2(p, g, buf, p_bf16, table, tiles, stats, lr, momentum, grad_scale=1.0, weight_decay=0.0, maximize=False, grad_norm=None,
                max_norm=0.0):
    """buf <- momentum * buf + r * u, p <- p - lr * buf with r = stats[tensor][2]; p_bf16 (may be None) <- its bf16 copy."""
    n, tiles = _layer_check("lars_stage2", table, tiles, (p, g, buf, stats, grad_norm), (p, g, buf, p_bf16), stats=(stats, 3 * table.shape[0]))
    call("pero_lars_stage2", ptr(p), ptr(g), ptr(buf), ptr(p_bf16), ptr(table), n, tiles, ptr(stats), float(lr), float(momentum),
         float(grad_scale), float(weight_decay), int(bool(maximize)), ptr(grad_norm), float(max_norm), stream())


def layer_ratio_finish(partials, table, tiles, coefficient, adapt, stats):
    """stats[t] = (|p|, |u|, r): r = coefficient * |p| / |u| if `adapt` and both norms are > 0, else exactly 1."""
    n, tiles = _layer_check("layer_ratio_finish", table, tiles, (partials, stats), partials=(partials, 2 * tiles), stats=(stats, 3 * table.shape[0]))
    call("pero_layer_ratio_finish", ptr(partials), ptr(table), n, float(coefficient), int(bool(adapt)), ptr(stats), stream())


def vq_argmin(x, codebook, want_dist=False):
    _req_cuda(x, codebook)
    M, D = x.shape
    K = codebook.shape[0]
    idx = torch.empty(M, device=x.device, dtype=torch.int64)
    best = torch.empty(M, device=x.device, dtype=torch.float32) if want_dist else None
    work = torch.empty(M + K, device=x.device, dtype=torch.float32)
    call("pero_vq_argmin", ptr(x), ptr(codebook), ptr(idx), ptr(best), ptr(work), M, K, D, stream())
    return (idx, best) if want_dist else idx


def vq_gather(x, codebook, idx):
    q = torch.empty_like(x)
    call("pero_vq_gather", ptr(x), ptr(codebook), ptr(idx), ptr(q), x.shape[0], x.shape[1], stream())
    return q


def vq_ema_update(x, idx, ema_cluster_size, ema_w, codebook, decay, epsilon):
    """In-place EMA codebook update (models/autoencoders.py:225-237); all tensors f32 contiguous on the device."""
    M, D = x.shape
    K = codebook.shape[0]
    work = torch.empty(K + K * D, device=x.device, dtype=torch.float32)
    call("pero_vq_ema_update", ptr(x), ptr(idx), ptr(ema_cluster_size), ptr(ema_w), ptr(codebook), ptr(work), M, K, D,
         float(decay), float(epsilon), stream())


def sum_scale(partial, scale=1.0, out=None):
    """out[0] = scale * sum(partial) in a fixed order (f32)."""
    out = torch.empty(1, device=partial.device, dtype=torch.float32) if out is None else out
    call("pero_sum_scale", ptr(partial), ptr(out), partial.numel(), float(scale), stream())
    return out


# ---- mini-batch k-means fit (scripts/kmeans.py) -------------------------------------------------------------------
def kmeans_update(x, labels, centers, weight_sums, shift=None):
    """In-place mini-batch centre update (sklearn _minibatch_update_dense): x (B, D) f32, labels (B) int64 from
    `vq_argmin` on the centres as they are now, centers (K, D) f32, weight_sums (K) f64.  Returns the f32 scalar
    tensor sum |c_new - c_old|^2.  Bit-identical from run to run: the stable sort fixes the order of every sum."""
    _req_cuda(x, labels, centers, weight_sums)
    B, D = x.shape
    K = centers.shape[0]
    assert labels.shape == (B,) and labels.dtype == torch.int64 and centers.shape == (K, D) and weight_sums.shape == (K,)
    assert x.dtype == centers.dtype == torch.float32 and weight_sums.dtype == torch.float64
    assert x.is_contiguous() and centers.is_contiguous() and weight_sums.is_contiguous()
    sorted_labels, order = torch.sort(labels, stable=True)
    shift = torch.empty(1, device=x.device, dtype=torch.float32) if shift is None else shift
    work = torch.empty(2 * K + 2, device=x.device, dtype=torch.int32)
    call("pero_kmeans_update", ptr(x), ptr(order), ptr(sorted_labels), ptr(centers), ptr(weight_sums), ptr(shift), ptr(work), B, K, D,
         stream())
    return shift


def kmeans_sqnorm(x):
    _req_cuda(x)
    rows, d = x.shape
    out = torch.empty(rows, device=x.device, dtype=torch.float32)
    call("pero_kmeans_sqnorm", ptr(x), ptr(out), rows, d, stream())
    return out


def kmeans_pp_workspace(n, t, device):
    return torch.empty(4 + t * n + t * ((n + 63) // 64), device=device, dtype=torch.float32)


def kmeans_pp_step(x, sqnorm, closest_dist_sq, candidates, chosen, potential, work=None):
    """One centre of greedy k-means++: of the candidate rows `candidates` (t int64) the one with the lowest potential
    is committed - its index to chosen[0] (int64), its potential to potential[0] (f64), closest_dist_sq updated in
    place.  No host synchronisation."""
    _req_cuda(x, sqnorm, closest_dist_sq, candidates, chosen, potential)
    n, d = x.shape
    t = candidates.numel()
    assert candidates.dtype == chosen.dtype == torch.int64 and potential.dtype == torch.float64 and x.is_contiguous()
    work = kmeans_pp_workspace(n, t, x.device) if work is None else work
    assert work.numel() >= 4 + t * n + t * ((n + 63) // 64)
    call("pero_kmeans_pp_step", ptr(x), ptr(sqnorm), ptr(closest_dist_sq), ptr(candidates), ptr(chosen), ptr(potential), ptr(work), n, d, t,
         stream())


def kmeans_converge(batch_inertia, shift, state, n_samples, batch_size, tol, max_no_improvement):
    """Advance the on-device early-stopping state (f64[6], see include/pero_hip.h) by one step."""
    call("pero_kmeans_converge", ptr(batch_inertia), ptr(shift), ptr(state), int(n_samples), int(batch_size), float(tol),
         -1 if max_no_improvement is None else int(max_no_improvement), stream())


def gather_rows(src, index, n_rows_out=None, out=None):
    n_idx = index.numel()
    n_out = n_idx if n_rows_out is None else n_rows_out
    d = src.shape[-1]
    dst = torch.empty((n_out, d), device=src.device, dtype=src.dtype) if out is None else out
    assert dst.shape == (n_out, d) and dst.is_contiguous()
    call("pero_gather_rows", ptr(src), ptr(index), ptr(dst), n_idx, n_out, d, dt(src), stream())
    return dst


def scatter_add_rows(src, index, dst):
    if index.numel():
        call("pero_scatter_add_rows", ptr(src), ptr(index), ptr(dst), index.numel(), dst.shape[-1], dt(src), stream())
    return dst


# ---- joint-embedding loss reductions ----------------------------------------------------------------------
def sqdiff_rows(x, ix, y, iy, scale):
    n, d = ix.numel(), x.shape[-1]
    partial = torch.empty(n, device=x.device, dtype=torch.float32)
    out = torch.empty(1, device=x.device, dtype=torch.float32)
    call("pero_sqdiff_rows", ptr(x), ptr(ix), ptr(y), ptr(iy), ptr(partial), ptr(out), n, d, float(scale), dt(x), stream())
    return out


def sqdiff_rows_bwd(x, ix, y, iy, dx, dy, g, coef):
    call("pero_sqdiff_rows_bwd", ptr(x), ptr(ix), ptr(y), ptr(iy), ptr(dx), ptr(dy), ptr(g), float(coef), ix.numel(),
         x.shape[-1], dt(x), stream())


def center_cols(z, colsum_, m):
    m_pad, d = z.shape
    zc = torch.empty_like(z)
    sumsq = zeros((d,), z.device, torch.float32)
    call("pero_center_cols", ptr(z), ptr(colsum_), ptr(zc), ptr(sumsq), m, m_pad, d, dt(z), stream())
    return zc, sumsq


def vicreg_var(sumsq, m, threshold, eps):
    d = sumsq.numel()
    cvar = torch.empty(d, device=sumsq.device, dtype=torch.float32)
    loss = torch.empty(1, device=sumsq.device, dtype=torch.float32)
    call("pero_vicreg_var", ptr(sumsq), ptr(cvar), ptr(loss), m, d, float(threshold), float(eps), stream())
    return cvar, loss


def vicreg_cov(cov, cvar, m, wv, wc, dtype):
    d = cov.shape[0]
    G = torch.empty((d, d), device=cov.device, dtype=dtype)
    rowpart = torch.empty(d, device=cov.device, dtype=torch.float32)
    loss = torch.empty(1, device=cov.device, dtype=torch.float32)
    call("pero_vicreg_cov", ptr(cov), ptr(cvar), ptr(G), ptr(rowpart), ptr(loss), d, m, float(wv), float(wc), dt(dtype), stream())
    return G, loss


BARLOW_TILE_ROWS = _lib.DEFINES["PERO_BARLOW_TILE_ROWS"]


def barlow_part_elems(n, d):
    """f32 elements of the Barlow Twins column reductions' workspace: the header's PERO_BARLOW_PART(n, d)."""
    return 4 * ((n + BARLOW_TILE_ROWS - 1) // BARLOW_TILE_ROWS) * d


def barlow_stats(x, ix, y, iy, eps):
    """(mean, rstd), f32 (2, d): the column statistics of the rows x[ix] (view 1) and y[iy] (view 2), biased variance."""
    n, d = ix.numel(), x.shape[-1]
    part = torch.empty(barlow_part_elems(n, d), device=x.device, dtype=torch.float32)
    mean = torch.empty((2, d), device=x.device, dtype=torch.float32)
    rstd = torch.empty((2, d), device=x.device, dtype=torch.float32)
    call("pero_barlow_stats", ptr(x), ptr(ix), ptr(y), ptr(iy), ptr(part), ptr(mean), ptr(rstd), n, d, float(eps), dt(x), stream())
    return mean, rstd


def barlow_standardize(x, ix, y, iy, mean, rstd, n_pad):
    """zh (2, n_pad, d): the standardised rows of both views, rows behind ix.numel() zero."""
    n, d = ix.numel(), x.shape[-1]
    zh = torch.empty((2, n_pad, d), device=x.device, dtype=x.dtype)
    call("pero_barlow_standardize", ptr(x), ptr(ix), ptr(y), ptr(iy), ptr(mean), ptr(rstd), ptr(zh), n, n_pad, d, dt(x), stream())
    return zh


def barlow_corr(c, n, lambda_offdiag, dtype):
    """(out, G): out f32 (3,) = loss, on-diagonal part, off-diagonal part of the cross-correlation c (d, d) f32; G (d, d) of `dtype`."""
    d = c.shape[0]
    G = torch.empty((d, d), device=c.device, dtype=dtype)
    rowpart = torch.empty(2 * d, device=c.device, dtype=torch.float32)
    out = torch.empty(3, device=c.device, dtype=torch.float32)
    call("pero_barlow_corr", ptr(c), ptr(G), ptr(rowpart), ptr(out), d, n, float(lambda_offdiag), dt(dtype), stream())
    return out, G


def barlow_bwd_stats(dzh, zh, n):
    """(a, b), f32 (2, d): column sums of dzh and of dzh * zh over the first n rows of each view."""
    _, n_pad, d = zh.shape
    part = torch.empty(barlow_part_elems(n, d), device=zh.device, dtype=torch.float32)
    a = torch.empty((2, d), device=zh.device, dtype=torch.float32)
    b = torch.empty((2, d), device=zh.device, dtype=torch.float32)
    call("pero_barlow_bwd_stats", ptr(dzh), ptr(zh), ptr(part), ptr(a), ptr(b), n, n_pad, d, dt(zh), stream())
    return a, b


def barlow_standardize_bwd(dzh, zh, rstd, a, b, ix, iy, dx, dy, g):
    """dx[ix[r]], dy[iy[r]] = the gradient rows of the standardisation (stored; the other rows of dx, dy are left as they are)."""
    _, n_pad, d = zh.shape
    call("pero_barlow_standardize_bwd", ptr(dzh), ptr(zh), ptr(rstd), ptr(a), ptr(b), ptr(ix), ptr(iy), ptr(dx), ptr(dy), ptr(g),
         ix.numel(), n_pad, d, dt(zh), stream())


def scatter_add_rows_scaled(src, index, dst, g):
    if index.numel():
        call("pero_scatter_add_rows_scaled", ptr(src), ptr(index), ptr(dst), ptr(g), index.numel(), dst.shape[-1], dt(src), stream())
    return dst


def rownorm_fwd(x, out=None):
    rows, d = x.shape
    if out is not None:
        xn, inv = out
        assert xn.shape == x.shape and xn.is_contiguous() and inv.numel() == rows and inv.is_contiguous()
    else:
        xn = torch.empty_like(x)
        inv = torch.empty(rows, device=x.device, dtype=torch.float32)
    call("pero_rownorm_fwd", ptr(x), ptr(xn), ptr(inv), rows, d, dt(x), stream())
    return xn, inv


def rownorm_bwd(xn, dxn, inv, g=None):
    dx = torch.empty_like(xn)
    call("pero_rownorm_bwd", ptr(xn), ptr(dxn), ptr(inv), ptr(g), ptr(dx), xn.shape[0], xn.shape[1], dt(xn), stream())
    return dx


def ntxent_cols(sim, want_grad_dtype=None):
    lines, S, _ = sim.shape
    line_loss = torch.empty(lines, device=sim.device, dtype=torch.float32)
    loss = torch.empty(1, device=sim.device, dtype=torch.float32)
    dsim = torch.empty(sim.shape, device=sim.device, dtype=want_grad_dtype) if want_grad_dtype is not None else None
    call("pero_ntxent_cols", ptr(sim), ptr(line_loss), ptr(loss), ptr(dsim), lines, S,
         dt(want_grad_dtype) if want_grad_dtype is not None else PERO_F32, stream())
    return loss, line_loss, dsim


def ntxent_cols_cross(sim, cross, own0, grad_dtype):
    """sim (lines, S, S) f32, cross (lines*S, L) f32 -> (loss [1], line_loss, dsim, dcross) - see pero_ntxent_cols_cross."""
    lines, S, _ = sim.shape
    L = cross.shape[1]
    line_loss = torch.empty(lines, device=sim.device, dtype=torch.float32)
    loss = torch.empty(1, device=sim.device, dtype=torch.float32)
    dsim = torch.empty(sim.shape, device=sim.device, dtype=grad_dtype)
    dcross = torch.empty(cross.shape, device=sim.device, dtype=grad_dtype)
    call("pero_ntxent_cols_cross", ptr(sim), ptr(cross), ptr(line_loss), ptr(loss), ptr(dsim), ptr(dcross), lines, S, L, int(own0),
         dt(grad_dtype), stream())
    return loss, line_loss, dsim, dcross


def line_mean(x2, lines, S):
    """x2 (lines*S, d) -> f32 (lines, d): mean over the rows of each line."""
    out = torch.empty((lines, x2.shape[1]), device=x2.device, dtype=torch.float32)
    call("pero_line_mean", ptr(x2), ptr(out), lines, S, x2.shape[1], dt(x2), stream())
    return out


def add_line_rows_(dst2, src, lines, S, scale):
    """dst2 (lines*S, d) += scale * src (lines, d) f32, row-broadcast per line; in place."""
    call("pero_add_line_rows", ptr(dst2), ptr(src), lines, S, dst2.shape[1], float(scale), dt(dst2), stream())
    return dst2


# ---- NT-Xent on collated batches (csrc/ntxent_ragged.hip) ---------------------------------------------------------
def _mask_u8(m, device):
    t = torch.as_tensor(m)
    if t.dtype != torch.uint8:
        t = t.to(torch.uint8)    # the masks hold 0, 1 and 2
    return t.to(device, non_blocking=True).contiguous()


def ntxent_slots(image_mask1, image_mask2, shift_mask1, shift_mask2, device=None):
    """Four (lines, S) integer masks -> (slot (2*lines, S) int32: view 1's lines, then view 2's; count (lines) int32) - see
    pero_ntxent_slots.  Masks of another integer dtype, or on the host, are converted / uploaded first."""
    if device is None:
        device = next(m.device for m in (image_mask1, image_mask2, shift_mask1, shift_mask2) if isinstance(m, torch.Tensor) and m.is_cuda)
    im1, im2, sm1, sm2 = (_mask_u8(m, device) for m in (image_mask1, image_mask2, shift_mask1, shift_mask2))
    lines, S = im1.shape
    assert im2.shape == sm1.shape == sm2.shape == (lines, S)
    slot = torch.empty((2 * lines, S), device=device, dtype=torch.int32)
    count = torch.empty(lines, device=device, dtype=torch.int32)
    call("pero_ntxent_slots", ptr(im1), ptr(im2), ptr(sm1), ptr(sm2), ptr(slot[:lines]), ptr(slot[lines:]), ptr(count), lines, S, stream())
    return slot, count


def ntxent_rows_fwd(x, slot, count, Sp, out=None):
    """x (lines*S, d), slot (lines, S), count (lines or lines / 2) -> compact normalised rows (lines*Sp, d) and inv (lines*Sp) f32."""
    lines, S = slot.shape
    d = x.shape[1]
    assert x.shape[0] == lines * S and x.is_contiguous() and slot.is_contiguous() and slot.dtype == count.dtype == torch.int32
    if out is not None:
        xn, inv = out
        assert xn.shape == (lines * Sp, d) and xn.is_contiguous() and inv.numel() == lines * Sp and inv.is_contiguous()
    else:
        xn = torch.empty((lines * Sp, d), device=x.device, dtype=x.dtype)
        inv = torch.empty(lines * Sp, device=x.device, dtype=torch.float32)
    call("pero_ntxent_rows_fwd", ptr(x), ptr(slot), ptr(count), ptr(xn), ptr(inv), lines, count.numel(), S, Sp, d, dt(x), stream())
    return xn, inv


def ntxent_rows_bwd(xn, dxn, inv, slot, count, Sp, g=None):
    """Compact xn, dxn (lines*Sp, d) -> dx (lines*S, d): rownorm_bwd at the selected positions, zeros elsewhere."""
    lines, S = slot.shape
    d = xn.shape[1]
    assert xn.shape == dxn.shape == (lines * Sp, d) and xn.is_contiguous() and dxn.is_contiguous() and slot.is_contiguous()
    dx = torch.empty((lines * S, d), device=xn.device, dtype=xn.dtype)
    call("pero_ntxent_rows_bwd", ptr(xn), ptr(dxn), ptr(inv), ptr(slot), ptr(count), ptr(g), ptr(dx), lines, count.numel(), S, Sp, d, dt(xn),
         stream())
    return dx


def ntxent_cols_ragged(sim, count, grad_dtype=None, cross=None, own0=0):
    """sim (lines, Sp, Sp) f32, count (lines) int32, cross (lines*Sp, L) f32 or None -> (loss [1], line_loss, dsim, dcross) - see
    pero_ntxent_cols_ragged.  grad_dtype None: no gradients."""
    lines, Sp, _ = sim.shape
    assert sim.is_contiguous() and count.numel() == lines and count.dtype == torch.int32
    L = 0
    if cross is not None:
        L = cross.shape[1]
        assert cross.shape == (lines * Sp, L) and cross.is_contiguous() and cross.dtype == torch.float32
    line_loss = torch.empty(lines, device=sim.device, dtype=torch.float32)
    loss = torch.empty(1, device=sim.device, dtype=torch.float32)
    dsim = torch.empty(sim.shape, device=sim.device, dtype=grad_dtype) if grad_dtype is not None else None
    dcross = torch.empty(cross.shape, device=sim.device, dtype=grad_dtype) if grad_dtype is not None and cross is not None else None
    call("pero_ntxent_cols_ragged", ptr(sim), ptr(count), ptr(cross), ptr(line_loss), ptr(loss), ptr(dsim), ptr(dcross), lines, Sp, L, int(own0),
         dt(grad_dtype) if grad_dtype is not None else PERO_F32, stream())
    return loss, line_loss, dsim, dcross


def line_mean_ragged(x2, count, Sp):
    """x2 (lines*Sp, d), count (lines) int32 -> f32 (lines, d): mean over the first count[l] rows of each line's block."""
    lines = count.numel()
    out = torch.empty((lines, x2.shape[1]), device=x2.device, dtype=torch.float32)
    call("pero_line_mean_ragged", ptr(x2), ptr(count), ptr(out), lines, Sp, x2.shape[1], dt(x2), stream())
    return out


def add_line_rows_ragged_(dst2, src, count, Sp):
    """dst2 (lines*Sp, d)[l*Sp + s] += src[l] / count[l] for s < count[l]; in place."""
    call("pero_add_line_rows_ragged", ptr(dst2), ptr(src), ptr(count), count.numel(), Sp, dst2.shape[1], dt(dst2), stream())
    return dst2


MAX_TOPK = _lib.DEFINES["PERO_MAX_TOPK"]


def label_rank(logits, labels, mask, ks=None, counters=None, want_ranks=False):
    """Rank of each masked row's label inside its logit row + accumulated top-k error counters
    (masked_pretraining/tester.py:72-113 on the device).  logits (rows, V) f32/bf16 (row pitch = stride(0));
    labels, mask (rows,) int64; ks: int32 device tensor of measured errors; counters: int64 device tensor
    [1 + len(ks)] that is ACCUMULATED into.  Returns (counters, ranks or None)."""
    rows, V = logits.shape
    assert logits.stride(1) == 1 and labels.numel() == rows and mask.numel() == rows
    nk = 0 if ks is None else int(ks.numel())
    ranks = torch.empty((rows, 3), device=logits.device, dtype=torch.int32) if want_ranks else None
    call("pero_label_rank", ptr(logits), logits.stride(0), ptr(labels), ptr(mask), rows, V, ptr(ks), nk, ptr(counters),
         ptr(ranks), dt(logits.dtype), stream())
    return counters, ranks


SIM_TOPK_MAX = _lib.DEFINES["PERO_SIM_TOPK_MAX"]


def sim_topk_key_splits(M, N):
    """The key-split count pero_sim_topk takes for key_splits = 0 (a function of M and N alone; no GPU needed)."""
    return int(_lib.lib().pero_sim_topk_key_splits(int(M), int(N)))


def sim_topk(q, keys, k, q_scale=None, key_scale=None, key_valid=None, skip=None, key_splits=0):
    """The k best keys of every query under score = (q . key) * q_scale * key_scale: higher score first, equal scores: lower key index
    first; keys with key_valid == 0, the key skip[m] and NaN scores never enter; unused slots are -1 / -inf (see pero_sim_topk).
    q (M, D), keys (N, D) f32 or bf16 with unit inner stride (row pitch = stride(0)); q_scale (M), key_scale (N) f32; key_valid (N) u8 or
    bool; skip (M) int32.  Returns (idx (M, k) int32, val (M, k) f32)."""
    _req_cuda(q, keys, q_scale, key_scale, key_valid, skip)
    M, D = q.shape
    N = keys.shape[0]
    if keys.shape[1] != D or keys.dtype != q.dtype or q.stride(1) != 1 or keys.stride(1) != 1:
        raise ValueError("sim_topk: q (M, D) and keys (N, D) need one dtype, one D and unit inner strides")
    for name, t, n, dtypes in (("q_scale", q_scale, M, (torch.float32,)), ("key_scale", key_scale, N, (torch.float32,)),
                               ("key_valid", key_valid, N, (torch.uint8, torch.bool)), ("skip", skip, M, (torch.int32,))):
        if t is not None and (t.numel() != n or t.dtype not in dtypes or not t.is_contiguous()):
            raise ValueError(f"sim_topk: {name} must be a contiguous {dtypes[0]} tensor of {n} elements")
    idx = torch.empty((M, int(k)), device=q.device, dtype=torch.int32)
    val = torch.empty((M, int(k)), device=q.device, dtype=torch.float32)
    splits = int(key_splits) if key_splits else sim_topk_key_splits(M, N)
    work = torch.empty(8 * splits * M * int(k), device=q.device, dtype=torch.uint8) if splits > 1 else None
    call("pero_sim_topk", ptr(q), q.stride(0), ptr(keys), keys.stride(0), ptr(q_scale), ptr(key_scale), ptr(key_valid), ptr(skip), ptr(idx),
         ptr(val), ptr(work), M, N, D, int(k), int(key_splits), dt(q), stream())
    return idx, val


def inv_rownorm(x):
    """inv (rows) f32 = 1 / max(|x_r|_2, 1e-12) of x (rows, D) f32 or bf16 (unit inner stride, row pitch = stride(0)): sim_topk's scales for the
    cosine."""
    _req_cuda(x)
    rows, D = x.shape
    inv = torch.empty(rows, device=x.device, dtype=torch.float32)
    call("pero_inv_rownorm", ptr(x), x.stride(0), ptr(inv), rows, D, dt(x), stream())
    return inv


def retrieval_hist(idx, target, hist):
    """hist (int64 [k + 2] on the device, ACCUMULATED): [0] += queries with target >= 0, [1 + r] += target at rank r of idx's row,
    [k + 1] += target not in the row (see pero_retrieval_hist).  idx (M, k) int32, target (M) int32."""
    M, k = idx.shape
    assert idx.dtype == target.dtype == torch.int32 and idx.is_contiguous() and target.is_contiguous() and target.numel() == M
    assert hist.dtype == torch.int64 and hist.numel() == k + 2 and hist.is_contiguous()
    call("pero_retrieval_hist", ptr(idx), ptr(target), ptr(hist), M, k, stream())
    return hist


def stack_lines(packed, offsets, widths, left_px, B, H, Wt, C):
    """Ragged uint8 lines (device, back to back, readable 8 bytes past the end) -> zero-padded (B, H, Wt, C) uint8 batch
    (common/dataloader.py:80-100).  offsets int64, widths / left_px int32 device tensors."""
    out = torch.empty((B, H, Wt, C), device=packed.device, dtype=torch.uint8)
    call("pero_stack_lines", ptr(packed), ptr(offsets), ptr(widths), ptr(left_px), ptr(out), B, H, Wt, C, stream())
    return out


AUGMENT_PARAMS = _lib.DEFINES["PERO_AUGMENT_PARAMS"]   # sy, ty, slope, slant, noise_amp, seed_lo, seed_hi


def augment_stack_lines(packed, offsets, widths, left_px, params, knots, lut, B, H, Wt, C, knot_shift=5):
    """stack_lines with a per-line warp, tone curve and noise on the way (include/pero_hip.h "line augmentation"): the same ragged
    upload in, the same zero-padded (B, H, Wt, C) uint8 batch out, line b still at columns [left_px[b], left_px[b] + widths[b]).
    params (B, AUGMENT_PARAMS) int32, knots (B, 2, (Wt >> knot_shift) + 2) int32, lut (B, C, 256) uint8 or None (identity): device
    tensors (common/augment.py LineAugmenter.draw makes them on the host).  C is at most 4."""
    NK = (Wt >> knot_shift) + 2
    want = [("packed", packed, torch.uint8, None), ("offsets", offsets, torch.int64, (B,)), ("widths", widths, torch.int32, (B,)),
            ("left_px", left_px, torch.int32, (B,)), ("params", params, torch.int32, (B, AUGMENT_PARAMS)),
            ("knots", knots, torch.int32, (B, 2, NK))]
    if lut is not None:
        want.append(("lut", lut, torch.uint8, (B, C, 256)))
    for name, t, dtype, shape in want:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.device != packed.device \
                or (shape is not None and tuple(t.shape) != shape):
            raise ValueError(f"augment_stack_lines: {name} must be a contiguous {dtype} tensor"
                             + (f" of shape {shape}" if shape is not None else "") + " on the device of packed")
    if not packed.is_cuda:
        raise ValueError("augment_stack_lines: the tensors must live on the GPU")
    if not 3 <= knot_shift <= 8 or (Wt * C) % 16 or not 1 <= C <= 4:
        raise ValueError("augment_stack_lines: knot_shift must be in [3, 8], Wt * C a multiple of 16 and C at most 4")
    out = torch.empty((B, H, Wt, C), device=packed.device, dtype=torch.uint8)
    call("pero_augment_stack_lines", ptr(packed), ptr(offsets), ptr(widths), ptr(left_px), ptr(params), ptr(knots), ptr(lut), ptr(out),
         B, H, Wt, C, AUGMENT_PARAMS, knot_shift, stream())
    return out


def line_masks(widths1, left1, S, subsampling, widths2=None, left2=None, crop_shifts=None):
    """Image masks, shifts and three-valued shift masks (common/dataloader.py:92-96, 124-138) from the per-line widths (px)
    and left paddings (label positions): int32 device tensors.  Returns (im1, im2, sm1, sm2, shifts); the last four are
    None for an unpaired batch."""
    B = widths1.numel()
    dev = widths1.device
    im1 = torch.empty((B, S), device=dev, dtype=torch.uint8)
    im2 = sm1 = sm2 = shifts = None
    if widths2 is not None:
        im2, sm1, sm2 = (torch.empty((B, S), device=dev, dtype=torch.uint8) for _ in range(3))
        shifts = torch.empty(B, device=dev, dtype=torch.int32)
    call("pero_line_masks", ptr(widths1), ptr(widths2), ptr(left1), ptr(left2), ptr(crop_shifts), ptr(im1), ptr(im2), ptr(sm1),
         ptr(sm2), ptr(shifts), B, S, subsampling, stream())
    return im1, im2, sm1, sm2, shifts


def _ctc_args(logits, targets, input_lengths, target_lengths):
    _req_cuda(logits, targets, input_lengths, target_lengths)
    n = input_lengths.numel()
    rows, C = logits.shape
    if not logits.is_contiguous() or rows % n or targets.dim() != 2 or targets.shape[0] != n or target_lengths.numel() != n:
        raise ValueError("ctc: logits must be contiguous (N*S, C), targets (N, Lmax), input_lengths and target_lengths (N)")
    for t in (targets, input_lengths, target_lengths):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError("ctc: targets and lengths must be contiguous int64 device tensors")
    return n, rows // n, C, targets.shape[1]


def _ctc_rows_args(name, logits, input_lengths):
    """The decoders' arguments: (N, S, C) of contiguous (N*S, C) logits and contiguous int64 input_lengths (N), N >= 1."""
    _req_cuda(logits, input_lengths)
    n = input_lengths.numel()
    rows, C = logits.shape
    if not logits.is_contiguous() or n == 0 or rows % n or input_lengths.dtype != torch.int64 or not input_lengths.is_contiguous():
        raise ValueError(f"{name}: logits must be contiguous (N*S, C), input_lengths contiguous int64 (N)")
    return n, rows // n, C


def ctc_fwd(logits, targets, input_lengths, target_lengths, blank=0):
    """logits (N*S, C) f32 / bf16; targets (N, Lmax), input_lengths, target_lengths (N) int64, all on the device.
    Returns (nll (N) f32, row_lse (N*S) f32, alpha (N, S, 2 Lmax + 1) f32); the last two go to ctc_bwd."""
    n, S, C, Lmax = _ctc_args(logits, targets, input_lengths, target_lengths)
    nll = torch.empty(n, device=logits.device, dtype=torch.float32)
    row_lse = torch.empty(n * S, device=logits.device, dtype=torch.float32)
    alpha = torch.empty((n, S, 2 * Lmax + 1), device=logits.device, dtype=torch.float32)
    call("pero_ctc_fwd", ptr(logits), ptr(targets), ptr(input_lengths), ptr(target_lengths), ptr(row_lse), ptr(alpha), ptr(nll),
         n, S, C, Lmax, blank, dt(logits), stream())
    return nll, row_lse, alpha


def ctc_bwd(logits, targets, input_lengths, target_lengths, row_lse, alpha, nll, g, blank=0, zero_infinity=False):
    """dlogits (N*S, C) in the logits' dtype = g[n] * d nll[n] / d logits (g: (N) f32 device tensor); the same bits on every call."""
    n, S, C, Lmax = _ctc_args(logits, targets, input_lengths, target_lengths)
    beta = torch.empty((n, S, 2 * Lmax + 1), device=logits.device, dtype=torch.float32)
    chain = torch.empty((n, Lmax), device=logits.device, dtype=torch.int32)
    dlogits = torch.empty_like(logits)
    call("pero_ctc_bwd", ptr(logits), ptr(targets), ptr(input_lengths), ptr(target_lengths), ptr(row_lse), ptr(alpha), ptr(nll), ptr(g),
         ptr(beta), ptr(chain), ptr(dlogits), n, S, C, Lmax, blank, int(bool(zero_infinity)), dt(logits), stream())
    return dlogits


def ctc_greedy(logits, input_lengths, blank=0):
    """Greedy CTC decoding of (N*S, C) logits: (labels (N, S) int64 padded with -1, lengths (N) int64), on the device."""
    n, S, C = _ctc_rows_args("ctc_greedy", logits, input_lengths)
    out = torch.empty((n, S), device=logits.device, dtype=torch.int64)
    out_lengths = torch.empty(n, device=logits.device, dtype=torch.int64)
    call("pero_ctc_greedy", ptr(logits), ptr(input_lengths), ptr(out), ptr(out_lengths), n, S, C, blank, dt(logits), stream())
    return out, out_lengths


def ctc_beam_workspace(S, C, beam_width):
    """(K, H) of pero_ctc_beam's workspaces (include/pero_hip.h): K best classes per row, H hash slots per line."""
    H = 1
    while H < 2 * S * beam_width:
        H *= 2
    return min(beam_width + 1, C - 1), H


def _ctc_beam_buffers(n, S, W, K, H, dev):
    """Outputs, trace and workspaces of pero_ctc_beam / pero_ctc_beam_lm: (out, out_lengths, out_scores, out_count, trace, row_lse, top_logp, top_class, hash)."""
    i32, i64, f32 = torch.int32, torch.int64, torch.float32
    trace = {"node_parent": torch.empty((n, S * W + 1), device=dev, dtype=i32), "node_label": torch.empty((n, S * W + 1), device=dev, dtype=i32),
             "node_count": torch.empty(n, device=dev, dtype=i32), "beam_node": torch.empty((n, S, W), device=dev, dtype=i32),
             "beam_score": torch.empty((n, S, W, 2), device=dev, dtype=f32)}
    return (torch.empty((n, W, S), device=dev, dtype=i64), torch.empty((n, W), device=dev, dtype=i64), torch.empty((n, W), device=dev, dtype=f32),
            torch.empty(n, device=dev, dtype=i64), trace, torch.empty(n * S, device=dev, dtype=f32), torch.empty((n * S, K), device=dev, dtype=f32),
            torch.empty((n * S, K), device=dev, dtype=i32), torch.empty((n, H), device=dev, dtype=i64))


def ctc_beam(logits, input_lengths, beam_width, blank=0, return_trace=False):
    """CTC prefix beam search of (N*S, C) logits, all on the device: (labels (N, W, S) int64 padded with -1, lengths (N, W) int64,
    scores (N, W) f32 best first, count (N) int64).  return_trace: also the dict of include/pero_hip.h's trace (node_parent, node_label,
    node_count, beam_node, beam_score)."""
    n, S, C = _ctc_rows_args("ctc_beam", logits, input_lengths)
    W = int(beam_width)
    if W < 1 or C < 2:
        raise ValueError("ctc_beam: beam_width >= 1 and C >= 2")
    K, H = ctc_beam_workspace(S, C, W)
    out, out_lengths, out_scores, out_count, trace, row_lse, top_logp, top_class, table = _ctc_beam_buffers(n, S, W, K, H, logits.device)
    call("pero_ctc_beam", ptr(logits), ptr(input_lengths), ptr(out), ptr(out_lengths), ptr(out_scores), ptr(out_count), ptr(trace["node_parent"]),
         ptr(trace["node_label"]), ptr(trace["node_count"]), ptr(trace["beam_node"]), ptr(trace["beam_score"]), ptr(row_lse), ptr(top_logp),
         ptr(top_class), ptr(table), n, S, C, blank, W, dt(logits), stream())
    return (out, out_lengths, out_scores, out_count, trace) if return_trace else (out, out_lengths, out_scores, out_count)


CTC_BEAM_MAX_CANDIDATES = 1088   # pero_ctc_beam_lm: W (K + 1) of one frame (include/pero_hip.h)


def ctc_beam_lm(logits, input_lengths, beam_width, lm, lm_weight=1.0, length_bonus=0.0, class_top=None, use_final=True, blank=0,
                return_trace=False):
    """ctc_beam with shallow fusion of an n-gram model (pero_ctc_beam_lm; lm: a recognition.NGramLM): (labels, lengths, scores, count,
    lm_scores (N, W) f32), the scores holding lm_weight * LM(string) + length_bonus * |string| (and, with use_final, the model's end term),
    lm_scores that part alone.  class_top: the K best classes of a frame that may start a new string, None = min(C - 1, 1088 // W - 1).
    return_trace: also the trace dict, with node_lm_state and node_lm_weight."""
    n, S, C = _ctc_rows_args("ctc_beam_lm", logits, input_lengths)
    W, dev = int(beam_width), logits.device
    if W < 1 or C < 2:
        raise ValueError("ctc_beam_lm: beam_width >= 1 and C >= 2")
    if lm.num_classes != C or lm.blank != blank:
        raise ValueError(f"ctc_beam_lm: the model is over {lm.num_classes} classes with blank {lm.blank}, the call has C = {C}, blank = {blank}")
    if class_top is None:
        K = max(min(C - 1, CTC_BEAM_MAX_CANDIDATES // W - 1), 1)
    else:
        K = min(max(int(class_top), 1), C - 1)
        if W * (K + 1) > CTC_BEAM_MAX_CANDIDATES:
            raise ValueError(f"ctc_beam_lm: beam_width * (class_top + 1) = {W} * {K + 1} exceeds the limit of {CTC_BEAM_MAX_CANDIDATES} "
                             f"candidates per frame (class_top <= {CTC_BEAM_MAX_CANDIDATES // W - 1} at this beam_width)")
    _, H = ctc_beam_workspace(S, C, W)
    t = lm.to(dev)
    out, out_lengths, out_scores, out_count, trace, row_lse, top_logp, top_class, table = _ctc_beam_buffers(n, S, W, K, H, dev)
    out_lm = torch.empty((n, W), device=dev, dtype=torch.float32)
    trace["node_lm_state"] = torch.empty((n, S * W + 1), device=dev, dtype=torch.int32)
    trace["node_lm_weight"] = torch.empty((n, S * W + 1), device=dev, dtype=torch.float32)
    call("pero_ctc_beam_lm", ptr(logits), ptr(input_lengths), ptr(t["backoff_state"]), ptr(t["backoff_weight"]), ptr(t["final"]), ptr(t["arc_begin"]),
         ptr(t["arc_label"]), ptr(t["arc_logp"]), ptr(t["arc_next"]), ptr(out), ptr(out_lengths), ptr(out_scores), ptr(out_lm), ptr(out_count),
         ptr(trace["node_parent"]), ptr(trace["node_label"]), ptr(trace["node_lm_state"]), ptr(trace["node_lm_weight"]), ptr(trace["node_count"]),
         ptr(trace["beam_node"]), ptr(trace["beam_score"]), ptr(row_lse), ptr(top_logp), ptr(top_class), ptr(table), n, S, C, blank, W, K,
         lm.num_states, lm.num_arcs, lm.start, float(lm_weight), float(length_bonus), int(bool(use_final)), dt(logits), stream())
    return (out, out_lengths, out_scores, out_count, out_lm, trace) if return_trace else (out, out_lengths, out_scores, out_count, out_lm)


CTC_ALIGN_LDS_BACK_BYTES = _lib.DEFINES["PERO_CTC_ALIGN_LDS_BACK_BYTES"]


def ctc_align(logits, targets, input_lengths, target_lengths, blank=0, global_back=False):
    """CTC forced alignment (pero_ctc_align) of (N*S, C) f32 / bf16 logits to targets (N, Lmax), all on the device.  Returns
    (states (N, S) int32, spans (N, Lmax, 2) int32, path_logit (N) f32, score (N) f32, label_logp (N, Lmax) f32) as include/pero_hip.h
    defines them.  global_back: keep the backpointers in the global workspace even where they fit LDS (the same bits; for measurements)."""
    n, S, C, Lmax = _ctc_args(logits, targets, input_lengths, target_lengths)
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("ctc_align: logits must be f32 or bf16")
    if not 0 <= blank < C:
        raise ValueError(f"ctc_align: blank {blank} outside [0, {C})")
    dev, i32, f32 = logits.device, torch.int32, torch.float32
    states = torch.empty((n, S), device=dev, dtype=i32)
    spans = torch.empty((n, Lmax, 2), device=dev, dtype=i32)
    path_logit, score = torch.empty(n, device=dev, dtype=f32), torch.empty(n, device=dev, dtype=f32)
    label_logp = torch.empty((n, Lmax), device=dev, dtype=f32)
    row_lse = torch.empty(n * S, device=dev, dtype=f32)
    in_lds = S * (2 * Lmax + 1) <= CTC_ALIGN_LDS_BACK_BYTES and not global_back
    back = torch.empty(1 if in_lds else n * S * (2 * Lmax + 1), device=dev, dtype=torch.uint8)   # untouched when the backpointers fit LDS
    call("pero_ctc_align", ptr(logits), ptr(targets), ptr(input_lengths), ptr(target_lengths), ptr(states), ptr(spans), ptr(path_logit),
         ptr(score), ptr(label_logp), ptr(row_lse), ptr(back), n, S, C, Lmax, blank, int(bool(global_back)), dt(logits), stream())
    return states, spans, path_logit, score, label_logp


def _edit_args(name, a, a_len, b, b_len, **accumulators):
    """The checks edit_distance and edit_ops share; the accumulators (named as the message names them) may be None.  Returns N."""
    tensors = (a, a_len, b, b_len, *accumulators.values())
    _req_cuda(*tensors)
    n = a_len.numel()
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != n or b.shape[0] != n or b_len.numel() != n or n == 0:
        raise ValueError(f"{name}: a (N, La), b (N, Lb), a_len and b_len (N)")
    if any(t is not None and (t.dtype != torch.int64 or not t.is_contiguous()) for t in tensors):
        what = ["labels", "lengths", *accumulators]
        raise ValueError(f"{name}: {', '.join(what[:-1])} and {what[-1]} must be contiguous int64 device tensors")
    return n


def edit_distance(a, a_len, b, b_len, totals=None):
    """Levenshtein distance per pair of padded int64 label matrices a (N, La), b (N, Lb) with lengths (N), all on the device: dist (N) int64.
    totals (2 int64 on the device): totals[0] += sum dist, totals[1] += sum b_len, exact (integer atomics)."""
    n = _edit_args("edit_distance", a, a_len, b, b_len, totals=totals)
    if totals is not None and totals.numel() != 2:
        raise ValueError("edit_distance: totals holds two int64")
    dist = torch.empty(n, device=a.device, dtype=torch.int64)
    call("pero_edit_distance", ptr(a), ptr(a_len), ptr(b), ptr(b_len), ptr(dist), ptr(totals), n, a.shape[1], b.shape[1], stream())
    return dist


def edit_separator_table(separators, num_classes, device):
    """The is_sep byte table of pero_edit_ops on `device`: (num_classes) uint8, 1 at every class id of `separators` (ids outside
    [0, num_classes) name no class and are dropped)."""
    table = torch.zeros(num_classes, dtype=torch.uint8)
    ids = sorted({int(c) for c in separators if 0 <= int(c) < num_classes})
    if ids:
        table[torch.tensor(ids)] = 1
    return table.to(device)


def edit_ops(a, a_len, b, b_len, num_classes=None, separators=None, totals=None, confusion=None, want_script=True, want_spans=False):
    """Edit operations (pero_edit_ops) of hypotheses a (N, La) against references b (N, Lb), padded int64 label matrices with lengths (N), all
    on the device.  Returns (counts (N, 4) int64: substitutions, insertions, deletions, hits; script (N, La + Lb) int8 and script_len (N)
    int32, or None, None without want_script; a_spans (N, (La + 1) / 2, 2), b_spans (N, (Lb + 1) / 2, 2) int32 with want_spans, else None,
    None) as include/pero_hip.h defines them.
    separators: an iterable of class ids (or a ready table of edit_separator_table) -> word level; needs num_classes.
    totals (6 int64 on the device) and confusion ((C + 1, C + 1) int64 on the device, symbol level only; C = num_classes, or taken from its
    shape) are ACCUMULATED, exact (integer atomics)."""
    n = _edit_args("edit_ops", a, a_len, b, b_len, totals=totals, confusion=confusion)
    if totals is not None and totals.numel() != 6:
        raise ValueError("edit_ops: totals holds six int64")
    if confusion is not None:
        if separators is not None:
            raise ValueError("edit_ops: the confusion matrix is symbol level only")
        if confusion.dim() != 2 or confusion.shape[0] != confusion.shape[1] or confusion.shape[0] < 2:
            raise ValueError("edit_ops: confusion is (C + 1, C + 1)")
        if num_classes is None:
            num_classes = confusion.shape[0] - 1
        if confusion.shape[0] != num_classes + 1:
            raise ValueError(f"edit_ops: confusion is {tuple(confusion.shape)}, expected ({num_classes + 1}, {num_classes + 1})")
    if want_spans and separators is None:
        raise ValueError("edit_ops: spans are word level only (give separators)")
    is_sep = None
    if separators is not None:
        if num_classes is None or num_classes < 1:
            raise ValueError("edit_ops: separators need num_classes >= 1")
        if isinstance(separators, torch.Tensor) and separators.dtype == torch.uint8:
            is_sep = separators
            _req_cuda(is_sep)
            if is_sep.numel() != num_classes or not is_sep.is_contiguous():
                raise ValueError("edit_ops: a separator table is (num_classes) contiguous uint8")
        else:
            is_sep = edit_separator_table(separators, num_classes, a.device)
    La, Lb, dev = a.shape[1], b.shape[1], a.device
    counts = torch.empty((n, 4), device=dev, dtype=torch.int64)
    script = torch.empty((n, La + Lb), device=dev, dtype=torch.int8) if want_script else None
    script_len = torch.empty(n, device=dev, dtype=torch.int32) if want_script else None
    a_spans = torch.empty((n, (La + 1) // 2, 2), device=dev, dtype=torch.int32) if want_spans else None
    b_spans = torch.empty((n, (Lb + 1) // 2, 2), device=dev, dtype=torch.int32) if want_spans else None
    call("pero_edit_ops", ptr(a), ptr(a_len), ptr(b), ptr(b_len), ptr(is_sep), ptr(counts), ptr(script), ptr(script_len), ptr(a_spans), ptr(b_spans),
         ptr(totals), ptr(confusion), n, La, Lb, num_classes or 0, stream())
    return counts, script, script_len, a_spans, b_spans


# ---- latent-target self-distillation (csrc/latent.hip; formulas and summation orders in include/pero_hip.h) ------------------------------
LATENT_MAX_K = _lib.DEFINES["PERO_LATENT_MAX_K"]
LATENT_MAX_D = _lib.DEFINES["PERO_LATENT_MAX_D"]


def ema_table(entries, device):
    """entries: [(source tensor or device address, destination offset, count)] -> (table int64 [n][4] = {source address, destination offset,
    count, first tile} on `device`, total tiles of LAYER_TILE elements).  The table carries its extent (the largest offset + count) as
    `_pero_extent`, a host integer, so that ema_update can refuse a flat buffer shorter than its table without reading the device."""
    rows_ = []
    for src, off, n in entries:
        if isinstance(src, torch.Tensor):
            if src.dtype != torch.float32 or not src.is_contiguous() or not src.is_cuda or src.numel() != n:
                raise TypeError("ema_table: sources are contiguous f32 device tensors of `count` elements")
            src = src.data_ptr()
        if off % 8 or off < 0 or n < 1 or src % 4 or src == 0:
            raise ValueError(f"ema_table: offsets are multiples of 8 elements, sources 4-byte aligned, segments not empty; got offset {off}, count {n}")
        rows_.append([src, off, n])
    return _tile_table(rows_, lambda r: layer_tiles(r[2]), lambda r: r[1] + r[2], device, refuse=("ema_table", "segments"))


def ema_update(avg, table, tiles, w, avg_bf16=None):
    """avg <- avg + w * (source - avg) over every segment of `table` in one launch, w = (float)(1 - tau); avg_bf16 (may be None) <- the
    bf16 copy of the new average."""
    _req_cuda(avg, table, avg_bf16)
    extent = _table_check("ema_update", table, 4, "ema_table")
    if avg.dtype != torch.float32 or not avg.is_contiguous() or avg.numel() < extent:
        raise ValueError(f"ema_update: avg is a contiguous f32 buffer of at least {extent} elements")
    if avg_bf16 is not None and (avg_bf16.dtype != torch.bfloat16 or not avg_bf16.is_contiguous() or avg_bf16.numel() < extent):
        raise ValueError(f"ema_update: avg_bf16 is a contiguous bf16 buffer of at least {extent} elements")
    call("pero_ema_update", ptr(avg), ptr(avg_bf16), ptr(table), table.shape[0], int(tiles), float(w), stream())
    return avg


def latent_targets(mats, index, n_pad=None, eps=1e-5):
    """y (n_pad, d) f32: row i < n is the mean over the K matrices of the row index[i] normalised to zero mean / unit variance over d
    (a LayerNorm without weights); rows behind n are zero.  mats: K matrices (rows, d), all f32 or all bf16, contiguous."""
    mats = list(mats)
    _req_cuda(index, *mats)
    rows, d = mats[0].shape
    if any(m.shape != (rows, d) or m.dtype != mats[0].dtype or not m.is_contiguous() for m in mats):
        raise TypeError("latent_targets: the matrices have one shape and dtype and are contiguous")
    if index.dtype != torch.int64 or not index.is_contiguous():
        raise TypeError("latent_targets: index is a contiguous int64 tensor")
    n = index.numel()
    n_pad = n if n_pad is None else int(n_pad)
    y = torch.empty((n_pad, d), device=mats[0].device, dtype=torch.float32)
    ptrs = (ctypes.c_void_p * len(mats))(*[m.data_ptr() for m in mats])
    call("pero_latent_targets", ctypes.cast(ptrs, ctypes.c_void_p), len(mats), ptr(index), ptr(y), rows, n, n_pad, d, float(eps), dt(mats[0]), stream())
    return y


def _latent_loss_args(name, pred, y, n):
    _req_cuda(pred, y)
    if pred.dim() != 2 or y.shape != pred.shape or y.dtype != torch.float32 or not pred.is_contiguous() or not y.is_contiguous():
        raise TypeError(f"{name}: pred (n_pad, d) f32 / bf16 and y (n_pad, d) f32, contiguous")
    if not 0 <= n <= pred.shape[0]:
        raise ValueError(f"{name}: n = {n} rows of {pred.shape[0]}")
    return pred.shape


def latent_loss_fwd(pred, y, n, beta):
    """loss (1,) f32 = mean over the first n rows of smooth_l1(pred - y, beta) (beta == 0: the squared error)."""
    _, d = _latent_loss_args("latent_loss_fwd", pred, y, n)
    work = torch.empty(max(n, 1), device=pred.device, dtype=torch.float32)
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    call("pero_latent_loss_fwd", ptr(pred), ptr(y), ptr(work), ptr(loss), n, d, float(beta), dt(pred), stream())
    return loss


def latent_loss_bwd(pred, y, n, beta, dloss=None):
    """dpred (n_pad, d) in pred's dtype: dloss * l'(pred - y) / (n d) on the first n rows, zero rows behind; dloss: one f32 on the device."""
    n_pad, d = _latent_loss_args("latent_loss_bwd", pred, y, n)
    dpred = torch.empty_like(pred)
    call("pero_latent_loss_bwd", ptr(pred), ptr(y), ptr(dloss), ptr(dpred), n, n_pad, d, float(beta), dt(pred), stream())
    return dpred


# ---- VGG tokenizer front end (csrc/conv.hip): activations in halo layout (N, H + 2, W + 2, C) --------------------------
CONV_SLACK_ROWS = _lib.DEFINES["PERO_CONV_SLACK_ROWS"]
CONV_ACTIVATIONS = {"none": _lib.DEFINES["PERO_CONV_ACT_NONE"], "relu": _lib.DEFINES["PERO_CONV_ACT_RELU"],
                    "leaky_relu": _lib.DEFINES["PERO_CONV_ACT_LEAKY_RELU"]}


def halo_buffer(n, h, w, c, dtype, device):
    """Uninitialised activation buffer in halo layout, (n, h + 2, w + 2, c), 16-byte aligned, with the header's PERO_CONV_SLACK_ROWS spare
    rows of c values in front of it and behind it (the kernels guard their loads, so that is 0 rows today)."""
    if min(n, h, w, c) < 1:
        raise ValueError(f"halo_buffer: n, h, w, c = {n}, {h}, {w}, {c} must all be >= 1")
    rows, slack = n * (h + 2) * (w + 2), CONV_SLACK_ROWS * (w + 3)
    esz = torch.empty((), dtype=dtype).element_size()
    front = -(-slack * c * esz // 16) * 16 // esz           # whole 16-byte units, so the first row stays aligned
    flat = torch.empty(front + (rows + slack) * c, device=device, dtype=dtype)
    return flat[front:front + rows * c].view(n, h + 2, w + 2, c)


def _halo_check(name, x, what="x"):
    _req_cuda(x)
    if x.dim() != 4 or x.shape[1] < 3 or x.shape[2] < 3 or not x.is_contiguous() or x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{name}: {what} must be a contiguous f32 / bf16 halo-layout tensor (N, H + 2, W + 2, C), got {tuple(x.shape)} {x.dtype}")
    n, hp, wp, c = x.shape
    return n, hp - 2, wp - 2, c


def conv3x3_pack_weight(weight, dtype, cin_pad=None):
    """Conv2d weight (Cout, Cin, 3, 3) -> the kernels' layout (Cout, 3, 3, cin_pad or Cin) in `dtype`, contiguous, zeros behind Cin (done
    once per checkpoint load).  `cin_pad`: the channel count of an input padded with zero channels (conv_channel_pad)."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"conv3x3_pack_weight: weight must be (Cout, Cin, 3, 3), got {tuple(weight.shape)}")
    packed = weight.detach().permute(0, 2, 3, 1).to(dtype)
    if cin_pad is not None:
        if cin_pad < weight.shape[1]:
            raise ValueError(f"conv3x3_pack_weight: cin_pad = {cin_pad} is below Cin = {weight.shape[1]}")
        packed = torch.nn.functional.pad(packed, (0, cin_pad - weight.shape[1]))
    return packed.contiguous()


def conv_channel_pad(c, dtype):
    """Channel count to pad a layer's input to so that pero_conv3x3 takes its tile kernel: the next multiple of 8 (bf16) or 4 (f32)."""
    unit = 8 if dtype == torch.bfloat16 else 4
    return -(-c // unit) * unit


def conv3x3(x, w, bias=None, activation="none", slope=0.01, out=None):
    """y = act(conv3x3(x) + bias), stride 1, padding 1.  x: halo layout (N, H + 2, W + 2, Cin); w: packed weight (Cout, 3, 3, Cin) of x's
    dtype (conv3x3_pack_weight); bias: f32 (Cout,) or None; activation: "none", "relu" or "leaky_relu" (with `slope`).  Returns the
    halo-layout output (N, H + 2, W + 2, Cout), halo pixels zero."""
    n, h, wd, cin = _halo_check("conv3x3", x)
    _req_cuda(w, bias)
    if w.dim() != 4 or tuple(w.shape[1:]) != (3, 3, cin) or w.dtype != x.dtype or not w.is_contiguous():
        raise ValueError(f"conv3x3: w must be a contiguous packed weight (Cout, 3, 3, {cin}) of {x.dtype}, got {tuple(w.shape)} {w.dtype}")
    cout = w.shape[0]
    if bias is not None and (tuple(bias.shape) != (cout,) or bias.dtype != torch.float32 or not bias.is_contiguous()):
        raise ValueError(f"conv3x3: bias must be f32 ({cout},), got {tuple(bias.shape)} {bias.dtype}")
    if activation not in CONV_ACTIVATIONS:
        raise ValueError(f"conv3x3: activation {activation!r} is not one of {sorted(CONV_ACTIVATIONS)}")
    if out is None:
        out = halo_buffer(n, h, wd, cout, x.dtype, x.device)
    elif tuple(out.shape) != (n, h + 2, wd + 2, cout) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError(f"conv3x3: out must be contiguous {(n, h + 2, wd + 2, cout)} of {x.dtype}, got {tuple(out.shape)} {out.dtype}")
    call("pero_conv3x3", ptr(x), ptr(w), ptr(bias), ptr(out), n, h, wd, cin, cout, CONV_ACTIVATIONS[activation], float(slope), dt(x), stream())
    return out


def image_to_halo(images, dtype, channels=None, out=None):
    """Line images -> the first layer's input, halo layout (N, H + 2, W + 2, channels or C) of `dtype`, the channels behind C zeros.
    uint8 (N, H, W, C) as BatchCreator delivers it is divided by 255 (autoencoders/batch_operator.py:14); float32 (N, C, H, W), as that
    batch operator builds it, is taken as it is."""
    _req_cuda(images)
    if images.dim() != 4 or not images.is_contiguous() or images.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"image_to_halo: images must be contiguous uint8 (N, H, W, C) or float32 (N, C, H, W), got {tuple(images.shape)} {images.dtype}")
    if images.dtype == torch.uint8:
        (n, h, w, c), kind = images.shape, _lib.DEFINES["PERO_IMAGE_U8_NHWC"]
    else:
        (n, c, h, w), kind = images.shape, _lib.DEFINES["PERO_IMAGE_F32_NCHW"]
    cp = c if channels is None else int(channels)
    if cp < c:
        raise ValueError(f"image_to_halo: channels = {cp} is below the images' {c}")
    if out is None:
        out = halo_buffer(n, h, w, cp, dtype, images.device)
    elif tuple(out.shape) != (n, h + 2, w + 2, cp) or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"image_to_halo: out must be contiguous {(n, h + 2, w + 2, cp)} of {dtype}, got {tuple(out.shape)} {out.dtype}")
    call("pero_image_to_halo", ptr(images), ptr(out), n, h, w, c, cp, kind, dt(dtype), stream())
    return out


def maxpool_nhwc(x, pool, a=None, b=None, token_rows=False, out=None):
    """MaxPool2d(kernel = stride = pool) of the halo-layout x (N, H + 2, W + 2, C), pool in {(2, 2), (2, 1), (1, 2), (1, 1)}, then
    y = max * a[c] + b[c] where a, b (f32 (C,)) are given.  Returns halo layout (N, H / ph + 2, W / pw + 2, C) or, with token_rows, the
    matrix (N * W / pw, (H / ph) * C) whose row n * (W / pw) + t holds column t's pixels top to bottom."""
    n, h, w, c = _halo_check("maxpool_nhwc", x)
    ph, pw = (int(p) for p in pool)
    if ph not in (1, 2) or pw not in (1, 2):
        raise ValueError(f"maxpool_nhwc: pool {tuple(pool)} is not one of (2, 2), (2, 1), (1, 2), (1, 1)")
    if h % ph or w % pw:
        raise ValueError(f"maxpool_nhwc: H = {h}, W = {w} are not divisible by the pool {(ph, pw)}")
    if (a is None) != (b is None):
        raise ValueError("maxpool_nhwc: the affine needs both a and b")
    for name, t in (("a", a), ("b", b)):
        _req_cuda(t)
        if t is not None and (tuple(t.shape) != (c,) or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"maxpool_nhwc: {name} must be f32 ({c},), got {tuple(t.shape)} {t.dtype}")
    ho, wo = h // ph, w // pw
    shape = (n * wo, ho * c) if token_rows else (n, ho + 2, wo + 2, c)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=x.dtype) if token_rows else halo_buffer(n, ho, wo, c, x.dtype, x.device)
    elif tuple(out.shape) != shape or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError(f"maxpool_nhwc: out must be contiguous {shape} of {x.dtype}, got {tuple(out.shape)} {out.dtype}")
    call("pero_maxpool_nhwc", ptr(x), ptr(out), ptr(a), ptr(b), n, h, w, c, ph, pw, int(bool(token_rows)), dt(x), stream())
    return out
