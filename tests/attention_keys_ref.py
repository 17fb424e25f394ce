"""The yardstick of the key-range attention tests: plain torch on the CPU, nothing read from the library.

* `attention(qkv, key_ranges, n, s, h)`: attention on the packed qkv rows with line b's keys restricted to [k0_b, k1_b), by masked fill of the
  scores, in the dtype of `qkv` (the tests hand it f64); `lse2` the base-2 log-sum-exp of the scaled scores over the same keys.
* `encoder_stack(...)`: the backbone - front end restated in torch, then a `torch.nn.TransformerEncoder` that carries the backbone's
  `encoder_layers.state_dict()` and gets the ranges as `src_key_padding_mask` - in f64, in `.train()` mode with dropout 0 (torch's eval-mode
  fast path zeroes the padded rows; the library computes every row, and so does the training path).
"""
import math

import torch


def key_padding_mask(key_ranges, s):
    """(N, S) bool, True where the key is OUTSIDE the line's range (torch's src_key_padding_mask convention)."""
    kr = torch.as_tensor(key_ranges).to(torch.int64)
    pos = torch.arange(s)[None, :]
    return ~((pos >= kr[:, :1]) & (pos < kr[:, 1:2]))


def split_heads(qkv, n, s, h):
    hd = qkv.shape[1] // 3 // h
    return qkv.reshape(n, s, 3, h, hd).permute(2, 0, 3, 1, 4)   # q, k, v: (N, h, S, hd)


def attention(qkv, key_ranges, n, s, h):
    """qkv (N*S, 3d) = [q | k | v], heads = contiguous hd slices -> out (N*S, d): every query of line b over the keys [k0_b, k1_b) only."""
    d = qkv.shape[1] // 3
    q, k, v = split_heads(qkv, n, s, h)
    scores = (q @ k.transpose(-1, -2)) / math.sqrt(d // h)
    scores = scores.masked_fill(key_padding_mask(key_ranges, s)[:, None, None, :], float("-inf"))
    return (torch.softmax(scores, -1) @ v).permute(0, 2, 1, 3).reshape(n * s, d)


def lse2(qkv, key_ranges, n, s, h):
    """(N, h, S): base-2 log-sum-exp of the scaled scores over the line's range."""
    d = qkv.shape[1] // 3
    q, k, _ = split_heads(qkv, n, s, h)
    scores = (q @ k.transpose(-1, -2)) / math.sqrt(d // h)
    scores = scores.masked_fill(key_padding_mask(key_ranges, s)[:, None, None, :], float("-inf"))
    return torch.logsumexp(scores, -1) / math.log(2.0)


def positional_table(d_model, max_len):
    pe = torch.zeros(max_len, d_model, dtype=torch.float64)
    position = torch.arange(0, max_len, dtype=torch.float64).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2).double() * (-math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def encoder_stack(backbone_sd, images_u8, offsets, key_ranges, num_heads, feedforward_dim, max_len=4096):
    """backbone_sd: the backbone's state_dict (conv_layer.*, intermediate_norm.*, encoder_layers.*); images_u8 (N, H, W, C) uint8; offsets: the
    lines' start rows in the positional table.  Returns (tokens (N*S, d) f64 with a graph, params: name -> f64 leaf with requires_grad)."""
    params = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in backbone_sd.items()}
    conv_w, conv_b = params["conv_layer.weight"], params["conv_layer.bias"]
    d, pw = conv_w.shape[0], conv_w.shape[-1]
    x = images_u8.cpu().double().permute(0, 3, 1, 2) / 255.0
    n, s = x.shape[0], x.shape[3] // pw
    y = torch.nn.functional.conv2d(x, conv_w, conv_b, stride=(conv_w.shape[-2], pw))   # (N, d, 1, S)
    t = y[:, :, 0, :].permute(0, 2, 1)                                                  # (N, S, d)
    t = torch.nn.functional.layer_norm(t, (d,), params["intermediate_norm.weight"], params["intermediate_norm.bias"], 1e-5)
    idx = torch.as_tensor(offsets, dtype=torch.int64)[:, None] + torch.arange(s)[None, :]
    t = t + positional_table(d, max_len)[idx]
    prefix = "encoder_layers."
    layer_sd = {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix)}
    num_layers = 1 + max(int(k.split(".")[1]) for k in layer_sd)
    layer = torch.nn.TransformerEncoderLayer(d_model=d, nhead=num_heads, dim_feedforward=feedforward_dim, dropout=0.0)
    enc = torch.nn.TransformerEncoder(layer, num_layers=num_layers, enable_nested_tensor=False).double().train()
    # the module computes with the f64 leaves themselves, so that their .grad is the reference gradient
    out = torch.func.functional_call(enc, layer_sd, (t.permute(1, 0, 2),), {"src_key_padding_mask": key_padding_mask(key_ranges, s)})   # (S, N, d)
    return out.permute(1, 0, 2).reshape(n * s, d), params
