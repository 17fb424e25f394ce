"""Plain torch f64 restatement of the VGG tokenizer front end (csrc/conv.hip, models/autoencoders.py VGGEncoder), written from the
formulas of include/pero_hip.h (not a test module; it never imports the library).  Tensors are (N, C, H, W) here; `to_halo` /
`from_halo` / `token_rows` translate to and from the layouts the kernels use.  Like tests/parity_ref.py every layer returns its result
and `mag`, the sum of the absolute values of the terms it adds: mag = |b| + sum |x| |w| for a convolution.

Also here, because the CPU test pins them and the GPU tests use them: the seeded weights of a stack (`seeded_state`) and the label
test's input (`label_case`)."""
import numpy as np
import torch
import torch.nn.functional as F

from parity_ref import f64

BN_EPS = 1e-5


# ---------------------------------------------------------------------------------------------- layouts
def to_halo(x, dtype=None):
    """(N, C, H, W) -> halo layout (N, H + 2, W + 2, C), border zeros."""
    y = F.pad(torch.as_tensor(x).permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1)).contiguous()
    return y if dtype is None else y.to(dtype)


def from_halo(y):
    """halo layout -> (interior as (N, C, H, W) f64, border values as a flat f64 tensor)."""
    y = f64(y)
    border = torch.ones(y.shape[1:3], dtype=torch.bool)
    border[1:-1, 1:-1] = False
    return y[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).contiguous(), y[:, border, :].reshape(-1)


def token_rows(x):
    """(N, C, h, T) -> (N * T, h * C): row n T + t holds column t top to bottom, C channels per pixel."""
    n, c, h, t = x.shape
    return x.permute(0, 3, 2, 1).reshape(n * t, h * c)


def from_token_rows(rows, n, c):
    rows = f64(rows)
    t, h = rows.shape[0] // n, rows.shape[1] // c
    return rows.reshape(n, t, h, c).permute(0, 3, 2, 1).contiguous()


# ---------------------------------------------------------------------------------------------- layers
def ingest(images, dtype=torch.float64):
    """uint8 (N, H, W, C) -> (N, C, H, W): value / 255, the f64 quotient rounded once to f32.  float (N, C, H, W): as it is."""
    images = torch.as_tensor(images)
    if images.dtype == torch.uint8:
        images = (images.double() / 255.0).float().permute(0, 3, 1, 2)
    return images.to(dtype).contiguous()


def activate(v, activation, slope=0.01):
    if activation == "relu":
        return torch.clamp_min(v, 0.0)
    if activation == "leaky_relu":
        return torch.where(v > 0, v, v * slope)
    assert activation == "none", activation
    return v


def conv(x, weight, bias, activation="none", slope=0.01, padding=(1, 1), dtype=torch.float64):
    """y = act(sum_{ci, ky, kx} x[ci][y + ky - 1][x + kx - 1] w[co][ci][ky][kx] + b[co]); n_terms = Cin kh kw + 1."""
    x, w = torch.as_tensor(x).to(dtype), torch.as_tensor(weight).to(dtype)
    b = None if bias is None else torch.as_tensor(bias).to(dtype)
    y = activate(F.conv2d(x, w, b, padding=padding), activation, slope)
    mag = F.conv2d(x.abs(), w.abs(), None if b is None else b.abs(), padding=padding)
    return y, mag


def bn_affine(weight, bias, running_mean, running_var, eps=BN_EPS, dtype=torch.float64):
    """Eval-mode BatchNorm2d as y = x a + b."""
    a = torch.as_tensor(weight).to(dtype) / torch.sqrt(torch.as_tensor(running_var).to(dtype) + eps)
    return a, torch.as_tensor(bias).to(dtype) - torch.as_tensor(running_mean).to(dtype) * a


def maxpool(x, pool, a=None, b=None):
    """max over (ph, pw) windows, then max * a[c] + b[c]; n_terms = 2 with the affine, the bare maximum is exact (mag = |max|)."""
    m = F.max_pool2d(x, kernel_size=tuple(pool), stride=tuple(pool))
    if a is None:
        return m, m.abs()
    a, b = a.to(m.dtype).view(1, -1, 1, 1), b.to(m.dtype).view(1, -1, 1, 1)
    return m * a + b, (m * a).abs() + b.abs()


# ---------------------------------------------------------------------------------------------- the stack
def stack(num_conv_blocks=3, num_conv_layers=(2, 2, 3), patch_size=(40, 8)):
    """[("conv", i) | ("pool", i, (ph, pw), has_bn)] with i the index inside the reference's `encoder` Sequential (models/helpers.py:4-56)."""
    out, reached, i = [], [1, 1], 0
    for block in range(num_conv_blocks):
        pool = [1, 1]
        for axis in (0, 1):
            if reached[axis] < patch_size[axis]:
                pool[axis], reached[axis] = 2, reached[axis] * 2
        for _ in range(num_conv_layers[block]):
            out.append(("conv", i))
            i += 2                      # Conv2d, ReLU
        out.append(("pool", i, tuple(pool), block == num_conv_blocks - 1))
        i += 1
    return out


def layer(step, x, state, dtype=torch.float64):
    """One step of the stack on (N, C, H, W) -> (y, mag, n_terms)."""
    if step[0] == "conv":
        w = state[f"encoder.{step[1]}.weight"]
        y, mag = conv(x, w, state[f"encoder.{step[1]}.bias"], "relu", dtype=dtype)
        return y, mag, 9 * w.shape[1] + 1
    a = b = None
    if step[3]:
        p = f"encoder.{step[1]}.1."
        a, b = bn_affine(state[p + "weight"], state[p + "bias"], state[p + "running_mean"], state[p + "running_var"], dtype=dtype)
    y, mag = maxpool(torch.as_tensor(x).to(dtype), step[2], a, b)
    return y, mag, 2


def aggregation(x, state, dtype=torch.float64):
    w = state["aggregation_layer.weight"]
    y, mag = conv(x, w, state["aggregation_layer.bias"], "none", padding=(0, 0), dtype=dtype)
    return y, mag, w.shape[1] * w.shape[2] + 1


def encoder_forward(state, images, steps=None, dtype=torch.float64):
    """The whole encoder in `dtype` on CPU: -> (features (N, C, 1, T), [every layer's output, ingestion first])."""
    steps = stack() if steps is None else steps
    x = ingest(images, dtype)
    outs = [x]
    for step in steps:
        x = layer(step, x, state, dtype)[0]
        outs.append(x)
    y = aggregation(x, state, dtype)[0]
    outs.append(y)
    return y, outs


# ---------------------------------------------------------------------------------------------- seeded weights, the label test's input
def seeded_state(shapes, seed):
    """{name: f32 tensor} for {name: shape}: He-scaled convolution weights N(0, 2 / fan_in), biases uniform in +-0.5, BatchNorm weight in
    +-[0.5, 1.5] (some negative), bias and running mean N(0, 0.5^2), running variance in [0.5, 2]."""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for name, shape in shapes.items():
        shape = tuple(int(s) for s in shape)
        if name.endswith("num_batches_tracked"):
            state[name] = torch.tensor(7, dtype=torch.int64)
        elif name.endswith("running_var"):
            state[name] = 0.5 + 1.5 * torch.rand(shape, generator=g)
        elif name.endswith("running_mean"):
            state[name] = 0.5 * torch.randn(shape, generator=g)
        elif len(shape) == 4:
            state[name] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif name.endswith(".1.weight"):
            sign = torch.where(torch.rand(shape, generator=g) < 0.25, -1.0, 1.0)
            state[name] = sign * (0.5 + torch.rand(shape, generator=g))
        elif name.endswith(".1.bias"):
            state[name] = 0.5 * torch.randn(shape, generator=g)
        else:
            state[name] = torch.rand(shape, generator=g) - 0.5
    return state


def encoder_shapes(base_channels, in_channels=3, height=40, num_conv_blocks=3, num_conv_layers=(2, 2, 3), patch_size=(40, 8)):
    """State-dict names and shapes of the reference's VGGEncoder, from its definition."""
    shapes, c = {}, in_channels
    for step in stack(num_conv_blocks, num_conv_layers, patch_size):
        if step[0] == "conv":
            width = base_channels << sum(1 for s in stack(num_conv_blocks, num_conv_layers, patch_size) if s[0] == "pool" and s[1] < step[1])
            shapes[f"encoder.{step[1]}.weight"], shapes[f"encoder.{step[1]}.bias"] = (width, c, 3, 3), (width,)
            c = width
        elif step[3]:
            p = f"encoder.{step[1]}.1."
            shapes.update({p + "weight": (c,), p + "bias": (c,), p + "running_mean": (c,), p + "running_var": (c,), p + "num_batches_tracked": ()})
    h = height // 2 ** num_conv_blocks
    shapes["aggregation_layer.weight"], shapes["aggregation_layer.bias"] = (c, c, h, 1), (c,)
    return shapes


LABEL_SEED = 3
LABEL_BASE_CHANNELS, LABEL_IMAGES = 16, (6, 40, 264, 3)
LABEL_DIM, LABEL_CODES, LABEL_DRAWN = 32, 96, 64
LABEL_MARGIN, LABEL_MAX_EXCLUDED, LABEL_MIN_DISTINCT = 1e-3, 0.05, 16


def smooth_images(shape, seed):
    """uint8 line images with structure (a few strokes over a noisy background), so the features differ from position to position."""
    rng = np.random.default_rng(seed)
    n, h, w, c = shape
    img = rng.integers(150, 256, shape).astype(np.int64)
    for i in range(n):
        for _ in range(w // 6):
            x0, y0 = int(rng.integers(0, w - 3)), int(rng.integers(0, h - 8))
            img[i, y0:y0 + int(rng.integers(4, 20)), x0:x0 + int(rng.integers(1, 4)), :] = rng.integers(0, 90)
    return np.clip(img, 0, 255).astype(np.uint8)


_label_case = {}


def label_case(seed=LABEL_SEED):
    """The label test's input, computed once per process: images, encoder state, projection and codebook, and in f64 the projected
    features, the argmin over the codebook and every row's relative margin (second - best) / |best| of the squared distances."""
    if seed in _label_case:
        return _label_case[seed]
    images = torch.from_numpy(smooth_images(LABEL_IMAGES, seed))
    state = seeded_state(encoder_shapes(LABEL_BASE_CHANNELS), seed)
    g = torch.Generator().manual_seed(seed + 1000)
    c = 4 * LABEL_BASE_CHANNELS
    proj_w = torch.randn((LABEL_DIM, c, 1, 1), generator=g) * (1.0 / c) ** 0.5
    proj_b = torch.rand((LABEL_DIM,), generator=g) - 0.5
    features = encoder_forward(state, images)[0]                                    # (N, C, 1, T) f64
    projected = conv(features, proj_w, proj_b, padding=(0, 0))[0]
    rows = projected.permute(0, 2, 3, 1).reshape(-1, LABEL_DIM)                     # (N T, D) f64
    pick = torch.randperm(rows.shape[0], generator=g)[:LABEL_DRAWN]
    codebook = torch.full((LABEL_CODES, LABEL_DIM), 1.0e3, dtype=torch.float64)
    codebook[:LABEL_DRAWN] = rows[pick] * (1.0 + 0.05 * torch.randn((LABEL_DRAWN, LABEL_DIM), generator=g).double())
    codebook = codebook.float()
    dist = ((rows[:, None, :] - codebook.double()[None, :, :]) ** 2).sum(-1)
    two = torch.topk(dist, 2, dim=1, largest=False)
    margin = (two.values[:, 1] - two.values[:, 0]) / two.values[:, 0].abs()
    case = {"images": images, "state": state, "proj_w": proj_w, "proj_b": proj_b, "codebook": codebook, "features": features,
            "rows": rows, "labels": two.indices[:, 0], "margin": margin}
    _label_case[seed] = case
    return case
