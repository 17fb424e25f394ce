"""VectorQuantizer with the interface of the reference's models/autoencoders.py:170-241 - the tokenizer step that
produces the labels masked pre-training predicts (config 3: codebook 8192 x 512).  Nearest-code search by the fused
exact-f32 HIP kernel (distances and one-hot matrices are never materialised), quantized output with the reference's
straight-through arithmetic and gradient; in training mode with decay > 0 the EMA codebook update
(autoencoders.py:225-237) runs as scatter kernels instead of two one-hot GEMMs.

`VGGEncoder` is the tokenizer's convolution stack (autoencoders.py:6-47) for INFERENCE: line images -> the feature map the quantizer
reads, on the implicit-GEMM 3x3 convolution, ingestion and pooling kernels of csrc/conv.hip; `VQVAETokenizer` puts
it in front of `VQVAEQuantizer`, so images -> labels stays on the device.  The VGG decoder, the reconstruction loss and tokenizer
training are not part of the package."""
import torch

from .. import ops, precision


class VectorQuantizer(torch.nn.Module):
    def __init__(self, num_embeddings, embeddings_dim, commitment_cost, decay, epsilon=1e-5):
        super().__init__()
        self.embeddings_dim = embeddings_dim
        self.num_embeddings = num_embeddings
        self.embedding = torch.nn.Embedding(self.num_embeddings, self.embeddings_dim)
        if decay > 0.0:  # same parameter / buffer set and the same RNG draws as the reference constructor
            self.embedding.weight.data.normal_()
            self.register_buffer("ema_cluster_size", torch.zeros(num_embeddings))
            self.ema_w = torch.nn.Parameter(torch.Tensor(num_embeddings, self.embeddings_dim))
            self.ema_w.data.normal_()
        else:
            self.embedding.weight.data.uniform_(-1 / self.num_embeddings, 1 / self.num_embeddings)
        self.commitment_cost = commitment_cost
        self.decay = decay
        self.epsilon = epsilon

    def calculate_loss(self, tokens, features):
        q_latent_loss = 0 if self.decay > 0.0 else torch.nn.functional.mse_loss(tokens, features.detach())
        e_latent_loss = torch.nn.functional.mse_loss(tokens.detach(), features)
        return q_latent_loss + self.commitment_cost * e_latent_loss

    @torch.no_grad()
    def nearest(self, flat_input):
        """(M, D) float32 rows -> int64 indices of the nearest code (first minimum), bit-exact f32 arithmetic."""
        if not flat_input.is_cuda:
            raise RuntimeError("pero_pretraining_amd VectorQuantizer runs on the GPU only (HIP kernel, no CPU fallback)")
        return ops.vq_argmin(flat_input.float().contiguous(), self.embedding.weight.detach().float().contiguous())

    def forward(self, inputs):
        """inputs (N, D, 1, T) -> (quantized (N, D, 1, T), indices (N*T,)) like autoencoders.py:204-241.
        The gradient of `quantized` flows straight through to `inputs` (autoencoders.py:239).  Training mode with
        decay > 0 updates ema_cluster_size / ema_w / embedding.weight IN PLACE after quantizing with the old codebook
        (the reference re-creates the two nn.Parameters every step, which detaches them from any optimizer and from
        DDP - not reproduced; values are the same)."""
        x = inputs.permute(0, 2, 3, 1).contiguous()
        flat = x.reshape(-1, self.embeddings_dim).float()
        q, idx = _QuantizeFn.apply(flat, self)
        return q.view(x.shape).permute(0, 3, 1, 2).contiguous(), idx


class _QuantizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, vq):
        flat = flat.detach().contiguous()
        weight = vq.embedding.weight.detach()
        idx = vq.nearest(flat)
        q = ops.vq_gather(flat, weight.float().contiguous(), idx)
        if vq.training and vq.decay > 0.0:
            ops.vq_ema_update(flat, idx, vq.ema_cluster_size, vq.ema_w.data, vq.embedding.weight.data, vq.decay, vq.epsilon)
        ctx.mark_non_differentiable(idx)
        return q, idx

    @staticmethod
    def backward(ctx, dq, _didx):
        return dq, None


class _Project1x1Fn(torch.autograd.Function):
    """Conv2d(C_in -> C_out, kernel 1) on (N, C_in, 1, T) features as ONE exact-f32 pero_gemm over the token rows (N*T, C_in): the
    quantizer behind it decides by f32 distances, so the projection keeps f32 operands whatever the autocast mode."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        n, c, h, t = x.shape
        rows = x.detach().permute(0, 2, 3, 1).reshape(-1, c).float().contiguous()
        w2 = weight.detach().reshape(weight.shape[0], c).float().contiguous()
        y = ops.gemm(rows, w2, bias=None if bias is None else bias.detach().float().contiguous())
        ctx.save_for_backward(rows, w2)
        ctx.shape, ctx.has_bias = x.shape, bias is not None
        return y.view(n, h, t, -1).permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(ctx, dy):
        rows, w2 = ctx.saved_tensors
        n, c, h, t = ctx.shape
        d2 = dy.permute(0, 2, 3, 1).reshape(-1, dy.shape[1]).float().contiguous()
        dx = ops.gemm(d2, w2, trans_b=True).view(n, h, t, c).permute(0, 3, 1, 2).contiguous()
        dw = ops.gemm(d2, rows, trans_a=True, trans_b=True).view(w2.shape[0], c, 1, 1)
        db = d2.sum(0) if ctx.has_bias else None
        return dx, dw, db


class VQVAEQuantizer(torch.nn.Module):
    """The quantizing middle of the reference's VQVAE (models/autoencoders.py:107-146): `encoder_projection_layer` (1x1 conv,
    encoder channels -> embeddings_dim), `vq`, `decoder_projection_layer` (1x1 conv, embeddings_dim -> decoder channels), with the
    reference's parameter names - a VQVAE checkpoint's `encoder_projection_layer.*`, `vq.*`, `decoder_projection_layer.*` entries
    load with `load_state_dict(..., strict=False)` on the full file or strictly on the filtered one.  `quantize(x)` is the
    reference's method: encoder features (N, C_enc, 1, T) -> (projected tokens (N, C_dec, 1, T), labels (N*T,)); the labels are
    what masked pre-training predicts (scripts/produce_vqvae_labels.py:27-46).  The VGG encoder / decoder around it are outside the
    hot path."""

    def __init__(self, encoder_channels, decoder_channels, num_embeddings, embeddings_dim, commitment_cost=0.25, decay=0.99):
        super().__init__()
        self.encoder_projection_layer = torch.nn.Conv2d(encoder_channels, embeddings_dim, 1)     # parameter containers (same init / keys)
        self.decoder_projection_layer = torch.nn.Conv2d(embeddings_dim, decoder_channels, 1)
        self.num_embeddings = num_embeddings
        self.embeddings_dim = embeddings_dim
        self.vq = VectorQuantizer(num_embeddings, embeddings_dim, commitment_cost, decay)

    def quantize(self, x):
        if not x.is_cuda:
            raise RuntimeError("pero_pretraining_amd VQVAEQuantizer runs on the GPU only (HIP kernels, no CPU fallback)")
        x = _Project1x1Fn.apply(x, self.encoder_projection_layer.weight, self.encoder_projection_layer.bias)
        tokens, labels = self.vq(x)
        projected_tokens = _Project1x1Fn.apply(tokens, self.decoder_projection_layer.weight, self.decoder_projection_layer.bias)
        return projected_tokens, labels

    def labels(self, x):
        """Labels only (the label-production path: no decoder projection)."""
        with torch.no_grad():
            x = _Project1x1Fn.apply(x, self.encoder_projection_layer.weight, self.encoder_projection_layer.bias)
            return self.vq(x)[1]


def kmeans_labels(features, centroids):
    """Feature-Quantization labels (scripts/produce_kmeans_labels.py:72-79): features (N, F, T), centroids (K, F)
    -> (N, T) int64 assignments.  argmin of the true L2 distance == argmin of the squared expanded form used by the
    kernel (up to exact ties)."""
    n, f, t = features.shape
    flat = features.permute(0, 2, 1).reshape(-1, f).float().contiguous()
    return ops.vq_argmin(flat, centroids.float().contiguous()).view(n, t)


def _vgg_layers(in_channels, base_channels, num_conv_blocks, num_conv_layers, patch_size, dropout):
    """The containers of models/helpers.py:4-56, nested the same way (so the state-dict keys are the reference's): per block its
    Conv2d(3x3) + ReLU pairs, then Sequential(MaxPool2d, [BatchNorm2d in the last block], Dropout).  A block halves a direction
    while the subsampling reached so far is below the patch size in that direction."""
    layers, reached, channels = [], [1, 1], in_channels
    for block in range(num_conv_blocks):
        width = base_channels << block
        pool = [1, 1]
        for axis in (0, 1):
            if reached[axis] < patch_size[axis]:
                pool[axis] = 2
                reached[axis] *= 2
        for _ in range(num_conv_layers[block]):
            layers += [torch.nn.Conv2d(channels, width, kernel_size=3, stride=1, padding=1), torch.nn.ReLU()]
            channels = width
        tail = [torch.nn.MaxPool2d(kernel_size=pool, stride=pool)]
        if block == num_conv_blocks - 1:
            tail.append(torch.nn.BatchNorm2d(width))
        tail.append(torch.nn.Dropout(dropout))
        layers.append(torch.nn.Sequential(*tail))
    return torch.nn.Sequential(*layers)


class VGGEncoder(torch.nn.Module):
    """The reference's VGGEncoder (models/autoencoders.py:6-47) for inference on the HIP kernels: same constructor, attributes and
    parameter containers, so `load_state_dict(strict=True)` takes a reference checkpoint's encoder (`encoder.0.weight` ...
    `encoder.16.1.running_var`, `aggregation_layer.*` at the defaults).

    forward(images): device uint8 (N, H, W, C) as BatchCreator delivers it (divided by 255 here, autoencoders/batch_operator.py:14) or
    float32 (N, C, H, W) as that batch operator builds it -> (N, out_channels, 1, W / subsampling) f32.  Runs in
    `precision.compute_dtype()`: exact f32 by default, bf16 storage and MFMA under `precision.autocast`.  Activations live in the
    halo layout of include/pero_hip.h; the last pool writes token rows and the (h, 1) aggregation convolution is one pero_gemm.  The
    batch is processed in chunks of lines so that the largest input + output pair of a layer stays under `max_workspace_bytes`; the
    result does not depend on the chunk size.

    Limits: inference only - BatchNorm always uses its running statistics, dropout is the identity, and a call with gradients enabled
    and a parameter that requires one raises (no backward pass exists).  H must equal `height`, and H and W must be divisible by the
    stack's total subsampling (the reference floors; the collator's widths are multiples of 32).  `pretrained_vgg_layers > 0` would
    download torchvision weights and is refused: load a checkpoint instead."""

    def __init__(self, height=40, patch_size=(40, 8), in_channels=3, dropout=0.0, base_channels=64, num_conv_blocks=3,
                 num_conv_layers=(2, 2, 3), pretrained_vgg_layers=0, aggregation="conv"):
        super().__init__()
        if pretrained_vgg_layers > 0:
            raise ValueError(f"VGGEncoder: pretrained_vgg_layers = {pretrained_vgg_layers} would download torchvision's VGG-16 weights; "
                             "construct with pretrained_vgg_layers=0 and load a checkpoint (load_state_dict) instead")
        if len(num_conv_layers) < num_conv_blocks:
            raise ValueError(f"VGGEncoder: num_conv_layers {tuple(num_conv_layers)} has fewer entries than num_conv_blocks = {num_conv_blocks}")
        self.height = height
        self.aggregation = aggregation
        self.in_channels = in_channels
        self.base_channels = base_channels
        self.num_conv_blocks = num_conv_blocks
        self.num_conv_layers = num_conv_layers
        self.patch_size = patch_size
        self.dropout = dropout
        self.pretrained_vgg_layers = pretrained_vgg_layers
        self.encoder = _vgg_layers(in_channels, base_channels, num_conv_blocks, num_conv_layers, patch_size, dropout)
        aggregation_height = height // 2 ** num_conv_blocks
        self.out_channels = base_channels * 2 ** (num_conv_blocks - 1)
        if aggregation != "conv":
            raise NotImplementedError()
        self.aggregation_layer = torch.nn.Conv2d(self.out_channels, self.out_channels, kernel_size=(aggregation_height, 1), stride=1, padding=0)
        self.max_workspace_bytes = 2 << 30
        self._packed = {}    # (step, dtype) -> (key of the parameter, kernel-layout copy): repacked once per checkpoint load

    def steps(self):
        """The stack as the kernels run it: ("conv", index, Conv2d, activation) and ("pool", index, (ph, pw), BatchNorm2d or None)."""
        out, mods = [], list(self.encoder)
        for i, m in enumerate(mods):
            if isinstance(m, torch.nn.Conv2d):
                out.append(("conv", i, m, "relu" if i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU) else "none"))
            elif isinstance(m, torch.nn.Sequential):
                pool = next(c for c in m if isinstance(c, torch.nn.MaxPool2d))
                k = pool.kernel_size if isinstance(pool.kernel_size, (tuple, list)) else (pool.kernel_size, pool.kernel_size)
                out.append(("pool", i, (int(k[0]), int(k[1])), next((c for c in m if isinstance(c, torch.nn.BatchNorm2d)), None)))
        return out

    def subsampling(self):
        sh = sw = 1
        for step in self.steps():
            if step[0] == "pool":
                sh, sw = sh * step[2][0], sw * step[2][1]
        return sh, sw

    def _cached(self, name, params, dtype, make):
        key = tuple((p._version, p.data_ptr(), tuple(p.shape)) for p in params)
        ent = self._packed.get((name, dtype))
        if ent is None or ent[0] != key:
            ent = self._packed[(name, dtype)] = (key, make())
        return ent[1]

    def _conv_operands(self, index, conv, dtype):
        """Kernel-layout weight (the first layer's input channels padded with zeros like the ingested image) and f32 bias."""
        cin = ops.conv_channel_pad(conv.in_channels, dtype) if index == 0 else conv.in_channels
        w = self._cached(("w", index), (conv.weight,), dtype, lambda: ops.conv3x3_pack_weight(conv.weight, dtype, cin_pad=cin))
        b = None if conv.bias is None else self._cached(("b", index), (conv.bias,), torch.float32, lambda: conv.bias.detach().float().contiguous())
        return w, b

    def _bn_affine(self, index, bn):
        """Eval-mode BatchNorm2d as y = x a + b: a = weight / sqrt(running_var + eps), b = bias - running_mean a, formed in f64, stored f32."""
        def make():
            rstd = 1.0 / torch.sqrt(bn.running_var.detach().double() + bn.eps)
            a = rstd if bn.weight is None else bn.weight.detach().double() * rstd
            b = -bn.running_mean.detach().double() * a
            if bn.bias is not None:
                b = b + bn.bias.detach().double()
            return a.float().contiguous(), b.float().contiguous()
        params = tuple(p for p in (bn.weight, bn.bias, bn.running_mean, bn.running_var) if p is not None)
        return self._cached(("bn", index), params, torch.float32, make)

    def _aggregation_operands(self, dtype):
        agg = self.aggregation_layer
        w = self._cached(("agg_w",), (agg.weight,), dtype,
                         lambda: agg.weight.detach().permute(0, 2, 3, 1).reshape(agg.weight.shape[0], -1).to(dtype).contiguous())
        b = None if agg.bias is None else self._cached(("agg_b",), (agg.bias,), torch.float32, lambda: agg.bias.detach().float().contiguous())
        return w, b

    def _geometry(self, images):
        if images.dim() != 4 or images.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"VGGEncoder: images must be uint8 (N, H, W, C) or float32 (N, C, H, W), got {tuple(images.shape)} {images.dtype}")
        n, h, w, c = images.shape if images.dtype == torch.uint8 else (images.shape[0], images.shape[2], images.shape[3], images.shape[1])
        sh, sw = self.subsampling()
        if c != self.in_channels or h != self.height:
            raise ValueError(f"VGGEncoder: images of height {h} with {c} channels, built for height {self.height} with {self.in_channels} channels")
        if h % sh or w % sw or h // sh != self.aggregation_layer.kernel_size[0]:
            raise ValueError(f"VGGEncoder: H = {h}, W = {w} must be divisible by the stack's subsampling {(sh, sw)} and H / {sh} must be the "
                             f"aggregation height {self.aggregation_layer.kernel_size[0]}")
        return n, h, w, c

    def lines_per_chunk(self, h, w, dtype):
        """Lines whose largest (input, output) activation pair of one layer fits into max_workspace_bytes (at least 1)."""
        esz, pair, c = torch.empty((), dtype=dtype).element_size(), 0, ops.conv_channel_pad(self.in_channels, dtype)
        for step in self.steps():
            before = (h + 2) * (w + 2) * c
            if step[0] == "conv":
                c = step[2].out_channels
            else:
                h, w = h // step[2][0], w // step[2][1]
            pair = max(pair, (before + (h + 2) * (w + 2) * c) * esz)
        return max(1, int(self.max_workspace_bytes) // pair)

    def forward(self, images, trace=None):
        """`trace`: a list that receives (kind, index, output) of every layer - halo-layout activations, the token rows of the last pool,
        ("aggregation", None, rows) - for tests; the batch then runs as one chunk."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("pero_pretraining_amd VGGEncoder is inference only (no backward pass): call it under torch.no_grad()")
        if not images.is_cuda:
            raise RuntimeError("pero_pretraining_amd VGGEncoder runs on the GPU only (HIP kernels, no CPU fallback)")
        n, h, w, _ = self._geometry(images)
        dtype = precision.compute_dtype()
        with torch.no_grad():
            steps = self.steps()
            sh, sw = self.subsampling()
            t, k = w // sw, (h // sh) * self.out_channels
            tokens = torch.empty((n * t, k), device=images.device, dtype=dtype)
            images = images.contiguous()
            chunk = n if trace is not None else self.lines_per_chunk(h, w, dtype)
            for n0 in range(0, n, chunk):
                n1 = min(n, n0 + chunk)
                x = ops.image_to_halo(images[n0:n1], dtype, channels=ops.conv_channel_pad(self.in_channels, dtype))
                if trace is not None:
                    trace.append(("ingest", None, x))
                for pos, step in enumerate(steps):
                    if step[0] == "conv":
                        wk, bk = self._conv_operands(step[1], step[2], dtype)
                        x = ops.conv3x3(x, wk, bk, activation=step[3])
                    else:
                        a, b = (None, None) if step[3] is None else self._bn_affine(step[1], step[3])
                        last = pos == len(steps) - 1
                        x = ops.maxpool_nhwc(x, step[2], a, b, token_rows=last, out=tokens[n0 * t:n1 * t] if last else None)
                    if trace is not None:
                        trace.append((step[0], step[1], x))
            wk, bk = self._aggregation_operands(dtype)
            rows = ops.gemm(tokens, wk, bias=bk, out_dtype=torch.float32)
            if trace is not None:
                trace.append(("aggregation", None, rows))
            return rows.view(n, t, self.out_channels).permute(0, 2, 1).unsqueeze(2).contiguous()


class VQVAETokenizer(VQVAEQuantizer):
    """The label-producing half of the reference's VQVAE (models/autoencoders.py:107-146): `encoder` (a VGGEncoder) in front of the
    quantizing middle, under the reference's parameter names.  `encode(images)` -> features (N, C_enc, 1, T), `quantize(features)` ->
    (projected tokens, labels), `labels(images)` -> (N * T,) int64 labels of the line images.  The 1x1 projection keeps f32 operands
    whatever the compute dtype of the encoder.  `load(path)` takes a reference VQVAE checkpoint strictly except for its `decoder.*`
    entries (the decoder is not part of the package)."""

    def __init__(self, encoder, num_embeddings, embeddings_dim, decoder_channels=256, commitment_cost=0.25, decay=0.99):
        super().__init__(encoder.out_channels, decoder_channels, num_embeddings, embeddings_dim, commitment_cost, decay)
        self.encoder = encoder

    def encode(self, images):
        return self.encoder(images)

    def forward(self, features):
        """= quantize(features): what `scripts.labels.compute_labels(tokenizer.encode, tokenizer, dataset)` calls per batch."""
        return self.quantize(features)

    def labels(self, images):
        with torch.no_grad():
            return super().labels(self.encode(images))

    def load(self, path_or_state):
        state = torch.load(path_or_state, map_location="cpu") if isinstance(path_or_state, (str, bytes)) or hasattr(path_or_state, "__fspath__") \
            else path_or_state
        self.load_state_dict({k: v for k, v in state.items() if not k.startswith("decoder.")}, strict=True)
        return self
