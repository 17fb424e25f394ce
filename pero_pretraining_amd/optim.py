"""Fused Adam over one flat parameter buffer (replaces the ~150 per-tensor kernels of torch.optim.Adam,
masked_pretraining/train.py:146, by ONE HIP launch per step that also refreshes the bf16 weight copies).

Drop-in: same constructor arguments and param_groups protocol as torch.optim.Adam (the reference's
WarmupSchleduler writes param_group["lr"]); parameters keep their identity, names and shapes - only their
storage is moved into the flat buffer, so state_dict()/load_state_dict() of the model are unaffected.

Every hyper-parameter is read per parameter group at each step, as torch does: lr, betas, eps, weight_decay (coupled as in
torch.optim.Adam, or decoupled as in torch.optim.AdamW with decoupled_weight_decay=True), amsgrad, maximize.  FusedAdamW mirrors
torch.optim.AdamW; decay_groups(model, weight_decay) builds the usual decay / no-decay pair of groups.

max_grad_norm clips by the global L2 norm over ALL groups inside the Adam launches: one sum-of-squares launch per group, one
finishing launch, and the Adam kernels read the norm from the device.  `optimizer.grad_norm` is that device tensor (one f32): the norm
before clipping, the value torch.nn.utils.clip_grad_norm_ returns, with grad_scale applied - under parallel.DataParallel the norm of
the averaged gradient, identical on every rank.  Nothing reads it on the host.  Unlike clip_grad_norm_, `.grad` itself is left
unscaled: the coefficient is applied to the gradient on its way into the moments, so a `.grad` read after step() still holds the raw sum.

FusedLAMB and FusedLARS subclass FusedAdam (the flat buffers, the bf16 and transposed copies, flat_grads / param_offsets / grad_scale /
grad_norm / refresh_lowp and the clip are its own) and replace the step's launch by three per group: the update u and the tile sums of
p^2 and u^2, the trust ratio r = c |p| / |u| of every parameter tensor, and the step with r (csrc/optim_layerwise.hip; formulas in
include/pero_hip.h).  layerwise_groups(model, weight_decay) builds their usual pair of groups.

WeightEMA keeps an exponential moving average of a module's parameters in a deep copy of it: one flat f32 buffer with FusedAdam's
layout, one launch per update however many tensors the module has (pero_ema_update, csrc/latent.hip), the bf16 copy written in the same
launch.  It is the teacher of latent_pretraining and the weight averaging a recogniser is usually evaluated with.
"""
import copy

import torch

from . import lowp, ops


def _flat_storage(ps, dev):
    """The parameters `ps` moved into ONE flat f32 buffer on `dev`, every tensor at an offset rounded up to 8 elements (16-byte aligned bf16
    views), and its bf16 copy registered view by view with lowp.put.  Both buffers are zero-filled (the library's linear fill: torch's
    elementwise one runs at a third of its rate), so the pads between the tensors are zeros.  Returns (offsets, total, f32, bf16)."""
    offs, total = [], 0
    for p in ps:
        offs.append(total)
        total += ((p.numel() + 7) // 8) * 8
    fp = ops.zeros((total,), dev, torch.float32)
    flp = ops.zeros((total,), dev, torch.bfloat16)
    for p, o in zip(ps, offs):
        fp[o:o + p.numel()].copy_(p.detach().reshape(-1))
        p.data = fp[o:o + p.numel()].view(p.shape)
    ops.cast_to_bf16(fp, flp)
    for p, o in zip(ps, offs):
        lowp.put(p, flp[o:o + p.numel()].view(p.shape))
    return offs, total, fp, flp


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, *,
                 decoupled_weight_decay=False, max_grad_norm=None):
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError(f"FusedAdam: invalid lr / betas / eps / weight_decay: {lr}, {betas}, {eps}, {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm >= 0:
            raise ValueError(f"FusedAdam: invalid max_grad_norm: {max_grad_norm}")
        # the remaining keys are torch.optim.Adam's group defaults, carried so that state_dict()s are interchangeable; max_grad_norm is
        # this class's own (torch keeps an unknown group key and ignores it)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                                      foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=decoupled_weight_decay, max_grad_norm=max_grad_norm))
        self._setup()

    def _setup(self):
        self._flat = []  # per group: dict(p, g, m, v, vmax, lp, step)
        self.grad_scale = 1.0
        self.grad_norm = None   # one f32 on the device: the global gradient norm of the last clipped step, before clipping
        self._partials = None   # workspace of the norm: the partial sums of every group, one group behind the other
        self._flatten()

    @staticmethod
    def _moments(total, dev, group):
        """The state buffers of one group beside p and g.  A subclass with other state allocates its own here and names it in _STATE:
        FusedLARS keeps v = None, which its map never reads, and never has amsgrad (_vmax)."""
        return dict(m=ops.zeros((total,), dev, torch.float32), v=ops.zeros((total,), dev, torch.float32),
                    vmax=ops.zeros((total,), dev, torch.float32) if group["amsgrad"] else None)

    def _flatten(self):
        self._flat = []
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.requires_grad]
            if not ps:
                self._flat.append(None)
                continue
            dev = ps[0].device
            if dev.type != "cuda":
                raise RuntimeError("FusedAdam needs the parameters on the GPU (move the model first)")
            offs, total, fp, flp = _flat_storage(ps, dev)
            fg = ops.zeros((total,), dev, torch.float32)
            for p, o in zip(ps, offs):
                n = p.numel()
                if p.grad is not None:
                    fg[o:o + n].copy_(p.grad.reshape(-1))
                p.grad = fg[o:o + n].view(p.shape)
            # transposed bf16 copies of the matrices (lowp.weight_t: the input-gradient products read them), same offsets
            mats = [(o, o, p.shape[0], p.numel() // p.shape[0]) for p, o in zip(ps, offs) if p.dim() >= 2]
            flpt, ttable, ttiles = None, None, 0
            if mats:
                flpt = ops.zeros((total,), dev, torch.bfloat16)
                ttable, ttiles = ops.transpose_table(mats, dev)
                ops.transpose_multi(flp, flpt, ttable, ttiles)
                for p, o in zip(ps, offs):
                    if p.dim() >= 2:
                        lowp.put_t(p, flpt[o:o + p.numel()].view(p.numel() // p.shape[0], p.shape[0]))
            self._flat.append(dict(p=fp, g=fg, **self._moments(total, dev, group), lp=flp, step=0,
                                   params=ps, offsets=offs, lpt=flpt, ttable=ttable, ttiles=ttiles))

    def refresh_lowp(self):
        """Re-cast the bf16 copies after the flat parameters were written from outside (broadcast, load)."""
        for f in self._flat:
            if f is not None:
                ops.cast_to_bf16(f["p"], f["lp"])
                self._transpose(f)

    @staticmethod
    def _transpose(f):
        if f["lpt"] is not None:
            ops.transpose_multi(f["lp"], f["lpt"], f["ttable"], f["ttiles"])

    # flat views for data-parallel gradient reduction
    def flat_grads(self):
        """{parameter-group index: flat f32 gradient buffer} (groups without parameters have none)"""
        return {gi: f["g"] for gi, f in enumerate(self._flat) if f is not None}

    def param_offsets(self):
        """{id(param): (group index, start, numel)} inside the flat buffers."""
        out = {}
        for gi, f in enumerate(self._flat):
            if f is not None:
                for p, o in zip(f["params"], f["offsets"]):
                    out[id(p)] = (gi, o, p.numel())
        return out

    def zero_grad(self, set_to_none=False):
        for f in self._flat:
            if f is None:
                continue
            f["g"].zero_()
            for p, o in zip(f["params"], f["offsets"]):
                if p.grad is None or p.grad.data_ptr() != f["g"].data_ptr() + 4 * o:
                    p.grad = f["g"][o:o + p.numel()].view(p.shape)

    # ---- checkpointing: the layout of torch.optim.Adam's state_dict (per-parameter 'step', 'exp_avg', 'exp_avg_sq' and, in an amsgrad
    # group, 'max_exp_avg_sq'; the group keys carry the real hyper-parameters), so optimizer state moves between this class and
    # torch.optim.Adam / AdamW (the reference's optimizer, masked_pretraining/train.py:146) in both directions.  The reference itself
    # never saves it.
    # state-dict key -> flat-buffer key (a subclass with other state replaces the maps); _STATE_STEP: the entries carry a 'step'
    _STATE = {"exp_avg": "m", "exp_avg_sq": "v"}
    _STATE_AMSGRAD = {"max_exp_avg_sq": "vmax"}
    _STATE_STEP = True

    def _state_keys(self, group, f):
        if not group.get("amsgrad"):
            return self._STATE
        self._vmax(f)
        return {**self._STATE, **self._STATE_AMSGRAD}

    def state_dict(self):
        state, groups, idx = {}, [], 0
        for group, f in zip(self.param_groups, self._flat):
            offs = {id(p): o for p, o in zip(f["params"], f["offsets"])} if f is not None else {}
            ids = []
            for p in group["params"]:
                if id(p) in offs and f["step"] > 0:
                    o, n = offs[id(p)], p.numel()
                    state[idx] = {"step": torch.tensor(float(f["step"]))} if self._STATE_STEP else {}
                    for key, buf in self._state_keys(group, f).items():
                        state[idx][key] = f[buf][o:o + n].view(p.shape).clone()
                ids.append(idx)
                idx += 1
            g = {k: v for k, v in group.items() if k != "params"}
            g["params"] = ids
            groups.append(g)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        for group, saved, f in zip(self.param_groups, groups, self._flat):
            if len(saved["params"]) != len(group["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
            for k, v in saved.items():
                if k != "params":
                    group[k] = v
            if f is None:
                continue
            offs = {id(p): o for p, o in zip(f["params"], f["offsets"])}
            if not group.get("amsgrad"):
                f["vmax"] = None
            keys = self._state_keys(group, f)
            for buf in keys.values():
                f[buf].zero_()
            steps, loaded = set(), False
            for p, idx in zip(group["params"], saved["params"]):
                st = state_dict["state"].get(idx)
                if st is None or id(p) not in offs:
                    continue
                o, n = offs[id(p)], p.numel()
                for key, buf in keys.items():
                    if key in self._STATE_AMSGRAD:   # a state saved without amsgrad starts its running maximum at v, where the next step's max() puts it anyway
                        val = st.get(key, st["exp_avg_sq"])
                    else:                            # torch.optim.Adam's entries are complete; SGD's may be empty, or hold None before the first step
                        val = st[key] if self._STATE_STEP else st.get(key)
                    if val is not None:
                        f[buf][o:o + n].copy_(val.reshape(-1))
                        loaded = True
                if self._STATE_STEP:
                    steps.add(int(float(st["step"])))
            f["step"] = self._step_after_load(steps, loaded)

    @staticmethod
    def _step_after_load(steps, loaded):
        if len(steps) > 1:
            raise ValueError(f"FusedAdam keeps one step counter per group, got {sorted(steps)}")
        return steps.pop() if steps else 0

    @staticmethod
    def _vmax(f):
        """The amsgrad running maximum of a group's flat buffers, made on first use (a group may turn amsgrad on after construction)."""
        if f["vmax"] is None:
            f["vmax"] = ops.zeros((f["v"].numel(),), f["v"].device, torch.float32)
        return f["vmax"]

    def _global_norm(self):
        """grad_norm <- grad_scale * ||all flat gradient buffers||_2: one partial-sums launch per group, one finishing launch, no host read."""
        flats = [f for f in self._flat if f is not None]
        devices = {f["g"].device for f in flats}
        if len(devices) > 1:
            raise RuntimeError(f"FusedAdam: max_grad_norm needs every parameter group on one device, got {sorted(map(str, devices))}")
        counts = [ops.sumsq_num_partials(f["g"].numel()) for f in flats]
        dev = flats[0]["g"].device
        if self._partials is None or self._partials.numel() != sum(counts) or self._partials.device != dev:
            self._partials = torch.empty(sum(counts), device=dev, dtype=torch.float32)
        if self.grad_norm is None or self.grad_norm.device != dev:
            self.grad_norm = torch.zeros(1, device=dev, dtype=torch.float32)
        start = 0
        for f, c in zip(flats, counts):
            ops.sumsq_partials(f["g"], self._partials[start:start + c])
            start += c
        ops.grad_norm_finish(self._partials, self.grad_scale, self.grad_norm)

    def _link_grads(self):
        """Every gradient into its flat buffer; True if any group clips."""
        clipped = False
        for group, f in zip(self.param_groups, self._flat):
            if f is None:
                continue
            # a gradient that no longer aliases the flat buffer (model.zero_grad(set_to_none=True) or `p.grad = ...` made the
            # backward write a fresh tensor) is copied in and relinked: stepping on the stale flat slice would be silent
            for p, o in zip(f["params"], f["offsets"]):
                if p.grad is not None and p.grad.data_ptr() != f["g"].data_ptr() + 4 * o:
                    if self.grad_scale != 1.0:
                        # a data-parallel driver reduced the FLAT buffer during the backward: this detached gradient is this rank's
                        # alone - copying it in would step every rank on its own gradient, scaled by 1 / world, silently diverging
                        raise RuntimeError("FusedAdam: a parameter's .grad no longer aliases the flat gradient buffer although a data-parallel "
                                           "driver is attached (grad_scale != 1): use optimizer.zero_grad() (it keeps the views), not "
                                           "model.zero_grad(set_to_none=True) / `p.grad = ...`")
                    f["g"][o:o + p.numel()].copy_(p.grad.reshape(-1))
                    p.grad = f["g"][o:o + p.numel()].view(p.shape)
            clipped = clipped or group.get("max_grad_norm") is not None
        return clipped

    def _step_group(self, group, f):
        """The launches of one group's step (f["step"] is already this step's number)."""
        b1, b2 = group["betas"]
        max_norm = group.get("max_grad_norm")
        ops.adam_step_ex(f["p"], f["g"], f["m"], f["v"], f["lp"], group["lr"], b1, b2, group["eps"], f["step"], self.grad_scale,
                         weight_decay=group["weight_decay"], decoupled=group.get("decoupled_weight_decay", False),
                         vmax=self._vmax(f) if group["amsgrad"] else None, maximize=group["maximize"],
                         grad_norm=self.grad_norm if max_norm is not None else None, max_norm=max_norm or 0.0)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self._link_grads():   # over ALL groups, whichever of them clip, and after every gradient is in its flat buffer
            self._global_norm()
        for group, f in zip(self.param_groups, self._flat):
            if f is None:
                continue
            f["step"] += 1
            self._step_group(group, f)
            self._transpose(f)
        return loss


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW's defaults on the same kernels: weight_decay=1e-2, decoupled (p *= 1 - lr * weight_decay before the update)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False, *,
                 decoupled_weight_decay=True, max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         decoupled_weight_decay=decoupled_weight_decay, max_grad_norm=max_grad_norm)


class _LayerWise(FusedAdam):
    """What FusedLAMB and FusedLARS share: the tile table of every group's tensors, the workspace of the tile sums, and `layer_stats`."""

    def _flatten(self):
        super()._flatten()
        for f in self._flat:
            if f is not None:
                dev = f["p"].device
                f["ltable"], f["ltiles"] = ops.layer_table([(o, p.numel()) for p, o in zip(f["params"], f["offsets"])], dev)
                f["lpartials"] = torch.empty(2 * f["ltiles"], device=dev, dtype=torch.float32)
                f["stats"] = ops.zeros((len(f["params"]), 3), dev, torch.float32)

    @property
    def layer_stats(self):
        """One entry per group (None for a group without parameters): the device tensor [n_tensors][3] = (|p| before the step, |u|, trust
        ratio r) of the last step, in the order of the group's parameters.  step() never reads it on the host."""
        return [f["stats"] if f is not None else None for f in self._flat]

    @staticmethod
    def _check(name, lr, weight_decay, max_grad_norm):
        if lr < 0 or weight_decay < 0:
            raise ValueError(f"{name}: invalid lr / weight_decay: {lr}, {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm >= 0:
            raise ValueError(f"{name}: invalid max_grad_norm: {max_grad_norm}")


class FusedLAMB(_LayerWise):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning", 2020) on FusedAdam's flat buffers: Adam's moments, the update
    u = mhat / (sqrt(vhat) + eps) + weight_decay * p, and p -= lr * r * u with the trust ratio r = |p| / |u| of each parameter TENSOR
    (1 where a norm is 0, or in a group with layer_adaptation=False).  Three launches per group and step (csrc/optim_layerwise.hip); the
    state dict has torch.optim.Adam's layout.  No amsgrad, no clamp on r."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, maximize=False, *, layer_adaptation=True,
                 max_grad_norm=None, amsgrad=False):
        if amsgrad:
            raise ValueError("FusedLAMB: amsgrad is not supported")
        self._check("FusedLAMB", lr, weight_decay, max_grad_norm)
        if eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError(f"FusedLAMB: invalid betas / eps: {betas}, {eps}")
        torch.optim.Optimizer.__init__(self, params, dict(
            lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize, foreach=None, capturable=False,
            differentiable=False, fused=None, decoupled_weight_decay=False, layer_adaptation=layer_adaptation, max_grad_norm=max_grad_norm))
        self._setup()

    def _step_group(self, group, f):
        if group["amsgrad"]:
            raise ValueError("FusedLAMB: amsgrad is not supported")
        b1, b2 = group["betas"]
        max_norm = group.get("max_grad_norm")
        ops.lamb_stage1(f["p"], f["g"], f["m"], f["v"], f["ltable"], f["ltiles"], f["lpartials"], b1, b2, f["step"], group["eps"],
                        self.grad_scale, group["weight_decay"], group["maximize"], self.grad_norm if max_norm is not None else None,
                        max_norm or 0.0)
        ops.layer_ratio_finish(f["lpartials"], f["ltable"], f["ltiles"], 1.0, group.get("layer_adaptation", True), f["stats"])
        ops.lamb_stage2(f["p"], f["m"], f["v"], f["lp"], f["ltable"], f["ltiles"], f["stats"], group["lr"], b1, b2, f["step"], group["eps"],
                        group["weight_decay"])


class FusedLARS(_LayerWise):
    """LARS (You et al., "Large Batch Training of Convolutional Networks", 2017) on FusedAdam's flat buffers: u = g + weight_decay * p,
    buf = momentum * buf + r * u, p -= lr * buf with r = trust_coefficient * |p| / |u| per parameter TENSOR (1 where a norm is 0, or in a
    group with layer_adaptation=False: torch.optim.SGD).  One state buffer (no second moment); the state dict has torch.optim.SGD's
    layout.  No Nesterov momentum, no dampening."""

    def __init__(self, params, lr, momentum=0.9, weight_decay=0, trust_coefficient=1e-3, maximize=False, *, layer_adaptation=True,
                 max_grad_norm=None):
        self._check("FusedLARS", lr, weight_decay, max_grad_norm)
        if momentum < 0 or trust_coefficient < 0:
            raise ValueError(f"FusedLARS: invalid momentum / trust_coefficient: {momentum}, {trust_coefficient}")
        torch.optim.Optimizer.__init__(self, params, dict(
            lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=maximize, foreach=None,
            differentiable=False, fused=None, trust_coefficient=trust_coefficient, layer_adaptation=layer_adaptation,
            max_grad_norm=max_grad_norm))
        self._setup()

    @staticmethod
    def _moments(total, dev, group):
        return dict(m=ops.zeros((total,), dev, torch.float32), v=None, vmax=None)   # m: the momentum buffer

    def _step_group(self, group, f):
        if group.get("nesterov") or group.get("dampening"):
            raise ValueError("FusedLARS: nesterov / dampening are not supported")
        max_norm = group.get("max_grad_norm")
        clip = dict(grad_scale=self.grad_scale, weight_decay=group["weight_decay"], maximize=group["maximize"],
                    grad_norm=self.grad_norm if max_norm is not None else None, max_norm=max_norm or 0.0)
        ops.lars_stage1(f["p"], f["g"], f["ltable"], f["ltiles"], f["lpartials"], **clip)
        ops.layer_ratio_finish(f["lpartials"], f["ltable"], f["ltiles"], group["trust_coefficient"], group.get("layer_adaptation", True),
                               f["stats"])
        ops.lars_stage2(f["p"], f["g"], f["m"], f["lp"], f["ltable"], f["ltiles"], f["stats"], group["lr"], group["momentum"], **clip)

    # ---- checkpointing: torch.optim.SGD's layout (per-parameter 'momentum_buffer', no step counter)
    _STATE = {"momentum_buffer": "m"}
    _STATE_AMSGRAD = {}
    _STATE_STEP = False

    @staticmethod
    def _step_after_load(steps, loaded):
        return int(loaded)   # counts this object's steps only: the update does not depend on it


def layerwise_groups(model, weight_decay):
    """decay_groups for FusedLAMB / FusedLARS: the biases and norm weights (dim() < 2) are neither decayed nor adapted (their group has
    weight_decay=0 and layer_adaptation=False), as the published LARS / LAMB recipes exclude them."""
    decayed, rest = decay_groups(model, weight_decay)
    return [dict(decayed, layer_adaptation=True), dict(rest, weight_decay=0.0, layer_adaptation=False)]


def decay_groups(model, weight_decay):
    """The usual two parameter groups: tensors with dim() >= 2 (matrices, convolution kernels, embeddings) are decayed, biases and
    LayerNorm / BatchNorm weights (dim() < 2) are not.  Inside each group the parameters keep the order of model.parameters()."""
    params = list(model.parameters())
    return [{"params": [p for p in params if p.dim() >= 2], "weight_decay": weight_decay},
            {"params": [p for p in params if p.dim() < 2], "weight_decay": 0.0}]


class WeightEMA:
    """Exponential moving average of `module`'s parameters: avg <- avg + (1 - tau) * (p - avg) per update.

    `.module` is a deep copy of `module` in eval() with requires_grad_(False); its parameters are views into ONE flat f32 buffer (8-element
    alignment per tensor, FusedAdam's layout) and a flat bf16 copy is registered with lowp.put, so a bf16 forward of `.module` reads what
    the kernel wrote (the kernel does not bump `_version`: without the registration lowp.get would serve stale weights).  update() is one
    launch plus a copy_ of the persistent buffers (BatchNorm statistics); it never synchronises with the host.  The decay of update k
    (0-based), in f64 on the host: tau_k = decay_start + (decay - decay_start) * min(k, ramp_updates) / ramp_updates, or simply `decay` with
    decay_start None or ramp_updates 0.  The source's addresses are checked at every update: the segment table is rebuilt when a parameter's
    data_ptr() changed (an optimizer flattened the student).  Not a torch Module: a model that owns one moves it in its own _apply (to())."""

    def __init__(self, module, decay=0.999, decay_start=None, ramp_updates=0):
        if not 0.0 <= decay <= 1.0 or (decay_start is not None and not 0.0 <= decay_start <= 1.0) or ramp_updates < 0:
            raise ValueError(f"WeightEMA: invalid decay / decay_start / ramp_updates: {decay}, {decay_start}, {ramp_updates}")
        self.source = module
        self.decay, self.decay_start, self.ramp_updates = float(decay), None if decay_start is None else float(decay_start), int(ramp_updates)
        self.n_updates = 0
        self.module = copy.deepcopy(module).eval().requires_grad_(False)
        self._flat = self._flat_bf16 = self._table = None
        self._tiles, self._ptrs = 0, None
        self.flatten()

    def decay_at(self, k):
        """tau of update k (0-based), a Python float (f64)."""
        if self.decay_start is None or self.ramp_updates == 0:
            return self.decay
        return self.decay_start + (self.decay - self.decay_start) * min(int(k), self.ramp_updates) / self.ramp_updates

    def flatten(self):
        """Move the average's parameters into the flat buffers (again after the module moved to another device).  A module that is not on
        the GPU yet is left as it is: update() needs the GPU and says so."""
        ps = list(self.module.parameters())
        self._flat = self._table = self._ptrs = None
        if not ps or ps[0].device.type != "cuda":
            return
        dev = ps[0].device
        if any(p.dtype != torch.float32 or p.device != dev for p in ps):
            raise TypeError("WeightEMA: f32 parameters on one device")
        self._offsets, _, self._flat, self._flat_bf16 = _flat_storage(ps, dev)

    def _pairs(self, module):
        src, avg = list(module.parameters()), list(self.module.parameters())
        if len(src) != len(avg) or any(a.shape != b.shape for a, b in zip(src, avg)):
            raise ValueError("WeightEMA: the module's parameters do not match the average's")
        return src, avg

    def _buffers(self, module):
        """(average, source) pairs of the persistent buffers (those a state_dict carries)."""
        mine = dict(self.module.named_buffers())
        theirs = dict(module.named_buffers())
        names = [k for k in self.module.state_dict().keys() if k in mine]
        return [(mine[k], theirs[k]) for k in names]

    @torch.no_grad()
    def update(self, module=None):
        module = self.source if module is None else module
        if self._flat is None:
            self.flatten()
            if self._flat is None:
                raise RuntimeError("WeightEMA needs the parameters on the GPU (move the model first)")
        src, _ = self._pairs(module)
        ptrs = [p.data_ptr() for p in src]
        if ptrs != self._ptrs:
            if any(p.dtype != torch.float32 or not p.is_contiguous() or p.device != self._flat.device for p in src):
                raise TypeError("WeightEMA: the source's parameters are contiguous f32 tensors on the average's device")
            self._table, self._tiles = ops.ema_table([(a, o, p.numel()) for a, o, p in zip(ptrs, self._offsets, src)], self._flat.device)
            self._ptrs = ptrs
        ops.ema_update(self._flat, self._table, self._tiles, 1.0 - self.decay_at(self.n_updates), self._flat_bf16)
        for mine, theirs in self._buffers(module):
            mine.copy_(theirs)
        self.n_updates += 1

    @torch.no_grad()
    def copy_from(self, module=None):
        """Reset the average to the module's current parameters and buffers (n_updates, and with it the place on the decay ramp, stays)."""
        module = self.source if module is None else module
        src, avg = self._pairs(module)
        for a, p in zip(avg, src):
            a.copy_(p.detach())
        for mine, theirs in self._buffers(module):
            mine.copy_(theirs)
        self.refresh_lowp()

    def refresh_lowp(self):
        """Re-cast the bf16 copy after the average was written from outside (copy_from, load_state_dict)."""
        if self._flat is not None:
            ops.cast_to_bf16(self._flat, self._flat_bf16)

    def state_dict(self):
        return {"module": self.module.state_dict(), "n_updates": self.n_updates, "decay": self.decay, "decay_start": self.decay_start,
                "ramp_updates": self.ramp_updates}

    def load_state_dict(self, state):
        self.module.load_state_dict(state["module"])   # copy_ into the flat views
        self.n_updates = int(state["n_updates"])
        self.decay = float(state["decay"])
        self.decay_start = None if state["decay_start"] is None else float(state["decay_start"])
        self.ramp_updates = int(state["ramp_updates"])
        self.refresh_lowp()
