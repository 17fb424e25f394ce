"""The bf16 training mode against trajectories the reference wrote itself (tests/golden, oracle/make_golden_r5.py g22; g5).

g22: three Trainer.train_step calls of a config-2-width model with 2 layers on 2 lines of 40 x 2048 - the shapes at which the bf16 mode runs
the fused attention, the n512 LayerNorm epilogues, the ReLU bit masks and the row-sparse last layer - once with fresh weights and once with
LayerNorm weights as training leaves them (oracle/pero_oracle.py trained_layernorm_columns).  f32 parity mode pins the fixture (loss 1e-4);
the bf16 mode's error against the reference is calibrated by the plainest bf16 arrangement (unfused LayerNorms with their input rows kept,
the dense last layer): under the default flags every tensor's weight update Delta w = sd3 - sd0 is within 1.5 x that arrangement's error +
a floor, and every loss within 3e-2 of the reference's.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BB = {"type": "vit", "num_blocks": 2, "model_dim": 512, "num_heads": 4, "feedforward_dim": 2048}
HD = {"type": "linear", "in_features": 512, "out_features": 4096}
BASELINE_FLAGS = {"FUSE_LN_FWD_MAX_K": 0, "LN_BWD_FROM_OUT": False, "FUSE_LN_BWD": False, "ROW_SPARSE_LAST_LAYER": False}
DW_FLOOR = 2e-2   # on ||Delta w_ours - Delta w_ref|| / ||Delta w_ref||: Adam's first steps move a weight by ~lr whatever its gradient's size, so a
                  # rounding-sized gradient flips a step's sign - the calibrating arrangement's own error is 1e-2..1e-1 per tensor


def g22_batches():
    """The images and labels of make_golden_r5.batches()."""
    rng = np.random.default_rng(2205)
    return [(rng.integers(0, 256, (2, 40, 2048, 3), dtype=np.uint8), rng.integers(0, 4096, (2, 256)).astype(np.int64)) for _ in range(3)]


def set_flags(flags):
    from pero_pretraining_amd import functional as F
    old = {k: getattr(F, k) for k in flags}
    for k, v in flags.items():
        setattr(F, k, v)
    return old


def dw_errors(sd0, sd3, ref_sd3, index):
    """Per tensor ||Delta w_ours - Delta w_ref|| / ||Delta w_ref|| on the stored entries (the key third of in_proj_bias left out: its gradient is
    mathematically zero and Adam turns rounding noise into +-lr steps)."""
    out = {}
    for k, ref in ref_sd3.items():
        a0, a3 = sd0[k].reshape(-1), sd3[k].reshape(-1)
        if k in index:
            a0, a3 = a0[index[k]], a3[index[k]]
        dref, dour = ref.reshape(-1).astype(np.float64) - a0, a3.astype(np.float64) - a0
        if k.endswith("in_proj_bias"):
            d = dref.shape[0] // 3
            dref, dour = np.delete(dref, np.s_[d:2 * d]), np.delete(dour, np.s_[d:2 * d])
        out[k] = float(np.linalg.norm(dour - dref) / max(np.linalg.norm(dref), 1e-30))
    return out


def run_g22(g, variant, bf16, flags=None):
    """The fixture's three steps through our Trainer: (losses, Delta w errors per tensor, number of row-sparse backward passes)."""
    from pero_pretraining_amd import functional as F
    from pero_pretraining_amd.common.lr_scheduler import WarmupSchleduler
    from pero_pretraining_amd.masked_pretraining import model as M
    from pero_pretraining_amd.masked_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.masked_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    torch.manual_seed(0)
    model = M.MaskedTransformerEncoder(M.init_backbone(dict(BB)), M.init_head(dict(HD)))
    if variant == "trained":
        model.load_state_dict({k[len("norms."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("norms.")}, strict=False)
    sd0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    for k, v in sd0.items():   # the seed recipe gave the reference's starting weights
        assert abs(v.astype(np.float64).sum() - float(g[f"{variant}.sd0sum.{k}"])) <= 1e-9 * max(1.0, np.abs(v).sum()), k
    model = model.cuda().train()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    sched = WarmupSchleduler(opt, 1e-3, 2, 1)
    trainer = Trainer(BatchOperator(torch.device("cuda", 0), 0.15), model, None, opt, sched, bfloat16=bf16)
    old = set_flags(flags or {})
    sparse0 = F.row_sparse_steps
    try:
        np.random.seed(5)   # the reference run's mask sequence (BatchOperator draws from the global numpy RNG)
        losses = []
        for i, (images, labels) in enumerate(g22_batches()):
            assert int(images.astype(np.int64).sum()) == int(g["image_sums"][i]) and np.array_equal(labels, g["labels"][i])
            sched.update_learning_rate(i + 1)
            assert sched.current_lr == float(g[f"{variant}.lr"][i])
            model.backbone.set_offsets(g[f"{variant}.offsets"][i])
            batch = {"images": images, "labels": labels}
            st = np.random.get_state()
            assert np.array_equal(trainer.batch_operator._create_mask(batch), g[f"{variant}.mask"][i])
            np.random.set_state(st)
            losses.append(float(trainer.train_step(batch)))
        torch.cuda.synchronize()
    finally:
        set_flags(old)
    sd3 = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}
    ref = {k[len(variant) + 5:]: g[k] for k in g.files if k.startswith(variant + ".sd3.")}
    index = {k[len("index."):]: g[k] for k in g.files if k.startswith("index.")}
    return losses, dw_errors(sd0, sd3, ref, index), F.row_sparse_steps - sparse0


@pytest.mark.parametrize("variant", ["fresh", "trained"])
def test_g22_f32_mode_matches_the_reference(golden, variant):
    g = golden("g22_bf16_trajectory.npz")
    losses, errs, _ = run_g22(g, variant, bf16=False)
    for i, (got, want) in enumerate(zip(losses, g[f"{variant}.loss"])):
        assert abs(got - want) < 1e-4 * want, (i, got, want)
    for k, e in errs.items():
        assert e < 1e-2, (k, e)


@pytest.mark.parametrize("variant", ["fresh", "trained"])
def test_g22_bf16_default_flags_within_the_plain_bf16_error(golden, variant):
    """The bf16 default (fused LayerNorm epilogues, backward from the output rows, row-sparse last layer) against the reference, next to the
    plainest bf16 arrangement.  "trained": columns with |beta / gamma| up to 4000 and a gamma == 0 column in both layers' norms - the layers must
    fall back to keeping their input rows (functional.ln_keep_rows), else norm weights and everything below them take wrong updates."""
    g = golden("g22_bf16_trajectory.npz")
    ref_loss = g[f"{variant}.loss"]
    base_losses, base, _ = run_g22(g, variant, bf16=True, flags=BASELINE_FLAGS)
    losses, errs, sparse = run_g22(g, variant, bf16=True)
    # (the row-sparse last layer runs from the output rows: the trained variant's layers keep their input rows and take the dense backward)
    assert sparse == (3 if variant == "fresh" else 0), sparse
    for name, ls in (("baseline", base_losses), ("default", losses)):
        for i, (got, want) in enumerate(zip(ls, ref_loss)):
            assert abs(got - want) <= 3e-2 * want, (name, i, got, want)
    bad = {k: (round(e, 4), round(base[k], 4)) for k, e in errs.items() if e > 1.5 * base[k] + DW_FLOOR}
    assert not bad, (variant, bad)


def test_trained_norms_are_fragile_fresh_ones_are_not(golden):
    """The fallback's decision on the two g22 variants: every layer of the trained one keeps its rows, no layer of the fresh one (the
    benchmark's kernel sequence is unchanged)."""
    from pero_pretraining_amd import functional as F
    from pero_pretraining_amd.masked_pretraining import model as M
    g = golden("g22_bf16_trajectory.npz")
    torch.manual_seed(0)
    model = M.MaskedTransformerEncoder(M.init_backbone(dict(BB)), M.init_head(dict(HD))).cuda()
    assert F.ln_keep_rows(model.backbone, torch.bfloat16) == (False, False)
    assert F.ln_keep_rows(model.backbone, torch.float32) is None
    model.load_state_dict({k[len("norms."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("norms.")}, strict=False)
    assert F.ln_keep_rows(model.backbone, torch.bfloat16) == (True, True)


@pytest.mark.parametrize("fragile, keep, sparse", [("layers.0.norm2", (True, False), 1), ("layers.1.norm1", (False, True), 0)])
def test_step_with_one_layer_keeping_its_rows_stays_within_the_f32_step(fragile, keep, sparse):
    """One of the two layers keeps its LayerNorms' input rows (a gamma == 0 column), the other runs them from the output - the two g22 variants have
    all layers alike.  Layer 0 keeps: layer 1 (the last) takes the row-sparse path and gets no lower norm2 to fuse into its in_proj product.  Layer 1
    keeps: it falls back to the dense backward from its rows, and layer 0's norm2 backward runs in layer 1's in_proj product, from layer 0's rstd2.
    One bf16 step (2 lines of 40 x 2048, fixed offsets and mask) against the same step in f32 parity mode, by the criterion of
    test_gpu_full_size.test_config2_step_under_every_layernorm_path_stays_within_the_f32_step: loss 1e-2, every parameter gradient within 1.5 x the
    error of the plainest bf16 arrangement on the same weights + 2e-2.  A statistic or a row matrix of the wrong layer or norm is tens of percent."""
    import pero_pretraining_amd as P
    from pero_pretraining_amd import functional as F
    from pero_pretraining_amd.masked_pretraining import model as M
    torch.manual_seed(0)
    model = M.MaskedTransformerEncoder(M.init_backbone(dict(BB)), M.init_head(dict(HD))).cuda().train()
    with torch.no_grad():
        model.backbone.encoder_layers.get_submodule(fragile).weight[0] = 0
    assert F.ln_keep_rows(model.backbone, torch.bfloat16) == keep
    images, labels = g22_batches()[0]
    images, labels = torch.from_numpy(images).cuda(), torch.from_numpy(labels).cuda()
    mask = (np.random.default_rng(3).random((2, 256)) < 0.15).astype(np.int64)

    def step(bf16, flags):
        old = set_flags(flags)
        try:
            model.zero_grad()
            model.backbone.set_offsets(np.array([5, 900]))
            taken = F.row_sparse_steps
            with P.autocast(bf16):
                loss = model(images, labels, mask)["loss"]
            loss.backward()
            torch.cuda.synchronize()
            return float(loss), {k: p.grad.detach().float().clone() for k, p in model.named_parameters()}, F.row_sparse_steps - taken
        finally:
            set_flags(old)

    loss32, g32, _ = step(False, {})
    errs = {}
    for name, flags in (("baseline", BASELINE_FLAGS), ("default", {})):
        loss, g, taken = step(True, flags)
        assert taken == (sparse if name == "default" else 0), (name, taken)
        assert abs(loss - loss32) <= 1e-2 * abs(loss32), (name, loss, loss32)
        errs[name] = {k: float((g[k] - g32[k]).norm() / g32[k].norm().clamp_min(1e-12)) for k in g32}
    assert F._row_grad_hint is None
    print({k: (round(v, 4), round(errs["baseline"][k], 4)) for k, v in errs["default"].items()})
    for k, v in errs["default"].items():
        if "in_proj_bias" in k:
            continue   # (its key third has a mathematically zero gradient: rounding noise only)
        assert v <= 1.5 * errs["baseline"][k] + 2e-2, (k, v, errs["baseline"][k])


def test_g5_bf16_within_the_plain_bf16_error(golden):
    """g5 (d = 64, the unfused bf16 path: layernorm_bwd_out at d = 64, dense attention) in bf16: default flags against the plain arrangement."""
    from pero_pretraining_amd.common.lr_scheduler import WarmupSchleduler
    from pero_pretraining_amd.masked_pretraining import model as M
    from pero_pretraining_amd.masked_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.masked_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    g = golden("g5_trajectory.npz")
    sd0 = {k[4:]: g[k] for k in g.files if k.startswith("sd0.")}
    ref = {k[4:]: g[k] for k in g.files if k.startswith("sd3.")}
    res = {}
    for name, flags in (("baseline", BASELINE_FLAGS), ("default", {})):
        model = M.MaskedTransformerEncoder(
            M.init_backbone({"type": "vit", "num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128}),
            M.init_head({"type": "linear", "in_features": 64, "out_features": 96}))
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd0.items()})
        model = model.cuda().train()
        opt = FusedAdam(model.parameters(), lr=2e-3)
        sched = WarmupSchleduler(opt, 2e-3, 2, 1)
        trainer = Trainer(BatchOperator(torch.device("cuda", 0), 0.15), model, None, opt, sched, bfloat16=True)
        old = set_flags(flags)
        try:
            np.random.seed(5)
            losses = []
            for i in range(3):
                sched.update_learning_rate(i + 1)
                model.backbone.set_offsets(g["offsets"][i])
                losses.append(float(trainer.train_step({"images": g["images"][i], "labels": g["labels"][i]})))
        finally:
            set_flags(old)
        res[name] = (losses, dw_errors(sd0, {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}, ref, {}))
    for name, (losses, _) in res.items():
        for i, (got, want) in enumerate(zip(losses, g["loss"])):
            assert abs(got - want) <= 3e-2 * want, (name, i, got, want)
    base = res["baseline"][1]
    # 16 token rows: one rounding-sized column sum flips an Adam step of a 128-entry bias (0.04 of its update norm with fresh weights, where the
    # two arrangements' arithmetic differs only in which bf16 rows the LayerNorm backward reads)
    floor = 6e-2
    bad = {k: (round(e, 4), round(base[k], 4)) for k, e in res["default"][1].items() if e > 1.5 * base[k] + floor}
    assert not bad, bad


def test_hip_graph_step_recaptures_when_a_layer_crosses_the_fragility_threshold(golden):
    """Trainer(hip_graph=True): which layers keep their LayerNorm input rows is baked into a captured graph, so it is decided before capture /
    replay and keys the graph cache.  A gamma of layer 1's norm1 set to 1e-3 next to its beta = 1 after the first step: two graphs, and the
    losses and weights of the eager Trainer (the g5 hip-graph test's tolerances)."""
    import copy
    from pero_pretraining_amd import functional as F
    from pero_pretraining_amd.common.lr_scheduler import WarmupSchleduler
    from pero_pretraining_amd.masked_pretraining import model as M
    from pero_pretraining_amd.masked_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    g = golden("g5_trajectory.npz")
    eager = M.MaskedTransformerEncoder(
        M.init_backbone({"type": "vit", "num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128}),
        M.init_head({"type": "linear", "in_features": 64, "out_features": 96}))
    eager.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd0.")})
    eager = eager.cuda().eval()
    graph = copy.deepcopy(eager)
    runs = {}
    for name, model, flag in (("eager", eager, False), ("graph", graph, True)):
        opt = FusedAdam(model.parameters(), lr=2e-3)
        sched = WarmupSchleduler(opt, 2e-3, 2, 1)
        trainer = Trainer(None, model, None, opt, sched, bfloat16=True, hip_graph=flag)
        losses, keeps = [], []
        for i in range(3):
            if i == 1:
                n1 = model.backbone.encoder_layers.layers[1].norm1
                with torch.no_grad():
                    n1.weight[5] = 1e-3
                    n1.bias[5] = 1.0
                opt.refresh_lowp()
            keeps.append(F.ln_keep_rows(model.backbone, torch.bfloat16))
            sched.update_learning_rate(i + 1)
            images = torch.from_numpy(g["images"][i]).cuda()
            labels = torch.from_numpy(g["labels"][i]).cuda()
            mask = torch.from_numpy(g["mask"][i]).cuda()
            losses.append(float(trainer.train_step_prepared(images, labels, mask)))
        torch.cuda.synchronize()
        assert keeps[0] == (False, False) and keeps[1] == keeps[2] == (False, True), keeps
        runs[name] = (losses, {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()})
        if flag:
            assert len(trainer._graphs) == 2
            assert model.backbone.ln_keep_rows_pinned is None
    for a, b in zip(runs["eager"][0], runs["graph"][0]):
        assert np.isfinite(a) and abs(a - b) <= 1e-5 * abs(a), runs
    for k, v in runs["eager"][1].items():
        w = runs["graph"][1][k]
        if k.endswith("in_proj_bias"):
            d = v.shape[0] // 3
            v, w = np.delete(v, np.s_[d:2 * d]), np.delete(w, np.s_[d:2 * d])
        assert np.abs(v - w).max() <= 1e-4, k


def test_row_sparse_hint_ignores_a_gradient_with_a_second_consumer():
    """The head's loss announces a backbone-output gradient that is zero outside the masked rows (functional.set_row_grad_hint).  When the output
    has a second differentiable consumer, autograd hands the backbone the SUM, which is dense: the hint must not match it (same tensor object,
    same version - not merely the same address), and the gradients equal those of the dense last layer (the row-sparse test's 1e-5)."""
    import pero_pretraining_amd as P
    from pero_pretraining_amd import functional as F
    from pero_pretraining_amd.masked_pretraining import model as M
    torch.manual_seed(0)
    model = M.MaskedTransformerEncoder(M.init_backbone(dict(BB)), M.init_head(dict(HD))).cuda().train()
    images, labels = g22_batches()[0]
    images, labels = torch.from_numpy(images).cuda(), torch.from_numpy(labels).cuda()
    mask = (np.random.default_rng(3).random((2, 256)) < 0.15).astype(np.int64)
    enc = model.backbone.encode_tokens
    tokens = []

    def encode_tokens(x, m=None):
        tokens.append(enc(x, m))
        return tokens[-1]

    model.backbone.encode_tokens = encode_tokens

    def step(flag, second):
        old = set_flags({"ROW_SPARSE_LAST_LAYER": flag})
        try:
            model.zero_grad()
            model.backbone.set_offsets(np.array([5, 900]))
            tokens.clear()
            taken = F.row_sparse_steps
            with P.autocast(True):
                loss = model(images, labels, mask)["loss"]
            if second:
                loss = loss + 0.1 * tokens[0].float().square().mean()
            loss.backward()
            torch.cuda.synchronize()
            return F.row_sparse_steps - taken, {k: p.grad.detach().float().clone() for k, p in model.named_parameters()}
        finally:
            set_flags(old)

    try:
        assert step(True, False)[0] == 1   # the hint reaches the backbone through a single consumer
        n_dense, g_dense = step(False, True)
        n_sparse, g_sparse = step(True, True)
    finally:
        del model.backbone.encode_tokens
    assert n_dense == 0 and n_sparse == 0
    assert F._row_grad_hint is None
    for k, ref in g_dense.items():
        assert float((g_sparse[k] - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-12, k
