"""Per-line key ranges through the encoder layers and the models: tiny 2-layer backbones (model_dim 256, feedforward 512) with 2 heads
(head_dim 128) and 4 heads (head_dim 64) on three lines of 40 x 1056 (S = 132: two key tiles, the second with 4 keys) whose labels are -1
outside [3, 100), [128, 132) and [0, 132) - a dead second tile, a dead first tile and a full line.

* f32 parity mode (batched GEMM + the row softmax with ranges) against torch.nn.TransformerEncoder with src_key_padding_mask in f64
  (tests/attention_keys_ref.py): tokens at the valid positions within 1e-4 (the bar of the backbone_eval golden in tests/test_gpu_model.py),
  parameter gradients of a sum of squares over the valid positions within 1e-3 of each tensor's largest entry (its gradient bar).
* the bf16 step with the fused kernels and with functional.FUSED_ATTENTION = False, each against the f32 step: the rule of
  tests/test_gpu_attention_ragged.py::test_layer_step_at_the_real_width_fused_against_unfused.
* attend_valid_only: a line's tokens at its valid positions, the loss and the gradients do not depend on the PIXELS of the padding.  Without
  the attribute they do (the reference attends over the padding), which the same test asserts so that it cannot pass vacuously.
* Trainer.train_step, the joint-embedding step (both view paths) and Trainer(hip_graph=True) with the attribute on."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_keys_ref as KR  # noqa: E402

N, S, FF, VOCAB = 3, 132, 512, 512
RANGES = [(3, 100), (128, 132), (0, 132)]
OFFSETS = [11, 500, 2000]
HEAD = {"type": "linear", "in_features": 256, "out_features": VOCAB}
REPEATS = 8     # identical runs that measure the run-to-run difference of the gradient


def bb_def(h):
    return {"type": "vit", "num_blocks": 2, "model_dim": 256, "num_heads": h, "feedforward_dim": FF}


def make_batch(padding):
    """uint8 images (N, 40, 8 S, 3), labels (-1 outside the line's range), a mask inside the ranges.  padding: "zeros" or "random" - the pixel
    values of the columns outside each line's range; everything else is the same in both."""
    rng = np.random.default_rng(1056)
    images = rng.integers(0, 256, (N, 40, 8 * S, 3), dtype=np.uint8)
    labels = rng.integers(0, VOCAB, (N, S)).astype(np.int64)
    mask = (rng.random((N, S)) < 0.3).astype(int)
    noise = np.random.default_rng(7).integers(0, 256, images.shape, dtype=np.uint8)
    for b, (k0, k1) in enumerate(RANGES):
        pad = np.ones(S, dtype=bool)
        pad[k0:k1] = False
        labels[b, pad] = -1
        mask[b, pad] = 0
        mask[b, k0] = 1
        cols = np.repeat(pad, 8)
        images[b][:, cols, :] = noise[b][:, cols, :] if padding == "random" else 0
    return torch.from_numpy(images).cuda(), torch.from_numpy(labels).cuda(), mask


def valid_rows():
    v = ~KR.key_padding_mask(RANGES, S)
    return torch.nonzero(v.flatten()).flatten()


def make_model(h, attend=None):
    from pero_pretraining_amd.masked_pretraining import model as M
    torch.manual_seed(0)
    model = M.MaskedTransformerEncoder(M.init_backbone(bb_def(h)), M.init_head(dict(HEAD)))
    # LayerNorm biases as training leaves them (beta ~ 0.3 N(0, 1)), not the fresh beta = 0: with gamma = 1 and beta = 0 every output row has the squared
    # norm d whatever the weights are, so the sum of squares of the f32 test would be a constant and its gradients pure cancellation.  gamma stays 1:
    # the 1e-4 absolute bar on the tokens belongs to LayerNorm outputs of unit scale
    g = torch.Generator().manual_seed(256)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
    model = model.cuda().train()
    if attend is not None:
        model.attend_valid_only = attend
    return model


def run_step(h, bf16, images, labels, mask, attend=True):
    """One forward and backward through the Trainer; returns (loss tensor, tokens the backbone produced, concatenated gradient)."""
    from pero_pretraining_amd.masked_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.masked_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    model = make_model(h, attend)
    model.backbone.set_offsets(np.array(OFFSETS))
    seen = []
    real = model.backbone.encode_tokens
    model.backbone.encode_tokens = lambda *a, **k: (seen.append(real(*a, **k)), seen[-1])[1]
    trainer = Trainer(BatchOperator(torch.device("cuda", 0), 0.3), model, None, FusedAdam(model.parameters(), lr=1e-3), None, bfloat16=bf16)
    loss = trainer._forward_backward(images, labels, mask)
    torch.cuda.synchronize()
    grad = torch.cat([p.grad.detach().flatten() for p in model.parameters() if p.grad is not None])
    return loss, seen[0].detach(), grad


@pytest.mark.parametrize("h", [2, 4])
def test_f32_encoder_with_key_ranges_against_torch_with_a_key_padding_mask(h):
    from pero_pretraining_amd import functional as F
    images, _, _ = make_batch("random")
    model = make_model(h)
    bb = model.backbone
    bb.set_offsets(np.array(OFFSETS))
    kr = torch.tensor(RANGES, dtype=torch.int32, device="cuda")
    tokens = bb.encode_tokens(images, None, key_ranges=kr)
    assert tokens.dtype == torch.float32 and tokens.shape == (N * S, 256)
    rows = valid_rows()
    (tokens[rows.cuda()] ** 2).sum().backward()
    torch.cuda.synchronize()
    ref, params = KR.encoder_stack(bb.state_dict(), images, OFFSETS, RANGES, h, FF)
    (ref[rows] ** 2).sum().backward()
    err = float((tokens.detach().cpu().double()[rows] - ref.detach()[rows]).abs().max())
    print(f"\nKEYS f32 h={h}: tokens max abs err {err:.3e}", end="")
    # the ranges matter: without them the same tokens are far from this reference
    bb.set_offsets(np.array(OFFSETS))
    with torch.no_grad():
        plain = bb.encode_tokens(images, None)
    assert float((plain.cpu().double()[rows] - ref.detach()[rows]).abs().max()) > 1e-2
    ratios = {}
    for name, p in bb.named_parameters():
        g_ref = params[name].grad
        assert p.grad is not None and g_ref is not None, name
        e = float((p.grad.cpu().double() - g_ref).abs().max())
        ratios[name] = e / (1e-3 * max(float(g_ref.abs().max()), 1e-3))
    worst = max(ratios, key=ratios.get)
    print(f"  worst gradient error / bar {ratios[worst]:.3f} ({worst})", end="")
    assert err < 1e-4
    assert ratios[worst] <= 1.0, {k: round(v, 3) for k, v in ratios.items() if v > 1.0}
    assert F.FUSED_ATTENTION   # (untouched)


@pytest.mark.parametrize("h", [2, 4])
def test_bf16_step_with_key_ranges_fused_against_unfused(monkeypatch, h):
    """attend_valid_only on: the bf16 step with the fused kernels and with the batched-GEMM path, each against the f32 step; the fused step's
    relative errors must be at most 1.5 x the unfused step's, loss and gradient.  The fused calls are counted, and each must carry the ranges.
    Measured on an MI355X: 2 heads - loss 1.3e-5 fused, 7.1e-5 unfused, gradient 1.42e-2 / 1.44e-2; 4 heads - loss 4.8e-5 / 6.1e-5, gradient
    1.63e-2 / 1.80e-2.  (The loss errors of both paths are noise of either sign at the 5e-5 level, with and without ranges - DESIGN.md 8.0000000; the
    gradient figures carry the comparison.)"""
    from pero_pretraining_amd import functional as F
    from pero_pretraining_amd import ops
    images, labels, mask = make_batch("random")
    fused_calls, unfused_ranges = [], []
    real_fwd, real_sm = ops.attention_fwd_fused, ops.softmax_fwd
    monkeypatch.setattr(ops, "attention_fwd_fused", lambda *a, **k: (fused_calls.append(k.get("key_ranges")), real_fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "softmax_fwd", lambda *a, **k: (unfused_ranges.append(k.get("key_ranges")), real_sm(*a, **k))[1])

    def step(bf16):
        loss, _, grad = run_step(h, bf16, images, labels, mask)
        return float(loss), grad.double().cpu()

    loss32, grad32 = step(False)
    assert not fused_calls and len(unfused_ranges) == 2 and all(k is not None for k in unfused_ranges)   # f32: batched GEMM + softmax with ranges
    loss_f, grad_f = step(True)
    assert len(fused_calls) == 2 and all(k is not None and k.tolist() == [list(r) for r in RANGES] for k in fused_calls)
    assert len(unfused_ranges) == 2
    monkeypatch.setattr(F, "FUSED_ATTENTION", False)
    loss_u, grad_u = step(True)
    assert len(fused_calls) == 2 and len(unfused_ranges) == 4 and all(k is not None for k in unfused_ranges)
    assert grad_f.shape == grad32.shape == grad_u.shape and math.isfinite(loss_f) and bool(torch.isfinite(grad_f).all())
    gn = float(grad32.norm())
    e_loss_f, e_loss_u = abs(loss_f - loss32) / abs(loss32), abs(loss_u - loss32) / abs(loss32)
    e_grad_f, e_grad_u = float((grad_f - grad32).norm()) / gn, float((grad_u - grad32).norm()) / gn
    print(f"\nKEYS LAYER h={h}: loss rel err fused {e_loss_f:.3e} unfused {e_loss_u:.3e}; gradient rel err fused {e_grad_f:.3e} unfused {e_grad_u:.3e}")
    assert e_grad_f <= 1.5 * e_grad_u, (e_grad_f, e_grad_u)
    assert e_loss_f <= 1.5 * e_loss_u, (e_loss_f, e_loss_u)


@pytest.mark.parametrize("h,bf16", [(2, True), (4, True), (2, False), (4, False)])
def test_valid_positions_do_not_depend_on_the_padding(h, bf16):
    """The same step on two batches that differ only in the pixels of the padded columns (zeros / random bytes).  attend_valid_only: tokens at the
    valid positions and the loss are equal bit for bit, and the gradient differs by no more than two identical runs do (bit-identical runs:
    equal).  Without it the tokens at the valid positions differ: every line attends over its padding, as in the reference."""
    zeros, rand = make_batch("zeros"), make_batch("random")
    assert not torch.equal(zeros[0], rand[0]) and torch.equal(zeros[1], rand[1]) and np.array_equal(zeros[2], rand[2])
    rows = valid_rows().cuda()
    loss_a, tok_a, grad_a = run_step(h, bf16, *zeros)
    loss_b, tok_b, grad_b = run_step(h, bf16, *rand)
    # How identical runs differ: the bias gradients of in_proj and linear1 are reduced with f32 atomics whose order varies between launches, so a few of
    # their sums differ in the last bit from run to run (which ones, and whether any, changes every time).  REPEATS identical runs: the largest
    # difference any element shows among them is the measured run-to-run difference
    lo, hi = grad_a.clone(), grad_a.clone()
    for _ in range(REPEATS - 1):
        loss_a2, tok_a2, grad_a2 = run_step(h, bf16, *zeros)
        assert torch.equal(tok_a[rows], tok_a2[rows]) and torch.equal(loss_a, loss_a2)      # tokens and loss repeat bit for bit
        lo, hi = torch.minimum(lo, grad_a2), torch.maximum(hi, grad_a2)
    assert tok_a.dtype == (torch.bfloat16 if bf16 else torch.float32)
    assert torch.equal(tok_a[rows], tok_b[rows]), "tokens at valid positions depend on the padding's pixels"
    assert torch.equal(loss_a, loss_b), (float(loss_a), float(loss_b))
    assert not torch.equal(tok_a, tok_b)            # (the padded positions themselves do see their own pixels)
    noise = float((hi - lo).max())
    diff = float((grad_a - grad_b).abs().max())
    print(f"\nKEYS PADDING h={h} bf16={bf16}: gradient run-to-run {noise:.3e} ({int((hi != lo).sum())} of {hi.numel()} elements vary), between paddings {diff:.3e} "
          f"({int((grad_a != grad_b).sum())} differ)", end="")
    if noise == 0.0:
        assert torch.equal(grad_a, grad_b)
    else:
        assert diff <= noise, (diff, noise)
    # the option off: the reference's arithmetic, where a line's tokens depend on its padding
    _, tok_c, _ = run_step(h, bf16, *zeros, attend=False)
    _, tok_d, _ = run_step(h, bf16, *rand, attend=False)
    assert not torch.equal(tok_c[rows], tok_d[rows])
    assert not torch.equal(tok_c[rows], tok_a[rows])


def test_trainer_train_step_with_attend_valid_only():
    from pero_pretraining_amd.masked_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.masked_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    images, labels, _ = make_batch("random")
    model = make_model(2, True)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    np.random.seed(4)
    trainer = Trainer(BatchOperator(torch.device("cuda", 0), 0.3), model, None, FusedAdam(model.parameters(), lr=1e-3), None, bfloat16=True)
    loss = float(trainer.train_step({"images": images, "labels": labels.cpu().numpy()}))
    torch.cuda.synchronize()
    assert math.isfinite(loss)
    for k, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[k]), k
    # host labels take the host path of the ranges: a line without a valid label is refused there
    bad = labels.cpu().numpy().copy()
    bad[1] = -1
    with pytest.raises(ValueError, match="line 1 has no valid position"):
        model(images, bad, np.zeros((N, S), dtype=int))


def test_joint_step_with_ranges_from_the_image_masks(monkeypatch):
    """NTXentLoss(apply_masks=True) on a collated pair of views, attend_valid_only on: view 1's ranges come from image_masks1, view 2's from
    image_masks2, on the batched-views path and on the two-encodes path - the same loss (f32 mode: within 1e-4 relative, the bar of the f32
    losses in tests/test_gpu_model.py; the two paths run the same kernels on 2N and on N lines)."""
    from pero_pretraining_amd import ops
    from pero_pretraining_amd.common.dataloader import BatchCreator
    from pero_pretraining_amd.joint_embedding_pretraining import model as JM
    from pero_pretraining_amd.joint_embedding_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.joint_embedding_pretraining.train import init_model
    rng = np.random.default_rng(15)
    data = [{"image": rng.integers(0, 256, (40, w, 3), dtype=np.uint8), "image2": rng.integers(0, 256, (40, w, 3), dtype=np.uint8), "labels": None,
             "image_id": str(i)} for i, w in enumerate((480, 512, 400, 512))]
    np.random.seed(3)
    batch = BatchCreator().create_batch(data)
    prepared = BatchOperator(torch.device("cuda", 0)).prepare_batch(batch)
    n, s = prepared[2].shape
    want1, want2 = ops.key_ranges_from_masks(prepared[2]), ops.key_ranges_from_masks(prepared[3].cpu().numpy())
    assert not torch.equal(want1, want2) and int((want1[:, 1] - want1[:, 0]).min()) == 50
    torch.manual_seed(0)
    definitions = ({"type": "vit", "num_blocks": 2, "model_dim": 256, "num_heads": 2, "feedforward_dim": 256},
                   {"type": "linear", "in_features": 256, "out_features": 80})
    model = init_model(torch.device("cuda", 0), *definitions, loss_type="ntxent", ntxent_apply_masks=True).train()
    model.attend_valid_only = True
    seen = []
    real = ops.softmax_fwd
    monkeypatch.setattr(ops, "softmax_fwd", lambda *a, **k: (seen.append(k.get("key_ranges")), real(*a, **k))[1])
    offs = (np.arange(n) * 7, np.arange(n) * 5 + 100)
    losses = {}
    for views in (True, False):
        monkeypatch.setattr(JM, "BATCH_VIEWS", views)
        model.backbone.set_offsets(*offs)
        del seen[:]
        out = model(*prepared)
        losses[views] = float(out["loss"])
        got = torch.cat([k for k in seen[::2]]) if not views else seen[0]
        assert torch.equal(got, torch.cat([want1, want2])), views       # view 1's lines, then view 2's
        assert len(seen) == (2 if views else 4)
    assert math.isfinite(losses[True]) and abs(losses[True] - losses[False]) <= 1e-4 * abs(losses[False]), losses
    model.attend_valid_only = False
    model.backbone.set_offsets(*offs)
    assert abs(float(model(*prepared)["loss"]) - losses[True]) > 1e-4 * abs(losses[True])   # the ranges change the step
    # one training step (bf16, the fused kernels) with the ranges on: finite, every parameter moves
    from pero_pretraining_amd.joint_embedding_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    monkeypatch.setattr(JM, "BATCH_VIEWS", True)
    model.attend_valid_only = True
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    trainer = Trainer(BatchOperator(torch.device("cuda", 0)), model, None, FusedAdam(model.parameters(), lr=1e-3), None, bfloat16=True)
    assert math.isfinite(float(trainer.train_step(batch)))
    torch.cuda.synchronize()
    assert all(not torch.equal(p.detach(), before[k]) for k, p in model.named_parameters())


def test_hip_graph_step_with_attend_valid_only_equals_the_eager_step():
    """Trainer(hip_graph=True) works with the attribute on: the ranges are a device tensor computed inside the captured step from the static label
    buffer, so a replay with other labels attends to other keys.  Two steps with different ranges against the eager Trainer, with the bars of
    tests/test_gpu_model.py::test_hip_graph_step_equals_eager_step (losses 1e-5 relative, weights 1e-4)."""
    from pero_pretraining_amd.common.lr_scheduler import WarmupSchleduler
    from pero_pretraining_amd.masked_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    images, labels, mask = make_batch("random")
    labels2 = labels.clone()
    labels2[0, 100:120] = 5           # line 0's range grows to [3, 120) in the second step
    eager = make_model(2, True).eval()
    graph = copy.deepcopy(eager)
    assert graph.attend_valid_only is True
    runs = {}
    for name, model, flag in (("eager", eager, False), ("graph", graph, True)):
        opt = FusedAdam(model.parameters(), lr=2e-3)
        sched = WarmupSchleduler(opt, 2e-3, 2, 1)
        trainer = Trainer(None, model, None, opt, sched, bfloat16=True, hip_graph=flag)
        losses = []
        for i, lab in enumerate((labels, labels2, labels)):
            sched.update_learning_rate(i + 1)
            losses.append(float(trainer.train_step_prepared(images, lab, torch.from_numpy(mask).cuda())))
        torch.cuda.synchronize()
        runs[name] = (losses, {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()})
        if flag:
            assert len(trainer._graphs) == 1   # one capture, three replays
    assert runs["eager"][0][0] != runs["eager"][0][1]
    for a, b in zip(runs["eager"][0], runs["graph"][0]):
        assert np.isfinite(a) and abs(a - b) <= 1e-5 * abs(a), runs
    for k, v in runs["eager"][1].items():
        w = runs["graph"][1][k]
        if k.endswith("in_proj_bias"):  # key-bias slice: zero gradient up to rounding noise, which Adam turns into +-lr steps
            d = v.shape[0] // 3
            v, w = np.delete(v, np.s_[d:2 * d]), np.delete(w, np.s_[d:2 * d])
        assert np.abs(v - w).max() <= 1e-4, k
