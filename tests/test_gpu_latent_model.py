"""GPU: the latent-target model, its EMA teacher, trainer, tester and checkpoint (pero_pretraining_amd/latent_pretraining, optim.WeightEMA,
TransformerEncoder.encode_layers) against the f64 step of tests/latent_ref.py, which runs the oracle's backbone (oracle/pero_oracle.py) layer
by layer.  The tiny configuration of tests/test_gpu_model.py (2 blocks, d 64, 4 heads, ff 128) on the images of its g4 / g5 fixtures.
Bars: those test_gpu_model.py holds the masked step to - f32 losses within 1e-4 relative, gradients within 1e-3 of the tensor's largest
magnitude, parameters after three Adam steps within 5e-4; the bf16 loss within 3e-2 of the f32 one (test_gpu_bf16_trajectory.py)."""
import copy

import numpy as np
import pytest
import torch

import latent_ref as LR
from oracle import pero_oracle as O

pytestmark = pytest.mark.gpu

CFG = {"type": "vit", "num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128}


def build(seed=0, **kw):
    from pero_pretraining_amd.latent_pretraining import model as M
    torch.manual_seed(seed)
    model = M.LatentTargetTransformerEncoder(M.init_backbone(dict(CFG)), M.init_head({"type": "linear", "in_features": 64, "out_features": 64}), **kw)
    return model.cuda()


def detune_teacher(model, seed=1):
    """A teacher that differs from the student (as it does after the first updates), so that a mix-up of the two shows."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.teacher.parameters():
            p.add_((torch.randn(p.shape, generator=g) * 0.02).to(p.device))
    model.ema.refresh_lowp()


def f64_sds(model):
    student = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    teacher = {"backbone." + k: v.detach().cpu().double() for k, v in model.teacher.state_dict().items()}
    return student, teacher


def bits(module):
    return [p.detach().clone() for p in module.parameters()]


@pytest.mark.parametrize("top_k", [1, 2])
def test_one_step_f32_against_the_f64_step(golden, top_k):
    g = golden("g4_masked_tiny.npz")
    model = build(top_k=top_k, beta=2.0).train()
    detune_teacher(model)
    student, teacher = f64_sds(model)
    before = bits(model.teacher)
    images, mask, offs = g["images"], g["mask"].copy(), g["train_offsets"]
    model.backbone.set_offsets(offs)           # train mode with injected offsets: the model draws them once, for teacher and student
    res = model(torch.from_numpy(images).cuda(), None, mask)
    res["loss"].backward()
    ref, targets, pred, index = LR.latent_step(student, teacher, images, mask, 4, top_k, 2.0, 1e-5, offs)
    ref.backward()
    err = abs(float(res["loss"]) - float(ref))
    print(f"\nlatent step f32 top_k={top_k}: loss {float(res['loss']):.8f} f64 {float(ref):.8f} (error {err:.2e}, bound {1e-4 * abs(float(ref)):.2e})")
    assert err < 1e-4 * abs(float(ref))
    assert torch.equal(res["rows"].cpu(), index) and res["targets"].shape == targets.shape == res["output_rows"].shape
    assert float((res["targets"].cpu().double() - targets).abs().max()) < 1e-4       # O(1) normalised values, as the masked step's logits
    assert float((res["output_rows"].detach().cpu().double() - pred.detach()).abs().max()) < 1e-4
    for k, p in model.named_parameters():
        want = student[k].grad
        e = float((p.grad.cpu().double() - want).abs().max())
        assert e <= 1e-3 * max(float(want.abs().max()), 1e-3), (k, e, float(want.abs().max()))
    # the teacher: no gradient, the same bits behind forward and backward
    assert all(p.grad is None and not p.requires_grad for p in model.teacher.parameters())
    assert all(torch.equal(a, b) for a, b in zip(before, bits(model.teacher)))
    assert not any(k.startswith(("ema", "teacher")) for k in model.state_dict())


def test_uint8_and_float32_inputs_and_the_teacher_sees_the_unmasked_line(golden):
    g = golden("g4_masked_tiny.npz")
    model = build(top_k=2).eval()
    detune_teacher(model)
    mask = g["mask"].copy()
    l8 = float(model(torch.from_numpy(g["images"]).cuda(), None, mask)["loss"])
    x = O.prepare_images(torch.from_numpy(g["images"])).contiguous().cuda()
    l32 = float(model(x, None, mask)["loss"])
    # (a student that ran first would have overwritten x: the teacher would see the masked line and the losses would differ)
    assert abs(l8 - l32) <= 1e-6 * abs(l8), (l8, l32)
    # the reference semantic of a float32 input: behind the call the tensor holds the masked image
    assert np.array_equal(x[:, :, :, :64].cpu().numpy(), g["masked_images_sample"])
    student, teacher = f64_sds(model)
    ref = float(LR.latent_step(student, teacher, g["images"], mask, 4, 2, 2.0, 1e-5)[0])
    assert abs(l8 - ref) < 1e-4 * abs(ref)
    # no mask: the head's output at every position; nothing masked: the NaN of an empty mean; a device-only mask: the same loss
    out = model(torch.from_numpy(g["images"]).cuda())["output"]
    assert out.shape == (g["images"].shape[0], g["images"].shape[2] // 8, 64)
    assert np.isnan(float(model(torch.from_numpy(g["images"]).cuda(), None, np.zeros_like(mask))["loss"]))
    ldev = float(model(torch.from_numpy(g["images"]).cuda(), None, torch.from_numpy(mask).cuda())["loss"])
    assert ldev == l8


def test_three_steps_fused_adam_against_adam_and_averaged_model_f64(golden):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from pero_pretraining_amd.latent_pretraining.trainer import Trainer
    from pero_pretraining_amd.optim import FusedAdam
    g = golden("g5_trajectory.npz")
    decay = 0.9
    model = build(top_k=2, beta=2.0, decay=decay).train()
    student, _ = f64_sds(model)

    class Bag(torch.nn.Module):    # the f64 student backbone's tensors as a module, for AveragedModel
        def __init__(self, tensors):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.detach().clone()) for t in tensors])

    bkeys = [k for k in student if k.startswith("backbone.")]
    bag = Bag([student[k] for k in bkeys])
    student.update({k: p for k, p in zip(bkeys, bag.ps)})
    ropt = torch.optim.Adam(list(student.values()), lr=2e-3)
    averaged = AveragedModel(bag, multi_avg_fn=get_ema_multi_avg_fn(decay))
    averaged.update_parameters(bag)            # its first call copies: the state WeightEMA starts from
    opt = FusedAdam(model.parameters(), lr=2e-3)
    trainer = Trainer(None, model, None, opt, None, bfloat16=False)
    for i in range(3):
        images, mask, offs = g["images"][i], g["mask"][i].copy(), g["offsets"][i]
        model.backbone.set_offsets(offs)
        loss = float(trainer.train_step_prepared(torch.from_numpy(images).cuda(), None, mask))
        teacher = {k: p.detach() for k, p in zip(bkeys, averaged.module.ps)}
        ropt.zero_grad()
        ref = LR.latent_step(student, teacher, images, mask, 4, 2, 2.0, 1e-5, offs)[0]
        ref.backward()
        ropt.step()
        averaged.update_parameters(bag)
        print(f"\nlatent trajectory step {i}: loss {loss:.8f} f64 {float(ref):.8f}")
        assert abs(loss - float(ref)) < 1e-4 * abs(float(ref)), (i, loss, float(ref))
    assert model.ema.n_updates == 3

    def close(got, want, k):
        got, want = got.detach().cpu().double().numpy(), want.detach().numpy()
        if k.endswith("in_proj_bias"):  # key-bias slice: mathematically zero gradient, Adam amplifies rounding noise
            d = got.shape[0] // 3
            got, want = np.delete(got, np.s_[d:2 * d]), np.delete(want, np.s_[d:2 * d])
        assert np.abs(got - want).max() < 5e-4, (k, np.abs(got - want).max())

    for k, v in model.state_dict().items():
        close(v, student[k], k)
    for (k, v), want in zip(model.teacher.state_dict().items(), averaged.module.ps):
        close(v, want, "teacher." + k)


def test_weight_ema_bf16_copies_and_a_bf16_step(golden):
    import pero_pretraining_amd as P
    from pero_pretraining_amd import lowp
    from pero_pretraining_amd.optim import FusedAdam
    g = golden("g4_masked_tiny.npz")
    model = build(top_k=2, decay=0.5).train()
    model.after_step()                             # the table over the student's own allocations
    ptrs0 = list(model.ema._ptrs)
    opt = FusedAdam(model.parameters(), lr=1e-2)   # flattens the student: its addresses change, the EMA's table follows
    with torch.no_grad():
        for p in model.backbone.parameters():
            p.add_(0.05)
    before = bits(model.teacher)
    model.after_step()
    assert model.ema.n_updates == 2 and model.ema._ptrs != ptrs0
    for p, old, src in zip(model.teacher.parameters(), before, model.backbone.parameters()):
        assert torch.equal(p.detach(), old + 0.5 * (src.detach() - old))     # a + w (p - a) in f32, w = 0.5
        assert torch.equal(lowp.get(p), p.detach().to(torch.bfloat16))       # the copy a bf16 forward reads is what the kernel wrote
    images, mask, offs = torch.from_numpy(g["images"]).cuda(), g["mask"].copy(), g["train_offsets"]
    model.backbone.set_offsets(offs)
    l32 = float(model(images, None, mask)["loss"])
    opt.zero_grad()
    model.backbone.set_offsets(offs)
    with P.autocast(True):
        res = model(images, None, mask)
    assert res["output_rows"].dtype == torch.bfloat16 and res["targets"].dtype == torch.float32
    res["loss"].backward()
    opt.step()
    model.after_step()
    lbf = float(res["loss"])
    print(f"\nlatent step bf16: loss {lbf:.6f} f32 {l32:.6f} (relative difference {abs(lbf - l32) / abs(l32):.2e}, bound 3e-2)")
    assert np.isfinite(lbf) and abs(lbf - l32) <= 3e-2 * abs(l32), (lbf, l32)
    for p in model.teacher.parameters():
        assert torch.equal(lowp.get(p), p.detach().to(torch.bfloat16))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_checkpoint_round_trip_and_the_recogniser_reads_it(golden, tmp_path):
    from pero_pretraining_amd.latent_pretraining import model as M
    from pero_pretraining_amd.recognition import model as RM
    model = build(seed=3, decay=0.99, decay_start=0.9, ramp_updates=10)
    detune_teacher(model)
    model.ema.n_updates = 7
    path = str(tmp_path / "latent.pth")
    model.save(path)
    other = M.init_model(torch.device("cuda", 0), dict(CFG), {"type": "linear", "in_features": 64, "out_features": 64}, path=path)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), other.state_dict().values()))
    assert all(torch.equal(a, b) for a, b in zip(model.teacher.state_dict().values(), other.teacher.state_dict().values()))
    assert (other.ema.n_updates, other.ema.decay, other.ema.decay_start, other.ema.ramp_updates) == (7, 0.99, 0.9, 10)
    assert other.ema.decay_at(7) == LR.ema_decay(7, 0.99, 0.9, 10)
    keys = set(torch.load(path, weights_only=True))
    assert {"backbone.conv_layer.weight", "head.linear.weight", "teacher.conv_layer.weight", "teacher.n_updates"} <= keys
    rec = RM.init_model(torch.device("cuda", 0), dict(CFG), {"type": "linear", "in_features": 64, "out_features": 40})
    rec.load_pretrained_backbone(path)
    assert all(torch.equal(a, b) for a, b in zip(rec.backbone.state_dict().values(), model.backbone.state_dict().values()))


def test_attend_valid_only_makes_a_line_independent_of_the_padding(golden):
    g = golden("g4_masked_tiny.npz")
    model = build(top_k=2).eval()
    detune_teacher(model)
    model.attend_valid_only = True
    rng = np.random.default_rng(4)
    line = g["images"][:1]                                             # one line, 16 positions
    mask = np.zeros((1, 16), dtype=np.int64)
    mask[0, [2, 3, 9]] = 1
    valid = np.ones((1, 16), dtype=np.int64)
    base = float(model(torch.from_numpy(line).cuda(), valid, mask)["loss"])
    pad = rng.integers(0, 256, (1, 40, 64, 3), dtype=np.uint8)         # 8 padding positions of other pixels
    wide = np.concatenate([line, pad], axis=2)
    wmask, wvalid = np.concatenate([mask, np.zeros((1, 8), np.int64)], 1), np.concatenate([valid, np.zeros((1, 8), np.int64)], 1)
    padded = float(model(torch.from_numpy(wide).cuda(), wvalid, wmask)["loss"])
    # the same f64 value evaluated twice in f32 with the sums of the attention and of the products grouped for another batch width: each of
    # the ~100 roundings between the pixels and the loss moves it by at most 2^-24 relative; 1e-5 is 100 * 2^-24 with headroom
    print(f"\nattend_valid_only: loss {base:.9f}, with 8 padding positions {padded:.9f} (relative difference {abs(padded - base) / abs(base):.2e}, bound 1e-5)")
    assert abs(padded - base) <= 1e-5 * abs(base), (base, padded)
    model.attend_valid_only = False
    assert abs(float(model(torch.from_numpy(wide).cuda(), wvalid, wmask)["loss"]) - base) > 1e-4 * abs(base)   # the padding is attended to


def test_tester_returns_loss_and_the_collapse_monitor(golden):
    from pero_pretraining_amd.latent_pretraining.batch_operator import BatchOperator
    from pero_pretraining_amd.latent_pretraining.tester import Tester
    g = golden("g4_masked_tiny.npz")
    model = build(top_k=2).train()
    detune_teacher(model)
    batches = [{"images": g["images"], "labels": g["labels"]}, {"images": g["images"][::-1].copy(), "labels": g["labels"][::-1].copy()}]
    bop = BatchOperator(torch.device("cuda", 0), 0.3, mask_span=2)
    np.random.seed(8)
    result = Tester(bop, model, batches).test()
    assert set(result) == {"loss", "target_std"} and model.training
    np.random.seed(8)
    student, teacher = f64_sds(model)
    losses, targets = [], []
    for b in batches:
        mask = bop._create_mask(b)
        loss, t, _, _ = LR.latent_step(student, teacher, b["images"], mask, 4, 2, 2.0, 1e-5)
        losses.append(float(loss))
        targets.append(t)
    want = LR.target_std(torch.cat(targets))
    print(f"\nlatent tester: loss {result['loss']:.8f} f64 {np.mean(losses):.8f}; target_std {result['target_std']:.8f} f64 {want:.8f}")
    assert abs(result["target_std"] - want) <= 1e-5 * want
    assert abs(result["loss"] - np.mean(losses)) < 1e-4 * np.mean(losses)


def test_encode_layers_taps_and_leaves_the_plain_forward_alone(golden):
    g = golden("g4_masked_tiny.npz")
    model = build().eval()
    bb = model.backbone
    x = torch.from_numpy(g["images"]).cuda()
    with torch.no_grad():
        tokens = bb.encode_tokens(x)
    taps = bb.encode_layers(x, [-1, 0, 1, -2])
    assert [t.shape for t in taps] == [tokens.shape] * 4
    assert torch.equal(taps[0], tokens) and torch.equal(taps[2], tokens)        # the top layer's matrix is the backbone's output, bit for bit
    assert torch.equal(taps[1], taps[3]) and not torch.equal(taps[1], tokens)   # negative indices count from the top
    sd = {"backbone." + k: v.detach().cpu().double() for k, v in bb.state_dict().items()}
    ref = LR.backbone_layers(sd, O.prepare_images(torch.from_numpy(g["images"])).double(), 4)
    for got, want in ((taps[1], ref[0]), (taps[0], ref[1])):
        assert float((got.cpu().double() - want).abs().max()) < 1e-4
    with pytest.raises(ValueError, match="encode_layers"):
        bb.encode_layers(x, [2])
    # injected offsets are consumed exactly as encode_tokens consumes them
    bb.train()
    bb.set_offsets(g["train_offsets"], g["train_offsets"])
    with torch.no_grad():
        a = bb.encode_tokens(x)
    b = bb.encode_layers(x, [-1])[0]
    assert torch.equal(a, b) and not torch.equal(a, tokens) and not bb.position_model._next_offsets


def test_weight_ema_of_a_recogniser_serves_its_tester(golden):
    """WeightEMA on its own: the average of a recogniser evaluates through recognition.Tester like the recogniser itself."""
    from pero_pretraining_amd.optim import WeightEMA
    from pero_pretraining_amd.recognition import model as RM
    from pero_pretraining_amd.recognition.batch_operator import BatchOperator
    from pero_pretraining_amd.recognition.tester import Tester
    g = golden("g4_masked_tiny.npz")
    torch.manual_seed(5)
    rec = RM.init_model(torch.device("cuda", 0), dict(CFG), {"type": "linear", "in_features": 64, "out_features": 12})
    ema = WeightEMA(rec, decay=0.75)
    n, s = g["images"].shape[0], g["images"].shape[2] // 8
    rng = np.random.default_rng(6)
    batch = {"images": g["images"], "targets": rng.integers(1, 12, (n, 5)), "target_lengths": np.full(n, 5), "widths": np.full(n, s * 8)}
    bop = BatchOperator(torch.device("cuda", 0))
    same = Tester(bop, ema.module, [batch]).test()
    own = Tester(bop, rec, [batch]).test()
    assert float(same["loss"]) == float(own["loss"]) and same["cer"] == own["cer"]     # a fresh average is a copy
    with torch.no_grad():
        for p in rec.parameters():
            p.mul_(1.5)
    before = bits(ema.module)
    ema.update()
    for p, old, src in zip(ema.module.parameters(), before, rec.parameters()):
        assert torch.equal(p.detach(), old + 0.25 * (src.detach() - old))
    moved = Tester(bop, ema.module, [batch]).test()
    assert np.isfinite(float(moved["loss"])) and float(moved["loss"]) != float(own["loss"])
    state = ema.state_dict()
    ema2 = WeightEMA(copy.deepcopy(rec))
    ema2.load_state_dict(state)
    assert ema2.n_updates == 1 and ema2.decay == 0.75
    assert all(torch.equal(a, b) for a, b in zip(ema.module.state_dict().values(), ema2.module.state_dict().values()))
