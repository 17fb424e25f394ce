"""GPU: models.autoencoders.VGGEncoder / VQVAETokenizer end to end, on the fixture's encoder (tests/golden/g30_vgg_encoder.npz: base 8,
uint8 (3, 40, 72, 3)) and on a base-16 encoder with a (6, 40, 264, 3) input (tests/vgg_ref.py label_case).

* Teacher-forced chain: every layer's stored output is fed to the f64 restatement of the NEXT layer and compared with the module's next
  output under parity_ref.assert_within (n_terms = 9 Cin + 1 / 2 / h C + 1), so no tolerance compounds.  bf16: the restatement uses the
  bf16-rounded weights the module uses.
* End to end, f32: |module - f64| <= 8 x max |restatement in torch CPU f32 - restatement in f64| on the same input and weights, computed
  here.  (The kernel adds up to 9 Cin terms in another order than torch's CPU convolution, and the two errors can add; a wrong tap, halo
  or channel is five orders larger.)  The fixture's reference output is held to the same bound.
* Labels, f32: equal to the f64 argmin on every row whose f64 relative margin is >= 1e-3; at most 5 % of the rows left out, at least 16
  distinct labels.  The share of labels bf16 mode gives differently is printed, not asserted.
Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_ref as P  # noqa: E402
import vgg_ref as V  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g30_vgg_encoder.npz")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
_cache = {}


def setup(name):
    """(module on the GPU, state, uint8 images, f64 features, f32-vs-f64 difference of the CPU restatement) - built once, never modified."""
    if name in _cache:
        return _cache[name]
    from pero_pretraining_amd.models.autoencoders import VGGEncoder
    if name == "fixture":
        z = np.load(GOLDEN)
        state = {str(k): torch.from_numpy(z["param." + str(k)]) for k in z["names"]}
        images, base = torch.from_numpy(z["images"]), int(z["base_channels"])
        ref64 = V.encoder_forward(state, images)[0]
    else:
        case = V.label_case()
        state, images, base, ref64 = case["state"], case["images"], V.LABEL_BASE_CHANNELS, case["features"]
    enc = VGGEncoder(base_channels=base)
    enc.load_state_dict(state, strict=True)
    ref32 = V.encoder_forward(state, images, dtype=torch.float32)[0]
    _cache[name] = (enc.cuda().eval(), state, images, ref64, float((ref32.double() - ref64).abs().max()))
    return _cache[name]


def as_nchw(kind, tensor, n, c):
    if tensor.dim() == 2:
        return V.from_token_rows(tensor, n, c)
    return V.from_halo(tensor)[0]


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("name", ["fixture", "base16"])
def test_teacher_forced_chain(name, mode):
    from pero_pretraining_amd import precision
    enc, state, images, _, _ = setup(name)
    dtype = DTYPES[mode]
    if mode == "bf16":      # the operands the module multiplies with
        state = {k: (v.bfloat16().float() if v.dim() == 4 else v) for k, v in state.items()}
    trace = []
    with torch.no_grad(), precision.autocast(mode == "bf16"):
        out = enc(images.cuda(), trace=trace)
    torch.cuda.synchronize()
    n, steps = images.shape[0], V.stack()
    assert [t[0] for t in trace] == ["ingest"] + [s[0] for s in steps] + ["aggregation"]
    assert all(t[2].dtype == dtype for t in trace[:-1]) and trace[-1][2].dtype == torch.float32 and out.dtype == torch.float32
    x, border = V.from_halo(trace[0][2])
    ingested = V.ingest(images)
    assert x.shape[1] == (8 if mode == "bf16" else 4) and not bool(x[:, 3:].any())      # zero channels pad a pixel to 16 bytes
    x = x[:, :3].contiguous()
    P.assert_within(x, ingested, ingested.abs(), 1, dtype, what="vgg ingest")
    assert not bool(border.any())
    for step, (kind, index, got) in zip(steps, trace[1:-1]):
        ref, mag, n_terms = V.layer(step, x, state)
        if got.dim() == 4:
            assert not bool(V.from_halo(got)[1].any()), f"{kind} {index}: halo pixels must be zeros"
        got = as_nchw(kind, got, n, ref.shape[1])
        worst = P.assert_within(got, ref, mag, n_terms, dtype, what=f"vgg {kind}")
        print(f"{name} {mode} {kind} {index} {tuple(ref.shape)}: worst error / bound {worst:.3f}")
        x = got                                                   # teacher forcing: the module's own output feeds the next restatement
    ref, mag, n_terms = V.aggregation(x, state)
    rows = trace[-1][2].double().cpu()
    got = rows.reshape(n, -1, rows.shape[1]).permute(0, 2, 1).unsqueeze(2)
    worst = P.assert_within(got, ref, mag, n_terms, torch.float32, what="vgg aggregation")
    print(f"{name} {mode} aggregation {tuple(ref.shape)}: worst error / bound {worst:.3f}")
    assert torch.equal(out.double().cpu(), got)
    print({k: round(v, 3) for k, v in P.RATIOS.items() if k.startswith("vgg")})


@pytest.mark.parametrize("name", ["fixture", "base16"])
def test_end_to_end_f32(name):
    enc, state, images, ref64, cpu_diff = setup(name)
    with torch.no_grad():
        out = enc(images.cuda())
        nchw = (images.double() / 255.0).float().permute(0, 3, 1, 2).contiguous()       # autoencoders/batch_operator.py:14-16
        out_nchw = enc(nchw.cuda())
        enc.max_workspace_bytes, keep = 1, enc.max_workspace_bytes
        try:
            assert enc.lines_per_chunk(40, images.shape[2], torch.float32) == 1
            out_lines = enc(images.cuda())
        finally:
            enc.max_workspace_bytes = keep
    torch.cuda.synchronize()
    assert tuple(out.shape) == (images.shape[0], enc.out_channels, 1, images.shape[2] // 8) and out.dtype == torch.float32
    scale, bound = float(ref64.abs().max()), 8.0 * cpu_diff
    err = float((out.double().cpu() - ref64).abs().max())
    print(f"{name}: feature scale {scale:.3f}, CPU f32 - f64 {cpu_diff:.3e}, bound {bound:.3e}, |module - f64| {err:.3e} (ratio {err / bound:.3f})")
    assert err <= bound
    if name == "fixture":
        fix = float((out.double().cpu() - torch.from_numpy(np.load(GOLDEN)["output"]).double()).abs().max())
        print(f"fixture: |module - reference output| {fix:.3e} (ratio {fix / bound:.3f})")
        assert fix <= bound
    assert torch.equal(out, out_nchw), "uint8 NHWC and the equivalent float NCHW input must give the same bits"
    assert torch.equal(out, out_lines), "the result must not depend on the chunk size"


def test_geometry_is_checked():
    enc = setup("fixture")[0]
    with torch.no_grad():
        with pytest.raises(ValueError, match="divisible"):
            enc(torch.zeros((1, 40, 36, 3), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError, match="height"):
            enc(torch.zeros((1, 32, 64, 3), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError, match="uint8"):
            enc(torch.zeros((1, 3, 40, 64), dtype=torch.float64, device="cuda"))


def tokenizer():
    if "tokenizer" in _cache:
        return _cache["tokenizer"]
    from pero_pretraining_amd.models.autoencoders import VQVAETokenizer
    case = V.label_case()
    tok = VQVAETokenizer(setup("base16")[0], num_embeddings=V.LABEL_CODES, embeddings_dim=V.LABEL_DIM).cuda().eval()
    with torch.no_grad():
        tok.encoder_projection_layer.weight.copy_(case["proj_w"])
        tok.encoder_projection_layer.bias.copy_(case["proj_b"])
        tok.vq.embedding.weight.copy_(case["codebook"])
    _cache["tokenizer"] = tok
    return tok


def test_labels_f32_and_bf16_share():
    from pero_pretraining_amd import precision
    case, tok = V.label_case(), tokenizer()
    images = case["images"].cuda()
    labels = tok.labels(images).cpu()
    with precision.autocast(True):
        labels_bf16 = tok.labels(images).cpu()
    keep = case["margin"] >= V.LABEL_MARGIN
    left_out, distinct = int((~keep).sum()), int(labels.unique().numel())
    wrong = int((labels[keep] != case["labels"][keep]).sum())
    share = float((labels_bf16 != labels).double().mean())
    print(f"labels: {labels.numel()} rows, {left_out} left out (margin < {V.LABEL_MARGIN}), {wrong} differ from the f64 argmin, {distinct} distinct; "
          f"bf16 mode differs from f32 mode on {share:.4f} of the rows")
    assert labels.dtype == torch.int64 and labels.shape == case["labels"].shape
    assert left_out <= V.LABEL_MAX_EXCLUDED * labels.numel()
    assert wrong == 0
    assert distinct >= V.LABEL_MIN_DISTINCT


def test_label_scripts_with_the_in_project_encoder(tmp_path):
    from pero_pretraining_amd.scripts import labels as L
    case, tok = V.label_case(), tokenizer()
    ckpt = dict(tok.state_dict())
    ckpt["decoder.decoder.0.weight"] = torch.zeros(4)             # a reference VQVAE checkpoint also holds its decoder
    torch.save(ckpt, tmp_path / "vqvae.pth")
    loaded = L.init_tokenizer(torch.device("cuda"), {"base_channels": V.LABEL_BASE_CHANNELS}, V.LABEL_CODES, V.LABEL_DIM, path=str(tmp_path / "vqvae.pth"))
    assert not loaded.training and all(torch.equal(a, b) for a, b in zip(loaded.state_dict().values(), tok.state_dict().values()))
    images = case["images"]
    t = images.shape[2] // 8
    rng = np.random.default_rng(4)
    dataset = []
    for b in range(2):
        masks = (rng.random((3, t)) < 0.8).astype(np.uint8)
        masks[0, 0] = 1
        dataset.append({"ids": [f"line_{b}_{i}.jpg" for i in range(3)], "image_masks": masks, "images": images[3 * b:3 * b + 3].cuda()})
    direct = loaded.labels(images.cuda()).reshape(6, t).cpu().numpy()
    data = L.compute_labels(loaded.encode, loaded, dataset)
    expect = {line_id: direct[3 * b + i][batch["image_masks"][i] == 1].tolist() for b, batch in enumerate(dataset) for i, line_id in enumerate(batch["ids"])}
    assert data == expect
    L.save_labels(data, str(tmp_path / "labels.txt"))
    lines = (tmp_path / "labels.txt").read_text().splitlines()
    assert lines[0] == "line_0_0.jpg " + " ".join(str(v) for v in expect["line_0_0.jpg"]) and len(lines) == 6
    assert [L.parse_line(l)[0] for l in lines] == list(expect)
    feats = L.compute_features(loaded.encoder, dataset)
    with torch.no_grad():
        whole = loaded.encoder(images.cuda()).squeeze(2).permute(0, 2, 1).cpu().numpy()          # (6, t, D)
    valid = np.concatenate([b["image_masks"] for b in dataset], 0) == 1
    # three lines per call here, six above: the aggregation product has other row counts, the convolutions see the same rows
    assert feats.is_cuda and feats.dtype == torch.float32 and tuple(feats.shape) == (int(valid.sum()), loaded.encoder.out_channels)
    assert np.allclose(feats.cpu().numpy(), whole[valid], rtol=0, atol=1e-5 * float(np.abs(whole).max()))
    centroids = torch.from_numpy(whole[valid][:7].copy()).cuda()
    assert L.compute_kmeans_labels(loaded.encoder, centroids, dataset, str(tmp_path / "km.txt")) == 6
    assert len((tmp_path / "km.txt").read_text().splitlines()) == 6
