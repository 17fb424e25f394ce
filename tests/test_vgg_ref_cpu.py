"""CPU side of the VGG tokenizer front end: tests/vgg_ref.py (the f64 restatement the GPU tests compare against) is pinned to the
reference's own output (tests/golden/g30_vgg_encoder.npz, tools/make_golden_vgg.py), and VGGEncoder's constructor, state dict and
refusals are checked without a GPU."""
import os

import numpy as np
import pytest
import torch

import vgg_ref as V
from pero_pretraining_amd.models.autoencoders import VGGEncoder, VQVAETokenizer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g30_vgg_encoder.npz")


@pytest.fixture(scope="module")
def g30():
    z = np.load(GOLDEN)
    return z, {str(k): torch.from_numpy(z["param." + str(k)]) for k in z["names"]}


def test_restatement_reproduces_the_reference_output(g30):
    z, state = g30
    out, outs = V.encoder_forward(state, torch.from_numpy(z["images"]))
    ref = torch.from_numpy(z["output"]).double()
    scale = float(ref.abs().max())
    err = float((out - ref).abs().max())
    print(f"feature scale {scale:.3f}, |f64 restatement - reference (f32)| max {err:.3e}")
    assert out.shape == ref.shape and scale > 1.0
    assert err <= 1e-5 * scale
    # every layer's shape: the reference's modules are Conv2d, ReLU, ..., Sequential(pool ...); the restatement has one output per conv / pool
    shapes = {str(n): tuple(int(v) for v in s) for n, s in zip(z["layer_names"], z["layer_shapes"])}
    for step, y in zip(V.stack(), outs[1:]):
        name = f"encoder.{step[1] + 1}" if step[0] == "conv" else f"encoder.{step[1]}"     # a conv's ReLU keeps the shape
        assert tuple(y.shape) == shapes[name], (step, tuple(y.shape), shapes[name])
    assert tuple(outs[-1].shape) == shapes["aggregation_layer"]


def test_constructs_with_the_reference_names_and_loads_strictly(g30):
    z, state = g30
    enc = VGGEncoder(pretrained_vgg_layers=0, base_channels=int(z["base_channels"]))
    own = enc.state_dict()
    assert list(own) == [str(k) for k in z["names"]]
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in state.items()}
    assert {k: tuple(v.shape) for k, v in own.items()} == V.encoder_shapes(int(z["base_channels"]))
    enc.load_state_dict(state, strict=True)
    assert enc.out_channels == int(z["out_channels"]) and enc.height == 40 and enc.patch_size == (40, 8) and enc.aggregation == "conv"
    assert enc.subsampling() == (8, 8) and enc.max_workspace_bytes == 2 << 30
    default = VGGEncoder()
    assert "encoder.16.1.running_var" in default.state_dict() and default.out_channels == 256 and default.pretrained_vgg_layers == 0
    assert tuple(default.aggregation_layer.weight.shape) == (256, 256, 5, 1)
    VGGEncoder(dropout=0.1)     # accepted: dropout is the identity in inference


def test_four_blocks_end_in_a_2x1_pool():
    enc = VGGEncoder(height=48, base_channels=4, num_conv_blocks=4, num_conv_layers=(2, 2, 3, 2))
    pools = [s[2] for s in enc.steps() if s[0] == "pool"]
    assert pools == [(2, 2), (2, 2), (2, 2), (2, 1)] and enc.subsampling() == (16, 8)
    assert [s[2] for s in V.stack(4, (2, 2, 3, 2)) if s[0] == "pool"] == pools
    assert enc.steps()[-1][3] is not None and all(s[3] is None for s in enc.steps()[:-1] if s[0] == "pool")    # BatchNorm in the last block only
    assert enc.out_channels == 32 and tuple(enc.aggregation_layer.weight.shape) == (32, 32, 3, 1)


def test_refusals():
    with pytest.raises(ValueError, match="checkpoint"):
        VGGEncoder(pretrained_vgg_layers=17)
    enc = VGGEncoder(base_channels=4)
    images = torch.zeros((1, 40, 32, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no_grad"):
        enc(images)                                           # gradients enabled, parameters require them
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU only"):
        enc(images)                                           # a CPU tensor
    tok = VQVAETokenizer(enc, num_embeddings=8, embeddings_dim=4)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU only"):
        tok.labels(images)
    assert [k for k in tok.state_dict() if k.startswith("encoder.")] == ["encoder." + k for k in enc.state_dict()]


def test_tokenizer_load_skips_only_the_decoder(g30):
    z, state = g30
    tok = VQVAETokenizer(VGGEncoder(base_channels=int(z["base_channels"])), num_embeddings=8, embeddings_dim=4, decoder_channels=16)
    ckpt = {k: v.clone() for k, v in tok.state_dict().items()}
    ckpt.update({"encoder." + k: v for k, v in state.items()})
    ckpt["decoder.decoder.0.weight"] = torch.zeros(3)
    tok.load(ckpt)
    assert torch.equal(tok.encoder.encoder[0].weight, state["encoder.0.weight"])
    ckpt["unexpected.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        tok.load(ckpt)


def test_label_case_satisfies_its_exclusion_cap_in_f64():
    case = V.label_case()
    margin, labels = case["margin"], case["labels"]
    excluded = int((margin < V.LABEL_MARGIN).sum())
    print(f"rows {margin.numel()}, excluded {excluded}, smallest margin {float(margin.min()):.3e}, distinct labels {labels.unique().numel()}")
    assert margin.numel() == 198
    assert excluded <= V.LABEL_MAX_EXCLUDED * margin.numel()
    assert labels.unique().numel() >= V.LABEL_MIN_DISTINCT and int(labels.max()) < V.LABEL_DRAWN
