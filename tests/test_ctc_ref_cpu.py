"""CPU: the CTC entry points are exported and bound; tests/ctc_ref.py (the f64 restatement the GPU tests compare against) agrees
with torch.nn.functional.ctc_loss in f64 on every case of the GPU list - losses under the three reductions and the gradients with
respect to the logits through torch autograd; its greedy decode and the Levenshtein helper are pinned by hand; a pre-training
checkpoint's backbone loads into a recogniser."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_ref  # noqa: E402

NAMES = ("pero_ctc_fwd", "pero_ctc_bwd", "pero_ctc_greedy")


def test_library_exports_and_binds_the_ctc_entry_points():
    from pero_pretraining_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    h = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    assert h.pero_abi_version() == _lib.ABI_VERSION == 2


def test_ctc_entry_points_validate_arguments_without_gpu():
    """Outside the supported range the host refuses before any launch: PERO_E_UNSUPPORTED above S = 512 / C = 8192, PERO_E_INVALID else."""
    import ctypes
    from pero_pretraining_amd import _lib
    h = _lib.lib()
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    fwd = lambda N, S, C, Lmax, blank, dtype=0: h.pero_ctc_fwd(buf, buf, buf, buf, buf, buf, buf, N, S, C, Lmax, blank, dtype, None)  # noqa: E731
    assert fwd(1, 513, 4, 2, 0) == -2 and b"512" in h.pero_last_error()
    assert fwd(1, 8, 8193, 2, 0) == -2
    assert fwd(1, 8, 1, 2, 0) == -1            # C >= 2
    assert fwd(1, 8, 4, 513, 0) == -2          # Lmax <= 512 (it may exceed S: a padded target matrix)
    assert fwd(1, 8, 4, -1, 0) == -1
    assert fwd(1, 8, 4, 2, 4) == -1 and b"blank" in h.pero_last_error()
    assert fwd(1, 8, 4, 2, 0, dtype=7) == -1
    assert h.pero_ctc_fwd(None, buf, buf, buf, buf, buf, buf, 1, 8, 4, 2, 0, 0, None) == -1
    assert h.pero_ctc_bwd(buf, buf, buf, buf, buf, buf, buf, None, buf, buf, buf, 1, 8, 4, 2, 0, 0, 0, None) == -1
    assert h.pero_ctc_greedy(buf, buf, buf, buf, 1, 600, 4, 0, 0, None) == -2


def _torch_oracle(c, reduction, zero_infinity):
    x = c["logits"].double().requires_grad_(True)
    C = x.shape[-1]
    tg = torch.where(c["targets"] == ctc_ref.SENTINEL, torch.zeros_like(c["targets"]), c["targets"])   # torch gets valid padding, ctc_ref the sentinel
    assert int(tg.max()) < C
    loss = torch.nn.functional.ctc_loss(torch.log_softmax(x, -1).transpose(0, 1), tg, c["input_lengths"], c["target_lengths"], blank=c["blank"],
                                        reduction=reduction, zero_infinity=zero_infinity)
    return x, loss


@pytest.mark.parametrize("name", list(ctc_ref.CASES))
def test_ctc_ref_matches_torch_f64(name):
    c = ctc_ref.case(name)
    N = c["logits"].shape[0]
    res, mag = ctc_ref.ctc(c["logits"], c["targets"], c["input_lengths"], c["target_lengths"], c["blank"], zero_infinity=True)
    feasible = [n for n in range(N) if n not in c["infeasible"]]
    assert all(math.isinf(float(res["nll"][n])) and float(res["nll"][n]) > 0 for n in c["infeasible"])
    assert bool(torch.isfinite(res["nll"][feasible]).all())
    for reduction in ("none", "sum", "mean"):
        for zero_infinity in (True, False):
            x, loss = _torch_oracle(c, reduction, zero_infinity)
            got = ctc_ref.reduce(res["nll"], c["target_lengths"], reduction, zero_infinity)
            torch.testing.assert_close(got, loss.detach(), rtol=1e-12, atol=0, equal_nan=False)
    # gradients with respect to the logits, with a distinct upstream scale per line (one of them 0)
    g = torch.linspace(-1.0, 2.0, N, dtype=torch.float64)
    g[1] = 0.0
    res, mag = ctc_ref.ctc(c["logits"], c["targets"], c["input_lengths"], c["target_lengths"], c["blank"], g=g, zero_infinity=True)
    x, loss = _torch_oracle(c, "none", True)
    (loss * g).sum().backward()
    torch.testing.assert_close(res["grad"], x.grad, rtol=1e-12, atol=1e-300 + 1e-12 * float(mag["grad"].max()))
    for n in range(N):
        T = int(c["input_lengths"][n])
        assert not res["grad"][n, T:].any()
    for n in c["infeasible"]:
        assert not res["grad"][n].any()
    # without zero_infinity the infeasible line's rows are unspecified (NaN here, as in torch); the others do not change
    res2, _ = ctc_ref.ctc(c["logits"], c["targets"], c["input_lengths"], c["target_lengths"], c["blank"], g=g, zero_infinity=False)
    assert torch.equal(res2["grad"][feasible], res["grad"][feasible])
    # alpha and beta meet: logsumexp_s(alpha_t(s) + beta_t(s) - emission_t(s)) = -nll at every t
    for n in feasible:
        T, L = int(c["input_lengths"][n]), int(c["target_lengths"][n])
        if T == 0:
            continue
        ext = ctc_ref.extended(c["targets"][n], L, c["blank"])
        lp = torch.log_softmax(c["logits"][n, :T].double(), -1)[:, ext]
        tot = torch.logsumexp(res["alpha"][n] + res["beta"][n] - lp, dim=1)
        torch.testing.assert_close(tot, -res["nll"][n].expand(T), rtol=1e-12, atol=1e-12)


def test_single_path_line_is_the_sum_of_its_log_probabilities():
    c = ctc_ref.case("mixed-C37-blank0-x4")
    res, _ = ctc_ref.ctc(c["logits"], c["targets"], c["input_lengths"], c["target_lengths"], c["blank"])
    lp = torch.log_softmax(c["logits"][4].double(), -1)
    want = -lp[torch.arange(24), c["targets"][4, :24]].sum()
    torch.testing.assert_close(res["nll"][4], want, rtol=1e-12, atol=0)


def test_error_budget_sits_between_f32_noise_and_a_wrong_answer():
    """The derived nll bound at the issue's yardstick (C = 37, logits 4 randn, T = 24): above what torch's own f32 ctc_loss is away from f64
    (3e-6 .. 4e-5), far below 1e-2; torch's f32 result itself passes it."""
    from parity_ref import U32
    c = ctc_ref.case("mixed-C37-blank0-x4")
    res, mag = ctc_ref.ctc(c["logits"], c["targets"], c["input_lengths"], c["target_lengths"], c["blank"])
    bound = mag["nll_terms"] * U32 * mag["nll"]
    fin = torch.isfinite(res["nll"])
    assert float(bound[fin].min()) > 4e-5 and float(bound[fin].max()) < 5e-3, bound
    tg = torch.where(c["targets"] == ctc_ref.SENTINEL, torch.zeros_like(c["targets"]), c["targets"])
    f32 = torch.nn.functional.ctc_loss(torch.log_softmax(c["logits"].float(), -1).transpose(0, 1), tg, c["input_lengths"], c["target_lengths"],
                                       blank=c["blank"], reduction="none")
    assert bool(((f32.double() - res["nll"]).abs()[fin] <= bound[fin]).all())


def _greedy_loop(x, input_lengths, blank):
    out = []
    for n in range(x.shape[0]):
        line, last = [], None
        for t in range(int(input_lengths[n])):
            row = x[n, t].tolist()
            c = row.index(max(row))
            if c != last and c != blank:
                line.append(c)
            last = c
        out.append(line)
    return out


def test_ctc_ref_greedy_matches_a_python_loop():
    x, il, blank = ctc_ref.greedy_case()
    for b in (blank, 6):
        out, lengths = ctc_ref.greedy(x, il, b)
        want = _greedy_loop(x, il, b)
        assert lengths.tolist() == [len(w) for w in want]
        for n, w in enumerate(want):
            assert out[n, :len(w)].tolist() == w and bool((out[n, len(w):] == -1).all())
    out, lengths = ctc_ref.greedy(x, il, 0)
    assert out[0, :2].tolist() == [2, 2] and out[1, :1].tolist() == [3] and int(lengths[1]) == 1 and int(lengths[3]) == 0


def test_levenshtein_on_hand_checked_pairs():
    from pero_pretraining_amd.recognition import levenshtein
    pairs = [((), (), 0), ((1, 2, 3), (), 3), ((), (4,), 1), ((1, 2, 3), (1, 2, 3), 0), ((1, 2, 3), (1, 9, 3), 1), ((1, 2, 3), (1, 3), 1),
             ((1, 3), (1, 2, 3), 1), (tuple("kitten"), tuple("sitting"), 3), (tuple("flaw"), tuple("lawn"), 2), ((1, 2), (2, 1), 2)]
    for a, b, d in pairs:
        assert levenshtein(list(a), list(b)) == d == ctc_ref.levenshtein(a, b), (a, b)
        assert levenshtein(list(b), list(a)) == d


def test_pretrained_backbone_loads_into_a_recogniser(tmp_path):
    from pero_pretraining_amd.masked_pretraining import model as M
    from pero_pretraining_amd.recognition import TransformerRecognizer
    definition = {"type": "vit", "num_blocks": 1, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128}
    torch.manual_seed(1)
    pre = M.MaskedTransformerEncoder(M.init_backbone(dict(definition)), M.init_head({"type": "linear", "in_features": 64, "out_features": 96}))
    path = str(tmp_path / "checkpoint.pth")
    pre.save(path)
    torch.manual_seed(2)
    rec = TransformerRecognizer(M.init_backbone(dict(definition)), M.init_head({"type": "linear", "in_features": 64, "out_features": 37}))
    head_before = {k: v.clone() for k, v in rec.head.state_dict().items()}
    assert not all(torch.equal(v, pre.backbone.state_dict()[k]) for k, v in rec.backbone.state_dict().items())   # two different initialisations
    rec.load_pretrained_backbone(path)
    want = pre.backbone.state_dict()
    got = rec.backbone.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert all(torch.equal(v, head_before[k]) for k, v in rec.head.state_dict().items()) and rec.head.linear.weight.shape == (37, 64)
    # strict: a checkpoint without the backbone's tensors is refused
    torch.save({"head.linear.weight": torch.zeros(3, 3)}, path)
    with pytest.raises(RuntimeError):
        rec.load_pretrained_backbone(path)


def test_ctc_loss_module_is_validated_on_the_host():
    from pero_pretraining_amd._lib import PeroHipError
    from pero_pretraining_amd.recognition import BatchOperator, CTCLoss
    with pytest.raises(ValueError, match="Unknown reduction"):
        CTCLoss(reduction="batchmean")
    with pytest.raises(ValueError, match="blank"):
        CTCLoss(blank=5)(torch.zeros(1, 4, 5), torch.zeros(1, 2), torch.tensor([4]), torch.tensor([2]))
    with pytest.raises((RuntimeError, PeroHipError)):   # no CPU fallback
        CTCLoss()(torch.zeros(1, 4, 5), torch.zeros(1, 2, dtype=torch.int64), torch.tensor([4]), torch.tensor([2]))
    op = BatchOperator(torch.device("cpu"))
    import numpy as np
    batch = {"images": np.zeros((2, 40, 32, 3), np.uint8), "targets": np.array([[1, 2], [3, 0]]), "target_lengths": np.array([2, 1]),
             "widths": np.array([32, 17])}
    images, targets, target_lengths, input_lengths = op.prepare_batch(batch)
    assert images.dtype == torch.uint8 and input_lengths.tolist() == [4, 3] and targets.dtype == torch.int64 and op.batch_size(batch) == 2
