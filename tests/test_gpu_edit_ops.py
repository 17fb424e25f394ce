"""GPU: pero_edit_ops (csrc/edit.hip) and its users in the recognition package against tests/edit_ops_ref.py, the specification in
plain Python that test_edit_ops_ref_cpu.py pins.  The arithmetic is integer and the tie rule makes the script unique, so every output
is compared with torch.equal: counts, script, script lengths, spans, totals and the confusion matrix; every case is also run twice (equal
bits, totals and confusion accumulated) and, at symbol level, checked against pero_edit_distance."""
import functools
import random

import numpy as np
import pytest
import torch

import edit_ops_ref as E

pytestmark = pytest.mark.gpu

I64 = torch.int64


@pytest.fixture(scope="module")
def ops():
    from pero_pretraining_amd import ops as _ops
    return _ops


def check(ops, a, a_len, b, b_len, C=None, separators=None, confusion=False):
    """One case through ops.edit_ops, twice, against the reference.  Returns the reference's outputs."""
    want = E.expected(a, a_len, b, b_len, C=C, separators=separators, confusion=confusion)
    N, La, Lb = a.shape[0], a.shape[1], b.shape[1]
    dev = [t.cuda() for t in (a, a_len, b, b_len)]
    assert La > 0 or dev[0].data_ptr() == 0          # a zero-width matrix goes in as a null pointer
    totals = torch.zeros(6, dtype=I64).cuda()
    conf = torch.zeros((C + 1, C + 1), dtype=I64).cuda() if confusion else None
    words = separators is not None
    kw = dict(num_classes=C, separators=separators, totals=totals, confusion=conf, want_spans=words)
    first = ops.edit_ops(*dev, **kw)
    counts, script, script_len, a_spans, b_spans = first
    assert counts.shape == (N, 4) and counts.dtype == I64 and script.shape == (N, La + Lb) and script.dtype == torch.int8
    assert script_len.shape == (N,) and script_len.dtype == torch.int32
    assert torch.equal(counts.cpu(), want["counts"])
    assert torch.equal(script_len.cpu(), want["script_len"])
    assert torch.equal(script.cpu(), want["script"])          # the whole matrix: -1 behind the script
    assert torch.equal(totals.cpu(), want["totals"])
    if words:
        assert a_spans.shape == (N, (La + 1) // 2, 2) and a_spans.dtype == torch.int32 and b_spans.shape == (N, (Lb + 1) // 2, 2)
        assert torch.equal(a_spans.cpu(), want["a_spans"]) and torch.equal(b_spans.cpu(), want["b_spans"])
    else:
        assert a_spans is None and b_spans is None
        assert torch.equal(counts[:, :3].sum(1), ops.edit_distance(*dev))
    if confusion:
        assert torch.equal(conf.cpu(), want["confusion"])
    again = ops.edit_ops(*dev, **kw)                           # two calls: equal bits, totals and confusion accumulated
    for x, y in zip(first, again):
        assert (x is None and y is None) or torch.equal(x, y)
    assert torch.equal(totals.cpu(), 2 * want["totals"])
    if confusion:
        assert torch.equal(conf.cpu(), 2 * want["confusion"])
    bare = ops.edit_ops(*dev, num_classes=C, separators=separators, want_script=False)   # counts alone: unchanged
    assert bare[1] is None and bare[2] is None and torch.equal(bare[0], counts)
    return want


def batch(pairs, La=None, Lb=None, fill=1):
    a, a_len = E.pad([p[0] for p in pairs], max(len(p[0]) for p in pairs) if La is None else La, fill)
    b, b_len = E.pad([p[1] for p in pairs], max(len(p[1]) for p in pairs) if Lb is None else Lb, fill)
    return a, a_len, b, b_len


def rand(rng, n, symbols):
    return [rng.randrange(symbols) for _ in range(n)]


@pytest.mark.parametrize("symbols", [2, 50])
def test_random_pairs(ops, symbols):
    """64 pairs, lengths 0..40; two symbols: a tie in nearly every cell."""
    want = check(ops, *batch(E.random_pairs(64, 40, symbols, seed=symbols), 40, 40), C=symbols, confusion=True)
    assert int(want["confusion"].sum()) == int(want["totals"][:4].sum())          # every label is a class: every operation is counted


@pytest.mark.parametrize("La,Lb", [(37, 5), (5, 37)])
def test_matrices_of_different_widths(ops, La, Lb):
    rng = random.Random(La)
    pairs = [(rand(rng, rng.randint(0, La), 3), rand(rng, rng.randint(0, Lb), 3)) for _ in range(16)] + [(rand(rng, La, 3), rand(rng, Lb, 3))]
    check(ops, *batch(pairs, La, Lb), C=3, confusion=True)


def test_lengths_around_the_packing_and_wave_edges(ops):
    """16 cells to a word of directions, 64 lanes to a wave: every pair of lengths of 15..17, 31..33, 63..65."""
    rng = random.Random(1)
    edges = [15, 16, 17, 31, 32, 33, 63, 64, 65]
    pairs = []
    for la in edges:
        for lb in edges:
            x = rand(rng, la, 3)
            pairs.append((x, (E.noisy_copy(x, 3, rng) + rand(rng, lb, 3))[:lb]))          # a noisy copy, cut or filled up to lb
    assert {(len(x), len(y)) for x, y in pairs} == {(la, lb) for la in edges for lb in edges}
    check(ops, *batch(pairs), C=3, confusion=True)


@functools.lru_cache(maxsize=None)
def long_pairs():
    rng = random.Random(2)
    x = rand(rng, 512, 2)
    return {"rows": [(rand(rng, la, 4), rand(rng, lb, 4)) for la in (257, 512) for lb in (1, 300)],
            "limit": [(rand(rng, 512, 2), rand(rng, 512, 2))],
            "extremes": [(x, list(x)), (rand(rng, 512, 2), [2 + c for c in rand(rng, 512, 2)]), (x, []), ([], x), ([], [])]}


def test_more_rows_than_threads(ops):
    check(ops, *batch(long_pairs()["rows"]), C=4, confusion=True)


def test_one_pair_at_the_limit(ops):
    """la = lb = 512 over two symbols, N = 1: the largest table, 1024 steps of walk at the most."""
    want = check(ops, *batch(long_pairs()["limit"]), C=2, confusion=True)
    assert 512 <= int(want["script_len"][0]) <= 1024


def test_lengths_around_the_thread_count_and_the_limit(ops):
    """The sweep both kernels share strides a diagonal by 256 threads and holds at most 512 + 1 cells of it: lengths at 0 and 1, on both
    sides of 256, and at 512, in matrices of the full width, over two symbols (a tie in nearly every cell)."""
    rng = random.Random(3)
    lengths = [(0, 0), (0, 1), (1, 0), (255, 257), (256, 256), (257, 255), (512, 0), (512, 512)]
    check(ops, *batch([(rand(rng, la, 2), rand(rng, lb, 2)) for la, lb in lengths], 512, 512), C=2, confusion=True)


def test_identical_disjoint_and_empty_strings(ops):
    """512 equal elements (512 hits), no equal element (512 substitutions), 512 against 0 and 0 against 512, both empty."""
    want = check(ops, *batch(long_pairs()["extremes"]), C=4, confusion=True)
    assert want["counts"].tolist() == [[0, 0, 0, 512], [512, 0, 0, 0], [0, 512, 0, 0], [0, 0, 512, 0], [0, 0, 0, 0]]
    assert want["totals"].tolist() == [512, 512, 512, 512, 5, 3]


def test_lengths_beyond_the_width_are_clamped_and_a_null_matrix_is_allowed(ops):
    a, a_len, b, b_len = batch(E.random_pairs(8, 20, 3, seed=5), 20, 20)
    check(ops, a, a_len + 1000, b, b_len + 1000, C=3, confusion=True)          # the padding (label 1) is part of the strings now
    check(ops, a, a_len - 1000, b, b_len, C=3, confusion=True)                 # negative lengths clamp to 0
    empty = torch.zeros((8, 0), dtype=I64)
    want = check(ops, empty, a_len, b, b_len, C=3, confusion=True)             # zero-width a: a null pointer; every element of b is deleted
    assert torch.equal(want["counts"][:, 2], b_len) and int(want["counts"][:, [0, 1, 3]].sum()) == 0
    check(ops, a, a_len, empty, b_len, C=3, confusion=True)
    check(ops, empty, a_len, empty, b_len)


def test_labels_outside_the_classes_are_counted_but_not_in_the_confusion_matrix(ops):
    C, rng = 5, random.Random(6)
    pairs = []
    for _ in range(24):
        x = [rng.choice([-1, C + 3, C, 0, 1, 2, 3, 4]) for _ in range(rng.randint(0, 30))]
        pairs.append((x, E.noisy_copy(x, C, rng, rate=0.4)))
    want = check(ops, *batch(pairs, fill=-1), C=C, confusion=True)
    inside = 0          # the operations that involve no label outside [0, C), counted from the walk
    for x, y in pairs:
        for code, i, j in E.walk(x, y):
            inside += (i == 0 or 0 <= x[i - 1] < C) and (j == 0 or 0 <= y[j - 1] < C)
    assert int(want["confusion"].sum()) == inside < int(want["totals"][:4].sum())


def test_word_level_cases(ops):
    want = check(ops, *batch(E.WORD_CASES, fill=0), C=E.WORD_C, separators=E.WORD_SEPS)
    assert want["counts"][4].tolist() == [1, 0, 0, 1] and want["counts"][5].tolist() == [1, 0, 0, 1]   # equal except for length / the last label
    check(ops, *batch(E.WORD_CASES, 19, 24, fill=3), C=E.WORD_C, separators=E.WORD_SEPS)               # the padding holds word labels


def test_word_level_random_lines(ops):
    """Lines of short words over five labels (many equal words), hypotheses = noisy copies; separators 0 and 7, also doubled and at the ends."""
    rng = random.Random(7)
    pairs = []
    for _ in range(48):
        ref = [rng.choice([0, 0, 7, 1, 2, 3, 4, 5, 1, 2, 9]) for _ in range(rng.randint(0, 70))]
        pairs.append((E.noisy_copy(ref, 6, rng), ref))
    check(ops, *batch(pairs), C=8, separators=(0, 7))
    check(ops, *batch(pairs), C=8, separators={7, 0, 12})          # any iterable of ids; ids that name no class are dropped


def test_word_level_at_the_limit(ops):
    """256 one-label words per side (the most a row of 512 holds), and two words of 255 labels that differ in the last label only."""
    rng = random.Random(8)
    ref = [c for _ in range(256) for c in (rng.randint(1, 3), 0)]
    hyp = [c for w in range(256) for c in (rng.randint(1, 3) if rng.random() < 0.2 else ref[2 * w], 0)]
    word = rand(rng, 255, 3)
    long_words = ([1 + c for c in word] + [0] + [1 + c for c in word] + [1], [1 + c for c in word] + [0] + [1 + c for c in word] + [2])
    want = check(ops, *batch([(hyp, ref), (hyp[:-1], ref[1:] + [0]), long_words], fill=0), C=4, separators=[0])
    assert int(want["counts"][0].sum()) >= 256 and want["counts"][2].tolist() == [1, 0, 0, 1]
    assert want["a_spans"][0, 255].tolist() == [510, 511]


# ------------------------------------------------------------------------------------------------ the recognition package
def test_edit_operations_pairs_and_top_confusions(ops):
    from pero_pretraining_amd import recognition
    hyp, hyp_len, ref, ref_len = batch([([1, 2, 2, 3], [1, 3, 4]), ([], [2]), ([2, 1], [1, 2])], 5, 4)
    conf = torch.zeros((6, 6), dtype=I64).cuda()
    r = recognition.edit_operations(hyp.cuda(), hyp_len.cuda(), ref.cuda(), ref_len.cuda(), num_classes=5, confusion=conf)
    want = E.expected(hyp, hyp_len, ref, ref_len, C=5, confusion=True)
    assert torch.equal(r.script.cpu(), want["script"]) and torch.equal(r.counts.cpu(), want["counts"]) and r.hyp_spans is None and r.ref_spans is None
    assert torch.equal(r.distance.cpu(), torch.tensor([3, 1, 2])) and torch.equal(conf.cpu(), want["confusion"])
    pairs = r.pairs()
    assert pairs.shape == (3, 9, 2) and pairs.dtype == torch.int32
    for n in range(3):          # against the walk's own indices (1-based there, 0 = the gap)
        steps = E.walk(hyp[n, :int(hyp_len[n])].tolist(), ref[n, :int(ref_len[n])].tolist())
        assert pairs[n, :len(steps)].tolist() == [[i - 1, j - 1] for _, i, j in steps] and bool((pairs[n, len(steps):] == -1).all())
    assert recognition.top_confusions(conf, k=3) == recognition.top_confusions(want["confusion"], k=3)
    w = recognition.edit_operations(hyp.cuda(), hyp_len.cuda(), ref.cuda(), ref_len.cuda(), separators=[2], num_classes=5)
    want = E.expected(hyp, hyp_len, ref, ref_len, C=5, separators=[2])
    assert torch.equal(w.script.cpu(), want["script"]) and torch.equal(w.hyp_spans.cpu(), want["a_spans"]) and torch.equal(w.ref_spans.cpu(), want["b_spans"])


@functools.lru_cache(maxsize=None)
def _recogniser():
    """A tiny recogniser (2 layers, d = 64) and two batches whose references are noisy copies of what it reads, so that hits, substitutions,
    insertions and deletions all occur; classes 1..6 separate words."""
    from pero_pretraining_amd.recognition import BatchOperator, greedy_decode, init_model
    torch.manual_seed(0)
    C = 37
    model = init_model(torch.device("cuda"), {"type": "vit", "num_blocks": 2, "model_dim": 64, "num_heads": 4, "feedforward_dim": 128},
                       {"type": "linear", "in_features": 64, "out_features": C}, blank=0, zero_infinity=True)
    rng, noise = np.random.default_rng(0), random.Random(0)
    operator = BatchOperator(torch.device("cuda"))
    batches = []
    for n, width in [(3, 192), (2, 160)]:
        b = {"images": rng.integers(0, 256, (n, 40, width, 3), dtype=np.uint8), "widths": rng.integers(width - 40, width + 1, n),
             "targets": np.zeros((n, 1), np.int64), "target_lengths": np.zeros(n, np.int64)}
        model.eval()
        with torch.no_grad():
            images, _, _, il = operator.prepare_batch(b)
            labels, lengths = greedy_decode(model(images, input_lengths=il)["output"], il, 0)
        model.train()
        refs = [E.noisy_copy(labels[k, :int(lengths[k])].tolist(), C, noise, rate=0.3) for k in range(n)]
        refs = [[c if c else 1 for c in r] for r in refs]          # no blank in a reference
        targets, tl = E.pad(refs, max(max(len(r) for r in refs), 1))
        b["targets"], b["target_lengths"] = targets.numpy(), tl.numpy()
        batches.append(b)
    return model, operator, batches, C


@pytest.mark.parametrize("beam_width", [None, 4])
def test_tester_reports_word_error_rate_and_details(beam_width):
    from pero_pretraining_amd.recognition import Tester, beam_decode, greedy_decode
    model, operator, batches, C = _recogniser()
    seps = [1, 2, 3, 4, 5, 6]
    plain = Tester(operator, model, batches, beam_width=beam_width).test()
    assert set(plain) == {"loss", "cer"}
    full = Tester(operator, model, batches, beam_width=beam_width, word_separators=seps, details=True).test()
    assert model.training and full["cer"] == plain["cer"] and full["loss"] == plain["loss"]          # the same floats
    assert set(full) == {"loss", "cer", "wer", "substitutions", "insertions", "deletions", "hits", "lines", "line_error_rate", "confusion",
                         "word_substitutions", "word_insertions", "word_deletions", "word_hits"}
    wer_only = Tester(operator, model, batches, beam_width=beam_width, word_separators=seps).test()
    assert set(wer_only) == {"loss", "cer", "wer"} and wer_only["wer"] == full["wer"] and wer_only["cer"] == plain["cer"]
    # the reference, on the host, over the decoder's strings
    totals, word_totals, confusion = torch.zeros(6, dtype=I64), torch.zeros(6, dtype=I64), torch.zeros((C + 1, C + 1), dtype=I64)
    model.eval()
    with torch.no_grad():
        for b in batches:
            images, targets, tl, il = operator.prepare_batch(b)
            output = model(images, targets, tl, il)["output"]
            labels, lengths = greedy_decode(output, il, 0) if beam_width is None else beam_decode(output, il, 0, beam_width)[:2]
            args = (labels.cpu(), lengths.cpu(), targets.cpu(), tl.cpu())
            sym, wrd = E.expected(*args, C=C, confusion=True), E.expected(*args, C=C, separators=seps)
            totals, word_totals, confusion = totals + sym["totals"], word_totals + wrd["totals"], confusion + sym["confusion"]
    model.train()
    sub, ins, dele, hit, lines, wrong = totals.tolist()
    assert (full["substitutions"], full["insertions"], full["deletions"], full["hits"], full["lines"]) == (sub, ins, dele, hit, lines) and lines == 5
    assert hit > 0 and sub + ins + dele > 0                                     # the batches hold hits and errors
    assert full["cer"] == (sub + ins + dele) / max(hit + sub + dele, 1) and full["line_error_rate"] == wrong / lines
    wsub, wins, wdel, whit = word_totals.tolist()[:4]
    assert (full["word_substitutions"], full["word_insertions"], full["word_deletions"], full["word_hits"]) == (wsub, wins, wdel, whit)
    assert full["wer"] == (wsub + wins + wdel) / max(whit + wsub + wdel, 1) and wsub + wins + wdel > 0
    assert full["confusion"].dtype == I64 and not full["confusion"].is_cuda and torch.equal(full["confusion"], confusion)


def test_tester_stops_at_max_lines_with_and_without_details():
    """max_lines = 3 over three batches of two lines: the loop ends behind the second batch (4 > 3 lines) in both modes, so the details count
    4 lines and both modes give the same 'cer'.  _recogniser's batches hold 3 and 2 lines; the two-line batches are cut from them."""
    from pero_pretraining_amd.recognition import Tester
    model, operator, (first, second), _ = _recogniser()
    batches = [{k: v[rows] for k, v in b.items()} for b, rows in [(first, slice(0, 2)), (first, slice(1, 3)), (second, slice(0, 2))]]
    assert [operator.batch_size(b) for b in batches] == [2, 2, 2]
    plain = Tester(operator, model, batches, max_lines=3).test()
    full = Tester(operator, model, batches, max_lines=3, details=True).test()
    assert full["lines"] == 4 and full["cer"] == plain["cer"] and full["loss"] == plain["loss"]
    assert Tester(operator, model, batches, details=True).test()["lines"] == 6          # without max_lines the third batch counts
