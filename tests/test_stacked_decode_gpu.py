"""capnet.stacked.StackedFactoredLSTM decoding (forward_step, sample, sample_batch) on the GPU, on the fused step
(csrc/lstm_decode_step.hip, folded weights) and on the composed one (CAPNET_NO_FUSED_DECODE_STEP=1), against the fp64
restatement of tests/stacked_decode_ref.py; one layer against DecoderFactoredLSTM; the validation and test-set loops.

Tolerance of a step (TOL, relative to max|ref| of each layer's h and c): the f32 MFMA product is an fmaf chain, about
1e-7 * sum|a b| at K = in + H <= 1024, and sum|a b| is about 20 |pre| at K = 1024 with unit-variance operands: 2e-6 of
the gate pre-activations. The fold (U S V, two f32 products at K = F) adds rounding of the same order to the weights,
and three layers feed each other's errors forward. 3e-5 leaves a factor of about five over that."""
import os
import re

import pytest
import torch
import torch.nn as nn

from capnet import ops
from capnet.metrics import corpus_bleu
from capnet.model import DecoderFactoredLSTM
from capnet.stacked import MODES, StackedFactoredLSTM
from capnet.train import CrossEntropyLoss, evaluate, val_emotion, val_factual
from stacked_decode_ref import beam_margin, decode_params, greedy_path, sample_stacked, stacked_step

pytestmark = pytest.mark.gpu

FUSED_OFF = "CAPNET_NO_FUSED_DECODE_STEP"
TOL = 3e-5
SHAPES = {"tiny": dict(E=12, H=64, F=32, V=37, seed=3), "cfg4": dict(E=300, H=512, F=1024, V=8192, seed=4)}
ROWS = (1, 5, 16, 17, 64, 320)
PATHS = ("fused", "composed")
_LAYER = re.compile(r"^[VSUW](\d+)_")
_cache = {}


def _params(shape, layers):
    """fp64 parameters of a `layers`-layer decoder: the first layers of one fixed 3-layer set per shape."""
    if shape not in _cache:
        s = SHAPES[shape]
        _cache[shape] = decode_params(StackedFactoredLSTM(s["E"], s["H"], s["F"], s["V"], 3), seed=s["seed"])
    return {k: v for k, v in _cache[shape].items() if not _LAYER.match(k) or int(_LAYER.match(k).group(1)) < layers}


def _decoder(shape, layers, dev, max_seq_length=20):
    s = SHAPES[shape]
    p = _params(shape, layers)
    dec = StackedFactoredLSTM(s["E"], s["H"], s["F"], s["V"], layers, max_seq_length=max_seq_length)
    dec.load_state_dict({k: v.float() for k, v in p.items()})
    return dec.to(dev).eval(), p


def _path(monkeypatch, path):
    if path == "fused":
        monkeypatch.delenv(FUSED_OFF, raising=False)
    else:
        monkeypatch.setenv(FUSED_OFF, "1")


def _inputs(shape, layers, rows=320, seed=9):
    s = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(rows, s["E"], generator=g, dtype=torch.float64) * 2 - 1
    hs = [(torch.rand(rows, s["H"], generator=g, dtype=torch.float64) - 0.5) * 0.6 for _ in range(layers)]
    cs = [(torch.rand(rows, s["H"], generator=g, dtype=torch.float64) - 0.5) * 2.0 for _ in range(layers)]
    state = torch.stack([t for l in range(layers) for t in (hs[l], cs[l])], 1).float()
    return x, hs, cs, state


def _err(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _state_err(st, ref_h, ref_c):
    return max(max(_err(st[:, 2 * l], ref_h[l]), _err(st[:, 2 * l + 1], ref_c[l])) for l in range(len(ref_h)))


# ---- 1. one step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tiny", "cfg4"])
@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES)
def test_forward_step_matches_restatement(dev, monkeypatch, shape, layers, mode):
    dec, p = _decoder(shape, layers, dev)
    x, hs, cs, state = _inputs(shape, layers)
    _, ref_h, ref_c = stacked_step(p, x, hs, cs, mode, layers)
    full = {}
    for path in PATHS:
        _path(monkeypatch, path)
        for rows in ROWS:
            top, st = dec.forward_step(x[:rows].float().to(dev), state[:rows].to(dev), mode)
            ops.check_device_errors()
            assert st.shape == (rows, 2 * layers, SHAPES[shape]["H"])
            assert torch.equal(top, st[:, 2 * layers - 2])
            err = _state_err(st.cpu(), [h[:rows] for h in ref_h], [c[:rows] for c in ref_c])
            assert err <= TOL, (path, rows, err)
        full[path] = st.cpu()
    # fused against composed, every layer's h and c
    assert _state_err(full["fused"], [full["composed"][:, 2 * l].double() for l in range(layers)],
                      [full["composed"][:, 2 * l + 1].double() for l in range(layers)]) <= TOL


def test_forward_step_takes_a_list_of_layer_states(dev):
    dec, p = _decoder("tiny", 2, dev)
    x, hs, cs, state = _inputs("tiny", 2, rows=7)
    pairs = [(state[:, 2 * l].to(dev), state[:, 2 * l + 1].to(dev)) for l in range(2)]
    a = dec.forward_step(x.float().to(dev), pairs, "happy")[1]
    b = dec.forward_step(x.float().to(dev), state.to(dev), "happy")[1]
    assert torch.equal(a, b)


@pytest.mark.parametrize("shape", ["tiny", "cfg4"])
def test_negative_controls_are_far(dev, monkeypatch, shape):
    """The restatement with the wrong mode's S, or with layers 1 and 2 swapped, lands >= 100 TOL from the GPU."""
    layers, mode = 3, "happy"
    dec, p = _decoder(shape, layers, dev)
    x, hs, cs, state = _inputs(shape, layers, rows=64)
    swapped = dict(p)
    for k, v in p.items():
        m = _LAYER.match(k)
        if m and int(m.group(1)) in (1, 2):
            swapped[k[0] + str(3 - int(m.group(1))) + k[2:]] = v
    _, wrong_h, wrong_c = stacked_step(p, x, hs, cs, "sad", layers)
    _, swap_h, swap_c = stacked_step(swapped, x, hs, cs, mode, layers)
    for path in PATHS:
        _path(monkeypatch, path)
        st = dec.forward_step(x.float().to(dev), state.to(dev), mode)[1].cpu()
        assert _state_err(st, wrong_h, wrong_c) >= 100 * TOL, path
        assert _state_err(st, swap_h, swap_c) >= 100 * TOL, path


# ---- 2. beam search ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tiny", "cfg4"])
@pytest.mark.parametrize("layers", [2, 3])
def test_sample_matches_restatement(dev, monkeypatch, shape, layers):
    """Identical sequences wherever the oracle's beam search never has two candidates within 1e-4 at the cut (nor two
    completed sequences within 1e-4 at the top). At V = 37 that holds in every case and is asserted. At V = 8192 the
    candidates crowd: with these parameters the case (L = 2, angry, k = 3) has a 1e-5 near-tie, where f32 rounding may
    pick either candidate. So a configs[4] case without the margin is not compared, and at most one per layer count
    may lack it."""
    dec, p = _decoder(shape, layers, dev)
    feat = torch.zeros(1, SHAPES[shape]["E"], device=dev)
    ill_posed = []
    for mode in MODES:
        end = greedy_path(p, layers, 1, 5, mode)[4]
        for k in (1, 3, 5):
            margin = beam_margin(p, layers, 1, end, k=k, mode=mode, max_seq_length=20)
            if margin <= 1e-4:
                assert shape == "cfg4", (mode, k, margin)
                ill_posed.append((mode, k, margin))
                continue
            want = sample_stacked(p, layers, 1, end, k=k, mode=mode, max_seq_length=20).tolist()
            for path in PATHS:
                _path(monkeypatch, path)
                got = dec.sample(feat, 1, end, k=k, mode=mode)
                assert got.cpu().tolist() == want, (mode, k, path)
    assert len(ill_posed) <= 1, ill_posed


@pytest.mark.parametrize("shape", ["tiny", "cfg4"])
def test_one_layer_sample_is_the_factored_decoders(dev, monkeypatch, shape):
    s = SHAPES[shape]
    dec, p = _decoder(shape, 1, dev)
    ref = DecoderFactoredLSTM(s["E"], s["H"], s["F"], s["V"], 1, max_seq_length=20)
    ref.load_state_dict(dec.state_dict())                     # the keys are identical
    ref.to(dev).eval()
    feat = torch.zeros(1, s["E"], device=dev)
    for mode in MODES:
        end = greedy_path(p, 1, 1, 5, mode)[4]
        for k in (3, 5):
            assert beam_margin(p, 1, 1, end, k=k, mode=mode, max_seq_length=20) > 1e-4, (mode, k)
            want = ref.sample(feat, 1, end, k=k, mode=mode).cpu().tolist()
            for path in PATHS:
                _path(monkeypatch, path)
                assert dec.sample(feat, 1, end, k=k, mode=mode).cpu().tolist() == want, (mode, k, path)


@pytest.mark.parametrize("shape,layers", [("tiny", 2), ("cfg4", 3)])
def test_sample_batch_matches_per_image_sample(dev, monkeypatch, shape, layers):
    dec, p = _decoder(shape, layers, dev)
    end = greedy_path(p, layers, 1, 5, "angry")[4]
    feats = torch.randn(7, SHAPES[shape]["E"], device=dev)
    for path in PATHS:
        _path(monkeypatch, path)
        batched = dec.sample_batch(feats, 1, end, k=5, mode="angry")           # 35 rows per step at first
        assert len(batched) == 7
        for i in range(7):
            assert list(batched[i]) == dec.sample(feats[i:i + 1], 1, end, k=5, mode="angry")[0].cpu().tolist(), (path, i)


# ---- 3. the validation and test-set loops ----------------------------------------------------------------------------
class _Vocab:
    def __init__(self, V):
        self.word2idx = {'<pad>': 0, '<start>': 1, '<end>': 2, '<unk>': 3}
        self.idx2word = {i: "w%d" % i for i in range(V)}
        self.idx2word.update({0: '<pad>', 1: '<start>', 2: '<end>', 3: '<unk>'})


class _FixedFeatures(nn.Module):
    """Stands in for EncoderCNN: the loader yields the features themselves."""

    def forward(self, images):
        return images


def test_validation_and_evaluation_run_on_the_stacked_decoder(dev):
    s = SHAPES["tiny"]
    dec, _ = _decoder("tiny", 2, dev)
    g = torch.Generator().manual_seed(12)
    batches = []
    for b in (5, 3):
        lengths = sorted([int(v) for v in torch.randint(3, 9, (b,), generator=g)], reverse=True)
        captions = torch.randint(3, s["V"], (b, max(lengths)), generator=g)
        captions[:, 0] = 1
        feats = torch.randn(b, s["E"], generator=g)
        all_caps = [[captions[i, :lengths[i]].clone(), captions[i, :lengths[i]].flip(0)] for i in range(b)]
        batches.append((feats, captions, lengths, all_caps))
    vocab, enc = _Vocab(s["V"]), _FixedFeatures()
    bt, top5, loss, bleu = val_factual(enc, dec, vocab, CrossEntropyLoss(), batches, device=dev)
    assert loss > 0 and 0 <= top5 <= 100 and 0 <= bleu <= 1
    _, top5s, losses, bleus = val_emotion(enc, dec, vocab, CrossEntropyLoss(), [batches, batches[:1]], ["happy", "sad"],
                                          device=dev)
    assert len(top5s) == len(losses) == len(bleus) == 2 and all(l > 0 for l in losses)
    got = evaluate(enc, dec, vocab, batches, mode="sad", k=3, device=dev)
    refs, hyps = [], []
    for feats, _, _, all_caps in batches:
        for i in range(feats.size(0)):
            hyps.append(dec.sample(feats[i:i + 1].to(dev), 1, 2, k=3, mode="sad")[0].cpu().tolist())
            refs.append([[int(w) for w in c.tolist()] for c in all_caps[i]])
    want = tuple(corpus_bleu(refs, hyps, weights=w)
                 for w in ((1, 0, 0, 0), (0.5, 0.5, 0, 0), (0.33, 0.33, 0.33, 0), (0.25, 0.25, 0.25, 0.25)))
    assert got == want
