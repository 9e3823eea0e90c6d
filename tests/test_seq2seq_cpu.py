"""capnet.seq2seq without a GPU: the fp64 restatement (tests/seq2seq_ref.py) is pinned to the REFERENCE's own classes
through tests/golden/seq2seq_tiny.npz before anything on the GPU is held to it; state_dict keys, shapes and initial values
of capnet.seq2seq.Seq2Seq; and the argmax margins of every greedy / fed-back case the GPU tests use.

Bounds of the fixture comparison: the fixture is the reference's fp32 run, the restatement fp64, so they differ by fp32
rounding through at most 6 steps x 3 layers: 2e-5 of max|ref| on logits and states, 1e-5 relative on the loss, 1e-4 of
max|ref| (+ 1e-7) on gradients -- the bounds the GPU tests of the other decoders apply to fp32-vs-fp64 comparisons."""
import json
import os

import pytest
import torch
import torch.nn.functional as Fn

import seq2seq_cases as SC
import seq2seq_ref as SR
from helpers import GOLDEN, load_golden, t

MODES = ("factual", "happy")
TAGS = ("tf10", "tf00", "tf05")


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def fixture(L):
    z = load_golden("seq2seq_tiny.npz")
    pre = "L%d.param." % L
    p = {k[len(pre):]: t(z[k]) for k in z.files if k.startswith(pre)}
    return z, p


def case_inputs(z):
    return (t(z["features"]), (t(z["src"]), z["src_lengths"].tolist()), (t(z["dst_in"]), z["dst_lengths"].tolist()),
            t(z["dst_tgt"]))


def packed(x, lengths):
    return torch.cat([x[:b, i] for i, b in enumerate(SR.batch_sizes(lengths))], 0)


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference_fixture(L, mode, tag):
    z, p32 = fixture(L)
    feats, src, dst, dst_tgt = case_inputs(z)
    c = "L%d.case.%s_%s." % (L, mode, tag)
    tf = (z[c + "draws"] < float(z[c + "ratio"])).tolist()
    p = {k: v.double().requires_grad_(True) for k, v in p32.items()}
    out = SR.seq2seq_forward(p, L, feats.double(), src, dst, tf, mode)
    targets = packed(src[0], src[1]) if mode == "factual" else packed(dst_tgt, dst[1])
    loss = Fn.cross_entropy(out, targets)
    loss.backward()
    assert _rel(out, z[c + "logits"]) < 2e-5
    assert abs(float(loss.detach()) - float(z[c + "loss"])) < 1e-5 * float(z[c + "loss"])
    n = 0
    for k, v in p.items():
        if c + "grad." + k in z.files:
            want = t(z[c + "grad." + k]).double()
            assert v.grad is not None, k
            assert (v.grad - want).abs().max().item() <= 1e-4 * want.abs().max().item() + 1e-7, k
            n += 1
        else:
            assert v.grad is None, k
    assert n == 3 + 4 * L                 # every parameter of the module that ran, and of no other
    if mode == "factual":
        _, (h, cc) = SR.rnn_forward(p, "encoder", L, feats.double(), src[0], src[1], tf)
        assert tuple(h.shape) == (L, 1, 16)      # the rows alive at the last step only
        assert _rel(h, z["L%d.states_%s.h" % (L, tag)]) < 2e-5 and _rel(cc, z["L%d.states_%s.c" % (L, tag)]) < 2e-5


@pytest.mark.parametrize("L", [1, 3])
def test_restatement_reproduces_the_reference_samples(L):
    z, p32 = fixture(L)
    p = {k: v.double() for k, v in p32.items()}
    feats = t(z["features"]).double()
    ids, (h, c), margin, scale = SR.greedy(p, "encoder", L, 40, features=feats)
    assert margin > SC.need(scale), (margin, scale)
    assert torch.equal(ids, t(z["L%d.sample.factual.ids" % L]))
    assert _rel(h, z["L%d.sample.factual.h" % L]) < 2e-5 and _rel(c, z["L%d.sample.factual.c" % L]) < 2e-5
    ids, margin, scale, _ = SR.seq2seq_sample(p, L, 40, feats[:1], int(z["start_token"]), "happy")
    assert margin > SC.need(scale), (margin, scale)
    assert torch.equal(ids, t(z["L%d.sample.happy.ids" % L]))


@pytest.mark.parametrize("L", [1, 3])
def test_state_dict_keys_shapes_and_strict_load(L):
    from capnet.seq2seq import Seq2Seq
    keys = json.load(open(os.path.join(GOLDEN, "seq2seq_state_dict_keys.json")))[str(L)]
    z, p32 = fixture(L)
    E, H, V = z["dims"].tolist()[:3]
    m = Seq2Seq(E, H, V, L)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == keys
    assert len(keys) == 4 * (3 + 4 * L)          # 60 tensors at 3 layers
    m.load_state_dict(p32, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, p32[k]), k
    assert m.encoder.max_seq_length == 40 and m.decoder_sad.num_layers == L and m.hidden_size == H


def test_initial_values_follow_torch_constructor_defaults():
    """Embedding N(0, 1); every LSTM tensor and Linear U(-1/sqrt(H), 1/sqrt(H)) (Linear: fan_in = H): bounds and
    moments per tensor, as tests/test_init_cpu.py does for the other decoders."""
    from capnet.seq2seq import Seq2Seq
    E, H, V, L = 48, 64, 400, 3
    torch.manual_seed(11)
    m = Seq2Seq(E, H, V, L)
    k = 1.0 / H ** 0.5
    for name, v in m.state_dict().items():
        v = v.double()
        n = v.numel()
        if name.endswith("embed.weight"):
            assert abs(v.mean().item()) < 5 / n ** 0.5 and abs(v.std().item() - 1) < 0.05 and v.abs().max() > 3, name
        else:
            assert v.abs().max().item() <= k and v.abs().max().item() > 0.9 * k, name
            assert abs(v.mean().item()) < 5 * k / (3 * n) ** 0.5, name
            assert abs(v.std().item() - k / 3 ** 0.5) < 0.1 * k, name
    # and the reference's draw order: the same seed gives torch's own modules' values, bit for bit
    torch.manual_seed(11)
    import torch.nn as nn
    emb, lstm, lin = nn.Embedding(V, E), nn.LSTM(E, H, L, batch_first=True), nn.Linear(H, V)
    assert torch.equal(m.encoder.embed.weight, emb.weight) and torch.equal(m.encoder.linear.weight, lin.weight)
    for kname, v in lstm.state_dict().items():
        assert torch.equal(getattr(m.encoder.lstm, kname), v), kname


def test_unknown_mode_and_layer_count_raise():
    from capnet import CapnetError
    from capnet.seq2seq import Seq2Seq
    m = Seq2Seq(12, 16, 37, 1)
    with pytest.raises(CapnetError):
        m(None, (None, [3, 2]), mode="joyful")
    with pytest.raises(CapnetError):
        m.sample(None, 1, mode="joyful")
    with pytest.raises(CapnetError):
        Seq2Seq(12, 16, 37, 9)


@pytest.mark.parametrize("name", sorted(SC.GREEDY))
def test_greedy_margins(name):
    """Every row and every one of the case's steps: the smallest top-1 / top-2 gap of the fp64 restatement exceeds the
    bound the GPU comparison relies on (tests/seq2seq_cases.py)."""
    c = SC.GREEDY[name]
    ids, margin, scale, _ = SC.greedy_reference(name)
    print("%s: smallest gap %.3e, needed %.3e (largest |logit| %.2f)" % (name, margin, SC.need(scale), scale))
    assert tuple(ids.shape) == (c["rows"], c["steps"]) and c["steps"] == 40
    assert margin > SC.need(scale), (name, margin, SC.need(scale))


@pytest.mark.parametrize("name", sorted(SC.TRAIN))
def test_fed_back_margins_of_the_training_cases(name):
    """Fed-back rows of the full-size training cases (dropout off: the mask is the kernels', the GPU test checks the
    masked run's margins itself): gap > 2 x TOL_LOGITS x the largest logit, as tests/test_long_inputs_cpu.py."""
    c, p, feats, (tokens, lengths), targets, tf = SC.train_case(name)
    margins = []
    prefix = "encoder" if c["mode"] == "factual" else "decoder_" + c["mode"]
    out, _ = SR.rnn_forward(p, prefix, c["layers"], feats if c["mode"] == "factual" else None, tokens, lengths, tf,
                            margins=margins)
    need = 2 * SC.TOL_LOGITS * float(out.abs().max())
    print("%s: %d fed-back steps, smallest gap %.3e, needed %.3e" % (name, len(margins), min(margins), need))
    assert len(margins) >= 2 and min(margins) > need, (name, min(margins), need)
