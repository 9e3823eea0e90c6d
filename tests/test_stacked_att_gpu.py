"""capnet.stacked_att.StackedFactoredLSTMAtt (BASELINE configs[3]: the attention path with a 2-layer LSTM). PARITY
UNPINNED with more than one layer: the reference ignores num_layers (stylenet/model_att.py:81). Checked: one layer against
the fixture of the reference's own DecoderFactoredLSTMAtt; two and three layers against the CPU restatement of the
definition (tests/stacked_att_ref.py: logits, alphas, loss, every gradient, scheduled sampling); the fused upper step
against the composed one with dropout on; decoding; one optimisation step and a checkpoint round trip."""
import os
import random

import pytest
import torch
import torch.nn as nn

import capnet
from capnet import ops
from capnet.model_att import DecoderFactoredLSTMAtt
from capnet.optim import Adam
from capnet.stacked_att import StackedFactoredLSTMAtt
from capnet.train import CrossEntropyLoss, train_step_att
from capnet.utils import load_checkpoint, save_checkpoint
from helpers import golden_case, golden_params, load_golden, rel_err, t
from oracle import decoders_ref as D
from stacked_att_ref import greedy_decode, stacked_factored_att_forward

pytestmark = pytest.mark.gpu

FUSED_OFF = "CAPNET_NO_FUSED_UPPER_STEP"


def grad_close(a, b, rtol):
    """max|a-b| <= rtol*max|b| + 1e-6 (full_att.bias has an exactly-zero gradient: rounding noise on both sides)."""
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return (a - b).abs().max().item() <= rtol * b.abs().max().item() + 1e-6


def _state(dec, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in dec.state_dict().items():
        lim = 0.3 if v.dim() > 1 else 0.05
        sd[k] = (torch.rand(v.shape, generator=g) * 2 - 1) * lim
    return sd


def _batch(B, V, T, seed):
    g = torch.Generator().manual_seed(seed)
    lengths = sorted([int(v) for v in torch.randint(3, T + 1, (B,), generator=g)], reverse=True)
    lengths[0] = T
    captions = torch.randint(3, V, (B, T), generator=g)
    return captions, lengths


def _features(B, P, Cf, seed):
    return torch.randn(B, P, Cf, generator=torch.Generator().manual_seed(seed)).abs() * 0.5


def _run(dec, captions, lengths, feats, tf, mode, dev):
    dec.zero_grad()
    out, alphas = dec(captions.to(dev), lengths, feats.to(dev), mode=mode, tf_mask=tf)
    loss = ops.cross_entropy(out, ops.packed_targets(captions.to(dev), lengths))
    loss = ops.attention_loss(loss, alphas, 1.0)
    loss.backward()
    ops.check_device_errors()
    return out, alphas, loss


# ---- 1. one layer is the reference's attention decoder ---------------------------------------
@pytest.mark.parametrize("cname,seed,ratio", [("tf1_factual", 100, 1.0), ("tf0_happy", 101, 0.0),
                                              ("tfmix_factual", 3, 0.6), ("tfmix_sad", 5, 0.6)])
def test_one_layer_matches_reference_fixture(dev, cname, seed, ratio):
    z = load_golden("decoder_att_tiny.npz")
    A, E, H, F, V, Cf, P = z["dims"].tolist()
    dec = StackedFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=Cf, dropout=0.0)
    dec.load_state_dict(golden_params(z))
    dec.to(dev).train()
    c = golden_case(z, cname)
    captions, lengths = t(z["captions"]), z["lengths"].tolist()
    lens = [l - 1 for l in lengths]
    targets = D.packed_targets(captions[:, 1:], lens).to(dev)
    random.seed(seed)
    out, alphas = dec(captions[:, :-1].contiguous().to(dev), lens, t(z["features"]).to(dev),
                      teacher_forcing_ratio=ratio, mode=str(c["mode"]))
    loss = ops.cross_entropy(out, targets) + 1.0 * ((1.0 - alphas.sum(dim=1)) ** 2).mean()
    loss.backward()
    ops.check_device_errors()
    assert rel_err(out, c["logits"]) < 2e-5
    assert rel_err(alphas, c["alphas"]) < 2e-5
    assert abs(loss.item() - float(c["loss"])) / float(c["loss"]) < 2e-6
    n = 0
    for k, prm in dec.named_parameters():
        key = "grad." + k
        if key in c:
            assert prm.grad is not None, k
            assert grad_close(prm.grad, c[key], 1e-4), k
            n += 1
        else:
            assert prm.grad is None, k
    assert n > 30


# ---- 2. two and three layers against the restatement ----------------------------------------
SMALL = dict(A=32, E=24, H=64, F=32, V=97, Cf=512, P=9)         # H = 64: the fused upper step's smallest width
WIDE = dict(A=64, E=48, H=512, F=64, V=97, Cf=512, P=9)         # H = 512: teacher-forced runs in the persistent kernel


def _tf(kind, steps, seed):
    if kind == "teacher":
        return [True] * steps
    if kind == "free":
        return [False] * steps
    random.seed(seed)
    tf = [random.random() < 0.5 for _ in range(steps)]
    tf[1], tf[2], tf[3] = True, True, False          # a run of teacher-forced steps, then a free one
    return tf


@pytest.mark.parametrize("layers,B,shape,mode,kind", [
    (2, 12, "small", "factual", "mixed"),
    (2, 12, "small", "sad", "free"),
    (3, 12, "small", "happy", "teacher"),
    (3, 40, "small", "factual", "mixed"),
    (2, 40, "small", "angry", "free"),
    (2, 12, "wide", "factual", "mixed"),
    (2, 40, "wide", "sad", "teacher"),
])
def test_stacked_matches_cpu_restatement(dev, layers, B, shape, mode, kind):
    s = SMALL if shape == "small" else WIDE
    dec = StackedFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], layers, feature_size=s["Cf"], dropout=0.0)
    p = _state(dec, 10 * layers + B)
    dec.load_state_dict(p)
    dec.to(dev).train()
    T = 9
    captions, lengths = _batch(B, s["V"], T, seed=B + layers)
    feats = _features(B, s["P"], s["Cf"], seed=B)
    tf = _tf(kind, T, seed=layers)
    out, alphas, loss = _run(dec, captions, lengths, feats, tf, mode, dev)
    leaves = {k: v.double().requires_grad_(True) for k, v in p.items()}
    ref, ref_alphas = stacked_factored_att_forward(leaves, captions, lengths, feats.double(), tf, mode, layers)
    ref_loss = D.att_loss(ref, ref_alphas, D.packed_targets(captions, lengths))
    ref_loss.backward()
    assert rel_err(out, ref.detach()) < 2e-5
    assert rel_err(alphas, ref_alphas.detach()) < 2e-5
    assert abs(loss.item() - ref_loss.item()) / ref_loss.item() < 1e-5
    got = dict(dec.named_parameters())
    n_checked = 0
    for k, leaf in leaves.items():
        if leaf.grad is None:
            assert got[k].grad is None, k                # the other modes' attention and S
            continue
        assert got[k].grad is not None, k
        assert grad_close(got[k].grad, leaf.grad, 2e-4), k
        n_checked += 1
    # every upper layer's V, S (this mode), U, W and initial state
    for l in range(1, layers):
        for name in ("init_h%d.weight" % l, "init_c%d.bias" % l, "V%d_i.weight" % l, "U%d_c.weight" % l, "W%d_o.weight" % l):
            assert leaves[name].grad is not None, name
    assert n_checked >= 44 + 36 * (layers - 1) - 2


# ---- 3. the fused upper step against the composed one, dropout on ----------------------------
@pytest.mark.parametrize("shape,kind", [("small", "free"), ("small", "mixed"), ("wide", "mixed")])
def test_fused_upper_step_matches_composed_with_dropout(dev, monkeypatch, shape, kind):
    s = SMALL if shape == "small" else WIDE
    B, T = 12, 8
    dec = StackedFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], 3, feature_size=s["Cf"], dropout=0.3)
    dec.load_state_dict(_state(dec, 5))
    dec.to(dev).train()
    captions, lengths = _batch(B, s["V"], T, seed=2)
    feats = _features(B, s["P"], s["Cf"], seed=3)
    tf = _tf(kind, T, seed=4)
    res = {}
    for fused in (True, False):
        if fused:
            monkeypatch.delenv(FUSED_OFF, raising=False)
        else:
            monkeypatch.setenv(FUSED_OFF, "1")
        torch.manual_seed(0)                 # the same dropout seed both ways
        out, alphas, loss = _run(dec, captions, lengths, feats, tf, "factual", dev)
        res[fused] = (out.detach().clone(), {k: v.grad.clone() for k, v in dec.named_parameters() if v.grad is not None})
    monkeypatch.delenv(FUSED_OFF, raising=False)
    assert rel_err(res[True][0], res[False][0]) < 1e-5
    assert sorted(res[True][1]) == sorted(res[False][1])
    for k, g in res[False][1].items():
        assert grad_close(res[True][1][k], g, 1e-4), k
    # and dropout did act between the layers: eval mode gives other logits
    dec.eval()
    with torch.no_grad():
        out_eval, _ = dec(captions.to(dev), lengths, feats.to(dev), mode="factual", tf_mask=tf)
    assert rel_err(out_eval, res[True][0]) > 1e-3


# ---- 4. decoding ---------------------------------------------------------------------------------
def _decoder_for_sampling(layers, seed):
    s = SMALL
    dec = StackedFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], layers, feature_size=s["Cf"], dropout=0.0,
                                 max_seq_length=12)
    p = _state(dec, seed)
    p["C.weight"] = p["C.weight"] * 8.0              # clear argmax margins
    dec.load_state_dict(p)
    return dec, p


def test_greedy_sample_matches_restatement(dev):
    dec, p = _decoder_for_sampling(2, 24)
    feats = _features(1, SMALL["P"], SMALL["Cf"], seed=6)
    pd = {k: v.double() for k, v in p.items()}
    free, _ = greedy_decode(pd, feats.double(), 1, -1, 8, "factual", 2)
    end = free[4]
    want, margin = greedy_decode(pd, feats.double(), 1, end, 8, "factual", 2)
    assert margin > 1e-3 and want[-1] == end
    dec.to(dev).eval()
    seq = dec.sample(feats.to(dev), 1, end, k=1)
    assert seq.cpu().tolist() == [want]


def test_sample_batch_matches_per_image_sample(dev):
    dec, _ = _decoder_for_sampling(3, 22)
    dec.to(dev).eval()
    feats = _features(3, SMALL["P"], SMALL["Cf"], seed=7).to(dev)
    batched = dec.sample_batch(feats, 1, 2, k=3)
    for i in range(3):
        one = dec.sample(feats[i:i + 1], 1, 2, k=3)
        assert list(batched[i]) == one[0].cpu().tolist(), i


def test_one_layer_sample_is_the_attention_decoders(dev):
    s = SMALL
    dec = StackedFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], 1, feature_size=s["Cf"], max_seq_length=12)
    ref = DecoderFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], 1, feature_size=s["Cf"], max_seq_length=12)
    p = _state(dec, 23)
    dec.load_state_dict(p)
    ref.load_state_dict(p)
    dec.to(dev).eval()
    ref.to(dev).eval()
    feats = _features(1, s["P"], s["Cf"], seed=8).to(dev)
    for mode in ("factual", "angry"):
        assert dec.sample(feats, 1, 2, k=3, mode=mode).cpu().tolist() == ref.sample(feats, 1, 2, k=3, mode=mode).cpu().tolist()


# ---- 5. training step and checkpoint ------------------------------------------------------------
class _FixedEncoder(nn.Module):
    """Stands in for EncoderCNN: the precomputed feature map, no parameters."""

    def __init__(self, feats):
        super().__init__()
        self.feats = feats

    def forward(self, images):
        return self.feats


def test_train_step_and_checkpoint_round_trip(dev, tmp_path):
    s = SMALL
    B, T = 12, 8
    dec = StackedFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], 2, feature_size=s["Cf"], dropout=0.0)
    p = _state(dec, 31)
    dec.load_state_dict(p)
    dec.to(dev).train()
    captions, lengths = _batch(B, s["V"], T, seed=9)
    feats = _features(B, s["P"], s["Cf"], seed=10)
    enc = _FixedEncoder(feats.to(dev))
    tf = _tf("mixed", T - 1, seed=5)
    opt = Adam(list(dec.parameters()), lr=1e-3)
    crit = CrossEntropyLoss()
    cap_d = captions.to(dev)
    loss1 = train_step_att(enc, dec, opt, crit, None, cap_d, lengths, 5.0, mode="happy", tf_mask=tf)
    torch.cuda.synchronize()
    lens = [l - 1 for l in lengths]
    pd = {k: v.double() for k, v in p.items()}
    ref, ref_alphas = stacked_factored_att_forward(pd, captions[:, :-1], lens, feats.double(), tf, "happy", 2)
    ref_loss = D.att_loss(ref, ref_alphas, D.packed_targets(captions[:, 1:], lens))
    assert abs(loss1.item() - ref_loss.item()) / ref_loss.item() < 1e-5
    assert not torch.equal(dec.V1_i.weight.detach().cpu(), p["V1_i.weight"])      # the step moved the upper layer
    save_checkpoint(str(tmp_path), "stk", "happy", 1, 0, enc, dec, opt, None, 0.0, False)
    loss2 = train_step_att(enc, dec, opt, crit, None, cap_d, lengths, 5.0, mode="happy", tf_mask=tf)
    after = {k: v.detach().cpu().clone() for k, v in dec.state_dict().items()}
    dec2 = StackedFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], 2, feature_size=s["Cf"], dropout=0.0).to(dev)
    dec2.train()
    opt2 = Adam(list(dec2.parameters()), lr=1e-3)
    load_checkpoint(os.path.join(str(tmp_path), "happy_checkpoint_stk.pth.tar"), None, dec2, opt2, map_location=dev)
    loss2b = train_step_att(enc, dec2, opt2, crit, None, cap_d, lengths, 5.0, mode="happy", tf_mask=tf)
    torch.cuda.synchronize()
    ops.check_device_errors()
    assert loss2b.item() == loss2.item()
    for k, v in dec2.state_dict().items():
        assert torch.equal(v.detach().cpu(), after[k]), k
