"""capnet.nic_stacked (StackedDecoderRNN, StackedDecoderRNNAtt) on the GPU. One layer against DecoderRNN /
DecoderRNNAtt; the plain stack under teacher forcing against torch's own nn.LSTM(num_layers) in fp64; scheduled sampling,
dropout and the fused upper step against the fp64 restatement (tests/nic_stacked_ref.py); forward_step, sample and
sample_batch on the fused step (the LSTM-cell instance of csrc/lstm_decode_step.hip) and on the composed one; the
training, validation and test-set loops.

Tolerances are the existing decoders': logits 2e-5, loss 1e-5, gradients 2e-4 of max|ref|; a decode step 3e-5 of max|ref|
(tests/test_stacked_decode_gpu.py explains the bound)."""
import random

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn
from torch.nn.utils.rnn import pack_padded_sequence

from capnet import ops
from capnet._lib import lib
from capnet.metrics import corpus_bleu
from capnet.nic_model import DecoderRNN
from capnet.nic_model_att import DecoderRNNAtt
from capnet.nic_stacked import StackedDecoderRNN, StackedDecoderRNNAtt, _pack_cell
from capnet.optim import Adam
from capnet.train import CrossEntropyLoss, evaluate, train_step, train_step_att, val_factual
from helpers import pin_dropout_seed
from nic_stacked_ref import (beam_margin, decode_params, greedy_path, sample_stacked, stacked_lstm_att_forward,
                             stacked_lstm_forward, stacked_step)
from oracle import dropout_ref as R

pytestmark = pytest.mark.gpu

FUSED_DECODE_OFF = "CAPNET_NO_FUSED_DECODE_STEP"
FUSED_UPPER_OFF = "CAPNET_NO_FUSED_UPPER_STEP"
TOL_LOGITS, TOL_LOSS, TOL_GRAD, TOL_STEP = 2e-5, 1e-5, 2e-4, 3e-5


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _grad_ok(a, b, rtol=TOL_GRAD):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return (a - b).abs().max().item() <= rtol * b.abs().max().item() + 1e-6


def _batch(B, V, T, seed, min_len=2):
    g = torch.Generator().manual_seed(seed)
    lengths = sorted([int(v) for v in torch.randint(min_len, T + 1, (B,), generator=g)], reverse=True)
    lengths[0] = T
    captions = torch.randint(3, V, (B, T), generator=g)
    return captions, lengths


def _plain(E, H, V, L, seed, dropout=0.0):
    dec = StackedDecoderRNN(E, H, V, L, dropout=dropout)
    p = decode_params(dec, seed=seed, out_scale=1.0)
    dec.load_state_dict({k: v.float() for k, v in p.items()})
    return dec, p


def _att(A, E, H, V, L, Cf, seed, dropout=0.0):
    dec = StackedDecoderRNNAtt(A, E, H, V, L, feature_size=Cf, dropout=dropout)
    p = decode_params(dec, seed=seed, out_scale=1.0)
    dec.load_state_dict({k: v.float() for k, v in p.items()})
    return dec, p


def _gpu_run(dec, captions, lengths, feats, tf, dev, att, seed_k=None):
    dec.zero_grad()
    if seed_k is not None:
        pin_dropout_seed(seed_k)
    out = dec(captions.to(dev), lengths, feats.to(dev), tf_mask=tf)
    alphas = None
    if att:
        out, alphas = out
    loss = ops.cross_entropy(out, ops.packed_targets(captions.to(dev), lengths))
    if att:
        loss = ops.attention_loss(loss, alphas, 1.0)
    loss.backward()
    ops.check_device_errors()
    grads = {k: v.grad.detach().cpu() for k, v in dec.named_parameters() if v.grad is not None}
    return out.detach().cpu(), None if alphas is None else alphas.detach().cpu(), float(loss), grads


def _ref_run(fwd, p, captions, lengths, feats, tf, att, **kw):
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    out = fwd(q, captions, lengths, feats.double(), tf, **kw)
    alphas = None
    targets = torch.cat([captions[:b, t] for t, b in enumerate(ops.batch_sizes_from_lengths(lengths))], 0)
    if att:
        out, alphas = out
        loss = Fn.cross_entropy(out, targets) + ((1.0 - alphas.sum(dim=1)) ** 2).mean()
    else:
        loss = Fn.cross_entropy(out, targets)
    loss.backward()
    return out.detach(), None if alphas is None else alphas.detach(), float(loss), {k: v.grad for k, v in q.items()}


def _check(got, want, names=None):
    out, alphas, loss, grads = got
    out_r, alphas_r, loss_r, grads_r = want
    assert _rel(out, out_r) < TOL_LOGITS, _rel(out, out_r)
    if alphas_r is not None:
        assert _rel(alphas, alphas_r) < TOL_LOGITS
    assert abs(loss - loss_r) <= TOL_LOSS * abs(loss_r), (loss, loss_r)
    for k in names or grads_r:
        assert k in grads, k
        assert _grad_ok(grads[k], grads_r[k]), (k, _rel(grads[k], grads_r[k]))


# ---- 1. one layer is DecoderRNN / DecoderRNNAtt -----------------------------------------------------------------
def test_one_layer_is_the_nic_decoders(dev):
    E, H, V, B, T, A, Cf, P = 12, 64, 37, 6, 7, 16, 512, 9
    captions, lengths = _batch(B, V, T, 1)
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(2))
    random.seed(3)
    tf = [random.random() < 0.6 for _ in range(max(lengths))]
    a, _ = _plain(E, H, V, 1, 4)
    b = DecoderRNN(E, H, V, 1, dropout=0.0)
    b.load_state_dict(a.state_dict())
    a.to(dev).train()
    b.to(dev).train()
    ga, gb = _gpu_run(a, captions, lengths, feats, tf, dev, False), _gpu_run(b, captions, lengths, feats, tf, dev, False)
    assert torch.equal(ga[0], gb[0]) and ga[2] == gb[2]
    for k in gb[3]:
        assert torch.equal(ga[3][k], gb[3][k]), k
    af = torch.randn(B, P, Cf, generator=torch.Generator().manual_seed(5)).abs()
    a, _ = _att(A, E, H, V, 1, Cf, 6)
    b = DecoderRNNAtt(A, E, H, V, 1, feature_size=Cf, dropout=0.0)
    b.load_state_dict(a.state_dict())
    a.to(dev).train()
    b.to(dev).train()
    ga, gb = _gpu_run(a, captions, lengths, af, tf, dev, True), _gpu_run(b, captions, lengths, af, tf, dev, True)
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1]) and ga[2] == gb[2]
    for k in gb[3]:
        assert torch.equal(ga[3][k], gb[3][k]), k


# ---- 2. pinned to torch's nn.LSTM ---------------------------------------------------------------------------------
def _torch_lstm_run(p, L, captions, lengths, feats):
    """fp64 linear(nn.LSTM(num_layers=L)) on the packed [feature, embed(w)...] with the decoder's weights: (logits, loss,
    gradients under the decoder's names)."""
    E, H = p["embed.weight"].shape[1], p["lstm.weight_hh"].shape[1]
    lstm = nn.LSTM(E, H, num_layers=L, batch_first=True).double()
    names = {}
    with torch.no_grad():
        for l in range(L):
            src = "lstm" if l == 0 else "lstm%d" % l
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(lstm, "%s_l%d" % (n, l)).copy_(p["%s.%s" % (src, n)])
                names["%s.%s" % (src, n)] = getattr(lstm, "%s_l%d" % (n, l))
    emb = p["embed.weight"].clone().requires_grad_(True)
    lw, lb = p["linear.weight"].clone().requires_grad_(True), p["linear.bias"].clone().requires_grad_(True)
    x = torch.cat([feats.double().unsqueeze(1), emb[captions]], 1)[:, :max(lengths)]
    out, _ = lstm(pack_padded_sequence(x, lengths, batch_first=True))
    logits = Fn.linear(out.data, lw, lb)
    targets = torch.cat([captions[:b, t] for t, b in enumerate(ops.batch_sizes_from_lengths(lengths))], 0)
    loss = Fn.cross_entropy(logits, targets)
    loss.backward()
    grads = {k: v.grad for k, v in names.items()}
    grads.update({"embed.weight": emb.grad, "linear.weight": lw.grad, "linear.bias": lb.grad})
    return logits.detach(), None, float(loss), grads


@pytest.mark.parametrize("size", ["tiny", "full", "full_per_step"])
@pytest.mark.parametrize("layers", [2, 3])
def test_plain_stack_is_torch_lstm(dev, size, layers):
    if size == "tiny":
        E, H, V, B, T = 12, 64, 37, 6, 7
    else:
        E, H, V, B, T = 300, 512, 500, 64, 12          # H = 512, <= 128 rows: the persistent kernel's size
    dec, p = _plain(E, H, V, layers, 10 + layers)
    captions, lengths = _batch(B, V, T, 11)
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(12)) * 0.5
    want = _torch_lstm_run(p, layers, captions, lengths, feats)
    dec.to(dev).train()
    old = lib().capnet_lstm_persist_set_mode(1) if size == "full_per_step" else None
    try:
        got = _gpu_run(dec, captions, lengths, feats, [True] * max(lengths), dev, False)
    finally:
        if old is not None:
            lib().capnet_lstm_persist_set_mode(old)
    _check(got, want)


# ---- 3. scheduled sampling ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [2, 3])
def test_scheduled_sampling_matches_restatement(dev, layers):
    E, H, V, B, T, A, Cf, P = 12, 64, 37, 6, 8, 16, 512, 9
    captions, lengths = _batch(B, V, T, 20 + layers)
    random.seed(layers)
    tf = [True] + [random.random() < 0.5 for _ in range(max(lengths) - 1)]
    tf[2] = False
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(21)) * 0.5
    dec, p = _plain(E, H, V, layers, 22)
    dec.to(dev).train()
    _check(_gpu_run(dec, captions, lengths, feats, tf, dev, False),
           _ref_run(stacked_lstm_forward, p, captions, lengths, feats, tf, False, num_layers=layers))
    af = torch.randn(B, P, Cf, generator=torch.Generator().manual_seed(23)).abs() * 0.5
    dec, p = _att(A, E, H, V, layers, Cf, 24)
    dec.to(dev).train()
    _check(_gpu_run(dec, captions, lengths, af, tf, dev, True),
           _ref_run(stacked_lstm_att_forward, p, captions, lengths, af, tf, True, num_layers=layers))


# ---- 4. dropout on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [2, 3])
def test_dropout_matches_restatement_with_the_oracle_masks(dev, layers):
    E, H, V, B, T, A, Cf, P, pd = 12, 64, 37, 6, 8, 16, 512, 9, 0.5
    captions, lengths = _batch(B, V, T, 30 + layers)
    N = sum(lengths)
    tf = [True] * max(lengths)
    tf[3] = False
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(31)) * 0.5
    dec, p = _plain(E, H, V, layers, 32, dropout=pd)
    dec.to(dev).train()
    seed = pin_dropout_seed(40 + layers)
    got = _gpu_run(dec, captions, lengths, feats, tf, dev, False, seed_k=40 + layers)
    m = torch.from_numpy(R.embedding_mask(seed, B, T, E, pd)).double()
    lm = {l: torch.from_numpy(R.layer_mask(seed, N, H, pd, l)).double() for l in range(1, layers)}
    _check(got, _ref_run(stacked_lstm_forward, p, captions, lengths, feats, tf, False, num_layers=layers, drop_mask=m,
                         layer_masks=lm))
    shifted = {l: v.roll(1, 0) for l, v in lm.items()}        # negative control: the neighbouring row's mask
    bad = stacked_lstm_forward(p, captions, lengths, feats.double(), tf, layers, drop_mask=m, layer_masks=shifted)
    assert _rel(got[0], bad) > 1e-2
    af = torch.randn(B, P, Cf, generator=torch.Generator().manual_seed(33)).abs() * 0.5
    dec, p = _att(A, E, H, V, layers, Cf, 34, dropout=pd)
    dec.to(dev).train()
    seed = pin_dropout_seed(50 + layers)
    got = _gpu_run(dec, captions, lengths, af, tf, dev, True, seed_k=50 + layers)
    m = torch.from_numpy(R.embedding_mask(seed, B, T, E, pd)).double()
    lm = {l: torch.from_numpy(R.layer_mask(seed, N, H, pd, l)).double() for l in range(1, layers)}
    _check(got, _ref_run(stacked_lstm_att_forward, p, captions, lengths, af, tf, True, num_layers=layers, drop_mask=m,
                         layer_masks=lm))


# ---- 5. the fused upper step of the attention stack ---------------------------------------------------------------
@pytest.mark.parametrize("layers", [2, 3])
def test_fused_upper_step_at_twelve_rows(dev, monkeypatch, layers):
    """12 rows, every other step free running: each upper layer's lone steps are one launch of the LSTM-cell instance of
    csrc/lstm_upper_step.hip; against the composed path (CAPNET_NO_FUSED_UPPER_STEP=1) and the restatement, with
    dropout on."""
    E, H, V, B, T, A, Cf, P, pd = 24, 128, 61, 12, 9, 32, 512, 16, 0.3
    captions, lengths = _batch(B, V, T, 60 + layers, min_len=4)
    N = sum(lengths)
    tf = [t % 2 == 0 for t in range(max(lengths))]
    af = torch.randn(B, P, Cf, generator=torch.Generator().manual_seed(61)).abs() * 0.5
    dec, p = _att(A, E, H, V, layers, Cf, 62, dropout=pd)
    dec.to(dev).train()
    runs = {}
    for path in ("fused", "composed"):
        if path == "fused":
            monkeypatch.delenv(FUSED_UPPER_OFF, raising=False)
        else:
            monkeypatch.setenv(FUSED_UPPER_OFF, "1")
        seed = pin_dropout_seed(70)
        runs[path] = _gpu_run(dec, captions, lengths, af, tf, dev, True, seed_k=70)
    m = torch.from_numpy(R.embedding_mask(seed, B, T, E, pd)).double()
    lm = {l: torch.from_numpy(R.layer_mask(seed, N, H, pd, l)).double() for l in range(1, layers)}
    want = _ref_run(stacked_lstm_att_forward, p, captions, lengths, af, tf, True, num_layers=layers, drop_mask=m,
                    layer_masks=lm)
    _check(runs["fused"], want)
    _check(runs["composed"], want)
    assert _rel(runs["fused"][0], runs["composed"][0]) < TOL_LOGITS


# ---- 6. one decode step ----------------------------------------------------------------------------------------------
def _path(monkeypatch, path):
    if path == "fused":
        monkeypatch.delenv(FUSED_DECODE_OFF, raising=False)
    else:
        monkeypatch.setenv(FUSED_DECODE_OFF, "1")


def _step_inputs(rows, n_in, H, layers, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(rows, n_in, generator=g, dtype=torch.float64) * 2 - 1
    hs = [(torch.rand(rows, H, generator=g, dtype=torch.float64) - 0.5) * 0.6 for _ in range(layers)]
    cs = [(torch.rand(rows, H, generator=g, dtype=torch.float64) - 0.5) * 2.0 for _ in range(layers)]
    return x, hs, cs


def _state_err(st, ref_h, ref_c, off=0):
    st = st.double().cpu()
    return max(max(_rel(st[:, 2 * l], ref_h[l + off]), _rel(st[:, 2 * l + 1], ref_c[l + off]))
               for l in range(st.shape[1] // 2))


@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_forward_step_matches_restatement(dev, monkeypatch, path, layers):
    _path(monkeypatch, path)
    for E, H, V in ((12, 64, 37), (300, 512, 500)):
        dec, p = _plain(E, H, V, layers, 80 + layers)
        dec.to(dev).eval()
        for rows in (1, 5, 16, 17, 64, 320):
            x, hs, cs = _step_inputs(rows, E, H, layers, rows)
            top_r, h_r, c_r = stacked_step(p, x, hs, cs, layers)
            state = torch.stack([t for l in range(layers) for t in (hs[l], cs[l])], 1).float().to(dev)
            top, st = dec.forward_step(x.float().to(dev), state)
            assert _rel(top, top_r) < TOL_STEP, (E, rows, _rel(top, top_r))
            assert _state_err(st, h_r, c_r) < TOL_STEP, (E, rows)
            if rows == 5:     # the list-of-pairs form of the states
                top2, st2 = dec.forward_step(x.float().to(dev), [(state[:, 2 * l], state[:, 2 * l + 1])
                                                                 for l in range(layers)])
                assert torch.equal(top2, top) and torch.equal(st2, st)
    # attention stack: layer 0 on [embedding | context], then the upper layers
    A, E, H, V, Cf = 16, 24, 128, 41, 512
    dec, p = _att(A, E, H, V, layers, Cf, 90 + layers)
    dec.to(dev).eval()
    for rows in (1, 12, 65, 320):
        x, hs, cs = _step_inputs(rows, E + Cf, H, layers, 100 + rows)
        top_r, h_r, c_r = stacked_step(p, x, hs, cs, layers)
        states = [(hs[l].float().to(dev), cs[l].float().to(dev)) for l in range(layers)]
        top, (h0, c0, upper) = dec.forward_step(x.float().to(dev), states)
        assert _rel(top, top_r) < TOL_STEP and _rel(h0, h_r[0]) < TOL_STEP and _rel(c0, c_r[0]) < TOL_STEP, rows
        if layers > 1:
            assert _state_err(upper, h_r, c_r, off=1) < TOL_STEP, rows


def test_negative_control_factored_epilogue_is_far(dev):
    """The LSTM cell's packed weights through the factored instance (h = o c) must miss the restatement by far."""
    E, H, V, layers, rows = 300, 512, 500, 2, 17
    dec, p = _plain(E, H, V, layers, 95)
    dec.to(dev).eval()
    x, hs, cs = _step_inputs(rows, E, H, layers, 96)
    top_r, _, _ = stacked_step(p, x, hs, cs, layers)
    packed = [_pack_cell(c, (E + 15) // 16 * 16 if l == 0 else H) for l, c in enumerate(dec._cells())]
    state = torch.stack([t for l in range(layers) for t in (hs[l], cs[l])], 1).float().to(dev)
    args = (state, [w for w, _ in packed], [b for _, b in packed], x.float().to(dev))
    good, _ = ops.stacked_decode_step(*args, cell=ops.CELL_LSTM)
    bad, _ = ops.stacked_decode_step(*args, cell=ops.CELL_FACTORED)
    assert _rel(good, top_r) < TOL_STEP
    assert _rel(bad, top_r) > 0.05


# ---- 7. beam search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_sample_matches_restatement(dev, monkeypatch, layers):
    E, H, V, A, Cf, P = 12, 64, 37, 16, 512, 6
    dec, p = _plain(E, H, V, layers, 110 + layers)
    p = {k: v * (8.0 if k == "linear.weight" else 1.0) for k, v in p.items()}      # well-separated candidates
    dec.load_state_dict({k: v.float() for k, v in p.items()})
    dec.max_seq_length = 20
    dec.to(dev).eval()
    feat = torch.zeros(1, E, device=dev)
    end = greedy_path(p, layers, 1, 5)[4]
    for k in (1, 3, 5):
        assert beam_margin(p, layers, 1, end, k=k, max_seq_length=20) > 1e-4, k
        want = sample_stacked(p, layers, 1, end, k=k, max_seq_length=20).tolist()
        for path in ("fused", "composed"):
            _path(monkeypatch, path)
            assert dec.sample(feat, 1, end, k=k).cpu().tolist() == want, (k, path)
    adec, ap = _att(A, E, H, V, layers, Cf, 120 + layers)
    ap = {k: v * (8.0 if k == "linear.weight" else 1.0) for k, v in ap.items()}
    adec.load_state_dict({k: v.float() for k, v in ap.items()})
    adec.max_seq_length = 20
    adec.to(dev).eval()
    f = torch.rand(1, P, Cf, generator=torch.Generator().manual_seed(121), dtype=torch.float64)
    end = greedy_path(ap, layers, 1, 5, features=f)[4]
    for k in (1, 3, 5):
        assert beam_margin(ap, layers, 1, end, k=k, features=f, max_seq_length=20) > 1e-4, k
        want = sample_stacked(ap, layers, 1, end, k=k, features=f, max_seq_length=20).tolist()
        for path in ("fused", "composed"):
            _path(monkeypatch, path)
            assert adec.sample(f.float().to(dev), 1, end, k=k).cpu().tolist() == want, (k, path)


@pytest.mark.parametrize("layers", [1, 3])
def test_one_layer_sample_and_sample_batch(dev, monkeypatch, layers):
    """sample_batch equals per-image sample on both stacks and paths; at one layer sample equals DecoderRNN's /
    DecoderRNNAtt's."""
    E, H, V, A, Cf, P = 12, 64, 37, 16, 512, 6
    dec, _ = _plain(E, H, V, layers, 130)
    dec.max_seq_length = 12
    dec.to(dev).eval()
    adec, _ = _att(A, E, H, V, layers, Cf, 131)
    adec.max_seq_length = 12
    adec.to(dev).eval()
    feats = torch.randn(7, E, device=dev)
    afeats = torch.rand(7, P, Cf, device=dev)
    if layers == 1:
        ref = DecoderRNN(E, H, V, 1, max_seq_length=12)
        ref.load_state_dict(dec.state_dict())
        aref = DecoderRNNAtt(A, E, H, V, 1, feature_size=Cf, max_seq_length=12)
        aref.load_state_dict(adec.state_dict())
        ref.to(dev).eval()
        aref.to(dev).eval()
    for path in ("fused", "composed"):
        _path(monkeypatch, path)
        for d, f, r in ((dec, feats, ref if layers == 1 else None), (adec, afeats, aref if layers == 1 else None)):
            batched = d.sample_batch(f, 1, 2, k=5)
            assert len(batched) == 7
            for i in range(7):
                one = d.sample(f[i:i + 1], 1, 2, k=5)[0].cpu().tolist()
                assert list(batched[i]) == one, (path, i)
                if r is not None:
                    assert r.sample(f[i:i + 1], 1, 2, k=5)[0].cpu().tolist() == one, (path, i)


# ---- 8. the training, validation and test-set loops -------------------------------------------------------------------
class _Vocab:
    def __init__(self, V):
        self.word2idx = {'<pad>': 0, '<start>': 1, '<end>': 2, '<unk>': 3}
        self.idx2word = {i: "w%d" % i for i in range(V)}
        self.idx2word.update({0: '<pad>', 1: '<start>', 2: '<end>', 3: '<unk>'})


class _FixedFeatures(nn.Module):
    """Stands in for EncoderCNN: the loader yields the features themselves."""

    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(1, 1)

    def forward(self, images):
        return images


def _loader(V, shape, seed):
    g = torch.Generator().manual_seed(seed)
    batches = []
    for b in (5, 3):
        lengths = sorted([int(v) for v in torch.randint(3, 9, (b,), generator=g)], reverse=True)
        captions = torch.randint(3, V, (b, max(lengths)), generator=g)
        captions[:, 0] = 1
        feats = torch.rand((b,) + shape, generator=g)
        all_caps = [[captions[i, :lengths[i]].clone(), captions[i, :lengths[i]].flip(0)] for i in range(b)]
        batches.append((feats, captions, lengths, all_caps))
    return batches


def _bleu_of_samples(dec, batches, dev, k):
    refs, hyps = [], []
    for feats, _, _, all_caps in batches:
        for i in range(feats.size(0)):
            hyps.append(dec.sample(feats[i:i + 1].to(dev), 1, 2, k=k)[0].cpu().tolist())
            refs.append([[int(w) for w in c.tolist()] for c in all_caps[i]])
    return tuple(corpus_bleu(refs, hyps, weights=w)
                 for w in ((1, 0, 0, 0), (0.5, 0.5, 0, 0), (0.33, 0.33, 0.33, 0), (0.25, 0.25, 0.25, 0.25)))


@pytest.mark.parametrize("layers", [2, 3])
def test_training_validation_and_evaluation_loops(dev, layers):
    E, H, V, A, Cf, P = 12, 64, 37, 16, 512, 6
    enc, vocab = _FixedFeatures().to(dev), _Vocab(V)
    dec = StackedDecoderRNN(E, H, V, layers).to(dev)
    batches = _loader(V, (E,), 140)
    opt = Adam(list(dec.parameters()), lr=1e-3)
    before = dec.lstm1.weight_hh.detach().clone()
    for feats, captions, lengths, _ in batches:
        loss = train_step(enc, dec, opt, CrossEntropyLoss(), feats.to(dev), captions.to(dev), lengths, 5.0,
                          teacher_forcing_ratio=0.5)
        assert torch.isfinite(torch.as_tensor(loss)).all()
    assert not torch.equal(before, dec.lstm1.weight_hh.detach())
    bt, top5, vloss, bleu = val_factual(enc, dec, vocab, CrossEntropyLoss(), batches, device=dev)
    assert vloss > 0 and 0 <= top5 <= 100 and 0 <= bleu <= 1
    assert evaluate(enc, dec, vocab, batches, mode=None, k=3, device=dev) == _bleu_of_samples(dec, batches, dev, 3)

    adec = StackedDecoderRNNAtt(A, E, H, V, layers, feature_size=Cf).to(dev)
    abatches = _loader(V, (P, Cf), 141)
    opt = Adam(list(adec.parameters()), lr=1e-3)
    before = adec.init_h1.weight.detach().clone()
    for feats, captions, lengths, _ in abatches:
        loss = train_step_att(enc, adec, opt, CrossEntropyLoss(), feats.to(dev), captions.to(dev), lengths, 5.0,
                              teacher_forcing_ratio=0.5)
        assert torch.isfinite(torch.as_tensor(loss)).all()
    assert not torch.equal(before, adec.init_h1.weight.detach())
    assert evaluate(enc, adec, vocab, abatches, mode=None, k=3, device=dev) == _bleu_of_samples(adec, abatches, dev, 3)
