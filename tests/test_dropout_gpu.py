"""Every decoder with dropout ON against the fp64 oracle run with the very masks the kernels draw.

The kernels draw the dropout mask from a counter hash of (seed, sample, column, unit) and draw it again in backward
(csrc/dropout_mask.h); oracle/dropout_ref.py restates that hash in numpy, and tests/helpers.pin_dropout_seed gives the
seed the decoder's forward draws (capnet.model._dropout_seed). So the oracles (oracle/decoders_ref.py,
tests/stacked_att_ref.py) run with the same masks, and logits, loss, every parameter gradient and dfeatures are held to
the bounds of each family's dropout-0 test. What only a dropout-on comparison sees: only teacher-forced embeddings are
dropped (not the image-feature row, not the free-running feedback B(predicted), not B(<start>) of a free-running first
step), the mask entry is the one of the caption column the step reads, kept units are scaled by 1/(1-p), forward and
backward draw at the same coordinates, and the masks between stacked layers are keyed by layer and packed row.

In one case per family a negative control runs the oracle with a deliberately wrong mask (shifted by one caption
column, or keyed by the wrong layer or row): it must land at least 100x farther from the GPU than the right mask, and
the mask-free oracle must too, so the comparison can tell the difference and dropout really acted."""
import random

import pytest
import torch
import torch.nn.functional as Fn

from capnet import ops, synthetic
from capnet.model import DecoderFactoredLSTM
from capnet.model_att import DecoderFactoredLSTMAtt
from capnet.nic_model import DecoderRNN
from capnet.nic_model_att import DecoderRNNAtt
from capnet.stacked import StackedFactoredLSTM
from capnet.stacked_att import StackedFactoredLSTMAtt
from helpers import pin_dropout_seed, rel_err
from oracle import decoders_ref as D
from oracle import dropout_ref as R
from stacked_att_ref import stacked_factored_att_forward
from test_edge_cases_gpu import LENGTH_SETS, _captions

pytestmark = pytest.mark.gpu


def grad_close(a, b, rtol):
    """max|a-b| <= rtol*max|b| + 1e-6 (full_att.bias has an exactly-zero gradient: rounding noise on both sides)."""
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return (a - b).abs().max().item() <= rtol * b.abs().max().item() + 1e-6


def _tf(kind, T, seed):
    if kind == "teacher":
        return [True] * T
    if kind == "free":
        return [False] * T
    random.seed(seed)
    tf = [random.random() < 0.6 for _ in range(T)]
    for i, v in enumerate([True, True, False, True, False, True]):     # free-running steps between dropped ones
        if 1 + i < T:
            tf[1 + i] = v
    return tf


def _emb_mask(seed, captions, E, p):
    B, T = captions.shape
    return torch.from_numpy(R.embedding_mask(seed, B, T, E, p)).double()


def _layer_masks(seed, N, H, p, layers, key=lambda l: l):
    return {l: torch.from_numpy(R.layer_mask(seed, N, H, p, key(l))).double() for l in range(1, layers)}


def _shift_columns(m):
    """The mask of caption column c - 1 at column c: the off-by-one a kernel would make by keying the mask with the step
    instead of the caption column it reads (or the other way round)."""
    return torch.roll(m, 1, dims=1)


class _Case:
    """One decoder and its inputs; runs the product and the fp64 oracle with the restated masks and compares them."""

    def __init__(self, dec, p, forward, captions, lengths, feats, tf, att=False, num_layers=None, **kw):
        self.dec, self.p, self.forward = dec, p, forward
        self.captions, self.lengths, self.feats, self.tf, self.att, self.kw = captions, lengths, feats, tf, att, kw
        self.okw = dict(kw, num_layers=num_layers) if num_layers else kw

    def product(self, dev, k):
        dec = self.dec
        dec.zero_grad()
        f = None
        if self.feats is not None:
            f = self.feats.to(dev)
            if not self.att:
                f.requires_grad_(True)
        cap = self.captions.to(dev)
        targets = D.packed_targets(self.captions, self.lengths).to(dev)
        seed = pin_dropout_seed(k)
        res = dec(cap, self.lengths, f, tf_mask=self.tf, **self.kw)
        if self.att:
            out, alphas = res
            loss = ops.attention_loss(ops.cross_entropy(out, targets), alphas, 1.0)
        else:
            out, alphas = res, None
            loss = ops.cross_entropy(out, targets)
        loss.backward()
        ops.check_device_errors()
        self.seed, self.out, self.alphas, self.loss, self.f = seed, out.detach(), alphas, loss, f
        return seed

    def _call(self, leaves, feats, **masks):
        res = self.forward(leaves, self.captions, self.lengths, feats, self.tf, **self.okw, **masks)
        return res if self.att else (res, None)

    def oracle(self, **masks):
        leaves = {k: v.double().requires_grad_(True) for k, v in self.p.items()}
        feats = None
        if self.feats is not None:
            feats = self.feats.double().requires_grad_(not self.att)
        logits, alphas = self._call(leaves, feats, **masks)
        targets = D.packed_targets(self.captions, self.lengths)
        loss = D.att_loss(logits, alphas, targets) if self.att else Fn.cross_entropy(logits, targets)
        loss.backward()
        self.ref = dict(logits=logits.detach(), alphas=None if alphas is None else alphas.detach(), loss=loss.item(),
                        grads={k: v.grad for k, v in leaves.items()},
                        dfeat=feats.grad if (feats is not None and not self.att) else None)
        return self.ref

    def logits_with(self, **masks):
        leaves = {k: v.double() for k, v in self.p.items()}
        with torch.no_grad():
            return self._call(leaves, None if self.feats is None else self.feats.double(), **masks)[0]

    def compare(self, name, tol_logits, tol_grad, control=None):
        """Asserts the family's bounds; control: {"label": oracle logits of a wrong mask (or none)}, each of which must
        be >= 100x farther from the GPU than the right mask."""
        ref = self.ref
        e_logits = rel_err(self.out, ref["logits"])
        e_loss = abs(self.loss.item() - ref["loss"]) / abs(ref["loss"])
        worst, worst_k, n, bad = 0.0, None, 0, []
        for k, prm in self.dec.named_parameters():
            gr = ref["grads"][k]
            if gr is None or float(gr.abs().max()) == 0.0:
                if not (prm.grad is None or float(prm.grad.abs().max()) == 0.0):    # the other modes' S
                    bad.append((k, "gradient where the oracle has none"))
                continue
            if prm.grad is None:
                bad.append((k, "no gradient"))
                continue
            if self.att:
                ok = grad_close(prm.grad, gr, tol_grad)
            else:
                ok = rel_err(prm.grad, gr) < tol_grad or float(gr.abs().max()) < 1e-7
            if not ok:
                bad.append((k, rel_err(prm.grad, gr)))
            if float(gr.abs().max()) > 1e-4:
                e = rel_err(prm.grad, gr)
                if e > worst:
                    worst, worst_k = e, k
            n += 1
        assert n > 0
        msg = "%s: seed %#x logits %.2e loss %.2e worst grad %.2e (%s)" % (name, self.seed, e_logits, e_loss, worst,
                                                                          worst_k)
        e_dfeat = None
        if ref["dfeat"] is not None and float(ref["dfeat"].abs().max()) > 0:
            e_dfeat = rel_err(self.f.grad, ref["dfeat"])
            msg += " dfeatures %.2e" % e_dfeat
        if self.alphas is not None:
            e_alphas = rel_err(self.alphas, ref["alphas"])
            msg += " alphas %.2e" % e_alphas
        for label, wrong in (control or {}).items():
            e_wrong = rel_err(self.out, wrong)
            msg += " | %s %.2e (%.0fx)" % (label, e_wrong, e_wrong / max(e_logits, 1e-30))
        print(msg)
        assert not bad, (msg, bad)
        assert e_logits < tol_logits, msg
        assert e_loss < 1e-5, msg
        if e_dfeat is not None:
            assert e_dfeat < tol_grad, msg
        if self.alphas is not None:
            assert e_alphas < tol_logits, msg
        for label, wrong in (control or {}).items():
            assert rel_err(self.out, wrong) >= 100 * e_logits, (label, msg)


# ---- DecoderFactoredLSTM: 5e-5 logits, 2e-4 gradients (test_decoder_gpu.py) --------------------------------------
def _factored(dev, B, V, E, F, H, mode, p, kind, feats=True, seed=0, lengths=None):
    dec = DecoderFactoredLSTM(E, H, F, V, 1, dropout=p)
    prm = synthetic.decoder_state(dec.state_dict(), seed=B + seed, bias_range=0.05)
    dec.load_state_dict(prm)
    dec.to(dev).train()
    if lengths is None:
        _, captions, lengths = synthetic.make_batch(B, V, seed=17 + B + seed, images=False, min_len=3, max_len=12)
    else:
        captions = _captions(lengths, V, 3 + seed)
    f = torch.randn(len(lengths), E, generator=torch.Generator().manual_seed(B + 1)) if feats else None
    return _Case(dec, prm, D.factored_lstm_forward, captions, lengths, f, _tf(kind, max(lengths), seed), mode=mode)


@pytest.mark.parametrize("p", [0.22, 0.5])
@pytest.mark.parametrize("kind", ["teacher", "free", "mixed"])
def test_factored_ragged(dev, p, kind):
    c = _factored(dev, 9, 203, 20, 24, 28, "sad", p, kind, seed=int(p * 100))
    seed = c.product(dev, 1)
    m = _emb_mask(seed, c.captions, 20, p)
    c.oracle(drop_mask=m)
    control = None
    if p == 0.5 and kind == "mixed":
        control = {"column-shifted mask": c.logits_with(drop_mask=_shift_columns(m)),
                   "no mask": c.logits_with()}
    c.compare("factored ragged p=%.2f %s" % (p, kind), 5e-5, 2e-4, control)


@pytest.mark.parametrize("p,kind", [(0.22, "mixed"), (0.5, "teacher")])
def test_factored_full_cell(dev, p, kind):
    c = _factored(dev, 64, 7411, 300, 512, 512, "factual", p, kind, seed=2)
    seed = c.product(dev, 2)
    c.oracle(drop_mask=_emb_mask(seed, c.captions, 300, p))
    c.compare("factored 64 x 7411 p=%.2f %s" % (p, kind), 5e-5, 2e-4)


@pytest.mark.parametrize("kind", ["free_first", "teacher"])
def test_factored_without_features(dev, kind):
    """features=None: step t reads caption column t; a free-running first step reads B(<start>) undropped."""
    p = 0.5
    c = _factored(dev, 9, 203, 20, 24, 28, "happy", p, "mixed" if kind == "free_first" else "teacher", feats=False,
                  seed=5)
    if kind == "free_first":
        c.tf[0] = False
    seed = c.product(dev, 3)
    m = _emb_mask(seed, c.captions, 20, p)
    c.oracle(drop_mask=m)
    control = None
    if kind == "free_first":
        control = {"column-shifted mask": c.logits_with(drop_mask=_shift_columns(m)), "no mask": c.logits_with()}
    c.compare("factored no features %s" % kind, 5e-5, 2e-4, control)


@pytest.mark.parametrize("name", list(LENGTH_SETS))
@pytest.mark.parametrize("kind", ["teacher", "free", "mixed"])
def test_factored_edge_lengths(dev, name, kind):
    p = 0.5
    c = _factored(dev, 0, 57, 20, 24, 32, "factual", p, kind, seed=len(LENGTH_SETS[name]),
                  lengths=LENGTH_SETS[name])
    seed = c.product(dev, 4)
    c.oracle(drop_mask=_emb_mask(seed, c.captions, 20, p))
    c.compare("factored edge %s %s" % (name, kind), 5e-5, 2e-4)


# ---- DecoderRNN: configs[0] (8 x V 8192), 5e-5 / 2e-4 -----------------------------------------------------------
@pytest.mark.parametrize("p", [0.22, 0.5])
def test_nic(dev, p):
    B, V, E, H = 8, 8192, 300, 512
    dec = DecoderRNN(E, H, V, 1, dropout=p)
    prm = synthetic.decoder_state(dec.state_dict(), seed=3, bias_range=0.05)
    dec.load_state_dict(prm)
    dec.to(dev).train()
    _, captions, lengths = synthetic.make_batch(B, V, seed=5, images=False, min_len=3, max_len=24)
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(6))
    c = _Case(dec, prm, D.lstm_forward, captions, lengths, feats, _tf("mixed", max(lengths), 7))
    seed = c.product(dev, 5)
    m = _emb_mask(seed, captions, E, p)
    c.oracle(drop_mask=m)
    control = None
    if p == 0.5:
        control = {"column-shifted mask": c.logits_with(drop_mask=_shift_columns(m)), "no mask": c.logits_with()}
    c.compare("nic 8 x 8192 p=%.2f" % p, 5e-5, 2e-4, control)


# ---- DecoderFactoredLSTMAtt: 1e-4 logits, grad_close 5e-4 (test_decoder_att_gpu.py) ------------------------------
@pytest.fixture(params=[-1, 1], ids=["chain-3-products", "chain-1-product"])
def chain(request):
    from capnet._lib import lib
    old = lib().capnet_att_set_chain_mode(request.param)
    yield request.param
    lib().capnet_att_set_chain_mode(old)


_ORACLE_CACHE = {}


def _att_case(dev, cls, forward, B, V, A, E, H, P, p, kind, F=None, mode=None, seed=0):
    Cf = 512 if P < 100 else 2048
    dec = cls(A, E, H, F, V, 1, feature_size=Cf, dropout=p) if F else cls(A, E, H, V, 1, feature_size=Cf, dropout=p)
    prm = synthetic.decoder_state(dec.state_dict(), seed=B + seed, bias_range=0.05)
    dec.load_state_dict(prm)
    dec.to(dev).train()
    _, captions, lengths = synthetic.make_batch(B, V, seed=40 + B + seed, images=False, min_len=3, max_len=10)
    feats = torch.randn(B, P, Cf, generator=torch.Generator().manual_seed(B)).abs() * 0.5
    kw = {"mode": mode} if mode else {}
    return _Case(dec, prm, forward, captions, lengths, feats, _tf(kind, max(lengths), seed), att=True, **kw)


def _att_oracle(c, key, E, p):
    """The fp64 oracle of a case (the same for both chain forms: the seed is pinned)."""
    if key not in _ORACLE_CACHE:
        m = _emb_mask(c.seed, c.captions, E, p)
        _ORACLE_CACHE[key] = (c.seed, c.oracle(drop_mask=m), m)
    seed, ref, m = _ORACLE_CACHE[key]
    assert seed == c.seed
    c.ref = ref
    return m


@pytest.mark.parametrize("B,V,A,E,F,H,P,p,kind", [
    (5, 203, 24, 20, 24, 28, 9, 0.22, "mixed"),
    (5, 203, 24, 20, 24, 28, 9, 0.5, "teacher"),
    (5, 203, 24, 20, 24, 28, 9, 0.5, "free"),
    (12, 1000, 512, 300, 512, 512, 196, 0.22, "mixed"),
    (40, 1000, 512, 300, 512, 512, 196, 0.5, "mixed"),
])
def test_factored_att(dev, chain, B, V, A, E, F, H, P, p, kind):
    c = _att_case(dev, DecoderFactoredLSTMAtt, D.factored_att_forward, B, V, A, E, H, P, p, kind, F=F, mode="angry")
    c.product(dev, 6)
    m = _att_oracle(c, ("factored_att", B, p, kind), E, p)
    control = None
    if B == 5 and kind == "mixed":
        control = {"column-shifted mask": c.logits_with(drop_mask=_shift_columns(m)), "no mask": c.logits_with()}
    c.compare("factored att B=%d p=%.2f %s chain %d" % (B, p, kind, chain), 1e-4, 5e-4, control)


# ---- DecoderRNNAtt: full size, 1e-4 / 5e-4 ----------------------------------------------------------------------
@pytest.mark.parametrize("B,p", [(12, 0.22), (33, 0.5)])
def test_nic_att(dev, B, p):
    V, A, E, H, P = 1000, 512, 300, 512, 196
    c = _att_case(dev, DecoderRNNAtt, D.lstm_att_forward, B, V, A, E, H, P, p, "mixed", seed=1)
    seed = c.product(dev, 7)
    m = _emb_mask(seed, c.captions, E, p)
    c.oracle(drop_mask=m)
    control = None
    if B == 12:
        control = {"column-shifted mask": c.logits_with(drop_mask=_shift_columns(m)), "no mask": c.logits_with()}
    c.compare("nic att B=%d p=%.2f" % (B, p), 1e-4, 5e-4, control)


# ---- StackedFactoredLSTM: embedding and between-layer masks, 2e-5 / 2e-4 (test_stacked_gpu.py) --------
@pytest.mark.parametrize("p,kind", [(0.22, "mixed"), (0.5, "teacher"), (0.5, "free")])
def test_stacked(dev, p, kind):
    E, H, F, V, B, L = 300, 512, 1024, 500, 8, 3
    dec = StackedFactoredLSTM(E, H, F, V, L, dropout=p)
    prm = synthetic.decoder_state(dec.state_dict(), seed=11, bias_range=0.05)
    dec.load_state_dict(prm)
    dec.to(dev).train()
    _, captions, lengths = synthetic.make_batch(B, V, seed=12, images=False, min_len=4, max_len=14)
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(13))
    c = _Case(dec, prm, D.stacked_factored_lstm_forward, captions, lengths, feats, _tf(kind, max(lengths), 14),
              mode="happy", num_layers=L)
    seed = c.product(dev, 8)
    N = sum(lengths)
    m, lm = _emb_mask(seed, captions, E, p), _layer_masks(seed, N, H, p, L)
    c.oracle(drop_mask=m, layer_masks=lm)
    control = None
    if kind == "mixed":
        control = {"layer masks keyed by layer + 1": c.logits_with(drop_mask=m, layer_masks=_layer_masks(
                       seed, N, H, p, L, key=lambda l: l + 1)),
                   "no layer masks": c.logits_with(drop_mask=m),
                   "no mask": c.logits_with()}
    c.compare("stacked 3 x F1024 p=%.2f %s" % (p, kind), 2e-5, 2e-4, control)


# ---- StackedFactoredLSTMAtt: 2e-5 / grad_close 2e-4 (test_stacked_att_gpu.py) -----------------------------------
SMALL = dict(A=32, E=24, H=64, F=32, V=97, Cf=512, P=9)
WIDE = dict(A=64, E=48, H=512, F=64, V=97, Cf=512, P=9)
CONFIG3 = dict(A=512, E=300, H=512, F=512, V=8192, Cf=2048, P=196)


def _stacked_att(dev, s, layers, B, T, p, kind, seed, xavier=False):
    """xavier: the reference's initialisation (capnet.synthetic.decoder_state) instead of test_stacked_att_gpu.py's
    U(+-0.3), which at 2048 feature channels saturates the cell: there an fp32 restatement on the CPU already lands
    0.5 - 0.8 (relative) from the fp64 one, a chaotic problem no fp32 implementation can be held to."""
    dec = StackedFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], layers, feature_size=s["Cf"], dropout=p)
    g = torch.Generator().manual_seed(seed)
    prm = {k: (torch.rand(v.shape, generator=g) * 2 - 1) * (0.3 if v.dim() > 1 else 0.05)
           for k, v in dec.state_dict().items()}
    if xavier:
        prm = synthetic.decoder_state(dec.state_dict(), seed=seed, bias_range=0.05)
    dec.load_state_dict(prm)
    dec.to(dev).train()
    lengths = sorted([int(v) for v in torch.randint(3, T + 1, (B,), generator=g)], reverse=True)
    lengths[0] = T
    captions = torch.randint(3, s["V"], (B, T), generator=g)
    feats = torch.randn(B, s["P"], s["Cf"], generator=g).abs() * 0.5
    return _Case(dec, prm, stacked_factored_att_forward, captions, lengths, feats, _tf(kind, T, seed), att=True,
                 mode="sad", num_layers=layers)


@pytest.mark.parametrize("shape,layers,B,p,kind", [
    ("small", 3, 12, 0.22, "free"),        # B <= 16: the fused upper step
    ("small", 2, 12, 0.5, "mixed"),
    ("small", 3, 40, 0.22, "teacher"),     # B 40: rows_dropout and the composed step
    ("small", 2, 40, 0.5, "mixed"),
    ("wide", 2, 12, 0.22, "mixed"),
    ("wide", 3, 12, 0.5, "teacher"),
    ("wide", 2, 40, 0.5, "free"),
    ("wide", 3, 40, 0.22, "mixed"),
    ("wide", 3, 12, 0.0, "teacher"),       # the two 3-layer WIDE shapes without dropout, for their bound
    ("wide", 3, 40, 0.0, "mixed"),
])
def test_stacked_att(dev, shape, layers, B, p, kind):
    """Bounds: test_stacked_att_gpu.py's 2e-5 logits / 2e-4 gradients, except 4e-5 on the logits with three layers at
    H 512 (only two are met there at dropout 0): an fp32 restatement on the CPU lands 1.4e-5 .. 4.3e-5 from the fp64
    one on these inputs, dropout or not (p = 0: 2.0e-5 and 3.5e-5), so 2e-5 is below what fp32 can do here."""
    s = SMALL if shape == "small" else WIDE
    c = _stacked_att(dev, s, layers, B, 9, p, kind, seed=B + layers)
    seed = c.product(dev, 9)
    N = sum(c.lengths)
    m, lm = _emb_mask(seed, c.captions, s["E"], p), _layer_masks(seed, N, s["H"], p, layers)
    if p == 0.0:
        m, lm = None, None
    c.oracle(drop_mask=m, layer_masks=lm)
    control = None
    if kind == "mixed" and layers == 2:
        shifted = {l: torch.roll(v, 1, dims=0) for l, v in lm.items()}
        control = {"layer mask of the neighbouring row": c.logits_with(drop_mask=m, layer_masks=shifted),
                   "no layer masks": c.logits_with(drop_mask=m), "no mask": c.logits_with()}
    tol = 4e-5 if (shape == "wide" and layers == 3) else 2e-5
    c.compare("stacked att %s L%d B=%d p=%.2f %s" % (shape, layers, B, p, kind), tol, 2e-4, control)


@pytest.mark.parametrize("p", [0.0, 0.22])
def test_stacked_att_config3_full_size(dev, p):
    """configs[3]'s decoder: 2 layers at the full attention cell and V 8192, B 12. The bounds are the attention family's
    at full size (1e-4 / 5e-4, test_decoder_att_gpu.py): the restatement had only been met at small widths before."""
    c = _stacked_att(dev, CONFIG3, 2, 12, 10, p, "mixed", seed=33, xavier=True)
    seed = c.product(dev, 10)
    if p == 0.0:
        c.oracle()
        c.compare("stacked att configs[3] p=0", 1e-4, 5e-4)
        return
    N = sum(c.lengths)
    c.oracle(drop_mask=_emb_mask(seed, c.captions, CONFIG3["E"], p),
             layer_masks=_layer_masks(seed, N, CONFIG3["H"], p, 2))
    c.compare("stacked att configs[3] p=%.2f" % p, 1e-4, 5e-4)
