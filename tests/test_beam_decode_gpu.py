"""The one-call beam search of the plain stacks (capnet_beam_decode) and the gathered decode step under it
(capnet_stacked_decode_step_gather): the gathered step against gather-then-step bit for bit; one_call=True against
on_device=True (equal: same kernels, rows and slab) and the fp64 restatement; the one-layer reference classes, whose
fold changes the arithmetic, under the margin rule; poll_every; the fallbacks; evaluate."""
import pytest
import torch

import capnet
from beam_decode_cases import families as one_layer_families
from capnet import _lib, ops
from capnet._lib import check, ptr, ptr_array
from capnet.model import DecoderFactoredLSTM
from capnet.nic_model import DecoderRNN
from device_beam_cases import IMAGES, KS, MAX_LEN, START, families
from helpers import load_golden, t

pytestmark = pytest.mark.gpu

STACKS = [f for f in families() if f.name in ("StackedFactoredLSTM-2", "StackedDecoderRNN-2")]
assert len(STACKS) == 2


def _family(name):
    return [f for f in families() if f.name == name][0]


# ---- 1. the gathered step ------------------------------------------------------------------------------------------
H, V = 64, 23


def _step_inputs(dev, L, E, rows, seed):
    g = torch.Generator().manual_seed(seed)
    kin = (E + 15) // 16 * 16

    def u(*shape, a=1.0):
        return ((torch.rand(shape, generator=g) * 2 - 1) * a).to(dev)
    wcat, beff = [], []
    for l in range(L):
        w = u(4 * H, (kin if l == 0 else H) + H, a=0.2)
        if l == 0:
            w[:, E:kin] = 0
        wcat.append(w.contiguous())
        beff.append(u(4 * H, a=0.1))
    emb = u(V, E)
    tokens = torch.randint(0, V, (rows,), generator=g).to(dev)
    state = u(rows, 2 * L, H)
    # a reversal in which every third row shares row 0's parent: repeats, and rows that nobody reads
    parent = [rows - 1 - r for r in range(rows)]
    parent = [parent[0] if r % 3 == 1 else p for r, p in enumerate(parent)]
    return wcat, beff, emb, tokens, state, torch.tensor(parent, dtype=torch.long, device=dev)


@pytest.mark.parametrize("rows", [1, 5, 17, 33])
@pytest.mark.parametrize("E", [12, 10], ids=["x-f32x4", "x-scalar"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("cell", [ops.CELL_FACTORED, ops.CELL_LSTM], ids=["factored", "lstm"])
def test_gathered_step_equals_gather_then_step(dev, cell, L, E, rows):
    wcat, beff, emb, tokens, state, parent = _step_inputs(dev, L, E, rows, 100 * L + 10 * E + rows)
    want_top, want = ops.stacked_decode_step(state.index_select(0, parent), wcat, beff, emb, tokens, cell=cell)
    top, out = ops.stacked_decode_step(state, wcat, beff, emb, tokens, cell=cell, parent_rows=parent)
    assert torch.equal(out, want) and torch.equal(top, want_top)
    assert rows < 3 or not torch.equal(out, ops.stacked_decode_step(state, wcat, beff, emb, tokens, cell=cell)[1])
    # layer 0 on given inputs instead of token ids: x stays on the row itself
    x = emb.index_select(0, tokens).contiguous()
    top, out = ops.stacked_decode_step(state, wcat, beff, x, None, cell=cell, parent_rows=parent)
    assert torch.equal(out, want) and torch.equal(top, want_top)
    # a null parent is the existing call
    want_top, want = ops.stacked_decode_step(state, wcat, beff, emb, tokens, cell=cell)
    out, top = torch.empty_like(state), torch.empty(rows, H, device=dev)
    check(_lib.lib().capnet_stacked_decode_step_gather(cell, L, rows, E, H, V, ptr(tokens), ptr(emb), ptr_array(wcat),
                                                       ptr_array(beff), ptr(state), None, ptr(out), ptr(top),
                                                       ptr(ops.err_flag(dev)), _lib.current_stream()), "gather")
    assert torch.equal(out, want) and torch.equal(top, want_top)
    ops.check_device_errors()


@pytest.mark.parametrize("bad", ["rows", -1])
@pytest.mark.parametrize("rows", [5, 17])
def test_a_parent_out_of_range_sets_the_flag_and_reads_the_row_itself(dev, rows, bad):
    ops.check_device_errors()
    wcat, beff, emb, tokens, state, parent = _step_inputs(dev, 2, 12, rows, 7)
    r = rows - 2
    mended = parent.clone()
    mended[r] = r
    want_top, want = ops.stacked_decode_step(state, wcat, beff, emb, tokens, parent_rows=mended)
    ops.check_device_errors()
    parent[r] = rows if bad == "rows" else bad
    top, out = ops.stacked_decode_step(state, wcat, beff, emb, tokens, parent_rows=parent)
    assert torch.equal(out, want) and torch.equal(top, want_top)
    with pytest.raises(capnet.CapnetError):
        ops.check_device_errors()
    ops.check_device_errors()                       # (the check cleared the flag)


# ---- 2. one call equals the device loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("family", STACKS, ids=lambda f: f.name)
def test_one_call_equals_the_device_loop(dev, monkeypatch, family):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    assert getattr(dec._beam(KS[0], *kw.values())[0], "plain", None) is not None      # the one call does run
    for k in KS:
        want = [family.reference(k, i) for i in range(IMAGES)]
        loop = dec.sample_batch(feats, START, end, k=k, on_device=True, **kw)
        assert dec.sample_batch(feats, START, end, k=k, one_call=True, **kw) == loop == want, k
        for i in range(IMAGES):
            one = dec.sample(feats[i:i + 1], START, end, k=k, one_call=True, **kw)
            assert one.dtype == torch.int64 and one.dim() == 2 and one.device.type == "cuda"
            assert one.cpu().tolist() == dec.sample(feats[i:i + 1], START, end, k=k, on_device=True, **kw).cpu().tolist() \
                == [want[i]], (k, i)
    ops.check_device_errors()


# ---- 3. the one-layer reference classes ----------------------------------------------------------------------------
@pytest.mark.parametrize("family", one_layer_families(), ids=lambda f: f.name)
def test_one_layer_classes(dev, monkeypatch, family):
    """DecoderFactoredLSTM (mode happy) and DecoderRNN: one_call=True runs the folded / packed cell on the fused step, the
    default host path the composed chain. Every (k, image) has the margin (tests/test_beam_decode_cpu.py), so all three
    -- one call, host path, fp64 restatement -- must agree; nothing is skipped."""
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    assert getattr(dec._beam(KS[0], *kw.values(), True)[0], "plain", None) is not None
    for k in KS:
        want = [family.reference(k, i) for i in range(IMAGES)]
        assert dec.sample_batch(feats, START, end, k=k, **kw) == want, k
        assert dec.sample_batch(feats, START, end, k=k, one_call=True, **kw) == want, k
        for i in range(IMAGES):
            assert dec.sample(feats[i:i + 1], START, end, k=k, one_call=True, **kw).cpu().tolist() == [want[i]], (k, i)
    ops.check_device_errors()


# ---- 4. poll_every -------------------------------------------------------------------------------------------------
def _biased(dev, end_bias):
    family = _family("StackedDecoderRNN-2")
    dec = family.make().to(dev).eval()
    with torch.no_grad():
        dec.linear.bias[family.end] += end_bias
    return family, dec


def _one_call(dec, n, k, end, poll):
    plain = dec._beam(n * k)[0].plain
    return ops.beam_decode(plain.cell, plain.wcat, plain.beff, plain.emb, plain.Cw, plain.Cb, n, k, dec.max_seq_length + 1,
                           START, end, poll_every=poll, return_steps=True)


@pytest.mark.parametrize("k", KS)
def test_poll_every_stops_early_with_the_same_result(dev, monkeypatch, k):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family, dec = _biased(dev, 60.0)                 # <end> wins on every row from the first step on
    feats, end = family.features().to(dev), family.end
    want, steps = _one_call(dec, IMAGES, k, end, 0)
    assert steps == MAX_LEN + 1
    assert all(2 <= len(s) <= 3 and s[0] == START and s[-1] == end for s in want), want
    assert want == dec.sample_batch(feats, START, end, k=k, on_device=True)
    for m in (1, 3):
        got, steps = _one_call(dec, IMAGES, k, end, m)
        assert got == want and steps <= 2 + m, (m, steps)
        assert dec.sample_batch(feats, START, end, k=k, one_call=True, poll_every=m) == want, m
    ops.check_device_errors()


def test_nothing_completed_returns_end(dev, monkeypatch):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family, dec = _biased(dev, -60.0)
    for m in (0, 3):
        got, steps = _one_call(dec, IMAGES, 3, family.end, m)
        assert got == [[family.end]] * IMAGES and steps == MAX_LEN + 1, m
    assert dec.sample_batch(family.features().to(dev), START, family.end, k=3, one_call=True) == [[family.end]] * IMAGES
    ops.check_device_errors()


# ---- 5. fallbacks --------------------------------------------------------------------------------------------------
Z = load_golden("sample_tiny.npz")


def _golden(name, dev):
    """The `sample_tiny` decoders without attention (hidden size 16: a shape the decode-step kernel does not take)."""
    pre = "case.%s." % name
    c = {k[len(pre):]: Z[k] for k in Z.files if k.startswith(pre)}
    params = {k[len("param."):]: t(v) for k, v in c.items() if k.startswith("param.")}
    kind = str(c["kind"])
    E, H_, F, V_, k, maxlen = [int(v) for v in c["dims"]][:6]
    if kind == "factored":
        dec = DecoderFactoredLSTM(E, H_, F, V_, 1, dropout=0.0, max_seq_length=maxlen)
    elif kind == "nic":
        dec = DecoderRNN(E, H_, V_, 1, dropout=0.0, max_seq_length=maxlen)
    else:
        return None
    dec.load_state_dict(params)
    return dec.to(dev).eval(), c, k, ({} if kind == "nic" else {"mode": str(c["mode"])}), torch.zeros(3, E, device=dev)


def test_an_unsupported_hidden_size_takes_the_device_loop(dev):
    start, end = [int(v) for v in Z["start_end"]]
    seen = 0
    for name in [str(c) for c in Z["cases"]]:
        g = _golden(name, dev)
        if g is None:
            continue
        dec, c, k, kw, feats = g
        assert dec.hidden_size == 16 and not ops.stacked_decode_supported(dec.embed_size, 16)
        assert dec.sample(feats[:1], start, end, k=k, one_call=True, **kw).cpu().tolist() == c["seq"].tolist()
        for poll in (0, 3):
            assert dec.sample_batch(feats, start, end, k=k, one_call=True, poll_every=poll, **kw) == \
                dec.sample_batch(feats, start, end, k=k, on_device=True, poll_every=poll, **kw)
        seen += 1
    assert seen >= 2
    ops.check_device_errors()


@pytest.mark.parametrize("family", STACKS + one_layer_families(), ids=lambda f: f.name)
def test_the_composed_step_switch_takes_the_device_loop(dev, monkeypatch, family):
    monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    assert getattr(dec._beam(5, *kw.values(), True)[0], "plain", None) is None
    assert dec.sample_batch(feats, START, end, k=5, one_call=True, **kw) == \
        dec.sample_batch(feats, START, end, k=5, on_device=True, **kw)
    ops.check_device_errors()


def test_an_attention_decoder_takes_the_device_loop(dev):
    family = _family("DecoderRNNAtt")
    dec = family.make().to(dev).eval()
    feats, end = family.features().to(dev), family.end
    for poll in (0, 3):
        assert dec.sample_batch(feats, START, end, k=5, one_call=True, poll_every=poll) == \
            dec.sample_batch(feats, START, end, k=5, on_device=True, poll_every=poll)
    assert dec.sample(feats[:1], START, end, k=3, one_call=True).cpu().tolist() == \
        dec.sample(feats[:1], START, end, k=3, on_device=True).cpu().tolist()
    ops.check_device_errors()


def test_a_start_token_out_of_range_raises_after_the_call(dev, monkeypatch):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family = STACKS[0]
    dec = family.make().to(dev).eval()
    feats = family.features().to(dev)
    ops.check_device_errors()
    with pytest.raises(capnet.CapnetError, match="token id out of range"):
        dec.sample_batch(feats, family.V + 3, family.end, k=3, one_call=True, **family.kw)
    ops.check_device_errors()                       # (raised and cleared)
    assert dec.sample_batch(feats, START, family.end, k=3, one_call=True, **family.kw) == \
        [family.reference(3, i) for i in range(IMAGES)]


# ---- 6. evaluate ---------------------------------------------------------------------------------------------------
def test_evaluate_one_call(dev, monkeypatch):
    from capnet.train import evaluate
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family = STACKS[0]
    dec = family.make().to(dev).eval()
    start, end, V_ = START, family.end, family.V

    class Vocab:
        word2idx = {"<start>": start, "<end>": end}
        idx2word = {i: ("<end>" if i == end else "<start>" if i == start else "w%d" % i) for i in range(V_)}

    class Enc(torch.nn.Module):
        def forward(self, images):
            return images
    # the references are what the decoder says, one of them cut short: BLEU is not degenerate, and a changed caption shows
    said = dec.sample_batch(family.features().to(dev), start, end, k=5, **family.kw)
    caps = [[torch.tensor(s), torch.tensor(s[:-2] + [end])] for s in said]
    batches = [(family.features(), None, None, caps)]
    mode = family.kw["mode"]
    one = evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=5, one_call=True)
    assert one == evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=5, on_device=True)
    assert one[0] > 0.99
