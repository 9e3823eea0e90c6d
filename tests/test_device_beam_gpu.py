"""Beam search with device-side bookkeeping (capnet_beam_init / _advance / _finish, capnet.beam.beam_search_device):
the kernels against the pure-Python fixed-slot model (tests/device_beam_ref.py) bit for bit, the argument refusals, and
every decoder's sample / sample_batch with on_device=True against the host bookkeeping and the stored sequences."""
import pytest
import torch

import capnet
from capnet import _lib, ops
from capnet._lib import check, ptr
from capnet.model import DecoderFactoredLSTM
from capnet.model_att import DecoderFactoredLSTMAtt
from capnet.nic_model import DecoderRNN
from device_beam_cases import IMAGES, KS, START, families
from device_beam_ref import DeviceBeam
from helpers import load_golden, t

pytestmark = pytest.mark.gpu

S, E_ = 1, 2                                       # <start>, <end> of the synthetic tables
SITUATIONS = {"several completions in one step", "nothing completed", "all beams complete before the last step",
              "the winner is not the first completion"}


# ---- 1. the kernels against the model ------------------------------------------------------------------------------
def _table(n, k, V, T, roles, seed):
    """Logits [T][n k][V]: unit normal noise, <end> held far down, then per image one of four scripts (by roles[i]):
      0  step 2: <end> wins on slots 0 and 1 (several completions in one step); step 4: on slot 0
      1  nothing (the image completes nothing)
      2  step 1: two words far ahead, <end> third and far behind; step 2: <end> wins on slot 0 -- the later completion
         has the better score (the winner is not the first completion)
      3  step 2: <end> wins on every slot (all beams complete before the last step)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, n * k, V, generator=g)
    x[:, :, E_] = -30.0
    for i, role in enumerate(roles):
        r0 = i * k
        if role == 0:
            if T >= 2:
                x[1, r0:r0 + min(k, 2), E_] = 30.0
            if T >= 4:
                x[3, r0, E_] = 30.0
        elif role == 2:
            x[0, r0, 3], x[0, r0, 4], x[0, r0, E_] = 12.0, 12.0, 6.0
            if T >= 2:
                x[1, r0, E_] = 30.0
        elif role == 3 and T >= 2:
            x[1, r0:r0 + k, E_] = 30.0
    return x


def _drive(dev, n, k, V, T, table, steps=None):
    """capnet_beam_advance and the model side by side over `table`; the model's top-k is ops.beam_topk_batched on the
    same rows. Every step: next_words, parent_rows, live counts and the live slots' scores are EQUAL; then the results."""
    words = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(2)]
    parent = torch.empty(n * k, dtype=torch.long, device=dev)
    beam = ops.beam_init(n, k, T, S, words[0])
    assert words[0].tolist() == [S] * (n * k) and int(beam.live_total.item()) == n * k
    model = DeviceBeam(n, k, V, S, E_)
    for step in range(1, (steps or T) + 1):
        logits = table[step - 1].to(dev)
        prev = torch.tensor(model.scores, dtype=torch.float32, device=dev).reshape(-1)
        meta = [(i * k, (1 if step == 1 else model.live[i]) if model.live[i] else 0, model.live[i]) for i in range(n)]
        sc, ix = ops.beam_topk_batched(logits, prev, torch.tensor(meta, dtype=torch.int32, device=dev))
        sc_l, ix_l = sc.tolist(), ix.tolist()
        want_words, want_rows = model.advance(step, lambda i, rows, kk: (sc_l[i][:kk], ix_l[i][:kk]))
        ops.beam_advance(beam, logits, step, E_, words[step & 1], parent)
        assert words[step & 1].tolist() == want_words, step
        assert parent.tolist() == want_rows, step
        assert beam.live.tolist() == model.live and int(beam.live_total.item()) == model.live_total, step
        for i in range(n):
            live = model.live[i]
            assert torch.equal(beam.scores[i, :live].cpu(), torch.tensor(model.scores[i][:live], dtype=torch.float32)), (step, i)
    seqs, lengths, _ = ops.beam_finish(beam, E_)
    got = [row[:ln] for row, ln in zip(seqs.tolist(), lengths.tolist())]
    assert got == model.finish()
    ops.check_device_errors()
    return model, got


@pytest.mark.parametrize("k", [1, 3, 5, 16])
@pytest.mark.parametrize("n", [1, 4])
def test_kernel_equals_model(dev, n, k):
    seen = set()
    for vi, V in enumerate((16, 37, 777, 8192)):
        for ti, T in enumerate((1, 2, 6)):
            roles = [(i + vi + ti) % 4 for i in range(n)]
            model, _ = _drive(dev, n, k, V, T, _table(n, k, V, T, roles, 1000 * n + 100 * k + 10 * vi + ti))
            seen |= model.events(T)
    possible = SITUATIONS if k >= 3 else {"nothing completed", "all beams complete before the last step"}
    assert seen >= possible, possible - seen


def test_equal_logits_tie_to_the_lower_flat_index(dev):
    n, k, V, T = 2, 3, 16, 3
    table = torch.zeros(T, n * k, V)
    table[:, :, E_] = -1.0                                     # (<end> = 2 would otherwise be among the first three)
    model, got = _drive(dev, n, k, V, T, table)
    assert model.seqs[0] == [[S, 0, 0, 0], [S, 0, 0, 1], [S, 0, 0, 3]] and got == [[E_], [E_]]


def test_of_two_equal_completed_scores_the_earlier_wins(dev):
    n, k, V, T = 1, 2, 16, 3
    table = torch.full((T, n * k, V), -20.0)
    table[0, 0, 5] = table[0, 0, 9] = 20.0                      # two words, equal score
    table[1, :, E_] = 40.0                                      # both beams end at step 2, equal score again
    model, got = _drive(dev, n, k, V, T, table)
    (s0, q0, _), (s1, q1, _) = model.done[0]
    assert s0 == s1 and q0 == [S, 5, E_] and q1 == [S, 9, E_] and got == [q0]


def test_early_stop_leaves_the_result_unchanged(dev):
    """Once live_total is zero, further steps change nothing: finish after step 2 equals finish after all 6 steps."""
    n, k, V, T = 4, 5, 37, 6
    table = _table(n, k, V, T, [3, 3, 3, 3], 7)
    m2, got2 = _drive(dev, n, k, V, T, table, steps=2)
    m6, got6 = _drive(dev, n, k, V, T, table)
    assert m2.live_total == 0 and got2 == got6


# ---- 2. refusals ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(dev):
    lib = _lib.lib()
    n, k, V, T = 2, 3, 16, 4
    words = torch.empty(n * 17, dtype=torch.long, device=dev)
    rows = torch.empty(n * 17, dtype=torch.long, device=dev)
    logits = torch.zeros(n * 17, V, device=dev)
    beam = ops.beam_init(n, k, T, S, words[:n * k].contiguous())
    stream = _lib.current_stream()

    def advance(k=k, V=V, ld=V, step=1):
        check(lib.capnet_beam_advance(ptr(beam.words), ptr(logits), ld, V, n, k, T, step, E_, ptr(words), ptr(rows), stream),
              "capnet_beam_advance")
    advance()                                                   # the good call passes
    for bad in (dict(k=17), dict(V=2, ld=2), dict(step=0), dict(step=T + 1), dict(ld=V - 1)):
        with pytest.raises(capnet.CapnetError):
            advance(**bad)
    with pytest.raises(capnet.CapnetError):
        ops.beam_init(n, 17, T, S, words)
    with pytest.raises(capnet.CapnetError):
        check(lib.capnet_beam_init(ptr(beam.words), n, k, T, S, None, stream), "capnet_beam_init")
    with pytest.raises(capnet.CapnetError):
        check(lib.capnet_beam_finish(ptr(beam.words), n, k, T, E_, None, None, stream), "capnet_beam_finish")
    with pytest.raises(capnet.CapnetError):
        ops.beam_advance(beam, logits[:n * k - 1], 1, E_, words[:n * k], rows[:n * k])
    torch.cuda.synchronize()
    ops.check_device_errors()


# ---- 3. the decoders -----------------------------------------------------------------------------------------------
Z = load_golden("sample_tiny.npz")
CASES = [str(c) for c in Z["cases"]]


def _golden(name, dev):
    pre = "case.%s." % name
    c = {k[len(pre):]: Z[k] for k in Z.files if k.startswith(pre)}
    params = {k[len("param."):]: t(v) for k, v in c.items() if k.startswith("param.")}
    kind = str(c["kind"])
    dims = [int(v) for v in c["dims"]]
    E, H, F, V, k, maxlen = dims[:6]
    if kind == "factored":
        dec = DecoderFactoredLSTM(E, H, F, V, 1, dropout=0.0, max_seq_length=maxlen)
    elif kind == "nic":
        dec = DecoderRNN(E, H, V, 1, dropout=0.0, max_seq_length=maxlen)
    else:
        dec = DecoderFactoredLSTMAtt(dims[6], E, H, F, V, 1, feature_size=dims[7], dropout=0.0, max_seq_length=maxlen)
    dec.load_state_dict(params)
    dec.to(dev).eval()
    kw = {} if kind == "nic" else {"mode": str(c["mode"])}
    if kind == "att":                                           # the feature sets of tests/test_sample_gpu.py
        base = t(c["features"]).to(dev)
        g = torch.Generator().manual_seed(3)
        feats = torch.cat([base] + [base * (0.5 + torch.rand(1, generator=g).item()) + 0.3 * torch.randn(base.shape, generator=g).to(dev)
                                    for _ in range(4)], 0)
    else:
        feats = torch.zeros(3, E, device=dev)
    return dec, c, k, kw, feats


@pytest.mark.parametrize("name", CASES)
def test_golden_sample_on_device(dev, name):
    dec, c, k, kw, feats = _golden(name, dev)
    start, end = [int(v) for v in Z["start_end"]]
    seq = dec.sample(feats[:1], start, end, k=k, on_device=True, **kw)
    assert seq.dtype == torch.int64 and seq.dim() == 2 and seq.shape[0] == 1
    assert seq.cpu().tolist() == c["seq"].tolist()
    want = dec.sample_batch(feats, start, end, k=k, **kw)
    for poll in (0, 1, 3):
        assert dec.sample_batch(feats, start, end, k=k, on_device=True, poll_every=poll, **kw) == want, poll
    ops.check_device_errors()


@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("family", families(), ids=lambda f: f.name)
def test_random_decoders_on_device(dev, monkeypatch, family, path):
    """on_device=True equals the host bookkeeping and the fp64 restatement, per image and batched, wherever the
    restatement's beam_margin exceeds device_beam_cases.MARGIN -- which tests/test_device_beam_cpu.py asserts of every case here, so
    nothing is skipped. Both decode-step paths (the composed one is the only one of a decoder without a stack)."""
    if path == "composed":
        monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
        monkeypatch.setenv("CAPNET_NO_FUSED_UPPER_STEP", "1")
    else:
        monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
        monkeypatch.delenv("CAPNET_NO_FUSED_UPPER_STEP", raising=False)
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    for k in KS:
        want = [family.reference(k, i) for i in range(IMAGES)]
        assert dec.sample_batch(feats, START, end, k=k, **kw) == want, k
        for poll in (0, 1, 3):
            assert dec.sample_batch(feats, START, end, k=k, on_device=True, poll_every=poll, **kw) == want, (k, poll)
        for i in range(IMAGES):
            assert dec.sample(feats[i:i + 1], START, end, k=k, on_device=True, **kw).cpu().tolist() == [want[i]], (k, i)
    ops.check_device_errors()


def test_nic_attention_sample_batch_equals_sample(dev):
    family = [f for f in families() if f.name == "DecoderRNNAtt"][0]
    dec = family.make().to(dev).eval()
    feats = family.features().to(dev)
    batched = dec.sample_batch(feats, START, family.end, k=5)
    assert batched == [dec.sample(feats[i:i + 1], START, family.end, k=5)[0].tolist() for i in range(IMAGES)]


def test_evaluate_on_device(dev):
    from capnet.train import evaluate
    family = [f for f in families() if f.name == "StackedFactoredLSTMAtt-2"][0]
    dec = family.make().to(dev).eval()
    start, end, V = START, family.end, family.V

    class Vocab:
        word2idx = {"<start>": start, "<end>": end}
        idx2word = {i: ("<end>" if i == end else "<start>" if i == start else "w%d" % i) for i in range(V)}

    class Enc(torch.nn.Module):
        def forward(self, images):
            return images
    g = torch.Generator().manual_seed(8)
    caps = [[torch.tensor([start] + torch.randint(3, V, (4,), generator=g).tolist() + [end]) for _ in range(2)] for _ in range(IMAGES)]
    batches = [(family.features(), None, None, caps)]
    assert evaluate(Enc(), dec, Vocab(), batches, mode="factual", k=5, on_device=True) == \
        evaluate(Enc(), dec, Vocab(), batches, mode="factual", k=5)
