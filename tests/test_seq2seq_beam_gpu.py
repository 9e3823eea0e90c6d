"""capnet.seq2seq's beam search and what it stands on: ops.vocab_topk (projection, per-row top-k and log-sum-exp in one launch)
against fp64; ops.beam_advance_topk against ops.beam_advance on the same logits; ops.lstm_beam_decode, fused and unfused,
on the existing stack families; sample_beam of the three classes on every case of tests/seq2seq_beam_cases.py and on every
route, against the fp64 restatement (every case clears the margin rule: tests/test_seq2seq_beam_cpu.py)."""
import pytest
import torch

import capnet
import seq2seq_beam_cases as BC
from capnet import ops
from capnet.decode import pack_cells
from device_beam_cases import IMAGES, KS, MAX_LEN, START, families
from seq2seq_cases import TOL_LOGITS, need

pytestmark = pytest.mark.gpu


# ---- 1. ops.vocab_topk against fp64 --------------------------------------------------------------------------------
NL = 17            # lifted columns: the k + 1 best of every k <= 16
ROWS = (1, 5, 16, 17, 33)
TOPK_KS = (1, 3, 5, 16)


def _placement(place, V, g):
    if place == "one-workgroup":
        cols = list(range(3, 3 + NL))                      # all in workgroup 0
    elif place == "last-columns":
        cols = list(range(V - NL, V))                      # V = 37: 20 .. 36 straddle workgroups 0 and 1, the last ragged
    else:
        cols = sorted({0, V - 1} | {int(v) for v in torch.linspace(1, V - 2, NL - 2).round().tolist()})
    assert len(cols) == NL and cols[0] >= 0 and cols[-1] < V
    return [cols[i] for i in torch.randperm(NL, generator=g).tolist()]


def _topk_inputs(H, V, rows, bias, place, seed):
    """Random h, w whose products have a standard deviation of about 0.17 at every H, and NL columns lifted to a_j + s_r c_j (s_r = +-1 by row parity: 152 + 2 j on even
    rows, 248 - 10 j on odd ones): every gap among a row's NL best is about 2 or more, in a different order on odd and even rows.
    a_j goes through the bias where there is one, else through the weights' column 0 (h[:, 0] = 1)."""
    g = torch.Generator().manual_seed(seed)
    amp = 0.25 * (64.0 / H) ** 0.25
    h = (torch.rand(rows, H, generator=g, dtype=torch.float64) * 2 - 1) * amp
    w = (torch.rand(V, H, generator=g, dtype=torch.float64) * 2 - 1) * amp
    h[:, 0], w[:, 0] = 1.0, 0.0
    h[:, 1], w[:, 1] = torch.tensor([1.0 if r % 2 == 0 else -1.0 for r in range(rows)], dtype=torch.float64), 0.0
    b = (torch.rand(V, generator=g, dtype=torch.float64) * 2 - 1) * 0.25 if bias else None
    for j, c in enumerate(_placement(place, V, g)):
        a = 200.0 - 4.0 * j
        if bias:
            b[c] = a
        else:
            w[c, 0] = a
        w[c, 1] = 6.0 * j - 48.0
    return h.float(), w.float(), None if b is None else b.float()


def _fp64(h, w, b):
    logits = h.double() @ w.double().t()
    return logits if b is None else logits + b.double()


def _check_topk(dev, h, w, b, k, logits=None):
    logits = _fp64(h, w, b) if logits is None else logits
    scale = float(logits[torch.isfinite(logits)].abs().max())
    best, idx = logits.topk(min(k + 1, logits.shape[1]), 1)
    assert float((best[:, :-1] - best[:, 1:]).min()) > need(scale)          # the inputs' own precondition
    values, index, lse = ops.vocab_topk(h.to(dev), w.to(dev), None if b is None else b.to(dev), k=k)
    assert values.dtype == torch.float32 and index.dtype == torch.int32 and lse.dtype == torch.float32
    assert index.cpu().tolist() == idx[:, :k].tolist(), (k, h.shape, w.shape)
    tol = TOL_LOGITS * max(1.0, scale)
    assert float((values.cpu().double() - best[:, :k]).abs().max()) <= tol
    assert float((lse.cpu().double() - torch.logsumexp(logits, 1)).abs().max()) <= tol


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("H,V", [(64, 37), (64, 211), (512, 37), (512, 211), (512, 8192), (1024, 37)])
def test_vocab_topk_against_fp64(dev, H, V, bias):
    for n, rows in enumerate(ROWS):
        for place in ("one-workgroup", "last-columns", "ends"):
            h, w, b = _topk_inputs(H, V, rows, bias, place, seed=100 * H + V + 7 * n)
            logits = _fp64(h, w, b)
            for k in TOPK_KS:
                _check_topk(dev, h, w, b, k, logits)


@pytest.mark.parametrize("rows", [1, 17])
def test_vocab_topk_one_workgroup(dev, rows):
    """V = 32: one workgroup, the last arriver is the only arriver and merges its own lists."""
    for bias in (True, False):
        for place in ("one-workgroup", "last-columns", "ends"):
            h, w, b = _topk_inputs(64, 32, rows, bias, place, seed=6400 + 32 + rows)
            logits = _fp64(h, w, b)
            for k in TOPK_KS:
                _check_topk(dev, h, w, b, k, logits)


def test_vocab_topk_tie_goes_to_the_lower_index(dev):
    h, w, b = _topk_inputs(64, 37, 5, True, "ends", seed=1)
    free = [c for c in range(37) if float(b[c]) < 1.0]          # not a lifted column
    lo, hi = free[1], free[-1]
    assert lo < 32 <= hi                                        # in different workgroups
    w[hi] = w[lo]
    b[lo] = b[hi] = 1000.0
    values, index, _ = ops.vocab_topk(h.to(dev), w.to(dev), b.to(dev), k=3)
    assert index[:, :2].cpu().tolist() == [[lo, hi]] * 5
    assert torch.equal(values[:, 0], values[:, 1])


def test_vocab_topk_never_returns_minus_infinity_and_pads(dev):
    h, w, b = _topk_inputs(64, 37, 17, True, "ends", seed=2)
    logits = _fp64(h, w, b)
    top = int(logits[0].argmax())
    b[top] = float("-inf")
    logits = _fp64(h, w, b)
    values, index, lse = ops.vocab_topk(h.to(dev), w.to(dev), b.to(dev), k=5)
    assert top not in index.cpu().flatten().tolist()
    assert index.cpu().tolist() == logits.topk(5, 1)[1].tolist()
    assert float((lse.cpu().double() - torch.logsumexp(logits, 1)).abs().max()) <= TOL_LOGITS * float(logits[torch.isfinite(logits)].abs().max())
    # three finite entries, in two workgroups: the tail is (-inf, -1)
    keep = [2, 31, 35]
    b2 = torch.full_like(b, float("-inf"))
    b2[keep] = torch.tensor([1.0, 3.0, 2.0])
    values, index, lse = ops.vocab_topk(h.to(dev), w.to(dev), b2.to(dev), k=5)
    logits = _fp64(h, w, b2)
    assert index[:, :3].cpu().tolist() == logits.topk(3, 1)[1].tolist()
    assert index[:, 3:].cpu().tolist() == [[-1, -1]] * 17
    assert bool(torch.isinf(values[:, 3:]).all()) and bool((values[:, 3:] < 0).all())
    assert float((lse.cpu().double() - torch.logsumexp(logits, 1)).abs().max()) <= TOL_LOGITS * 10


def test_vocab_topk_leaves_its_counter_zero(dev):
    h, w, b = _topk_inputs(512, 211, 33, True, "ends", seed=3)
    h, w, b = h.to(dev), w.to(dev), b.to(dev)
    ws = ops.vocab_topk_workspace(33, 5, 211, dev)
    one = ops.vocab_topk(h, w, b, k=5, workspace=ws)
    two = ops.vocab_topk(h, w, b, k=5, workspace=ws)
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    assert int(ws.view(torch.int32)[0]) == 0
    assert all(torch.equal(x, y) for x, y in zip(one, ops.vocab_topk(h, w, b, k=5)))


# ---- 2. ops.beam_advance_topk against ops.beam_advance --------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_beam_advance_topk_equals_beam_advance(dev, k):
    n, V, T, end = 3, 37, 6, 4
    g = torch.Generator().manual_seed(50 + k)
    beams, words, parents = [], [], []
    for _ in range(2):
        w = torch.empty(n * k, dtype=torch.long, device=dev)
        beams.append(ops.beam_init(n, k, T, START, w))
        words.append(torch.empty(n * k, dtype=torch.long, device=dev))
        parents.append(torch.empty(n * k, dtype=torch.long, device=dev))
    for step in range(1, T + 1):
        logits = torch.randn(n * k, V, generator=g) * 3
        if step <= 2:
            logits[2 * k:, end] += 50.0        # image 2: one completion at step 1, every live beam at step 2 -- dead from there on
        if step == 3:
            logits[0, end] += 50.0             # image 0: its best beam completes
        logits = logits.to(dev)
        ops.beam_advance(beams[0], logits, step, end, words[0], parents[0])
        values, index = logits.topk(k, 1)
        ops.beam_advance_topk(beams[1], values.contiguous(), index.int().contiguous(), torch.logsumexp(logits, 1), step, end,
                              words[1], parents[1], V=V if step % 2 else None)
        assert torch.equal(words[0], words[1]) and torch.equal(parents[0], parents[1]), step
        assert torch.equal(beams[0].live, beams[1].live) and int(beams[0].live_total) == int(beams[1].live_total)
        if step == 2:
            assert beams[1].live.cpu().tolist()[2] == 0
    a, b = ops.beam_finish(beams[0], end), ops.beam_finish(beams[1], end)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    lens = a[1].cpu().tolist()
    assert lens[2] in (2, 3) and lens[0] >= 2            # image 2 completed at step 1 or 2; image 0 completed something


def test_beam_advance_topk_never_takes_a_padded_candidate(dev):
    n, k, V, T, end = 2, 3, 37, 4, 4
    w = torch.empty(n * k, dtype=torch.long, device=dev)
    beam = ops.beam_init(n, k, T, START, w)
    nxt, par = torch.empty_like(w), torch.empty_like(w)
    values = torch.tensor([[2.0, 1.0, float("-inf")]] * (n * k), device=dev)
    index = torch.tensor([[7, 9, -1]] * (n * k), dtype=torch.int32, device=dev)
    lse = torch.full((n * k,), 3.0, device=dev)
    ops.beam_advance_topk(beam, values, index, lse, 1, end, nxt, par, V=V)       # step 1: row 0 alone offers two candidates
    assert beam.live.cpu().tolist() == [2, 2]
    assert nxt.cpu().tolist() == [7, 9, end, 7, 9, end] and par.cpu().tolist() == [0, 0, 2, 3, 3, 5]
    ops.check_device_errors()


# ---- 3. ops.lstm_beam_decode on the existing stack families ---------------------------------------------------------
STACKS = [f for f in families() if f.name in ("StackedFactoredLSTM-2", "StackedDecoderRNN-2")]
assert len(STACKS) == 2


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("family", STACKS, ids=lambda f: f.name)
def test_lstm_beam_decode_on_the_stack_families(dev, monkeypatch, family, fused):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    dec = family.make().to(dev).eval()
    for k in KS:
        plain = dec._beam(IMAGES * k, *family.kw.values())[0].plain
        got = ops.lstm_beam_decode(plain.cell, plain.wcat, plain.beff, plain.emb, plain.Cw, plain.Cb, IMAGES, k, MAX_LEN + 1,
                                   START, family.end, fused_topk=fused)
        assert got == [family.reference(k, i) for i in range(IMAGES)], k
    ops.check_device_errors()


# ---- 4. sample_beam -------------------------------------------------------------------------------------------------
def _want(case, k):
    return [case.reference(k, r) for r in range(case.rows)]


@pytest.mark.parametrize("case", BC.CASES + BC.COMPOSED, ids=repr)
def test_sample_beam_on_every_route(dev, monkeypatch, case):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    monkeypatch.delenv("CAPNET_NO_FUSED_TOPK", raising=False)
    model = case.module().to(dev)
    feats, end = case.features.float().to(dev), case.end
    assert ops.stacked_decode_supported(case.E, case.H) == (case not in BC.COMPOSED)
    for k in case.ks:
        want = _want(case, k)
        for fused in (True, False, None):
            assert model.sample_beam(feats, START, end, mode=case.mode, k=k, fused_topk=fused) == want, (k, fused)
        if case.mode == "factual":
            assert model.encoder.sample_beam(feats, START, end, k=k, fused_topk=True) == want, k
        else:
            _, states = model.encoder.sample(feats)
            got = model._decoder(case.mode).sample_beam(START, end, states, k=k, fused_topk=True)
            assert got == want and all(s[0] == START or s == [end] for s in got), k
        for switch in ("CAPNET_NO_FUSED_TOPK", "CAPNET_NO_FUSED_DECODE_STEP"):
            monkeypatch.setenv(switch, "1")
            assert model.sample_beam(feats, START, end, mode=case.mode, k=k, fused_topk=True) == want, (k, switch)
            monkeypatch.delenv(switch)
    ops.check_device_errors()


def test_the_switch_really_takes_the_unfused_step(dev, monkeypatch):
    """CAPNET_NO_FUSED_TOPK=1 beats fused_topk=True: ops.lstm_beam_decode is then called with fused_topk False."""
    case = BC.case("small-happy-s5")
    model = case.module().to(dev)
    seen = []
    real = ops.lstm_beam_decode

    def spy(*a, **kw):
        seen.append(kw["fused_topk"])
        return real(*a, **kw)
    monkeypatch.setattr(ops, "lstm_beam_decode", spy)
    feats = case.features.float().to(dev)
    monkeypatch.delenv("CAPNET_NO_FUSED_TOPK", raising=False)
    model.sample_beam(feats, START, case.end, mode="happy", k=3, fused_topk=True)
    monkeypatch.setenv("CAPNET_NO_FUSED_TOPK", "1")
    model.sample_beam(feats, START, case.end, mode="happy", k=3, fused_topk=True)
    assert seen == [True, False]


def _biased_decoder(dev, case, end_bias):
    model = case.module().to(dev)
    dec = model._decoder(case.mode)
    with torch.no_grad():
        dec.linear.bias[case.end] += end_bias
    _, states = model.encoder.sample(case.features.float().to(dev))
    return dec, states


def _one_call(dec, states, k, end, poll, fused):
    packed = pack_cells(dec._layers(), dec.embed_size)
    B = states[0].size(1)
    state = dec._rows_state(states, B, states[0].device).repeat_interleave(k, 0).contiguous()
    return ops.lstm_beam_decode(ops.CELL_LSTM, [w for w, _ in packed], [b for _, b in packed], dec.embed.weight, dec.linear.weight,
                                dec.linear.bias, B, k, dec.max_seq_length + 1, START, end, state=state, fused_topk=fused,
                                poll_every=poll, return_steps=True)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("k", KS)
def test_poll_every_stops_early_with_the_same_lists(dev, monkeypatch, k, fused):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    monkeypatch.delenv("CAPNET_NO_FUSED_TOPK", raising=False)
    case = BC.case("small-happy-s5")
    dec, states = _biased_decoder(dev, case, 60.0)            # <end> wins on every row from the first step on
    want, steps = _one_call(dec, states, k, case.end, 0, fused)
    assert steps == MAX_LEN + 1
    assert all(2 <= len(s) <= 3 and s[0] == START and s[-1] == case.end for s in want), want
    for m in (1, 3):
        got, steps = _one_call(dec, states, k, case.end, m, fused)
        assert got == want and steps <= 2 + m, (m, steps)
        assert dec.sample_beam(START, case.end, states, k=k, poll_every=m, fused_topk=fused) == want, m
    ops.check_device_errors()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_nothing_completed_returns_end(dev, monkeypatch, fused):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    monkeypatch.delenv("CAPNET_NO_FUSED_TOPK", raising=False)
    case = BC.case("small-happy-s5")
    dec, states = _biased_decoder(dev, case, -60.0)
    for m in (0, 3):
        got, steps = _one_call(dec, states, 3, case.end, m, fused)
        assert got == [[case.end]] * case.rows and steps == MAX_LEN + 1, m
    assert dec.sample_beam(START, case.end, states, k=3, fused_topk=fused) == [[case.end]] * case.rows
    ops.check_device_errors()


def test_a_start_token_out_of_range_raises_after_the_call(dev, monkeypatch):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    monkeypatch.delenv("CAPNET_NO_FUSED_TOPK", raising=False)
    case = BC.case("small-happy-s5")
    model = case.module().to(dev)
    feats = case.features.float().to(dev)
    ops.check_device_errors()
    for fused in (True, False):
        with pytest.raises(capnet.CapnetError, match="token id out of range"):
            model.sample_beam(feats, case.V + 3, case.end, mode="happy", k=3, fused_topk=fused)
        ops.check_device_errors()                       # (raised and cleared)
    assert model.sample_beam(feats, START, case.end, mode="happy", k=3, fused_topk=True) == _want(case, 3)
