"""Seq2Seq.sample_beam_styles and what it stands on: ops.vocab_topk_groups (the grouped projection / top-k / log-sum-exp launch)
against fp64 and against ops.vocab_topk group by group; ops.lstm_beam_decode_groups, fused and unfused; sample_beam_styles on
every case of tests/seq2seq_beam_style_cases.py and on every route, against the fp64 restatement (every mode of every case
clears the margin rule at its own <end>: tests/test_seq2seq_beam_styles_cpu.py) and against sample_beam(mode=...)."""
import pytest
import torch

import capnet
import seq2seq_beam_style_cases as SBC
from capnet import ops, seq2seq
from capnet.decode import pack_cells
from device_beam_cases import MAX_LEN, START
from seq2seq_cases import TOL_LOGITS, need

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_routes(monkeypatch):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    monkeypatch.delenv("CAPNET_NO_FUSED_TOPK", raising=False)


# ---- 1. ops.vocab_topk_groups against fp64 and against the single call ---------------------------------------------
NL = 17            # lifted columns: the k + 1 best of every k <= 16
RPGS = (1, 5, 15, 16, 17, 33)
TOPK_KS = (1, 5, 16)


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
    """tests/test_seq2seq_beam_gpu.py's recipe: random h, w whose products have a standard deviation of about 0.17 at every H,
    and NL columns lifted to a_j + s_r c_j (s_r = +-1 by row parity), every gap among a row's NL best about 2 or more, in a
    different order on odd and even rows. a_j goes through the bias where there is one, else through the weights' column 0
    (h[:, 0] = 1). The lifted columns and their order are drawn from the seed: a different seed per group gives every group
    its own best entries."""
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


def _group_inputs(groups, H, V, rpg, seed):
    """Per group (h, w, b or None): its own seed, placement and bias choice."""
    places = ("ends", "last-columns", "one-workgroup")
    return [_topk_inputs(H, V, rpg, bias=(g % 3 != 1), place=places[g % 3], seed=seed + 31 * g) for g in range(groups)]


@pytest.mark.parametrize("groups", [2, 3, 8])
@pytest.mark.parametrize("H,V", [(64, 37), (512, 211), (1024, 37)])
def test_vocab_topk_groups_against_fp64_and_the_single_call(dev, groups, H, V):
    for n, rpg in enumerate(RPGS):
        parts = _group_inputs(groups, H, V, rpg, seed=1000 * H + V + 7 * n + groups)
        assert any(b is None for _, _, b in parts) and any(b is not None for _, _, b in parts)
        logits = [_fp64(*p) for p in parts]
        # the groups' best entries differ: a workgroup on the wrong group's weights is caught
        assert len({tuple(l.topk(3, 1)[1][0].tolist()) for l in logits}) > 1
        h = torch.cat([p[0] for p in parts]).to(dev)
        ws = [p[1].to(dev) for p in parts]
        bs = [None if p[2] is None else p[2].to(dev) for p in parts]
        for k in TOPK_KS:
            values, index, lse = ops.vocab_topk_groups(h, ws, bs, k=k)
            assert values.dtype == torch.float32 and index.dtype == torch.int32 and lse.dtype == torch.float32
            assert tuple(values.shape) == (groups * rpg, k) == tuple(index.shape) and tuple(lse.shape) == (groups * rpg,)
            for g in range(groups):
                lg = logits[g]
                scale = float(lg.abs().max())
                best, idx = lg.topk(k + 1, 1)
                assert float((best[:, :-1] - best[:, 1:]).min()) > need(scale)          # the inputs' own precondition
                blk = slice(g * rpg, (g + 1) * rpg)
                assert index[blk].cpu().tolist() == idx[:, :k].tolist(), (g, k, rpg)
                tol = TOL_LOGITS * max(1.0, scale)
                assert float((values[blk].cpu().double() - best[:, :k]).abs().max()) <= tol
                assert float((lse[blk].cpu().double() - torch.logsumexp(lg, 1)).abs().max()) <= tol
                one = ops.vocab_topk(h[blk], ws[g], bs[g], k=k)
                assert torch.equal(values[blk], one[0]) and torch.equal(index[blk], one[1]) and torch.equal(lse[blk], one[2]), \
                    (g, k, rpg)


def test_one_group_is_vocab_topk(dev):
    h, w, b = (t.to(dev) for t in _topk_inputs(512, 211, 17, True, "ends", seed=5))
    ws = ops.vocab_topk_workspace(17, 5, 211, dev)
    one = ops.vocab_topk(h, w, b, k=5, workspace=ws)
    two = ops.vocab_topk_groups(h, [w], [b], k=5, workspace=ws)          # the same workspace layout
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    assert int(ws.view(torch.int32)[0]) == 0


# ---- 2. counters ------------------------------------------------------------------------------------------------------
def test_vocab_topk_groups_leaves_every_counter_zero(dev):
    groups, rpg, H, V, k = 3, 33, 512, 211, 5
    parts = _group_inputs(groups, H, V, rpg, seed=77)
    h = torch.cat([p[0] for p in parts]).to(dev)
    ws = [p[1].to(dev) for p in parts]
    bs = [None if p[2] is None else p[2].to(dev) for p in parts]
    space = ops.vocab_topk_groups_workspace(groups, rpg, k, V, dev)
    one = ops.vocab_topk_groups(h, ws, bs, k=k, workspace=space)
    two = ops.vocab_topk_groups(h, ws, bs, k=k, workspace=space)
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    words = space.view(torch.int32)[:4 * groups].cpu().tolist()
    assert words == [0] * (4 * groups)                                   # group g's counter: word 4 g
    assert all(torch.equal(x, y) for x, y in zip(one, ops.vocab_topk_groups(h, ws, bs, k=k)))


def test_padding_stays_in_its_group(dev):
    groups, rpg, H, V, k = 3, 17, 64, 37, 5
    parts = _group_inputs(groups, H, V, rpg, seed=9)
    h = torch.cat([p[0] for p in parts]).to(dev)
    ws = [p[1].to(dev) for p in parts]
    bs = [None if p[2] is None else p[2] for p in parts]
    masked = torch.full((V,), float("-inf"))
    masked[[2, 35]] = torch.tensor([1.0, 3.0])                           # two finite entries, one in each workgroup
    for only in range(groups):
        bb = [masked.to(dev) if g == only else (None if b is None else b.to(dev)) for g, b in enumerate(bs)]
        values, index, lse = ops.vocab_topk_groups(h, ws, bb, k=k)
        for g in range(groups):
            blk = slice(g * rpg, (g + 1) * rpg)
            if g == only:
                lg = _fp64(parts[g][0], parts[g][1], masked)
                assert index[blk, :2].cpu().tolist() == lg.topk(2, 1)[1].tolist()
                assert index[blk, 2:].cpu().tolist() == [[-1] * (k - 2)] * rpg
                assert bool(torch.isinf(values[blk, 2:]).all()) and bool((values[blk, 2:] < 0).all())
                assert float((lse[blk].cpu().double() - torch.logsumexp(lg, 1)).abs().max()) <= TOL_LOGITS * 10
            else:
                assert int(index[blk].min()) >= 0 and bool(torch.isfinite(values[blk]).all())
                one = ops.vocab_topk(h[blk], ws[g], bb[g], k=k)
                assert torch.equal(values[blk], one[0]) and torch.equal(index[blk], one[1]) and torch.equal(lse[blk], one[2])


# ---- 3. ops.lstm_beam_decode_groups ------------------------------------------------------------------------------------
def _grouped_args(model, emotions, feats, k):
    """What sample_beam_styles hands ops.lstm_beam_decode_groups for `emotions`, built here from the modules."""
    decoders = [model._decoder(m) for m in emotions]
    d = decoders[0]
    _, (h, c) = model.encoder.sample(feats)
    with torch.no_grad():
        packed = [pack_cells(x._layers(), d.embed_size) for x in decoders]
        wcat = [torch.stack([p[l][0] for p in packed]) for l in range(d.num_layers)]
        beff = [torch.stack([p[l][1] for p in packed]) for l in range(d.num_layers)]
        state = seq2seq._to_rows(h, c)
    return decoders, wcat, beff, state, (h, c)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_lstm_beam_decode_groups_against_the_references(dev, fused):
    case = SBC.case("small-all")
    model = case.module().to(dev)
    feats = case.features.float().to(dev)
    emotions, B = case.emotions, case.rows
    for k in case.ks:
        decoders, wcat, beff, state, _ = _grouped_args(model, emotions, feats, k)
        G = len(decoders)
        st = state.repeat(G, 1, 1).repeat_interleave(k, 0).contiguous()
        for g, m in enumerate(emotions):                     # m's margins hold at m's own <end>
            lists = ops.lstm_beam_decode_groups(ops.CELL_LSTM, wcat, beff, [x.embed.weight for x in decoders],
                                                [x.linear.weight for x in decoders], [x.linear.bias for x in decoders], B, k,
                                                MAX_LEN + 1, START, case.end(m), state=st, fused_topk=fused)
            assert len(lists) == G * B
            assert lists[g * B:(g + 1) * B] == case.reference(k, m), (k, m)
        # one group through the grouped entry: ops.lstm_beam_decode's lists
        x = decoders[1]
        packed = pack_cells(x._layers(), x.embed_size)
        st1 = state.repeat_interleave(k, 0).contiguous()
        end = case.end(emotions[1])
        want = ops.lstm_beam_decode(ops.CELL_LSTM, [w for w, _ in packed], [b for _, b in packed], x.embed.weight, x.linear.weight,
                                    x.linear.bias, B, k, MAX_LEN + 1, START, end, state=st1, fused_topk=fused)
        got = ops.lstm_beam_decode_groups(ops.CELL_LSTM, [w.unsqueeze(0).contiguous() for w, _ in packed],
                                          [b.unsqueeze(0).contiguous() for _, b in packed], [x.embed.weight], [x.linear.weight],
                                          [x.linear.bias], B, k, MAX_LEN + 1, START, end, state=st1, fused_topk=fused)
        assert got == want == case.reference(k, emotions[1]), k
    ops.check_device_errors()


# ---- 4. sample_beam_styles on every case and route ---------------------------------------------------------------------
def _grouped(case, k):
    return len(case.emotions) >= 2 and ops.stacked_decode_supported(case.E, case.H)


def _check_styles_call(model, case, feats, k, fused, grouped=None, **kw):
    """One sample_beam_styles call per listed mode m, at m's <end>: entry m against the restatement; every other entry
    against sample_beam(mode=...) at the same <end> on the same step (the same arithmetic: no margin needed)."""
    grouped = _grouped(case, k) if grouped is None else grouped
    for m in case.modes:
        end = case.end(m)
        got = model.sample_beam_styles(feats, START, end, modes=case.modes, k=k, fused_topk=fused, **kw)
        assert list(got) == list(case.modes)
        assert got[m] == case.reference(k, m), (case, k, fused, m)
        for o in case.modes:
            # fused_topk=None: the grouped call routes on FUSED_TOPK_GROUPS_MAX_ROWS, a single search on FUSED_TOPK_MAX_ROWS
            flag = fused
            if fused is None and o != "factual" and grouped:
                flag = case.rows * k <= seq2seq.FUSED_TOPK_GROUPS_MAX_ROWS
            assert got[o] == model.sample_beam(feats, START, end, mode=o, k=k, fused_topk=flag, **kw), (case, k, fused, m, o)


@pytest.mark.parametrize("case", SBC.CASES + SBC.COMPOSED, ids=repr)
def test_sample_beam_styles_on_every_route(dev, monkeypatch, case):
    model = case.module().to(dev)
    feats = case.features.float().to(dev)
    assert ops.stacked_decode_supported(case.E, case.H) == (case not in SBC.COMPOSED)
    calls = []
    real = ops.lstm_beam_decode_groups
    monkeypatch.setattr(ops, "lstm_beam_decode_groups", lambda *a, **kw: (calls.append(kw["fused_topk"]), real(*a, **kw))[1])
    for k in case.ks:
        for fused in (True, False, None):
            del calls[:]
            _check_styles_call(model, case, feats, k, fused)
            assert len(calls) == (len(case.modes) if _grouped(case, k) else 0)          # the composed case: the fallback
        monkeypatch.setenv("CAPNET_NO_FUSED_TOPK", "1")
        del calls[:]
        _check_styles_call(model, case, feats, k, True)
        assert not any(calls)
        monkeypatch.delenv("CAPNET_NO_FUSED_TOPK")
        monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
        del calls[:]
        _check_styles_call(model, case, feats, k, True, grouped=False)
        assert not calls
        monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP")
    ops.check_device_errors()


def test_the_keys_are_the_modes_asked_for(dev, monkeypatch):
    case = SBC.case("small-all")
    model = case.module().to(dev)
    feats = case.features.float().to(dev)
    end = case.end("sad")
    full = model.sample_beam_styles(feats, START, end, k=3)
    assert list(full) == ["factual", "happy", "sad", "angry"]
    assert full["sad"] == case.reference(3, "sad")
    for modes in (("angry", "factual", "happy"), ("sad", "happy"), ("angry",), ("sad", "factual"), "happy"):
        got = model.sample_beam_styles(feats, START, end, modes=modes, k=3, fused_topk=True)
        want = (modes,) if isinstance(modes, str) else modes
        assert list(got) == list(want)
        for m in want:
            assert got[m] == model.sample_beam(feats, START, end, mode=m, k=3, fused_topk=True), (modes, m)
    # `factual` alone never runs the encoder's greedy sample
    ran = []
    real = model.encoder.sample
    monkeypatch.setattr(model.encoder, "sample", lambda *a, **kw: (ran.append(1), real(*a, **kw))[1])
    got = model.sample_beam_styles(feats, START, case.end("factual"), modes=("factual",), k=3)
    assert not ran and got == {"factual": case.reference(3, "factual")}
    ops.check_device_errors()


# ---- 5. routing -------------------------------------------------------------------------------------------------------
def test_routing(dev, monkeypatch):
    case = SBC.case("small-all")
    model = case.module().to(dev)
    feats = case.features.float().to(dev)
    end = case.end("happy")
    grouped, single, greedy = [], [], []
    real_g, real_s, real_e = ops.lstm_beam_decode_groups, ops.lstm_beam_decode, model.encoder.sample
    monkeypatch.setattr(ops, "lstm_beam_decode_groups", lambda *a, **kw: (grouped.append(kw), real_g(*a, **kw))[1])
    monkeypatch.setattr(ops, "lstm_beam_decode", lambda *a, **kw: (single.append(kw), real_s(*a, **kw))[1])
    monkeypatch.setattr(model.encoder, "sample", lambda *a, **kw: (greedy.append(1), real_e(*a, **kw))[1])

    def run(modes, **kw):
        del grouped[:], single[:], greedy[:]
        return model.sample_beam_styles(feats, START, end, modes=modes, k=3, **kw)
    run(("happy", "sad", "angry"), fused_topk=True)
    assert len(grouped) == 1 and not single and len(greedy) == 1
    assert grouped[0]["fused_topk"] is True
    run(("factual", "sad", "angry"))
    assert len(grouped) == 1 and len(single) == 1 and len(greedy) == 1
    assert single[0].get("first_inputs") is not None                   # the one single search is the encoder's
    assert grouped[0]["fused_topk"] is (case.rows * 3 <= seq2seq.FUSED_TOPK_GROUPS_MAX_ROWS)
    run(("factual", "sad"))
    assert not grouped and len(single) == 2 and len(greedy) == 1
    run(("angry",))
    assert not grouped and len(single) == 1 and len(greedy) == 1
    monkeypatch.setenv("CAPNET_NO_FUSED_TOPK", "1")
    run(("happy", "sad"), fused_topk=True)
    assert len(grouped) == 1 and grouped[0]["fused_topk"] is False and not single
    monkeypatch.delenv("CAPNET_NO_FUSED_TOPK")
    monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
    run(("happy", "sad"), fused_topk=True)
    assert not grouped and not single and len(greedy) == 1               # capnet.beam.beam_search_device, one after the other
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP")
    # decoders of unequal shapes: one after the other
    model.decoder_sad.max_seq_length = MAX_LEN - 1
    run(("happy", "sad"), fused_topk=True)
    assert not grouped and len(single) == 2 and len(greedy) == 1
    ops.check_device_errors()


# ---- 6. poll_every ----------------------------------------------------------------------------------------------------
def _biased(dev, case, bias, only=None):
    model = case.module().to(dev)
    with torch.no_grad():
        for m in case.emotions:
            if only is None or m == only:
                model._decoder(m).linear.bias[case.end("happy")] += bias
    return model


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_poll_every_stops_early_with_the_same_lists(dev, fused):
    case = SBC.case("small-all")
    feats = case.features.float().to(dev)
    end, emotions, B, k = case.end("happy"), case.emotions, case.rows, 3
    model = _biased(dev, case, 60.0)                       # <end> wins on every row of every decoder from the first step on
    decoders, wcat, beff, state, _ = _grouped_args(model, emotions, feats, k)
    st = state.repeat(len(decoders), 1, 1).repeat_interleave(k, 0).contiguous()

    def one_call(poll):
        return ops.lstm_beam_decode_groups(ops.CELL_LSTM, wcat, beff, [x.embed.weight for x in decoders],
                                           [x.linear.weight for x in decoders], [x.linear.bias for x in decoders], B, k,
                                           MAX_LEN + 1, START, end, state=st, fused_topk=fused, poll_every=poll, return_steps=True)
    want, steps = one_call(0)
    assert steps == MAX_LEN + 1
    assert all(2 <= len(s) <= 3 and s[0] == START and s[-1] == end for s in want), want
    for m in (1, 3):
        got, steps = one_call(m)
        assert got == want and steps <= 2 + m, (m, steps)
        styles = model.sample_beam_styles(feats, START, end, modes=emotions, k=k, poll_every=m, fused_topk=fused)
        assert [s for e in emotions for s in styles[e]] == want, m
    ops.check_device_errors()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_one_finished_decoder_waits_for_the_others(dev, fused):
    case = SBC.case("small-all")
    feats = case.features.float().to(dev)
    end, emotions, B, k = case.end("happy"), case.emotions, case.rows, 3
    model = _biased(dev, case, 60.0, only="sad")
    decoders, wcat, beff, state, states = _grouped_args(model, emotions, feats, k)
    st = state.repeat(len(decoders), 1, 1).repeat_interleave(k, 0).contiguous()
    single = {m: model._decoder(m).sample_beam(START, end, states, k=k, fused_topk=fused) for m in emotions}
    x = model._decoder("sad")
    packed = pack_cells(x._layers(), x.embed_size)
    alone, alone_steps = ops.lstm_beam_decode(ops.CELL_LSTM, [w for w, _ in packed], [b for _, b in packed], x.embed.weight,
                                              x.linear.weight, x.linear.bias, B, k, MAX_LEN + 1, START, end,
                                              state=state.repeat_interleave(k, 0).contiguous(), fused_topk=fused, poll_every=1,
                                              return_steps=True)
    assert alone == single["sad"] and all(2 <= len(s) <= 3 for s in alone) and alone_steps <= 3
    longest = max(len(s) for m in emotions for s in single[m])
    assert longest > 4                                                   # `angry` completes a five-token list at this <end>
    lists, steps = ops.lstm_beam_decode_groups(ops.CELL_LSTM, wcat, beff, [x.embed.weight for x in decoders],
                                               [x.linear.weight for x in decoders], [x.linear.bias for x in decoders], B, k,
                                               MAX_LEN + 1, START, end, state=st, fused_topk=fused, poll_every=1,
                                               return_steps=True)
    assert steps >= longest - 1 > alone_steps                            # the search ran on for the other decoders
    for g, m in enumerate(emotions):
        assert lists[g * B:(g + 1) * B] == single[m], m
    assert model.sample_beam_styles(feats, START, end, modes=emotions, k=k, poll_every=1, fused_topk=fused) == single
    ops.check_device_errors()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_nothing_completed_returns_end(dev, fused):
    case = SBC.case("small-all")
    feats = case.features.float().to(dev)
    end = case.end("happy")
    model = _biased(dev, case, -60.0)
    for m in (0, 3):
        got = model.sample_beam_styles(feats, START, end, modes=case.emotions, k=3, poll_every=m, fused_topk=fused)
        assert got == {e: [[end]] * case.rows for e in case.emotions}, m
    ops.check_device_errors()


# ---- 7. an out-of-range start token --------------------------------------------------------------------------------------
def test_a_start_token_out_of_range_raises_after_the_call(dev):
    case = SBC.case("small-all")
    model = case.module().to(dev)
    feats = case.features.float().to(dev)
    end = case.end("happy")
    ops.check_device_errors()
    for fused in (True, False):
        with pytest.raises(capnet.CapnetError, match="token id out of range"):
            model.sample_beam_styles(feats, case.V + 3, end, modes=case.emotions, k=3, fused_topk=fused)
        ops.check_device_errors()                       # (raised and cleared)
    got = model.sample_beam_styles(feats, START, end, modes=case.emotions, k=3, fused_topk=True)
    assert got["happy"] == case.reference(3, "happy")
