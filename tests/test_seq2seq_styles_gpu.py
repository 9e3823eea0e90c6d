"""Seq2Seq.sample_styles on the GPU: the grouped vocab_argmax kernel and the grouped decode step with per-group tables
each alone (against single-group launches, bit for bit), sample_styles against the fp64 restatement on every case of
tests/seq2seq_styles_cases.py (ids exactly: tests/test_seq2seq_styles_cpu.py asserts the margins of all four modes), and
against sample(mode=...) of the same model on every route (grouped call, one emotion, given states, more than 16 rows,
CAPNET_NO_FUSED_GREEDY=1) with the encoder's greedy loops counted: one per call."""
import pytest
import torch

import seq2seq_cases as SC
import seq2seq_ref as SR
import seq2seq_styles_cases as SS
from capnet import CapnetError, ops
from capnet.seq2seq import FUSED_GREEDY_OFF, EncoderRNN, Seq2Seq

pytestmark = pytest.mark.gpu

TOL_STEP = SC.TOL_STEP
G = 3


def _model(c, p, dev):
    m = Seq2Seq(c["E"], c["H"], c["V"], c["layers"], dropout=0.0)
    m.load_state_dict({k: v.float() for k, v in p.items()}, strict=True)
    return SS.set_steps(m.to(dev).eval(), c["steps"])


# ---- 1. the grouped vocab_argmax kernel, alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("V", [211, 8192])
def test_grouped_vocab_argmax(dev, H, V):
    g = torch.Generator().manual_seed(7 * V + H)
    W = torch.randn(G, V, H, generator=g) / H ** 0.5
    b = torch.randn(G, V, generator=g) * 0.1
    Wd, bd = [W[i].to(dev) for i in range(G)], [b[i].to(dev) for i in range(G)]
    for rpg in (1, 7, 16, 17, 33):
        # a planted margin: row r of group i points along row t[i, r] of group i's projection
        t = torch.randint(V, (G, rpg), generator=g)
        h = torch.stack([3.0 * W[i, t[i]] / W[i, t[i]].norm(dim=1, keepdim=True) for i in range(G)])      # [G, rpg, H]
        h = h + 0.05 * torch.randn(G, rpg, H, generator=g)
        logits = torch.einsum("grh,gvh->grv", h.double(), W.double()) + b.double()[:, None, :]
        top2 = logits.topk(2, 2)[0]
        assert float((top2[..., 0] - top2[..., 1]).min()) > 2 * TOL_STEP * float(logits.abs().max())
        want = logits.argmax(2)
        assert torch.equal(want, t)
        hd = h.reshape(G * rpg, H).to(dev)
        ws = ops.vocab_argmax_groups_workspace(G, rpg, V, dev)
        got = ops.vocab_argmax_groups(hd, Wd, bd, workspace=ws)
        again = ops.vocab_argmax_groups(hd, Wd, bd, workspace=ws)          # the same workspace: every counter re-armed
        torch.cuda.synchronize()
        assert got.dtype == torch.int64 and tuple(got.shape) == (G * rpg,)
        assert [int(ws[2 * i].item()) & 0xffffffff for i in range(G)] == [0] * G
        single = torch.cat([ops.vocab_argmax(hd[i * rpg:(i + 1) * rpg], Wd[i], bd[i]) for i in range(G)])
        assert torch.equal(got, single) and torch.equal(again, single), rpg
        assert torch.equal(got.cpu(), want.reshape(-1)), rpg
        # without biases, and with one group's bias missing
        nb = torch.cat([ops.vocab_argmax(hd[i * rpg:(i + 1) * rpg], Wd[i]) for i in range(G)])
        assert torch.equal(ops.vocab_argmax_groups(hd, Wd, workspace=ws), nb)
        mixed = ops.vocab_argmax_groups(hd, Wd, [bd[0], None, bd[2]], workspace=ws)
        assert torch.equal(mixed, torch.cat([single[:rpg], nb[rpg:2 * rpg], single[2 * rpg:]]))
        # one group's h all NaN: that group yields 0s, the others are untouched
        hn = hd.clone()
        hn[rpg:2 * rpg] = float("nan")
        nan = ops.vocab_argmax_groups(hn, Wd, bd, workspace=ws)
        assert nan[rpg:2 * rpg].cpu().tolist() == [0] * rpg
        assert torch.equal(nan[:rpg], single[:rpg]) and torch.equal(nan[2 * rpg:], single[2 * rpg:])
        assert torch.equal(ops.vocab_argmax_groups(hd, Wd, bd, workspace=ws), single)      # and the workspace is still good
    # one group is the plain kernel
    assert torch.equal(ops.vocab_argmax_groups(hd[:rpg], Wd[:1], bd[:1]), single[:rpg])
    ops.check_device_errors()


# ---- 2. the grouped decode step with per-group tables, alone -----------------------------------------------------------
def _step_inputs(E, H, rpg, L, V, seed, dev):
    g = torch.Generator().manual_seed(seed)
    kin = (E + 15) // 16 * 16
    rows = G * rpg
    tables = [torch.randn(V, E, generator=g).to(dev) for _ in range(G)]
    wcat = [(torch.randn(G, 4 * H, (kin if l == 0 else H) + H, generator=g) * 0.1).to(dev) for l in range(L)]
    beff = [(torch.randn(G, 4 * H, generator=g) * 0.1).to(dev) for l in range(L)]
    state = (torch.rand(rows, 2 * L, H, generator=g) * 2 - 1).to(dev)
    tokens = torch.randint(V, (rows,), generator=g).to(dev)
    local = torch.randint(rpg, (G, rpg), generator=g)                        # parents inside the group, repeats allowed
    return tables, wcat, beff, state, tokens, local


@pytest.mark.parametrize("E, H", [(20, 64), (30, 128), (300, 512)])
def test_grouped_decode_step_with_tables(dev, E, H):
    L, V = 2, 53
    for rpg in (1, 7, 16):
        tables, wcat, beff, state, tokens, local = _step_inputs(E, H, rpg, L, V, 100 * E + rpg, dev)
        parents = (local + torch.arange(G)[:, None] * rpg).reshape(-1).to(dev)
        for par in (None, parents):
            top, out = ops.stacked_decode_step_tables(state, wcat, beff, tables, tokens, parent_rows=par)
            assert tuple(top.shape) == (G * rpg, H) and tuple(out.shape) == tuple(state.shape)
            for i in range(G):
                rs = slice(i * rpg, (i + 1) * rpg)
                top1, out1 = ops.stacked_decode_step(state[rs], [w[i] for w in wcat], [b[i] for b in beff], tables[i], tokens[rs],
                                                     cell=ops.CELL_LSTM, parent_rows=None if par is None else local[i].to(dev))
                assert torch.equal(top[rs], top1) and torch.equal(out[rs], out1), (rpg, i, par is not None)
            # the tables are really the groups' own: group 1 on group 0's table is another result
            if par is None:
                swapped, _ = ops.stacked_decode_step_tables(state, wcat, beff, [tables[0], tables[0], tables[2]], tokens)
                assert torch.equal(swapped[:rpg], top[:rpg]) and not torch.equal(swapped[rpg:2 * rpg], top[rpg:2 * rpg])
    ops.check_device_errors()


def test_out_of_range_token_in_one_group_sets_the_error_word(dev):
    E, H, L, V, rpg = 30, 128, 2, 53, 7
    tables, wcat, beff, state, tokens, _ = _step_inputs(E, H, rpg, L, V, 9, dev)
    top, out = ops.stacked_decode_step_tables(state, wcat, beff, tables, tokens)
    ops.check_device_errors()
    bad = tokens.clone()
    bad[2 * rpg + 3] = V + 3
    top_b, out_b = ops.stacked_decode_step_tables(state, wcat, beff, tables, bad)
    with pytest.raises(CapnetError, match="token id out of range"):
        ops.check_device_errors()
    assert torch.equal(top_b[:2 * rpg], top[:2 * rpg]) and torch.equal(out_b[:2 * rpg], out[:2 * rpg])
    ops.check_device_errors()                                                # the word is cleared: the process stays usable


# ---- 3. sample_styles against the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SS.CASES))
def test_sample_styles_matches_restatement(dev, name):
    c, p, feats = SS.case(name)
    ref = SS.reference(name)
    m = _model(c, p, dev)
    got = m.sample_styles(feats.float().to(dev), SS.START)
    assert list(got) == list(SS.MODES)
    for mode in SS.MODES:
        assert got[mode].dtype == torch.int64 and tuple(got[mode].shape) == (c["rows"], c["steps"])
        assert torch.equal(got[mode].cpu(), ref[mode][0]), (name, mode)


# ---- 4. sample_styles against sample(mode=...) on the same model, one encoder run per call ---------------------------------
class _Count:
    def __init__(self, monkeypatch):
        self.n = 0
        real = EncoderRNN._greedy

        def counting(enc, *a, **kw):
            self.n += 1
            return real(enc, *a, **kw)

        monkeypatch.setattr(EncoderRNN, "_greedy", counting)

    def take(self):
        n, self.n = self.n, 0
        return n


def _per_mode(m, f, states=(None, None)):
    return {mode: m.sample(f, SS.START, states, mode=mode) for mode in SS.MODES}


def _check_styles(m, f, want, count, grouped_calls, expect_grouped, **kw):
    modes = kw.get("modes", SS.MODES)
    count.take()
    del grouped_calls[:]
    got = m.sample_styles(f, SS.START, **kw)
    assert count.take() == 1                                               # the encoder's greedy loop ran once
    assert len(grouped_calls) == expect_grouped, (grouped_calls, kw)
    assert list(got) == list(modes)
    for mode in modes:
        assert torch.equal(got[mode], want[mode]), (mode, kw)


@pytest.fixture
def grouped_calls(monkeypatch):
    calls = []
    real = ops.lstm_greedy_decode_groups
    monkeypatch.setattr(ops, "lstm_greedy_decode_groups", lambda *a, **kw: (calls.append(len(a[3])), real(*a, **kw))[1])
    return calls


EXTRA = dict(E=300, H=512, V=8192, layers=3, rows=12, steps=40, seed=0)     # no margin needed: the same arithmetic per row


@pytest.mark.parametrize("name", sorted(SS.CASES) + ["extra_r12_l3_v8192"])
def test_sample_styles_equals_sample(dev, monkeypatch, grouped_calls, name):
    if name in SS.CASES:
        c, p, feats = SS.case(name)
    else:
        c = EXTRA
        p, feats = SS.make_case(c)
    m = _model(c, p, dev)
    f = feats.float().to(dev)
    monkeypatch.delenv(FUSED_GREEDY_OFF, raising=False)
    want = _per_mode(m, f)
    count = _Count(monkeypatch)
    _check_styles(m, f, want, count, grouped_calls, 1)
    assert grouped_calls == [3]
    _check_styles(m, f, want, count, grouped_calls, 1, modes=("sad", "happy"))
    _check_styles(m, f, want, count, grouped_calls, 0, modes=("angry",))
    _check_styles(m, f, want, count, grouped_calls, 0, modes=("factual",))
    # nothing else moved
    again = _per_mode(m, f)
    for mode in SS.MODES:
        assert torch.equal(again[mode], want[mode]), mode
    ops.check_device_errors()


@pytest.mark.parametrize("name", ["e20_h64_v211_l3_r16", "e300_h512_v1000_l2_r16"])
def test_sample_styles_routes(dev, monkeypatch, grouped_calls, name):
    c, p, feats = SS.case(name)
    m = _model(c, p, dev)
    L, H, rows = c["layers"], c["H"], c["rows"]
    f = feats.float().to(dev)
    monkeypatch.delenv(FUSED_GREEDY_OFF, raising=False)
    g = torch.Generator().manual_seed(5)
    states = tuple((torch.rand(L, rows, H, generator=g) - 0.5).to(dev) for _ in range(2))
    f17 = torch.cat([f, f[:1] * 0.5])                                         # 17 rows: past FUSED_GREEDY_MAX_ROWS
    want = _per_mode(m, f)
    want_states = _per_mode(m, f, states)
    want_h_only = _per_mode(m, f, (states[0], None))
    want17 = _per_mode(m, f17)
    assert not torch.equal(want_states["happy"], want["happy"])
    count = _Count(monkeypatch)
    _check_styles(m, f, want_states, count, grouped_calls, 1, states=states)
    _check_styles(m, f, want_h_only, count, grouped_calls, 1, states=(states[0], None))
    _check_styles(m, f17, want17, count, grouped_calls, 0)
    monkeypatch.setenv(FUSED_GREEDY_OFF, "1")
    want_off = _per_mode(m, f)
    _check_styles(m, f, want_off, count, grouped_calls, 0)
    monkeypatch.delenv(FUSED_GREEDY_OFF)
    for mode in SS.MODES:
        assert torch.equal(want_off[mode], want[mode]), mode                  # (the composed loop decodes the same ids here)
    # an out-of-range start token raises through the device error word, and the process stays usable
    with pytest.raises(CapnetError):
        m.sample_styles(f, c["V"] + 5)
    _check_styles(m, f, want, count, grouped_calls, 1)
    again = _per_mode(m, f)
    for mode in SS.MODES:
        assert torch.equal(again[mode], want[mode]), mode
    ops.check_device_errors()


def test_grouped_greedy_op_is_three_single_calls(dev):
    """ops.lstm_greedy_decode_groups itself: ids and final state of every group are those of ops.lstm_greedy_decode on
    that group alone, bit for bit, also with differing start tokens and no given state."""
    from capnet.decode import pack_cells
    c, p, feats = SS.case("e30_h128_v211_l1_r7")
    m = _model(c, p, dev)
    decs = [m.decoder_happy, m.decoder_sad, m.decoder_angry]
    rows, L, E, H = 5, c["layers"], c["E"], c["H"]
    packed = [pack_cells(d._layers(), E) for d in decs]
    wcat = [torch.stack([q[l][0] for q in packed]) for l in range(L)]
    beff = [torch.stack([q[l][1] for q in packed]) for l in range(L)]
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(c["V"], (G * rows,), generator=g).to(dev)
    for state in (None, (torch.rand(G * rows, 2 * L, H, generator=g) - 0.5).to(dev)):
        ids, out = ops.lstm_greedy_decode_groups(9, wcat, beff, [d.embed.weight for d in decs], [d.linear.weight for d in decs],
                                                 [d.linear.bias for d in decs], tokens, state)
        assert tuple(ids.shape) == (G * rows, 9)
        for i, d in enumerate(decs):
            rs = slice(i * rows, (i + 1) * rows)
            ids1, out1 = ops.lstm_greedy_decode(9, [q[0] for q in packed[i]], [q[1] for q in packed[i]], d.embed.weight,
                                                d.linear.weight, d.linear.bias, start_tokens=tokens[rs],
                                                state=None if state is None else state[rs])
            assert torch.equal(ids[rs], ids1) and torch.equal(out[rs], out1), i
    with pytest.raises(CapnetError, match="per group"):                      # a table is used where it lies, never copied
        ops.lstm_greedy_decode_groups(9, wcat, beff, [d.embed.weight.t().contiguous().t() for d in decs],
                                      [d.linear.weight for d in decs], [d.linear.bias for d in decs], tokens)
    ops.check_device_errors()
