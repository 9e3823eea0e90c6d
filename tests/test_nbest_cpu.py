"""N-best lists from the beam searches, what needs no GPU: the new symbols, the host-side argument checks, the workspace
offsets against their _ws_bytes siblings, the host ranking (capnet.beam.rank_completed) on hand-written lists, the keyword's
refusals -- and the admission of every case tests/test_nbest_gpu.py runs (tests/nbest_cases.py: THE RULE), so that nothing is
skipped there."""
import ctypes as C
import inspect

import pytest

import capnet
import nbest_cases as NC
import nbest_ref
from capnet import _lib, beam, decode, ops
from nbest_cases import MARGIN, MAX_LEN, PENALTIES

NEW = ("capnet_beam_nbest", "capnet_beam_nbest_traced", "capnet_beam_decode_ws_beam_offset",
       "capnet_att_beam_decode_alphas_ws_trace_offset", "capnet_att_beam_decode_alphas_ws_hist_offset", "capnet_alpha_gather")


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_exported():
    lib = capnet.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.capnet_abi_version() == 1


def _p(addr):
    return C.c_void_p(addr)


def _refused(rc, word):
    msg = capnet.lib().capnet_last_error().decode()
    assert rc != 0 and word in msg, (rc, msg)


def test_nbest_argument_checks_need_no_gpu():
    lib = capnet.lib()
    a = _p(0x1000)                                       # never dereferenced: every check precedes the launch
    ok = (a, 3, 5, 6, 0.0, a, a, a, a, None)
    for bad in (0, 5, 6, 7, 8):                          # a null state, sequences, lengths, scores, counts
        args = list(ok)
        args[bad] = None
        _refused(lib.capnet_beam_nbest(*args), "null")
    for bad, addr in ((0, 0x1002), (5, 0x1004), (6, 0x1002), (7, 0x1001), (8, 0x1002)):
        args = list(ok)
        args[bad] = _p(addr)
        _refused(lib.capnet_beam_nbest(*args), "aligned")
    _refused(lib.capnet_beam_nbest(a, 3, 17, 6, 0.0, a, a, a, a, None), "k=17")
    _refused(lib.capnet_beam_nbest(a, 3, 0, 6, 0.0, a, a, a, a, None), "k=0")
    _refused(lib.capnet_beam_nbest(a, 0, 5, 6, 0.0, a, a, a, a, None), "n=0")
    _refused(lib.capnet_beam_nbest(a, 3, 5, 0, 0.0, a, a, a, a, None), "max_steps=0")
    _refused(lib.capnet_beam_nbest(a, 3, 5, 6, float("inf"), a, a, a, a, None), "finite")
    _refused(lib.capnet_beam_nbest(a, 3, 5, 6, float("nan"), a, a, a, a, None), "finite")
    # traced: capnet_beam_finish_traced's checks -- the trace and the rows are both required, 4-byte aligned
    okt = (a, a, 3, 5, 6, 0.0, a, a, a, a, a, None)
    for bad in (1, 10):
        args = list(okt)
        args[bad] = None
        _refused(lib.capnet_beam_nbest_traced(*args), "null trace or rows")
    for bad in (0, 1, 10):
        args = list(okt)
        args[bad] = _p(0x1002)
        _refused(lib.capnet_beam_nbest_traced(*args), "4-byte aligned")
    _refused(lib.capnet_beam_nbest_traced(a, a, 3, 17, 6, 0.0, a, a, a, a, a, None), "k=17")
    _refused(lib.capnet_beam_nbest_traced(None, a, 3, 5, 6, 0.0, a, a, a, a, a, None), "null")


def test_alpha_gather_argument_checks_need_no_gpu():
    lib = capnet.lib()
    a = _p(0x1000)
    ok = (a, a, 15, 15, 13, 9, a, None)
    for bad in (0, 1, 6):
        args = list(ok)
        args[bad] = None
        _refused(lib.capnet_alpha_gather(*args), "null")
        args[bad] = _p(0x1002)
        _refused(lib.capnet_alpha_gather(*args), "aligned")
    for bad, v in ((2, 0), (3, 0), (4, 0), (4, 65536), (5, 0)):
        args = list(ok)
        args[bad] = v
        _refused(lib.capnet_alpha_gather(*args), "alpha_gather")


def test_workspace_offsets_follow_their_ws_bytes():
    lib = capnet.lib()
    nl, H, V, T = 2, 64, 37, 13
    for groups, n, k, fused in ((1, 3, 5, 0), (1, 3, 5, 1), (3, 3, 5, 0), (3, 3, 5, 1), (1, 1, 1, 0), (8, 2, 16, 1), (1, 64, 5, 0)):
        total = lib.capnet_lstm_beam_decode_groups_ws_bytes(nl, groups, n, k, H, V, T, fused)
        off = lib.capnet_beam_decode_ws_beam_offset(nl, n, k, H, V, T, fused, groups)
        assert total and off and off % 16 == 0
        assert off + lib.capnet_beam_state_bytes(groups * n, k, T) <= total, (groups, n, k, fused)
        if groups == 1:        # the same layout as the one-group searches'
            assert total == lib.capnet_lstm_beam_decode_ws_bytes(nl, n, k, H, V, T, fused)
            if not fused:
                assert total == lib.capnet_beam_decode_ws_bytes(nl, n, k, H, V, T)
        elif not fused:        # capnet_beam_decode_groups: the state of groups x n images behind the unfused layout
            assert off == lib.capnet_beam_decode_ws_beam_offset(nl, groups * n, k, H, V, T, 0, 1)
            assert total == lib.capnet_beam_decode_ws_bytes(nl, groups * n, k, H, V, T)
    # refused wherever the sibling refuses
    for args in ((0, 1, 3, 5, H, V, T, 0), (9, 1, 3, 5, H, V, T, 0), (nl, 0, 3, 5, H, V, T, 0), (nl, 9, 3, 5, H, V, T, 0),
                 (nl, 1, 0, 5, H, V, T, 0), (nl, 1, 3, 17, H, V, T, 0), (nl, 1, 3, 0, H, V, T, 0), (nl, 1, 3, 5, 0, V, T, 0),
                 (nl, 1, 3, 5, H, 4, T, 0), (nl, 1, 3, 5, H, V, 0, 0), (nl, 1, 3, 5, 48, V, T, 1)):
        nlay, groups, n, k, h, v, t, fused = args
        sibling = lib.capnet_lstm_beam_decode_groups_ws_bytes(nlay, groups, n, k, h, v, t, fused)
        assert (lib.capnet_beam_decode_ws_beam_offset(nlay, n, k, h, v, t, fused, groups) == 0) == (sibling == 0), args
    assert lib.capnet_beam_decode_ws_beam_offset(nl, 3, 17, H, V, T, 0, 1) == 0
    # the attention searches: the state at the unfused offset, the trace and the history behind the search's own workspace
    P, A, Cf, E = 9, 32, 512, 24
    for groups, n, k in ((1, 3, 5), (3, 3, 3), (1, 1, 16)):
        dims = (nl, groups, n, k, P, A, Cf, E, H, 97, T)
        nq = groups * n
        total = lib.capnet_att_beam_decode_alphas_ws_bytes(*dims)
        base = lib.capnet_att_beam_decode_ws_bytes(nl, nq, k, P, A, Cf, E, H, 97, T)
        trace, hist = lib.capnet_att_beam_decode_alphas_ws_trace_offset(*dims), lib.capnet_att_beam_decode_alphas_ws_hist_offset(*dims)
        beam_off = lib.capnet_beam_decode_ws_beam_offset(nl, nq, k, H, 97, T, 0, 1)
        assert total and trace == base and trace % 16 == 0 and hist % 16 == 0
        assert beam_off + lib.capnet_beam_state_bytes(nq, k, T) <= base
        assert trace + lib.capnet_beam_trace_bytes(nq, k, T) + nq * T * 4 <= hist
        assert hist + T * nq * k * P * 4 <= total
    for dims in ((nl, 0, 3, 5, P, A, Cf, E, H, 97, T), (nl, 9, 3, 5, P, A, Cf, E, H, 97, T), (nl, 1, 0, 5, P, A, Cf, E, H, 97, T),
                 (nl, 1, 3, 17, P, A, Cf, E, H, 97, T), (nl, 1, 3, 5, P, A, Cf, E, H, 97, 0), (0, 1, 3, 5, P, A, Cf, E, H, 97, T)):
        assert lib.capnet_att_beam_decode_alphas_ws_bytes(*dims) == 0, dims
        assert lib.capnet_att_beam_decode_alphas_ws_trace_offset(*dims) == 0, dims
        assert lib.capnet_att_beam_decode_alphas_ws_hist_offset(*dims) == 0, dims


# ---- 2. the host ranking ---------------------------------------------------------------------------------------------
S, E_ = 1, 2
DONE = [(-6.5, [S, E_]),                        # completion order: the worst first
        (-0.5, [S, 3, E_]),
        (-1.0, [S, 4, 5, 5, 5, 5, E_]),
        (-0.5, [S, 7, E_]),                     # equal to the second, later
        (-2.0, [S, 8, 9, E_])]


def test_host_ranking_of_a_hand_written_list():
    tokens = lambda out: [q for q, _ in out]      # noqa: E731
    r0 = beam.rank_completed(DONE)
    assert tokens(r0) == [[S, 3, E_], [S, 7, E_], [S, 4, 5, 5, 5, 5, E_], [S, 8, 9, E_], [S, E_]]        # the tie: the earlier
    assert [s for _, s in r0] == [-0.5, -0.5, -1.0, -2.0, -6.5] and all(isinstance(s, float) for _, s in r0)
    # penalty 1: -6.5, -0.25, -1/6, -0.25, -2/3
    r1 = beam.rank_completed(DONE, 1.0)
    assert tokens(r1) == [[S, 4, 5, 5, 5, 5, E_], [S, 3, E_], [S, 7, E_], [S, 8, 9, E_], [S, E_]]
    assert [s for _, s in r1] == [-1.0, -0.5, -0.5, -2.0, -6.5]                                        # the raw scores
    # penalty 0.7: -6.5, -0.5 / 2^0.7 = -0.3078, -1 / 6^0.7 = -0.2853, -0.3078, -2 / 3^0.7 = -0.9270
    r07 = beam.rank_completed(DONE, 0.7)
    assert tokens(r07) == tokens(r1)
    assert beam.rank_completed([]) == [] and beam.rank_completed([], 1.0) == []
    assert beam.rank_completed(DONE[:1], 0.7) == [([S, E_], -6.5)]
    # the lists are copies; entry 0 at penalty 0 is the first maximum, the searches' winner
    assert r0[0][0] is not DONE[1][1]
    scores = [s for s, _ in DONE]
    assert r0[0][0] == DONE[scores.index(max(scores))][1]
    # the reference side states the same rule
    for p in (0.0, 0.7, 1.0):
        assert beam.rank_completed(DONE, p) == nbest_ref.rank(DONE, p)
    assert nbest_ref.reordered(DONE, 0.0) and nbest_ref.min_gap(DONE, 0.0) == 0.0


def test_length_penalty_without_nbest_raises():
    for fn in (ops.beam_decode, ops.lstm_beam_decode, ops.lstm_beam_decode_groups, ops.att_beam_decode, decode.beam_decode,
               decode.plain_styles, decode.att_styles, beam.beam_search, beam.beam_search_device, beam.beam_search_batched):
        par = inspect.signature(fn).parameters
        assert par["nbest"].default is False and par["length_penalty"].default == 0.0, fn
    with pytest.raises(capnet.CapnetError, match="nbest=True"):
        ops.check_length_penalty("x", False, 0.7)
    with pytest.raises(capnet.CapnetError, match="finite"):
        ops.check_length_penalty("x", True, float("nan"))
    assert ops.check_length_penalty("x", True, 1) == 1.0 and ops.check_length_penalty("x", False, 0) == 0.0
    # the keyword is refused before anything runs, on every front end
    with pytest.raises(capnet.CapnetError, match="nbest=True"):
        decode.beam_decode(None, None, (None,), 3, 5, 1, 2, length_penalty=0.5)
    with pytest.raises(capnet.CapnetError, match="nbest=True"):
        ops.beam_decode(ops.CELL_LSTM, [], [], None, None, None, 3, 5, 13, 1, 2, length_penalty=0.5)
    with pytest.raises(capnet.CapnetError, match="nbest=True"):
        ops.lstm_beam_decode(ops.CELL_LSTM, [], [], None, None, None, 3, 5, 13, 1, 2, length_penalty=0.5)
    with pytest.raises(capnet.CapnetError, match="nbest=True"):
        ops.lstm_beam_decode_groups(ops.CELL_LSTM, [], [], [], [], None, 3, 5, 13, 1, 2, length_penalty=0.5)
    from capnet.seq2seq import Seq2Seq
    m = Seq2Seq(12, 16, 37, 1, dropout=0.0, max_seq_length=MAX_LEN)
    import torch
    with pytest.raises(capnet.CapnetError, match="nbest=True"):
        m.sample_beam_styles(torch.zeros(2, 12), 1, 2, length_penalty=1.0)


def test_the_keyword_is_on_the_public_interface():
    from capnet.model import DecoderFactoredLSTM
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model import DecoderRNN
    from capnet.nic_model_att import DecoderRNNAtt
    from capnet.nic_stacked import StackedDecoderRNN, StackedDecoderRNNAtt
    from capnet.seq2seq import DecoderRNN as S2SDecoder, EncoderRNN, Seq2Seq
    from capnet.stacked import StackedFactoredLSTM
    from capnet.stacked_att import StackedFactoredLSTMAtt
    fns = []
    for cls in (DecoderFactoredLSTM, DecoderFactoredLSTMAtt, DecoderRNN, DecoderRNNAtt, StackedDecoderRNN, StackedDecoderRNNAtt,
                StackedFactoredLSTM, StackedFactoredLSTMAtt):
        fns += [cls.sample, cls.sample_batch]
    fns += [EncoderRNN.sample_beam, S2SDecoder.sample_beam, Seq2Seq.sample_beam, Seq2Seq.sample_beam_styles]
    for fn in fns:
        par = inspect.signature(fn).parameters
        assert list(par)[-2:] == ["nbest", "length_penalty"], fn
        assert par["nbest"].default is False and par["length_penalty"].default == 0.0, fn
    # sample_styles' parameter list is pinned (tests/test_style_decode_cpu.py): its n-best comes from a method beside it
    for cls in (DecoderFactoredLSTM, StackedFactoredLSTM, DecoderFactoredLSTMAtt, StackedFactoredLSTMAtt):
        par = inspect.signature(cls.sample_styles_nbest).parameters
        assert list(par)[:7] == list(inspect.signature(cls.sample_styles).parameters) and par["length_penalty"].default == 0.0
        assert ("return_alphas" in par) == hasattr(cls, "sample_styles_alphas")


# ---- 3. the stored-logits tables hold what the GPU test needs ---------------------------------------------------------
@pytest.mark.parametrize("k", NC.TABLE_KS)
def test_tables_hold_every_situation_with_room(k):
    model, gap = NC.drive_model(k)
    assert gap > NC.TABLE_GAP, gap
    for p in (0.0, 0.7, 1.0):
        assert NC.table_rank_gap(model, p) > NC.TABLE_GAP, p
    if k >= 3:
        assert NC.SITUATIONS <= model.events(NC.TABLE_T), NC.SITUATIONS - model.events(NC.TABLE_T)
    counts = [len(model.completed(i)) for i in range(NC.TABLE_N)]
    assert counts == [k, k, 0]
    nb = model.nbest(0.0)
    assert [q for q, _ in nb[0]][0] == model.finish()[0] and [q for q, _ in nb[1]][0] == model.finish()[1]
    if k >= 3:
        # the tie: same step, equal scores, the earlier completion first at every penalty
        (qa, sa), (qb, sb) = nb[1][0], nb[1][1]
        assert sa == sb and qa == [1, 3, 2] and qb == [1, 4, 2]
        assert float(torch_f32(sa)) == float(torch_f32(sb))
        assert model.nbest(1.0)[0][0][0] == [1, 4, 5, 5, 5, 5, 2] and nb[0][0][0] == [1, 3, 2]
    rows = model.nbest_rows(NC.TABLE_T, 1.0)
    for i in range(NC.TABLE_N):
        for r, (q, _) in enumerate(model.nbest(1.0)[i]):
            m = len(q) - 1
            assert all(i * k <= x < (i + 1) * k for x in rows[i][r][:m]) and rows[i][r][m:] == [-1] * (NC.TABLE_T - m)
        assert rows[i][counts[i]:] == [[-1] * NC.TABLE_T] * (k - counts[i])


def torch_f32(x):
    import torch
    return torch.tensor(x, dtype=torch.float32)


# ---- 4. admission: THE RULE ------------------------------------------------------------------------------------------
def _unit_ids():
    return list(NC.units())


@pytest.mark.parametrize("name", _unit_ids())
def test_every_case_of_every_unit_is_admitted(name):
    u = NC.units()[name]
    bound = u.bound()
    for k, i in u.cases():
        s = u.search(k, i)
        assert s.margin > bound, (k, i, s.margin, bound)
        for p in PENALTIES:
            assert s.gap(p) > bound, (k, i, p, s.gap(p), bound)
            assert u.admitted(k, i, p)
        # the fp64 n-best agrees with the fp64 winner of the search the other tests compare with
        if s.done:
            assert s.nbest(0.0)[0][0] == _winner(u, k, i)
        else:
            assert _winner(u, k, i) == [u.end]


@pytest.mark.parametrize("key", list(NC.families()), ids=lambda key: "%s-%s" % key)
def test_every_family_completes_three_and_is_reordered_somewhere(key):
    us = NC.families()[key]
    searches = [u.search(k, i) for u in us for k, i in u.cases()]
    assert any(len(s.done) >= 3 for s in searches), "no case of %s completes three hypotheses" % (key,)
    assert any(nbest_ref.reordered(s.done, 1.0) for s in searches), "penalty 1 reorders no case of %s" % (key,)


def _winner(u, k, i):
    src = u.source
    if u.kind == "image":
        return src.reference(k, i)
    if u.kind == "style":
        return src.reference(u.mode, k, i)
    case = src if u.kind == "seq2seq" else src.cases[u.mode]
    return case.beam(k, i)


def test_the_24_device_cases_are_as_the_issue_states():
    """The four families of tests/device_beam_cases.py: every case completes at least two hypotheses, penalty 0 never
    reorders the list against completion order; the smallest neighbour gaps span 0.0074 .. 4.7 at penalty 0 and 0.0030 ..
    0.21 at penalty 1. Penalty 1 reorders the list in 18 of the 24 (the issue counted 16; 17 change rank 0): all six of
    each plain family, five of DecoderRNNAtt, one of StackedFactoredLSTMAtt-2."""
    gaps, moved0, moved1, cases = {0.0: [], 1.0: []}, 0, 0, 0
    for u in NC.device_units():
        assert u.bound() == MARGIN
        for k, i in u.cases():
            s = u.search(k, i)
            cases += 1
            assert len(s.done) >= 2, (u.name, k, i)
            for p in PENALTIES:
                gaps[p].append(s.gap(p))
            moved0 += nbest_ref.reordered(s.done, 0.0)
            moved1 += nbest_ref.reordered(s.done, 1.0)
    print("penalty 0: gaps %.4f .. %.4f; penalty 1: %.4f .. %.4f; reordered %d / %d of %d"
          % (min(gaps[0.0]), max(gaps[0.0]), min(gaps[1.0]), max(gaps[1.0]), moved0, moved1, cases))
    assert cases == 24 and moved0 == 0 and moved1 == 18
    assert 0.0073 < min(gaps[0.0]) < 0.0075 and 4.6 < max(gaps[0.0]) < 4.8
    assert 0.0029 < min(gaps[1.0]) < 0.0031 and 0.20 < max(gaps[1.0]) < 0.22
