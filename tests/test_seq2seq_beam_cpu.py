"""What tests/test_seq2seq_beam_gpu.py relies on, checked without a GPU: every case of tests/seq2seq_beam_cases.py clears the
margin rule at every (k, sentence); the cases contain the situations a beam search must get right; the new C entry points
refuse bad arguments before any launch; sample_beam refuses a wrong mode or beam width."""
import ctypes as C

import pytest
import torch

import capnet
import seq2seq_beam_cases as BC
from capnet import _lib
from capnet.seq2seq import DecoderRNN, EncoderRNN, Seq2Seq
from device_beam_cases import MARGIN, MAX_LEN, START

ALL = BC.CASES + BC.COMPOSED


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_every_case_clears_the_rule(case):
    for k in case.ks:
        for r in range(case.rows):
            m = case.margin(k, r)
            bound = max(MARGIN, (MAX_LEN + 1) * BC.SC.need(case.scale))
            assert m > bound, (case, k, r, m, bound)
    m, bound, gap, gbound = case.check()          # (the bound at the largest |logit| of the whole case)
    assert m > bound and gap > gbound, (case, m, bound, gap, gbound)


def test_the_cases_cover_the_shapes():
    shapes = {(c.E, c.H, c.V, c.L) for c in BC.CASES}
    assert any(H == 64 and V == 37 for _, H, V, _ in shapes)                   # two workgroups, the last ragged
    assert any(V % 32 and E % 4 for E, _, V, _ in shapes)
    assert {1, 3} <= {L for _, _, _, L in shapes}
    full = [c for c in BC.CASES if (c.E, c.H, c.V) == (300, 512, 8192)]
    assert {"factual"} < {c.mode for c in full}
    assert all(c.H == 16 for c in BC.COMPOSED) and {c.mode for c in BC.COMPOSED} > {"factual"}


def test_the_cases_contain_what_a_beam_search_must_get_right():
    lists = {(c.name, k, r): c.reference(k, r) for c in BC.CASES for k in c.ks for r in range(c.rows)}
    assert any(len(s) >= 5 for s in lists.values())
    assert all(s == [c.end] or s[-1] == c.end for c in BC.CASES for (n, _, _), s in lists.items() if n == c.name)
    assert all(s[0] == START for c in BC.CASES if c.mode != "factual" for (n, _, _), s in lists.items()
               if n == c.name and len(s) > 1)
    # a sentence whose lists differ between k = 3 and k = 5
    assert any(lists[(c.name, 3, r)] != lists[(c.name, 5, r)] for c in BC.CASES if c.ks == (3, 5) for r in range(c.rows))
    # beams of one sentence completing at different steps: the completed list of some search holds two lengths
    from device_beam_ref import DeviceBeam
    seen = False
    for c in BC.CASES[:3]:
        for r in range(c.rows):
            step_fn, state = c.initial(5, r)
            beam = DeviceBeam(1, 5, c.V, START, c.end)
            words = torch.LongTensor([[START]] * 5)
            for step in range(1, MAX_LEN + 2):
                out, state = step_fn(words, state)
                sc = torch.tensor(beam.scores[0], dtype=torch.float64).unsqueeze(1) + torch.log_softmax(out, 1)

                def topk(i, rows, live, sc=sc):
                    v, f = sc[:rows].reshape(-1).topk(live)
                    return v.tolist(), f.tolist()
                nxt, par = beam.advance(step, topk)
                if not beam.live_total:
                    break
                words = torch.LongTensor(nxt).unsqueeze(1)
                state = tuple(s[par] for s in state)
            assert beam.finish()[0] == c.beam(5, r)
            seen |= len({len(sq) for _, sq, _ in beam.done[0]}) > 1
    assert seen


# ---- the C entry points refuse before any launch (no device is touched: every pointer below is a dummy) ---------------
def _lib_or_skip():
    return _lib.lib()


def test_the_size_functions_return_zero_outside_their_limits():
    L = _lib_or_skip()
    assert L.capnet_vocab_topk_ws_bytes(15, 5, 8192) == 16 + 256 * 15 * 8 * 6
    for rows, k, V in ((0, 5, 37), (3, 0, 37), (3, 17, 37), (3, 5, 4), (-1, 1, 1)):
        assert L.capnet_vocab_topk_ws_bytes(rows, k, V) == 0, (rows, k, V)
    ok = (2, 3, 5, 64, 37, 13)
    fused, unfused = L.capnet_lstm_beam_decode_ws_bytes(*ok, 1), L.capnet_lstm_beam_decode_ws_bytes(*ok, 0)
    assert fused > 0 and unfused == L.capnet_beam_decode_ws_bytes(*ok)             # unfused: capnet_beam_decode's layout
    assert L.capnet_lstm_beam_decode_ws_bytes(2, 3, 5, 512, 8192, 21, 1) < L.capnet_lstm_beam_decode_ws_bytes(2, 3, 5, 512, 8192, 21, 0)
    for bad in ((0, 3, 5, 64, 37, 13), (9, 3, 5, 64, 37, 13), (2, 0, 5, 64, 37, 13), (2, 3, 0, 64, 37, 13),
                (2, 3, 17, 64, 37, 13), (2, 3, 5, 64, 4, 13), (2, 3, 5, 64, 37, 0)):
        assert L.capnet_lstm_beam_decode_ws_bytes(*bad, 1) == 0 and L.capnet_lstm_beam_decode_ws_bytes(*bad, 0) == 0, bad
    assert L.capnet_lstm_beam_decode_ws_bytes(2, 3, 5, 100, 37, 13, 1) == 0        # the fused top-k's hidden sizes


_BUF = (C.c_char * 4096)()
_P = C.cast(C.addressof(_BUF) + (-C.addressof(_BUF)) % 16, C.c_void_p)      # 16-B aligned host memory: never dereferenced


def test_vocab_topk_refuses_bad_arguments():
    L = _lib_or_skip()

    def call(rows=3, H=64, V=37, k=5, h=_P, w=_P, ws=_P, values=_P, index=_P, lse=_P):
        return L.capnet_vocab_topk(h, w, None, rows, H, V, k, ws, values, index, lse, None)
    for kw in (dict(k=0), dict(k=17), dict(k=5, V=4), dict(H=100), dict(H=16), dict(rows=0), dict(h=None), dict(w=None),
               dict(ws=None), dict(values=None), dict(index=None), dict(lse=None), dict(h=C.c_void_p(_P.value + 4))):
        assert call(**kw) != 0, kw


def test_beam_advance_topk_refuses_bad_arguments():
    L = _lib_or_skip()

    def call(beam=_P, values=_P, index=_P, lse=_P, V=37, n=2, k=3, max_steps=5, step=1, nxt=_P, par=_P):
        return L.capnet_beam_advance_topk(beam, values, index, lse, V, n, k, max_steps, step, 2, nxt, par, None)
    for kw in (dict(k=0), dict(k=17), dict(k=5, V=4), dict(n=0), dict(step=0), dict(step=6), dict(beam=None), dict(values=None),
               dict(index=None), dict(lse=None), dict(nxt=None), dict(par=None)):
        assert call(**kw) != 0, kw


def test_lstm_beam_decode_refuses_bad_arguments():
    L = _lib_or_skip()
    two = (C.c_void_p * 2)(_P, _P)
    null2 = (C.c_void_p * 2)(_P, None)
    steps = C.c_int(-1)

    def call(cell=1, nl=2, n=2, k=3, E=12, H=64, V=37, T=5, start=1, emb=_P, wcat=two, beff=two, Cw=_P, ws=_P, slab=_P,
             slab_floats=1 << 20, fused=1, poll=0, seqs=_P, lengths=_P, flag=_P, first=None):
        return L.capnet_lstm_beam_decode(cell, nl, n, k, E, H, V, T, start, 2, first, emb, wcat, beff, Cw, None, None, ws, slab,
                                         slab_floats, fused, poll, seqs, lengths, C.byref(steps), flag, None)
    for kw in (dict(k=0), dict(k=17), dict(k=5, V=4), dict(H=100), dict(H=16), dict(cell=2), dict(nl=0), dict(nl=9), dict(n=0),
               dict(T=0), dict(poll=-1), dict(start=-1), dict(emb=None), dict(wcat=None), dict(beff=None), dict(Cw=None),
               dict(ws=None), dict(seqs=None), dict(lengths=None), dict(flag=None), dict(wcat=null2), dict(beff=null2),
               dict(fused=0, slab=None), dict(fused=0, slab_floats=10), dict(first=C.c_void_p(_P.value + 4)),
               dict(ws=C.c_void_p(_P.value + 8))):
        assert call(**kw) != 0, kw
    assert steps.value == -1                       # nothing ran


# ---- Python: refused without a device ------------------------------------------------------------------------------
def test_sample_beam_refuses_a_wrong_mode_or_width():
    model = Seq2Seq(12, 64, 37, 1, dropout=0.0, max_seq_length=4)
    feats = torch.zeros(2, 12)
    for mode in ("joyful", "", None, "Factual"):
        with pytest.raises(capnet.CapnetError, match="mode name wrong"):
            model.sample_beam(feats, 1, 2, mode=mode)
    zeros = torch.zeros(1, 2, 64)
    for k in (0, 17, 38):
        with pytest.raises(capnet.CapnetError, match="sample_beam: k="):
            model.encoder.sample_beam(feats, 1, 2, k=k)
        with pytest.raises(capnet.CapnetError, match="sample_beam: k="):
            model.decoder_happy.sample_beam(1, 2, (zeros, zeros), k=k)
    assert isinstance(model.encoder, EncoderRNN) and isinstance(model.decoder_sad, DecoderRNN)
