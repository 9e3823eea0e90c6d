"""Seq2Seq.sample_styles, the part that needs no GPU: the grouped greedy entries are declared and exported, bad arguments
are refused before any launch, the Python surface exists, bad `modes` raise before anything runs, and every case of the
GPU test has the margin its exact comparison needs in all four modes -- with ids that differ between the emotions in
every row, so a kernel that used one group's embedding or projection for every group could not pass there."""
import ctypes as C
import inspect
import os

import pytest

import capnet
import seq2seq_cases as SC
import seq2seq_styles_cases as SS
from capnet import CapnetError, _lib, ops
from capnet.seq2seq import Seq2Seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capnet_lstm_greedy_decode_groups", "capnet_lstm_greedy_decode_groups_ws_bytes")
ALSO = ("capnet_vocab_argmax_groups", "capnet_vocab_argmax_groups_ws_bytes", "capnet_stacked_decode_step_tables")


def test_new_entries_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "capnet.h")) as f:
        src = f.read()
    lib = capnet.lib()
    for name in NEW + ALSO:
        assert name + "(" in src, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.capnet_abi_version() == 1


def test_workspace_sizes():
    lib = capnet.lib()
    # one group: today's sizes, byte for byte
    for rows, V in ((1, 37), (12, 8192), (16, 7411)):
        assert lib.capnet_vocab_argmax_groups_ws_bytes(1, rows, V) == lib.capnet_vocab_argmax_ws_bytes(rows, V)
        for L in (1, 3):
            assert (lib.capnet_lstm_greedy_decode_groups_ws_bytes(L, 1, rows, 512, V)
                    == lib.capnet_lstm_greedy_decode_ws_bytes(L, rows, 512, V))
    # a 16-byte counter block per group and groups x workgroups x rows-per-group partials
    assert lib.capnet_vocab_argmax_groups_ws_bytes(3, 7, 211) == 3 * 16 + 3 * 7 * 7 * 8
    assert lib.capnet_vocab_argmax_groups_ws_bytes(0, 7, 211) == 0 and lib.capnet_vocab_argmax_groups_ws_bytes(9, 7, 211) == 0
    assert lib.capnet_lstm_greedy_decode_groups_ws_bytes(2, 9, 4, 512, 100) == 0
    assert lib.capnet_lstm_greedy_decode_groups_ws_bytes(2, 3, 0, 512, 100) == 0


# fake, suitably aligned addresses: every call below must be refused before anything is launched or dereferenced on the
# device (no GPU is present when this file runs)
P = 0x10000


def _arr(*vals):
    return (C.c_void_p * len(vals))(*vals)


def _greedy(**kw):
    a = dict(nlayers=1, groups=3, rpg=5, E=12, H=64, V=37, steps=4, start=P, emb=_arr(P, P, P), wcat=_arr(P), beff=_arr(P),
             Cw=_arr(P, P, P), Cb=_arr(P, P, P), state0=None, ws=P, ids=P, sout=P, err=P)
    a.update(kw)
    lib = capnet.lib()
    rc = lib.capnet_lstm_greedy_decode_groups(a["nlayers"], a["groups"], a["rpg"], a["E"], a["H"], a["V"], a["steps"], a["start"],
                                              a["emb"], a["wcat"], a["beff"], a["Cw"], a["Cb"], a["state0"], a["ws"], a["ids"],
                                              a["sout"], a["err"], None)
    return rc, lib.capnet_last_error().decode()


@pytest.mark.parametrize("bad, word", [
    (dict(groups=0), "groups 0"), (dict(groups=9), "groups 9"), (dict(groups=-1), "groups"),
    (dict(rpg=0), "rows 0"), (dict(rpg=-3), "rows -3"),
    (dict(start=None), "start_tokens"), (dict(emb=None), "null"), (dict(wcat=None), "null"), (dict(beff=None), "null"),
    (dict(Cw=None), "null"), (dict(ws=None), "null"), (dict(ids=None), "null"), (dict(sout=None), "null"), (dict(err=None), "null"),
    (dict(emb=_arr(P, None, P)), "group 1"), (dict(emb=_arr(P, P, None)), "group 2"), (dict(Cw=_arr(None, P, P)), "group 0"),
    (dict(Cb=_arr(P, P, None)), "group 2"), (dict(wcat=_arr(None)), "layer 0"), (dict(beff=_arr(None)), "layer 0"),
    (dict(nlayers=2, wcat=_arr(P, None), beff=_arr(P, P)), "layer 1"),
    (dict(ws=P + 8), "aligned"), (dict(state0=P + 4), "aligned"), (dict(sout=P + 4), "aligned"),
    (dict(Cw=_arr(P, P + 4, P)), "aligned"), (dict(wcat=_arr(P + 8)), "aligned"),
    (dict(H=16), "unsupported"), (dict(H=96), "unsupported"), (dict(E=0), "unsupported"), (dict(E=2048), "unsupported"),
    (dict(nlayers=0), "layers 0"), (dict(nlayers=9, wcat=_arr(*[P] * 9), beff=_arr(*[P] * 9)), "layers 9"),
    (dict(steps=0), "steps 0"), (dict(steps=-1), "steps"),
])
def test_grouped_greedy_decode_refuses_bad_arguments(bad, word):
    rc, msg = _greedy(**bad)
    assert rc != 0 and msg.startswith("lstm_greedy_decode") and word in msg, msg


def test_the_one_group_entry_still_refuses_bad_arguments():
    lib = capnet.lib()

    def call(**kw):
        a = dict(nlayers=1, rows=5, E=12, H=64, V=37, steps=4, feats=None, start=P, emb=P, wcat=_arr(P), beff=_arr(P), Cw=P, Cb=None,
                 state0=None, ws=P, ids=P, sout=P, err=P)
        a.update(kw)
        rc = lib.capnet_lstm_greedy_decode(a["nlayers"], a["rows"], a["E"], a["H"], a["V"], a["steps"], a["feats"], a["start"],
                                           a["emb"], a["wcat"], a["beff"], a["Cw"], a["Cb"], a["state0"], a["ws"], a["ids"],
                                           a["sout"], a["err"], None)
        return rc, lib.capnet_last_error().decode()

    for bad, word in ((dict(rows=0), "rows 0"), (dict(emb=None), "null"), (dict(Cw=None), "null"), (dict(Cw=P + 4), "aligned"),
                      (dict(feats=P), "either"), (dict(start=None), "either"), (dict(steps=0), "steps 0"),
                      (dict(nlayers=9), "layers"), (dict(H=96), "unsupported"), (dict(wcat=_arr(None)), "layer 0")):
        rc, msg = call(**bad)
        assert rc != 0 and msg.startswith("lstm_greedy_decode") and word in msg, (bad, msg)


def test_grouped_argmax_and_table_step_refuse_bad_arguments():
    lib = capnet.lib()
    w3, t3 = _arr(P, P, P), _arr(P, P, P)
    for args, word in (((P, w3, None, 0, 5, 64, 37, P, P, None), "groups 0"), ((P, w3, None, 9, 5, 64, 37, P, P, None), "groups 9"),
                       ((P, w3, None, 3, 0, 64, 37, P, P, None), "rows per group"), ((P, w3, None, 3, 5, 96, 37, P, P, None), "unsupported"),
                       ((P, _arr(P, None, P), None, 3, 5, 64, 37, P, P, None), "group 1"),
                       ((P, _arr(P, P, P + 4), None, 3, 5, 64, 37, P, P, None), "group 2"),
                       ((None, w3, None, 3, 5, 64, 37, P, P, None), "null"), ((P, w3, None, 3, 5, 64, 37, P + 8, P, None), "aligned")):
        rc = lib.capnet_vocab_argmax_groups(*args)
        msg = lib.capnet_last_error().decode()
        assert rc != 0 and msg.startswith("vocab_argmax") and word in msg, (args, msg)
    base = dict(cell=1, nlayers=1, groups=3, rpg=5, E=12, H=64, V=37, tokens=P, tables=t3, wcat=_arr(P), beff=_arr(P), sin=P,
                parent=None, sout=2 * P, top=P, err=P)
    for bad, word in ((dict(groups=0), "groups 0"), (dict(groups=9), "groups 9"), (dict(rpg=0), "rows per group"),
                      (dict(tokens=None), "token ids"), (dict(tables=None), "token ids"), (dict(tables=_arr(P, P, None)), "group 2"),
                      (dict(H=96), "unsupported"), (dict(sout=P), "differ"), (dict(wcat=_arr(None)), "layer 0"), (dict(err=None), "err_flag")):
        a = dict(base, **bad)
        rc = lib.capnet_stacked_decode_step_tables(a["cell"], a["nlayers"], a["groups"], a["rpg"], a["E"], a["H"], a["V"], a["tokens"],
                                                   a["tables"], a["wcat"], a["beff"], a["sin"], a["parent"], a["sout"], a["top"],
                                                   a["err"], None)
        msg = lib.capnet_last_error().decode()
        assert rc != 0 and msg.startswith("stacked_decode_step") and word in msg, (bad, msg)


def test_the_python_surface():
    par = inspect.signature(Seq2Seq.sample_styles).parameters
    assert list(par) == ["self", "features", "start_token", "states", "modes"]
    assert par["states"].default == (None, None) and tuple(par["modes"].default) == SS.MODES
    par = inspect.signature(ops.lstm_greedy_decode_groups).parameters
    assert list(par) == ["steps", "wcat", "beff", "embs", "Cws", "Cbs", "start_tokens", "state"] and par["state"].default is None
    assert ops.MAX_GROUPS == 8
    # Seq2Seq.sample keeps its signature
    assert list(inspect.signature(Seq2Seq.sample).parameters) == ["self", "features", "start_token", "states", "mode"]


def test_modes_are_checked_before_anything_runs(monkeypatch):
    from capnet.seq2seq import EncoderRNN
    m = Seq2Seq(12, 64, 37, 2)
    monkeypatch.setattr(EncoderRNN, "sample", lambda *a, **k: pytest.fail("the encoder ran"))
    for bad in ((), ("happy", "happy"), ("factual", "sad", "factual")):
        with pytest.raises(ValueError, match="distinct"):
            m.sample_styles(None, 1, modes=bad)
    with pytest.raises(CapnetError, match="mode name wrong"):      # as sample()
        m.sample_styles(None, 1, modes=("happy", "glad"))
    with pytest.raises(CapnetError, match="mode name wrong"):
        m.sample(None, 1, mode="glad")


@pytest.mark.parametrize("name", sorted(SS.CASES))
def test_cases_have_the_margin_in_every_mode_and_the_emotions_differ(name):
    c = SS.CASES[name]
    ref = SS.reference(name)
    assert set(ref) == set(SS.MODES)
    for mode in SS.MODES:                                          # none is skipped
        ids, margin, scale = ref[mode]
        assert tuple(ids.shape) == (c["rows"], c["steps"])
        print("%s %s: margin %.3e, need %.3e (%.2f x)" % (name, mode, margin, SC.need(scale), margin / SC.need(scale)))
        assert margin > SC.need(scale), (mode, margin, SC.need(scale))
    emo = [m for m in SS.MODES if m != "factual"]
    for i, a in enumerate(emo):
        for b in emo[i + 1:]:
            assert bool((ref[a][0] != ref[b][0]).any(1).all()), (a, b)
