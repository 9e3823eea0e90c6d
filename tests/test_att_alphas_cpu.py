"""Attention maps from the one-call beam search (return_alphas), the part that needs no GPU: the new entries are declared
and exported, refuse every bad argument before a launch and size their workspace as documented; the sizes the existing
tests pin are unchanged; the cases of tests/att_alpha_cases.py are meaningful -- admitted by margin, travelling, with an
image that completes nothing, with P = 260 -- and two wrong readings of the per-slot map history (decoys) are far from the
right maps; the stored-logits searches contain every situation; the keyword is on all four classes.

Decoys (test_two_wrong_readings_are_far_from_the_right_maps). Siblings of one parent have identical maps and every row
has the same map at steps 1 and 2, so a decoy can differ only where the winner changes slot after step 2, and by no more
than maps of different parents differ. Measured here in fp64, best admitted case of a family, smaller of the two decoys'
largest row error (of max|alpha_ref| of the row), against 10 x BOUND = 3.9e-3:
    DecoderFactoredLSTMAtt-P260@34  3.6e-2    StackedFactoredLSTMAtt-2@22  1.6e-2    DecoderRNNAtt@10  7.6e-3
    StackedDecoderRNNAtt-2@3        3.4e-3    StackedFactoredLSTMAtt-2-wide@55  2.9e-3
    DecoderFactoredLSTMAtt@57       0 / 2.2e-2 (4 - 5 token winners: the final-slot reading cannot differ)
    DecoderRNNAtt-wide@8, @2        0 (no end token of its 37 makes a winner leave slot 0)
Every end token of every family was scanned; none lifts the last four above 10 x BOUND with at most one case left out
for margin. The 10 x BOUND assertion is therefore made on the first three (three of the four classes, the P = 260 family
among them), and 1 x BOUND -- the level at which the GPU comparison tells a wrong trace from the right one -- on the two
families whose winners change slot after step 2 but whose maps lie closer together."""
import ctypes as C
import inspect
import os

import pytest
import torch

import capnet
from att_alpha_cases import (BOUND, CLASSES, IMAGES, KS, MARGIN, MAX_LEN, P260, SITUATIONS, START, TABLE_KV, TABLE_N, TABLE_T,
                             admitted, alpha_families, class_of, drive_model, margin, row_error, search)
from att_alpha_ref import replay
from capnet import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capnet_beam_trace_bytes", "capnet_beam_advance_traced", "capnet_beam_finish_traced", "capnet_att_decode_step_alphas",
       "capnet_att_beam_decode_alphas_ws_bytes", "capnet_att_beam_decode_alphas")
FAR = ("DecoderFactoredLSTMAtt-P260@34", "StackedFactoredLSTMAtt-2@22", "DecoderRNNAtt@10")
NEAR = ("StackedDecoderRNNAtt-2@3", "StackedFactoredLSTMAtt-2-wide@55")


# ---- 1. entries ------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "capnet.h")) as f:
        src = f.read()
    lib = capnet.lib()
    for name in NEW:
        assert name + "(" in src, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


# ---- 2. bad arguments: fake, suitably aligned addresses; every call must be refused before anything is launched -------
P = 0x10000


def _arr(*vals):
    return (C.c_void_p * len(vals))(*vals)


def _base(**kw):
    a = dict(cell=0, nlayers=1, groups=1, n=2, k=3, P=9, A=32, C=512, E=24, H=64, V=97, att1=P, feat=P, emb=P, wz=P, bz=P, wf=P,
             bf=P, wcat=_arr(P), beff=_arr(P), ws=P, slab=P, slab_floats=1 << 20, err=P, alphas=P)
    a.update(kw)
    return a


def _beam(**kw):
    a = _base(T=13, start=1, end=2, Cw=P, Cb=P, state0=P, poll=0, seqs=P, lengths=P, steps=None)
    a.update(kw)
    lib = capnet.lib()
    rc = lib.capnet_att_beam_decode_alphas(a["cell"], a["nlayers"], a["groups"], a["n"], a["k"], a["P"], a["A"], a["C"], a["E"],
                                           a["H"], a["V"], a["T"], a["start"], a["end"], a["att1"], a["feat"], a["emb"], a["wz"],
                                           a["bz"], a["wf"], a["bf"], a["wcat"], a["beff"], a["Cw"], a["Cb"], a["state0"], a["ws"],
                                           a["slab"], a["slab_floats"], a["poll"], a["seqs"], a["lengths"], a["steps"], a["err"],
                                           None, a["alphas"])
    return rc, lib.capnet_last_error().decode()


def _step(**kw):
    a = _base(tokens=P, sin=P, parent=P, sout=2 * P, top=P)
    a.update(kw)
    lib = capnet.lib()
    rc = lib.capnet_att_decode_step_alphas(a["cell"], a["nlayers"], a["groups"], a["n"], a["k"], a["P"], a["A"], a["C"], a["E"],
                                           a["H"], a["V"], a["att1"], a["feat"], a["tokens"], a["emb"], a["wz"], a["bz"], a["wf"],
                                           a["bf"], a["wcat"], a["beff"], a["sin"], a["parent"], a["sout"], a["top"], a["ws"],
                                           a["slab"], a["slab_floats"], a["err"], None, a["alphas"])
    return rc, lib.capnet_last_error().decode()


SHARED = [
    (dict(att1=None), "null"), (dict(feat=None), "null"), (dict(emb=None), "null"), (dict(wz=None), "null"),
    (dict(bz=None), "null"), (dict(wf=None), "null"), (dict(bf=None), "null"), (dict(ws=None), "null"), (dict(slab=None), "null"),
    (dict(err=None), "null"), (dict(wcat=None), "null"), (dict(wcat=_arr(None)), "layer 0"), (dict(beff=_arr(None)), "layer 0"),
    (dict(alphas=None), "alphas"), (dict(alphas=P + 2), "alignment"),
    (dict(k=98), "k=98"), (dict(k=17), "k=17"), (dict(k=0), "k=0"), (dict(k=5, V=4), "k=5"),
    (dict(E=10), "unsupported"), (dict(C=768), "unsupported"), (dict(H=96), "unsupported"), (dict(A=30), "unsupported"),
    (dict(P=0), "unsupported"), (dict(P=4097), "unsupported"), (dict(E=1540, C=2048, H=512), "unsupported"),
    (dict(nlayers=9, wcat=_arr(*[P] * 9), beff=_arr(*[P] * 9)), "layers"), (dict(cell=2), "cell"), (dict(n=0), "n 0"),
    (dict(groups=0), "groups"), (dict(groups=9), "groups"),
    (dict(slab_floats=2 * 3 * 544 - 1), "slab"), (dict(groups=2, slab_floats=2 * 2 * 3 * 544 - 1), "slab"),
    (dict(slab=P + 4), "aligned"), (dict(ws=P + 8), "aligned"), (dict(att1=P + 4), "aligned"), (dict(feat=P + 8), "aligned"),
    (dict(emb=P + 4), "aligned"), (dict(wz=P + 4), "aligned"), (dict(wf=P + 4), "aligned"), (dict(wcat=_arr(P + 4)), "aligned"),
]


@pytest.mark.parametrize("bad, word", SHARED + [
    (dict(Cw=None), "null"), (dict(state0=None), "state0"), (dict(seqs=None), "null"), (dict(lengths=None), "null"),
    (dict(Cw=P + 4), "aligned"), (dict(state0=P + 4), "aligned"), (dict(seqs=P + 4), "alignment"),
    (dict(start=-1), "start_token"), (dict(start=1 << 31), "start_token"), (dict(T=0), "max_steps"), (dict(poll=-1), "poll_every"),
])
def test_att_beam_decode_alphas_refuses_bad_arguments(bad, word):
    rc, msg = _beam(**bad)
    assert rc != 0 and msg.startswith("att_beam_decode") and word in msg, msg


@pytest.mark.parametrize("bad, word", SHARED + [
    (dict(tokens=None), "null"), (dict(sin=None), "null"), (dict(sout=None), "null"), (dict(top=None), "null"),
    (dict(sout=P), "differ"), (dict(sin=P + 4), "alignment"), (dict(sout=2 * P + 8), "alignment"),
])
def test_att_decode_step_alphas_refuses_bad_arguments(bad, word):
    rc, msg = _step(**bad)
    assert rc != 0 and msg.startswith("att_decode_step") and word in msg, msg


def _traced(which, **kw):
    a = dict(beam=P, trace=P, logits=P, ld=16, V=16, n=2, k=3, T=6, step=1, end=2, words=P, rows=P, seqs=P, lengths=P, out=P)
    a.update(kw)
    lib = capnet.lib()
    if which == "advance":
        rc = lib.capnet_beam_advance_traced(a["beam"], a["trace"], a["logits"], a["ld"], a["V"], a["n"], a["k"], a["T"], a["step"],
                                            a["end"], a["words"], a["rows"], None)
    else:
        rc = lib.capnet_beam_finish_traced(a["beam"], a["trace"], a["n"], a["k"], a["T"], a["end"], a["seqs"], a["lengths"],
                                           a["out"], None)
    return rc, lib.capnet_last_error().decode()


@pytest.mark.parametrize("bad, word", [
    (dict(trace=None), "null trace"), (dict(beam=None), "null"), (dict(logits=None), "null"), (dict(words=None), "null"),
    (dict(rows=None), "null"), (dict(trace=P + 2), "aligned"), (dict(beam=P + 1), "aligned"), (dict(k=17), "k=17"),
    (dict(k=0), "k=0"), (dict(n=0), "n=0"), (dict(T=0), "max_steps=0"), (dict(step=0), "step=0"), (dict(step=7), "step=7"),
    (dict(V=2), "V=2"), (dict(ld=15), "ld=15"),
])
def test_beam_advance_traced_refuses_bad_arguments(bad, word):
    rc, msg = _traced("advance", **bad)
    assert rc != 0 and msg.startswith("beam_advance") and word in msg, msg


@pytest.mark.parametrize("bad, word", [
    (dict(trace=None), "null trace"), (dict(out=None), "rows"), (dict(beam=None), "null"), (dict(seqs=None), "null"),
    (dict(lengths=None), "null"), (dict(trace=P + 2), "aligned"), (dict(out=P + 2), "aligned"), (dict(k=17), "k=17"),
    (dict(n=0), "n=0"), (dict(T=0), "max_steps=0"),
])
def test_beam_finish_traced_refuses_bad_arguments(bad, word):
    rc, msg = _traced("finish", **bad)
    assert rc != 0 and msg.startswith("beam_finish") and word in msg, msg


# ---- 3. workspace sizes ----------------------------------------------------------------------------------------------
def _a16(n):
    return (n + 15) // 16 * 16


def test_workspace_is_the_search_plus_the_trace_the_rows_and_the_history():
    lib = capnet.lib()
    #        L  G  n  k  P   A    C   E   H   V   T
    good = (2, 2, 3, 5, 9, 32, 512, 24, 64, 97, 13)
    L, G, n, k, Pp, A, Cc, E, H, V, T = good
    size = lib.capnet_att_beam_decode_alphas_ws_bytes(*good)
    trace = lib.capnet_beam_trace_bytes(G * n, k, T)
    assert trace == 3 * G * n * k * (T + 2) * 4                      # rows[2][n][k][L] | done_rows[n][k][L], int32
    assert size == lib.capnet_att_beam_decode_ws_bytes(L, G * n, k, Pp, A, Cc, E, H, V, T) + _a16(trace) + _a16(G * n * T * 4) + \
        _a16(T * G * n * k * Pp * 4)
    one = (2, 1, 3, 5, 9, 32, 512, 24, 64, 97, 13)
    assert lib.capnet_att_beam_decode_alphas_ws_bytes(*one) > lib.capnet_att_beam_decode_ws_bytes(2, 3, 5, 9, 32, 512, 24, 64, 97, 13)
    for field, bad in ((3, 0), (3, 17), (0, 9), (0, 0), (2, 0), (4, 0), (4, 4097), (6, 768), (7, 10), (1, 0), (1, 9)):
        args = list(good)
        args[field] = bad
        assert lib.capnet_att_beam_decode_alphas_ws_bytes(*args) == 0, (field, bad)
    for bad in ((0, 5, 13), (3, 0, 13), (3, 17, 13), (3, 5, 0)):
        assert lib.capnet_beam_trace_bytes(*bad) == 0, bad


def test_the_pinned_sizes_are_unchanged():
    """The beam state and the search's workspace at the shapes tests/test_att_beam_decode_cpu.py and
    tests/test_device_beam_cpu.py use: the trace lies beside the state, not in it."""
    lib = capnet.lib()
    assert lib.capnet_beam_state_bytes(4, 5, 21) == 4 * (4 + 2 * 4 + 3 * 20 + 3 * 20 * 23)
    assert lib.capnet_beam_state_bytes(3, 5, 13) == 4 * (4 + 2 * 3 + 3 * 15 + 3 * 15 * 15)
    step = lib.capnet_att_decode_step_ws_bytes(3, 5, 9, 32, 512, 24)
    assert step == 15 * (32 + 512 + 24 + 512 + 12) * 4
    assert lib.capnet_att_beam_decode_ws_bytes(2, 3, 5, 9, 32, 512, 24, 64, 97, 13) == \
        lib.capnet_beam_decode_ws_bytes(2, 3, 5, 64, 97, 13) + _a16(step)
    # capnet_beam_decode's parts: two states, h_top, the logits, two word buffers, the parents, the beam state
    nk = 15
    assert lib.capnet_beam_decode_ws_bytes(2, 3, 5, 64, 97, 13) == 2 * _a16(nk * 4 * 64 * 4) + _a16(nk * 64 * 4) + _a16(nk * 97 * 4) + \
        3 * _a16(nk * 8) + _a16(lib.capnet_beam_state_bytes(3, 5, 13))


# ---- 4. the cases are meaningful -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", alpha_families(), ids=lambda f: f.name)
def test_cases_have_the_margin_and_the_model_agrees_with_the_reference(family):
    """At most one (k, image) of a family is left out for margin; on the rest the fixed-slot model with paths returns the
    fp64 beam search's tokens, and the maps read along its path are the fp64 replay's."""
    ok = admitted(family)
    assert len(ok) >= len(KS) * IMAGES - 1, [(k, i, margin(family, k, i)) for k in KS for i in range(IMAGES)]
    for k, i in ok:
        s = search(family, k, i)
        assert s.tokens == family.reference(k, i), (k, i)
        assert len(s.path) == len(s.tokens) - 1 and s.maps.shape[0] == len(s.tokens) - 1
        want = replay(family, i, s.tokens)
        assert want.shape == s.maps.shape
        assert row_error(s.maps, want) < 1e-9, (k, i)
        if len(s.tokens) > 1:
            assert torch.allclose(want.sum(1), torch.ones(len(s.tokens) - 1, dtype=torch.float64), atol=1e-12)


def test_every_class_travels_some_image_completes_nothing_and_p260_is_there():
    travels, nothing = {c: 0 for c in CLASSES}, 0
    for family in alpha_families():
        for k, i in admitted(family):
            s = search(family, k, i)
            travels[class_of(family)] = max(travels[class_of(family)], s.leaves_slot_0)
            nothing += s.tokens == [family.end]
    assert all(v >= 2 for v in travels.values()), travels
    assert nothing >= 1
    p260 = [f for f in alpha_families() if f.name.startswith(P260)]
    assert len(p260) == 1 and p260[0].features().shape[1:] == (260, 512) and p260[0].make().attention_size == 16


# ---- 5. decoys -------------------------------------------------------------------------------------------------------
def _separation(family):
    """Best admitted case: the smaller of the two decoys' largest row errors against the right maps."""
    best = 0.0
    for k, i in admitted(family):
        s = search(family, k, i)
        best = max(best, min(row_error(s.final_slot, s.maps), row_error(s.late, s.maps)))
    return best


@pytest.mark.parametrize("family", alpha_families(), ids=lambda f: f.name)
def test_two_wrong_readings_are_far_from_the_right_maps(family):
    """Reading the per-slot history along the winner's final slot, or along the right path one step late, differs from the
    right maps, compared as whole sequences (the module docstring has the figures and the reasoning)."""
    sep = _separation(family)
    print("%s: decoys differ by %.2e of max|alpha| (10 x BOUND = %.2e)" % (family.name, sep, 10 * BOUND))
    if family.name in FAR:
        assert sep > 10 * BOUND, sep
    elif family.name in NEAR:
        assert sep > BOUND, sep


def test_the_far_families_cover_three_classes_and_p260():
    fams = {f.name: f for f in alpha_families()}
    assert {class_of(fams[n]) for n in FAR} == {"DecoderFactoredLSTMAtt", "StackedFactoredLSTMAtt", "DecoderRNNAtt"}
    assert {class_of(fams[n]) for n in NEAR} == {"StackedDecoderRNNAtt", "StackedFactoredLSTMAtt"}
    assert any(n.startswith(P260) for n in FAR)


# ---- 6. stored logits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, V", TABLE_KV)
def test_stored_logits_hold_every_situation_and_a_dead_image(k, V):
    beam, gap = drive_model(k, V)
    assert beam.events(TABLE_T) == SITUATIONS
    assert gap > MARGIN, gap                               # no f32 top-k orders two candidates differently
    assert beam.live[3] == 0 and beam.live[1] == k and beam.live_total > 0      # a dead image beside live ones
    assert not beam.done[1] and beam.winner_rows(TABLE_T)[1] == [-1] * TABLE_T
    path = beam.winner_path(0)
    assert beam.best(0) != 0 and sum(1 for s in path if s != 0) >= 2, path     # a late winner from a travelled slot
    rows = beam.winner_rows(TABLE_T)
    for i in range(TABLE_N):
        m = len(beam.finish()[i]) - 1
        assert all(i * k <= r < (i + 1) * k for r in rows[i][:m]) and rows[i][m:] == [-1] * (TABLE_T - m)


# ---- 7. the keyword --------------------------------------------------------------------------------------------------
def test_the_keyword_is_on_every_attention_class():
    from capnet import decode, ops
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model_att import DecoderRNNAtt
    from capnet.nic_stacked import StackedDecoderRNNAtt
    from capnet.stacked_att import StackedFactoredLSTMAtt
    for cls in (DecoderFactoredLSTMAtt, DecoderRNNAtt, StackedDecoderRNNAtt, StackedFactoredLSTMAtt):
        for name in ("sample", "sample_batch"):
            p = inspect.signature(getattr(cls, name)).parameters
            assert "return_alphas" in p and p["return_alphas"].default is False, (cls, name)
        # sample_styles' parameter list is pinned by tests/test_style_decode_cpu.py: its maps come from a method beside it
        if hasattr(cls, "sample_styles"):
            assert list(inspect.signature(cls.sample_styles_alphas).parameters) == list(inspect.signature(cls.sample_styles).parameters)
        params = list(inspect.signature(cls._beam).parameters.values())
        assert params[-1].name == "one_call" and params[-1].default is False, cls
    for fn in (decode.beam_decode, decode.att_styles, ops.att_beam_decode):
        assert inspect.signature(fn).parameters["return_alphas"].default is False, fn
    assert callable(decode.replay_alphas) and decode.ALPHA_TRACE_MAX_BYTES == 256 << 20
    assert inspect.signature(ops.att_decode_step).parameters["alphas"].default is None
