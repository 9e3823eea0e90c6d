"""Every style in one search, the part that needs no GPU: the four grouped entries are declared and exported, bad
arguments are refused before any launch, the Python surface exists, and every whole-search case of the GPU test has the
margin its comparison needs -- with captions that differ between the modes, so a search that used one mode's weights
for every group could not pass there."""
import ctypes as C
import inspect
import os

import pytest

import capnet
from capnet import _lib, ops
from style_decode_cases import IMAGES, KS, MARGIN, MODES, NAMES, family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capnet_stacked_decode_step_groups", "capnet_beam_decode_groups", "capnet_att_decode_step_groups",
       "capnet_att_beam_decode_groups")


def test_new_entries_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "capnet.h")) as f:
        src = f.read()
    lib = capnet.lib()
    for name in NEW:
        assert name + "(" in src, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.capnet_abi_version() == 1


# fake, suitably aligned addresses: every call below must be refused before anything is launched or dereferenced on the
# device (no GPU is present when this file runs)
P = 0x10000


def _arr(*vals):
    return (C.c_void_p * len(vals))(*vals)


def _step(**kw):
    a = dict(cell=0, nlayers=1, groups=4, rpg=5, E=12, H=64, V=37, tokens=P, x=P, wcat=_arr(P), beff=_arr(P), sin=P, parent=P,
             sout=2 * P, top=P, err=P)
    a.update(kw)
    lib = capnet.lib()
    rc = lib.capnet_stacked_decode_step_groups(a["cell"], a["nlayers"], a["groups"], a["rpg"], a["E"], a["H"], a["V"], a["tokens"],
                                               a["x"], a["wcat"], a["beff"], a["sin"], a["parent"], a["sout"], a["top"], a["err"],
                                               None)
    return rc, lib.capnet_last_error().decode()


@pytest.mark.parametrize("bad, word", [
    (dict(groups=0), "groups 0"), (dict(groups=9), "groups 9"), (dict(groups=-1), "groups"), (dict(rpg=0), "rows per group"),
    (dict(x=None), "null"), (dict(sin=None), "null"), (dict(sout=None), "null"), (dict(top=None), "null"),
    (dict(wcat=None), "null"), (dict(beff=_arr(None)), "layer 0"), (dict(err=None), "err_flag"),
    (dict(err=None, tokens=None), "parent rows need err_flag"),
    (dict(H=16), "unsupported"), (dict(H=96), "unsupported"), (dict(E=2048), "unsupported"), (dict(nlayers=0), "layers"),
    (dict(cell=3), "cell"), (dict(sout=P), "differ"), (dict(sin=P + 4), "alignment"), (dict(wcat=_arr(P + 8)), "aligned"),
])
def test_grouped_step_refuses_bad_arguments(bad, word):
    rc, msg = _step(**bad)
    assert rc != 0 and msg.startswith("stacked_decode_step") and word in msg, msg


def _beam(**kw):
    a = dict(cell=0, nlayers=1, groups=4, n=2, k=3, E=12, H=64, V=37, T=13, start=1, end=2, emb=P, wcat=_arr(P), beff=_arr(P),
             Cw=P, Cb=P, state0=None, ws=P, slab=P, slab_floats=1 << 20, poll=0, seqs=P, lengths=P, steps=None, err=P)
    a.update(kw)
    lib = capnet.lib()
    rc = lib.capnet_beam_decode_groups(a["cell"], a["nlayers"], a["groups"], a["n"], a["k"], a["E"], a["H"], a["V"], a["T"],
                                       a["start"], a["end"], a["emb"], a["wcat"], a["beff"], a["Cw"], a["Cb"], a["state0"],
                                       a["ws"], a["slab"], a["slab_floats"], a["poll"], a["seqs"], a["lengths"], a["steps"],
                                       a["err"], None)
    return rc, lib.capnet_last_error().decode()


@pytest.mark.parametrize("bad, word", [
    (dict(groups=0), "groups 0"), (dict(groups=9), "groups 9"),
    (dict(emb=None), "null"), (dict(Cw=None), "null"), (dict(ws=None), "null"), (dict(slab=None), "null"),
    (dict(seqs=None), "null"), (dict(lengths=None), "null"), (dict(err=None), "null"), (dict(wcat=None), "null"),
    (dict(wcat=_arr(None)), "layer 0"), (dict(k=38), "k=38"), (dict(k=0), "k=0"), (dict(H=16), "unsupported"),
    (dict(nlayers=9, wcat=_arr(*[P] * 9), beff=_arr(*[P] * 9)), "layers"), (dict(cell=2), "cell"),
    # the slab holds all groups' rows: one group's worth is refused
    (dict(slab_floats=4 * 2 * 3 * 37 - 1), "slab"), (dict(slab_floats=2 * 3 * 37), "slab"),
    (dict(slab=P + 4), "aligned"), (dict(ws=P + 8), "aligned"), (dict(Cw=P + 4), "aligned"), (dict(state0=P + 4), "aligned"),
    (dict(wcat=_arr(P + 4)), "aligned"), (dict(seqs=P + 4), "alignment"), (dict(start=-1), "start_token"),
    (dict(T=0), "max_steps"), (dict(n=0), "n 0"), (dict(poll=-1), "poll_every"),
])
def test_grouped_beam_decode_refuses_bad_arguments(bad, word):
    rc, msg = _beam(**bad)
    assert rc != 0 and msg.startswith("beam_decode") and word in msg, msg


ATT = dict(cell=0, nlayers=1, groups=4, n=2, k=3, P=9, A=32, C=512, E=24, H=64, V=97, att1=P, feat=P, tokens=P, emb=P, wz=P, bz=P,
           wf=P, bf=P, wcat=_arr(P), beff=_arr(P), sin=P, parent=None, sout=2 * P, top=P, ws=P, slab=P, slab_floats=1 << 22, err=P)


def _att_step(**kw):
    a = dict(ATT, **kw)
    lib = capnet.lib()
    rc = lib.capnet_att_decode_step_groups(a["cell"], a["nlayers"], a["groups"], a["n"], a["k"], a["P"], a["A"], a["C"], a["E"],
                                           a["H"], a["V"], a["att1"], a["feat"], a["tokens"], a["emb"], a["wz"], a["bz"], a["wf"],
                                           a["bf"], a["wcat"], a["beff"], a["sin"], a["parent"], a["sout"], a["top"], a["ws"],
                                           a["slab"], a["slab_floats"], a["err"], None)
    return rc, lib.capnet_last_error().decode()


def _att_beam(**kw):
    a = dict(ATT, T=13, start=1, end=2, Cw=P, Cb=P, state0=P, poll=0, seqs=P, lengths=P, steps=None)
    a.update(kw)
    lib = capnet.lib()
    rc = lib.capnet_att_beam_decode_groups(a["cell"], a["nlayers"], a["groups"], a["n"], a["k"], a["P"], a["A"], a["C"], a["E"],
                                           a["H"], a["V"], a["T"], a["start"], a["end"], a["att1"], a["feat"], a["emb"], a["wz"],
                                           a["bz"], a["wf"], a["bf"], a["wcat"], a["beff"], a["Cw"], a["Cb"], a["state0"],
                                           a["ws"], a["slab"], a["slab_floats"], a["poll"], a["seqs"], a["lengths"], a["steps"],
                                           a["err"], None)
    return rc, lib.capnet_last_error().decode()


SHARED_BAD = [
    (dict(groups=0), "groups 0"), (dict(groups=9), "groups 9"), (dict(n=0), "n 0"), (dict(k=17), "k=17"), (dict(k=0), "k=0"),
    (dict(att1=None), "null"), (dict(feat=None), "null"), (dict(wz=None), "null"), (dict(bz=None), "null"),
    (dict(wf=None), "null"), (dict(bf=None), "null"), (dict(ws=None), "null"), (dict(slab=None), "null"),
    (dict(err=None), "null"), (dict(wcat=_arr(None)), "layer 0"), (dict(E=10), "unsupported"), (dict(C=500), "unsupported"),
    (dict(H=96), "unsupported"), (dict(A=30), "unsupported"), (dict(cell=2), "cell"), (dict(att1=P + 4), "aligned"),
    (dict(wz=P + 8), "aligned"), (dict(wcat=_arr(P + 4)), "aligned"),
    # the slab holds all groups' rows
    (dict(slab_floats=4 * 2 * 3 * (32 + 512) - 1), "slab"), (dict(slab_floats=2 * 3 * (32 + 512)), "slab"),
]


@pytest.mark.parametrize("bad, word", SHARED_BAD + [
    (dict(tokens=None), "null"), (dict(sin=None), "null"), (dict(top=None), "null"), (dict(sout=P), "differ"),
    (dict(sin=P + 4), "alignment"),
])
def test_grouped_attention_step_refuses_bad_arguments(bad, word):
    rc, msg = _att_step(**bad)
    assert rc != 0 and msg.startswith("att_decode_step") and word in msg, msg


@pytest.mark.parametrize("bad, word", SHARED_BAD + [
    (dict(state0=None), "state0"), (dict(Cw=None), "null"), (dict(seqs=None), "null"), (dict(lengths=None), "null"),
    (dict(state0=P + 4), "aligned"), (dict(seqs=P + 4), "alignment"), (dict(T=0), "max_steps"), (dict(poll=-1), "poll_every"),
    (dict(start=-1), "start_token"),
])
def test_grouped_attention_beam_decode_refuses_bad_arguments(bad, word):
    rc, msg = _att_beam(**bad)
    assert rc != 0 and msg.startswith("att_beam_decode") and word in msg, msg


def test_the_python_surface():
    from capnet.model import DecoderFactoredLSTM
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model import DecoderRNN
    from capnet.stacked import StackedFactoredLSTM
    from capnet.stacked_att import StackedFactoredLSTMAtt
    from capnet.train import evaluate_styles
    for fn in (ops.stacked_decode_step, ops.beam_decode, ops.att_beam_decode, ops.att_decode_step):
        assert inspect.signature(fn).parameters["groups"].default == 1, fn
    for cls in (DecoderFactoredLSTM, StackedFactoredLSTM, DecoderFactoredLSTMAtt, StackedFactoredLSTMAtt):
        par = inspect.signature(cls.sample_styles).parameters
        assert list(par) == ["self", "features", "start_token", "end_token", "k", "modes", "poll_every"], cls
        assert par["k"].default == 5 and tuple(par["modes"].default) == MODES and par["poll_every"].default == 0
    assert not hasattr(DecoderRNN, "sample_styles")             # no modes, no styles
    par = inspect.signature(evaluate_styles).parameters
    assert list(par) == ["encoder", "decoder", "vocab", "data_loader", "modes", "k", "device"]
    assert tuple(par["modes"].default) == MODES and par["k"].default == 5 and par["device"].default is None


def test_modes_are_checked_before_anything_runs(capsys):
    from capnet.model import DecoderFactoredLSTM
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.stacked import StackedFactoredLSTM
    for dec in (DecoderFactoredLSTM(12, 64, 32, 37, 1), StackedFactoredLSTM(12, 64, 32, 37, 2),
                DecoderFactoredLSTMAtt(32, 24, 64, 32, 97, 1, feature_size=512)):
        for bad in ((), ("happy", "happy"), ("factual", "sad", "factual")):
            with pytest.raises(ValueError, match="distinct"):
                dec.sample_styles(None, 1, 2, modes=bad)
        with pytest.raises(ValueError, match="unknown mode"):      # as sample(): the reference's message, then the error
            dec.sample_styles(None, 1, 2, modes=("happy", "glad"))
        assert "mode name wrong!" in capsys.readouterr().err


@pytest.mark.parametrize("name", NAMES)
def test_whole_search_cases_have_the_margin_and_differ_by_mode(name):
    """Every (mode, k, image) the GPU test compares is well-posed in fp64 -- none is skipped there -- every beam search
    completes, and the modes' captions differ: four of four on the plain decoders, at least three on the attention ones."""
    fam = family(name)
    for k in KS:
        for i in range(IMAGES):
            caps = set()
            for m in MODES:
                assert fam.margin(m, k, i) > MARGIN, (m, k, i)
                ref = fam.reference(m, k, i)
                assert ref[-1] == fam.end, (m, k, i)
                caps.add(tuple(ref))
            assert len(caps) >= fam.distinct, (k, i, len(caps))
