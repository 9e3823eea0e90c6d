"""The one-call beam search of the attention decoders (capnet_att_decode_step, capnet_att_beam_decode), the part that
needs no GPU: the entries are declared and exported, the workspace and the shape predicate keep their limits, bad
arguments are refused before any launch, the keyword reaches the classes' _beam, and every case of the GPU test has the
margin its comparison needs."""
import ctypes as C
import inspect
import os

import pytest

import capnet
from att_beam_cases import IMAGES, KS, MARGIN, new_families
from capnet import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capnet_att_decode_step", "capnet_att_decode_supported", "capnet_att_beam_decode_ws_bytes", "capnet_att_beam_decode")


@pytest.mark.parametrize("family", new_families(), ids=lambda f: f.name)
def test_every_case_has_the_margin(family):
    """Every (k, image) the GPU test compares is well-posed in fp64: none is skipped there."""
    for k in KS:
        for i in range(IMAGES):
            assert family.margin(k, i) > MARGIN, (k, i)


def test_new_entries_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "capnet.h")) as f:
        src = f.read()
    lib = capnet.lib()
    for name in NEW + ("capnet_att_decode_step_ws_bytes",):
        assert name + "(" in src, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def _a16(n):
    return (n + 15) // 16 * 16


def test_workspace_limits_and_parts():
    lib = capnet.lib()
    #        L  n  k  P   A    C   E   H   V   T
    good = (2, 3, 5, 9, 32, 512, 24, 64, 97, 13)
    size = lib.capnet_att_beam_decode_ws_bytes(*good)
    assert size > 0 and size % 16 == 0
    step = lib.capnet_att_decode_step_ws_bytes(3, 5, 9, 32, 512, 24)
    assert step == 15 * (32 + 512 + 24 + 512 + 12) * 4             # z | xa | the raw scores, P rounded up to 4
    assert size == lib.capnet_beam_decode_ws_bytes(2, 3, 5, 64, 97, 13) + _a16(step)
    for field, bad in ((2, 0), (2, 17), (0, 9), (0, 0), (1, 0), (3, 0), (3, 4097), (5, 768), (6, 10)):
        args = list(good)
        args[field] = bad
        assert lib.capnet_att_beam_decode_ws_bytes(*args) == 0, (field, bad)


def test_supported_shapes():
    ok = capnet.lib().capnet_att_decode_supported
    assert ok(300, 2048, 512, 512, 196, 5, 2) and ok(12, 512, 64, 16, 1, 1, 1) and ok(12, 2048, 64, 260, 4096, 16, 8)
    assert ok(1536, 2048, 512, 512, 196, 5, 2)                      # 3584 + 512 = 4096 exactly
    for bad in ((10, 2048, 512, 512, 196, 5, 2), (300, 768, 512, 512, 196, 5, 2), (300, 2048, 512, 512, 196, 17, 2),
                (300, 2048, 512, 512, 196, 0, 2), (1540, 2048, 512, 512, 196, 5, 2),      # E + C + H > 4096
                (2048, 2048, 512, 512, 196, 5, 2), (300, 2048, 96, 512, 196, 5, 2), (300, 2048, 512, 510, 196, 5, 2),
                (300, 2048, 512, 512, 0, 5, 2), (300, 2048, 512, 512, 4097, 5, 2), (300, 2048, 512, 512, 196, 5, 9),
                (300, 2048, 512, 512, 196, 5, 0)):
        assert not ok(*bad), bad


# fake, suitably aligned addresses: every call below must be refused before anything is launched or dereferenced on the
# device (no GPU is present when this file runs)
P = 0x10000


def _arr(*vals):
    return (C.c_void_p * len(vals))(*vals)


def _base(**kw):
    a = dict(cell=0, nlayers=1, n=2, k=3, P=9, A=32, C=512, E=24, H=64, V=97, att1=P, feat=P, emb=P, wz=P, bz=P, wf=P, bf=P,
             wcat=_arr(P), beff=_arr(P), ws=P, slab=P, slab_floats=1 << 20, err=P)
    a.update(kw)
    return a


def _beam(**kw):
    a = _base(T=13, start=1, end=2, Cw=P, Cb=P, state0=P, poll=0, seqs=P, lengths=P, steps=None)
    a.update(kw)
    lib = capnet.lib()
    rc = lib.capnet_att_beam_decode(a["cell"], a["nlayers"], a["n"], a["k"], a["P"], a["A"], a["C"], a["E"], a["H"], a["V"], a["T"],
                                    a["start"], a["end"], a["att1"], a["feat"], a["emb"], a["wz"], a["bz"], a["wf"], a["bf"],
                                    a["wcat"], a["beff"], a["Cw"], a["Cb"], a["state0"], a["ws"], a["slab"], a["slab_floats"],
                                    a["poll"], a["seqs"], a["lengths"], a["steps"], a["err"], None)
    return rc, lib.capnet_last_error().decode()


def _step(**kw):
    a = _base(tokens=P, sin=P, parent=P, sout=2 * P, top=P)
    a.update(kw)
    lib = capnet.lib()
    rc = lib.capnet_att_decode_step(a["cell"], a["nlayers"], a["n"], a["k"], a["P"], a["A"], a["C"], a["E"], a["H"], a["V"],
                                    a["att1"], a["feat"], a["tokens"], a["emb"], a["wz"], a["bz"], a["wf"], a["bf"], a["wcat"],
                                    a["beff"], a["sin"], a["parent"], a["sout"], a["top"], a["ws"], a["slab"], a["slab_floats"],
                                    a["err"], None)
    return rc, lib.capnet_last_error().decode()


SHARED = [
    (dict(att1=None), "null"), (dict(feat=None), "null"), (dict(emb=None), "null"), (dict(wz=None), "null"),
    (dict(bz=None), "null"), (dict(wf=None), "null"), (dict(bf=None), "null"), (dict(ws=None), "null"), (dict(slab=None), "null"),
    (dict(err=None), "null"), (dict(wcat=None), "null"), (dict(wcat=_arr(None)), "layer 0"), (dict(beff=_arr(None)), "layer 0"),
    (dict(k=98), "k=98"), (dict(k=17), "k=17"), (dict(k=0), "k=0"), (dict(k=5, V=4), "k=5"),
    (dict(E=10), "unsupported"), (dict(C=768), "unsupported"), (dict(H=96), "unsupported"), (dict(A=30), "unsupported"),
    (dict(P=0), "unsupported"), (dict(P=4097), "unsupported"), (dict(E=1540, C=2048, H=512), "unsupported"),
    (dict(nlayers=9, wcat=_arr(*[P] * 9), beff=_arr(*[P] * 9)), "layers"), (dict(cell=2), "cell"), (dict(n=0), "n 0"),
    (dict(slab_floats=2 * 3 * 544 - 1), "slab"), (dict(V=1000, slab_floats=2 * 3 * 1000 - 1), "slab"),
    (dict(slab=P + 4), "aligned"), (dict(ws=P + 8), "aligned"), (dict(att1=P + 4), "aligned"), (dict(feat=P + 8), "aligned"),
    (dict(emb=P + 4), "aligned"), (dict(wz=P + 4), "aligned"), (dict(wf=P + 4), "aligned"), (dict(wcat=_arr(P + 4)), "aligned"),
]


@pytest.mark.parametrize("bad, word", SHARED + [
    (dict(Cw=None), "null"), (dict(state0=None), "state0"), (dict(seqs=None), "null"), (dict(lengths=None), "null"),
    (dict(Cw=P + 4), "aligned"), (dict(state0=P + 4), "aligned"), (dict(seqs=P + 4), "alignment"),
    (dict(start=-1), "start_token"), (dict(start=1 << 31), "start_token"), (dict(T=0), "max_steps"), (dict(poll=-1), "poll_every"),
])
def test_att_beam_decode_refuses_bad_arguments(bad, word):
    rc, msg = _beam(**bad)
    assert rc != 0 and msg.startswith("att_beam_decode") and word in msg, msg


@pytest.mark.parametrize("bad, word", SHARED + [
    (dict(tokens=None), "null"), (dict(sin=None), "null"), (dict(sout=None), "null"), (dict(top=None), "null"),
    (dict(sout=P), "differ"), (dict(sin=P + 4), "alignment"), (dict(sout=2 * P + 8), "alignment"),
])
def test_att_decode_step_refuses_bad_arguments(bad, word):
    rc, msg = _step(**bad)
    assert rc != 0 and msg.startswith("att_decode_step") and word in msg, msg


def test_the_keyword_reaches_every_attention_class():
    from capnet import decode, ops
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model_att import DecoderRNNAtt
    from capnet.nic_stacked import StackedDecoderRNNAtt
    from capnet.stacked_att import StackedFactoredLSTMAtt
    for cls in (DecoderFactoredLSTMAtt, DecoderRNNAtt, StackedDecoderRNNAtt, StackedFactoredLSTMAtt):
        params = list(inspect.signature(cls._beam).parameters.values())
        assert params[-1].name == "one_call" and params[-1].default is False, cls
    assert hasattr(decode, "AttStack") and hasattr(decode, "PlainStack")
    assert callable(ops.att_decode_step) and callable(ops.att_beam_decode)
