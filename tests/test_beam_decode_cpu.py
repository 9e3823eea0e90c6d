"""The one-call beam search (capnet_beam_decode, capnet_stacked_decode_step_gather), the part that needs no GPU: the
entries are declared and exported, the workspace size is the sum of its parts, bad arguments are refused before any
launch, the Python keyword exists on every decoder, and the one-layer cases of the GPU test have the margin its
comparison needs."""
import ctypes as C
import inspect
import os

import pytest

import capnet
from beam_decode_cases import families
from capnet import _lib, ops
from device_beam_cases import IMAGES, KS, MARGIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capnet_stacked_decode_step_gather", "capnet_beam_decode_ws_bytes", "capnet_beam_decode")


def test_new_entries_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "capnet.h")) as f:
        src = f.read()
    lib = capnet.lib()
    for name in NEW:
        assert name + "(" in src, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def _a16(n):
    return (n + 15) // 16 * 16


def test_workspace_is_the_sum_of_its_parts():
    lib = capnet.lib()
    L, n, k, H, V, T = 2, 3, 5, 64, 37, 13
    nk = n * k
    beam = lib.capnet_beam_state_bytes(n, k, T)
    assert beam == 4 * (4 + 2 * 3 + 3 * 15 + 3 * 15 * 15) == 2920
    parts = [2 * _a16(nk * 2 * L * H * 4),      # the two state buffers [n k][2L][H]
             _a16(nk * H * 4),                  # h_top
             _a16(nk * V * 4),                  # logits
             2 * _a16(nk * 8),                  # the two word buffers
             _a16(nk * 8),                      # parent_rows
             _a16(beam)]
    assert parts == [30720, 3840, 2224, 256, 128, 2928]
    assert lib.capnet_beam_decode_ws_bytes(L, n, k, H, V, T) == sum(parts) == 40096


def test_workspace_is_zero_outside_the_limits():
    lib = capnet.lib()
    assert lib.capnet_beam_decode_ws_bytes(2, 3, 5, 64, 37, 13) > 0
    assert lib.capnet_beam_decode_ws_bytes(2, 3, 17, 64, 37, 13) == 0
    assert lib.capnet_beam_decode_ws_bytes(2, 3, 0, 64, 37, 13) == 0
    assert lib.capnet_beam_decode_ws_bytes(9, 3, 5, 64, 37, 13) == 0


# fake, suitably aligned addresses: every call below must be refused before anything is launched or dereferenced on the
# device (no GPU is present when this file runs)
P = 0x10000


def _arr(*vals):
    return (C.c_void_p * len(vals))(*vals)


def _beam_decode(**kw):
    a = dict(cell=0, nlayers=1, n=2, k=3, E=12, H=64, V=37, T=13, start=1, end=2, emb=P, wcat=_arr(P), beff=_arr(P), Cw=P,
             Cb=P, state0=None, ws=P, slab=P, slab_floats=1 << 20, poll=0, seqs=P, lengths=P, steps=None, err=P)
    a.update(kw)
    lib = capnet.lib()
    rc = lib.capnet_beam_decode(a["cell"], a["nlayers"], a["n"], a["k"], a["E"], a["H"], a["V"], a["T"], a["start"], a["end"],
                                a["emb"], a["wcat"], a["beff"], a["Cw"], a["Cb"], a["state0"], a["ws"], a["slab"],
                                a["slab_floats"], a["poll"], a["seqs"], a["lengths"], a["steps"], a["err"], None)
    return rc, lib.capnet_last_error().decode()


@pytest.mark.parametrize("bad, word", [
    (dict(emb=None), "null"), (dict(Cw=None), "null"), (dict(ws=None), "null"), (dict(slab=None), "null"),
    (dict(seqs=None), "null"), (dict(lengths=None), "null"), (dict(err=None), "null"), (dict(wcat=None), "null"),
    (dict(wcat=_arr(None)), "layer 0"),
    (dict(k=38), "k=38"), (dict(k=17, V=100), "k=17"), (dict(k=0), "k=0"),
    (dict(H=16), "unsupported"), (dict(H=96), "unsupported"), (dict(E=2048), "unsupported"),
    (dict(nlayers=9, wcat=_arr(*[P] * 9), beff=_arr(*[P] * 9)), "layers"), (dict(cell=2), "cell"),
    (dict(slab_floats=2 * 3 * 37 - 1), "slab"), (dict(slab=P + 4), "aligned"), (dict(ws=P + 8), "aligned"),
    (dict(Cw=P + 4), "aligned"), (dict(state0=P + 4), "aligned"), (dict(wcat=_arr(P + 4)), "aligned"),
    (dict(seqs=P + 4), "alignment"), (dict(start=-1), "start_token"), (dict(start=1 << 31), "start_token"),
    (dict(T=0), "max_steps"), (dict(n=0), "n 0"), (dict(poll=-1), "poll_every"),
])
def test_beam_decode_refuses_bad_arguments(bad, word):
    rc, msg = _beam_decode(**bad)
    assert rc != 0 and msg.startswith("beam_decode") and word in msg, msg


def _gather(**kw):
    a = dict(cell=0, nlayers=1, rows=5, E=12, H=64, V=37, tokens=P, x=P, wcat=_arr(P), beff=_arr(P), sin=P, parent=P,
             sout=2 * P, top=P, err=P)
    a.update(kw)
    lib = capnet.lib()
    rc = lib.capnet_stacked_decode_step_gather(a["cell"], a["nlayers"], a["rows"], a["E"], a["H"], a["V"], a["tokens"], a["x"],
                                               a["wcat"], a["beff"], a["sin"], a["parent"], a["sout"], a["top"], a["err"], None)
    return rc, lib.capnet_last_error().decode()


@pytest.mark.parametrize("bad, word", [
    (dict(x=None), "null"), (dict(sin=None), "null"), (dict(sout=None), "null"), (dict(top=None), "null"),
    (dict(wcat=None), "null"), (dict(beff=_arr(None)), "layer 0"), (dict(err=None), "err_flag"),
    (dict(err=None, tokens=None), "parent rows need err_flag"),
    (dict(H=16), "unsupported"), (dict(H=96), "unsupported"), (dict(rows=0), "rows"), (dict(nlayers=0), "layers"),
    (dict(cell=3), "cell"), (dict(sout=P), "differ"), (dict(sin=P + 4), "alignment"), (dict(wcat=_arr(P + 8)), "aligned"),
])
def test_gathered_step_refuses_bad_arguments(bad, word):
    rc, msg = _gather(**bad)
    assert rc != 0 and msg.startswith("stacked_decode_step") and word in msg, msg


def test_supported_shapes():
    assert ops.beam_decode_supported(300, 512, 5, 8192, 3) and ops.beam_decode_supported(12, 64, 16, 16, 8)
    for bad in ((12, 16, 5, 37, 1), (12, 64, 17, 37, 1), (12, 64, 5, 4, 1), (12, 64, 0, 37, 1), (12, 64, 5, 37, 9),
                (12, 64, 5, 37, 0), (2048, 64, 5, 37, 1)):
        assert not ops.beam_decode_supported(*bad), bad


def test_the_keyword_is_on_every_decoder():
    from capnet.decode import beam_decode
    from capnet.model import DecoderFactoredLSTM
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model import DecoderRNN
    from capnet.nic_model_att import DecoderRNNAtt
    from capnet.nic_stacked import StackedDecoderRNN, StackedDecoderRNNAtt
    from capnet.stacked import StackedFactoredLSTM
    from capnet.stacked_att import StackedFactoredLSTMAtt
    from capnet.train import evaluate
    fns = [beam_decode, evaluate]
    for cls in (DecoderFactoredLSTM, DecoderRNN, StackedFactoredLSTM, StackedDecoderRNN, DecoderFactoredLSTMAtt, DecoderRNNAtt,
                StackedDecoderRNNAtt, StackedFactoredLSTMAtt):
        fns += [cls.sample, cls.sample_batch]
    for fn in fns:
        assert inspect.signature(fn).parameters["one_call"].default is False, fn
    assert inspect.signature(ops.stacked_decode_step).parameters["parent_rows"].default is None


def test_the_fold_is_shared():
    """DecoderFactoredLSTM's one-layer fold is StackedFactoredLSTM._fold's function, not a copy."""
    from capnet import decode, model, stacked
    assert model.fold_factored is decode.fold_factored is stacked.fold_factored


@pytest.mark.parametrize("family", families(), ids=lambda f: f.name)
def test_one_layer_cases_have_the_margin(family):
    """Every (k, image) the GPU test compares is well-posed in fp64: none is skipped there."""
    for k in KS:
        for i in range(IMAGES):
            assert family.margin(k, i) > MARGIN, (k, i)
