"""What tests/test_seq2seq_beam_styles_gpu.py relies on, checked without a GPU: every case of
tests/seq2seq_beam_style_cases.py clears seq2seq_beam_cases' margin rule in every listed mode; the four new C entries are
declared, exported and bound; the size functions agree with the one-group ones and refuse what they must; bad arguments
are refused before any device work; sample_beam_styles refuses a wrong list of modes."""
import ctypes as C
import os
import re

import pytest
import torch

import capnet
import seq2seq_beam_style_cases as SBC
from capnet import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capnet_vocab_topk_groups_ws_bytes", "capnet_vocab_topk_groups", "capnet_lstm_beam_decode_groups_ws_bytes",
       "capnet_lstm_beam_decode_groups")


@pytest.mark.parametrize("case", SBC.CASES + SBC.COMPOSED, ids=repr)
def test_every_case_clears_the_rule_in_every_mode(case):
    assert len(case.modes) >= 2 and len(set(case.modes)) == len(case.modes)
    for mode in case.modes:
        m, bound, gap, gbound = case.cases[mode].check()
        assert m > bound and gap > gbound, (case, mode, m, bound, gap, gbound)
        assert case.cases[mode].clears()
    # one seed: every mode on the same parameters and features
    first = case.cases[case.modes[0]]
    for mode in case.modes[1:]:
        other = case.cases[mode]
        assert torch.equal(first.features, other.features)
        assert all(torch.equal(first.params[k], other.params[k]) for k in first.params)


def test_the_cases_are_the_ones_listed():
    got = {c.name: ((c.E, c.H, c.V, c.L, c.rows), c.seed, c.modes, c.ks) for c in SBC.CASES}
    E3 = ("happy", "sad", "angry")
    assert got == {
        "small-all": ((12, 64, 37, 2, 3), 50, ("factual",) + E3, (3, 5)),
        "small-all-b": ((12, 64, 37, 2, 3), 104, ("factual",) + E3, (3, 5)),
        "e10-l1": ((10, 64, 37, 1, 3), 23, E3, (3, 5)),
        "l3": ((12, 64, 37, 3, 3), 45, E3, (3, 5)),
        "rows4": ((12, 64, 37, 2, 4), 313, E3, (3, 5)),
        "rows7": ((12, 64, 37, 2, 7), 49, ("sad", "angry"), (5,)),
        "k12": ((12, 64, 37, 2, 3), 3, ("happy", "sad"), (12,)),
        "mid": ((30, 128, 211, 1, 3), 220, ("sad", "angry"), (3, 5)),
        "full": ((300, 512, 8192, 2, 2), 180, E3, (5,)),
    }
    (composed,) = SBC.COMPOSED
    assert (composed.E, composed.H, composed.V, composed.L, composed.rows) == (12, 16, 37, 1, 3)
    assert "factual" in composed.modes and len(composed.emotions) == 1
    assert not capnet.ops.stacked_decode_supported(composed.E, composed.H)


def test_the_emotions_of_a_case_differ():
    """A kernel that used one group's weights for every group cannot pass: the emotions' lists differ."""
    for case in SBC.CASES[:2]:
        k = case.ks[-1]
        lists = [case.reference(k, m) for m in case.emotions]
        assert all(a != b for i, a in enumerate(lists) for b in lists[i + 1:]), case


# ---- the C entries -------------------------------------------------------------------------------------------------
def test_the_new_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "capnet.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    kernels = open(os.path.join(ROOT, "image-caption-emotion-indonesia_amd", "csrc", "kernels.h")).read()
    capi = open(os.path.join(ROOT, "image-caption-emotion-indonesia_amd", "csrc", "capi.cpp")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name[len("capnet_"):], kernels), name
        assert re.search(r"\b%s\(" % name, capi), name


def test_the_size_functions():
    L = _lib.lib()
    for rows, k, V in ((1, 1, 1), (15, 5, 8192), (16, 16, 37), (33, 3, 211)):
        assert L.capnet_vocab_topk_groups_ws_bytes(1, rows, k, V) == L.capnet_vocab_topk_ws_bytes(rows, k, V) > 0
    assert L.capnet_vocab_topk_ws_bytes(15, 5, 8192) == 16 + 256 * 15 * 8 * 6
    assert L.capnet_vocab_topk_groups_ws_bytes(3, 15, 5, 8192) == 3 * (16 + 256 * 15 * 8 * 6)
    sizes = [L.capnet_vocab_topk_groups_ws_bytes(g, 15, 5, 211) for g in range(0, 10)]
    assert sizes[0] == 0 and sizes[9] == 0 and all(a < b for a, b in zip(sizes[1:8], sizes[2:9])) and sizes[1] > 0
    for rows, k, V in ((0, 5, 37), (3, 0, 37), (3, 17, 37), (3, 5, 4)):                # vocab_topk's limits
        assert L.capnet_vocab_topk_groups_ws_bytes(2, rows, k, V) == 0, (rows, k, V)
    for fused in (0, 1):
        for nl, n, k, H, V, T in ((2, 3, 5, 64, 37, 13), (1, 1, 1, 512, 8192, 21), (3, 12, 5, 512, 8192, 21)):
            assert (L.capnet_lstm_beam_decode_groups_ws_bytes(nl, 1, n, k, H, V, T, fused)
                    == L.capnet_lstm_beam_decode_ws_bytes(nl, n, k, H, V, T, fused) > 0)
        sizes = [L.capnet_lstm_beam_decode_groups_ws_bytes(2, g, 3, 5, 64, 37, 13, fused) for g in range(0, 10)]
        assert sizes[0] == 0 and sizes[9] == 0 and all(a < b for a, b in zip(sizes[1:8], sizes[2:9])) and sizes[1] > 0
        for bad in ((0, 3, 5, 64, 37, 13), (9, 3, 5, 64, 37, 13), (2, 0, 5, 64, 37, 13), (2, 3, 0, 64, 37, 13),
                    (2, 3, 17, 64, 37, 13), (2, 3, 5, 64, 4, 13), (2, 3, 5, 64, 37, 0)):
            assert L.capnet_lstm_beam_decode_groups_ws_bytes(bad[0], 3, *bad[1:], fused) == 0, bad
    assert L.capnet_lstm_beam_decode_groups_ws_bytes(2, 3, 3, 5, 100, 37, 13, 1) == 0     # the fused top-k's hidden sizes
    assert L.capnet_lstm_beam_decode_groups_ws_bytes(2, 3, 3, 5, 100, 37, 13, 0) > 0


_BUF = (C.c_char * 4096)()
_P = C.cast(C.addressof(_BUF) + (-C.addressof(_BUF)) % 16, C.c_void_p)      # 16-B aligned host memory: never dereferenced
_OFF = C.c_void_p(_P.value + 4)


def _arr(*ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _refused(rc, word):
    """Refused, with a message that names the argument."""
    assert rc != 0
    msg = _lib.lib().capnet_last_error().decode()
    assert word in msg, (msg, word)


def test_vocab_topk_groups_refuses_bad_arguments():
    L = _lib.lib()
    three = _arr(_P, _P, _P)

    def call(groups=3, rpg=3, H=64, V=37, k=5, h=_P, w=three, b=None, ws=_P, values=_P, index=_P, lse=_P):
        return L.capnet_vocab_topk_groups(h, w, b, groups, rpg, H, V, k, ws, values, index, lse, None)
    for kw in (dict(groups=0), dict(groups=9), dict(k=0), dict(k=17), dict(k=5, V=4), dict(H=100), dict(H=16), dict(rpg=0),
               dict(h=None), dict(w=None), dict(ws=None), dict(values=None), dict(index=None), dict(lse=None), dict(h=_OFF),
               dict(w=_arr(_P, None, _P)), dict(w=_arr(_P, _P, _OFF))):
        assert call(**kw) != 0, kw


def test_lstm_beam_decode_groups_refuses_bad_arguments():
    L = _lib.lib()
    two, three = _arr(_P, _P), _arr(_P, _P, _P)
    steps = C.c_int(-1)

    def call(cell=1, nl=2, groups=3, n=2, k=3, E=12, H=64, V=37, T=5, start=1, emb=three, wcat=two, beff=two, Cw=three, Cb=None,
             ws=_P, slab=_P, slab_floats=1 << 20, fused=1, poll=0, seqs=_P, lengths=_P, flag=_P):
        return L.capnet_lstm_beam_decode_groups(cell, nl, groups, n, k, E, H, V, T, start, 2, emb, wcat, beff, Cw, Cb, None, ws,
                                                slab, slab_floats, fused, poll, seqs, lengths, C.byref(steps), flag, None)
    # the ones the issue names, with their message
    named = ((dict(groups=0), "groups"), (dict(groups=9), "groups"), (dict(emb=_arr(_P, None, _P)), "group 1"),
             (dict(Cw=_arr(_P, _P, _OFF)), "group 2"), (dict(k=17), "k=17"), (dict(H=100, fused=1), "H=100"))
    for kw, word in named:
        _refused(call(**kw), word)
    for kw in (dict(k=0), dict(k=5, V=4), dict(H=16), dict(cell=2), dict(nl=0), dict(nl=9), dict(n=0), dict(T=0), dict(poll=-1),
               dict(start=-1), dict(emb=None), dict(wcat=None), dict(beff=None), dict(Cw=None), dict(ws=None), dict(seqs=None),
               dict(lengths=None), dict(flag=None), dict(wcat=_arr(_P, None)), dict(beff=_arr(_P, None)),
               dict(fused=0, slab=None), dict(fused=0, slab_floats=10), dict(ws=C.c_void_p(_P.value + 8)),
               dict(emb=_arr(_OFF, _P, _P)), dict(Cw=_arr(None, _P, _P))):
        assert call(**kw) != 0, kw
    assert steps.value == -1                       # nothing ran


# ---- Python: refused without a device ------------------------------------------------------------------------------
def test_sample_beam_styles_refuses_a_wrong_list_of_modes():
    from capnet.seq2seq import FUSED_TOPK_GROUPS_MAX_ROWS, Seq2Seq
    model = Seq2Seq(12, 64, 37, 1, dropout=0.0, max_seq_length=4)
    feats = torch.zeros(2, 12)
    for modes in (("happy", "glad"), ("joyful",), ("Factual", "sad"), (None,)):
        with pytest.raises(capnet.CapnetError, match="mode name wrong"):
            model.sample_beam_styles(feats, 1, 2, modes=modes)
    for modes in (("happy", "happy"), ("factual", "sad", "factual"), ()):
        with pytest.raises(capnet.CapnetError, match="distinct"):
            model.sample_beam_styles(feats, 1, 2, modes=modes)
    assert isinstance(FUSED_TOPK_GROUPS_MAX_ROWS, int) and FUSED_TOPK_GROUPS_MAX_ROWS >= 0
