"""capnet.seq2seq under constraints, what needs no GPU: THE RULE of tests/seq2seq_constrained_cases.py for every
(case, set) -- so that tests/test_seq2seq_constrained_gpu.py skips nothing --, that every set binds, the front ends' checks,
the pinned parameter order, and the new C entries' declarations, sizes and refusals."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import seq2seq_constrained_cases as XC
from capnet import _lib, ops
from capnet.beam import Constraints
from capnet.seq2seq import DecoderRNN, EncoderRNN, Seq2Seq
from constrained_beam_ref import violations
from device_beam_cases import MARGIN, MAX_LEN, START
from forced_beam_ref import missing
from seq2seq_cases import need

NEW = ("capnet_beam_exclusion_mask", "capnet_vocab_topk_select", "capnet_vocab_topk_groups_masked",
       "capnet_lstm_beam_decode_constrained_ws_bytes", "capnet_lstm_beam_decode_constrained",
       "capnet_lstm_beam_decode_groups_constrained_ws_bytes", "capnet_lstm_beam_decode_groups_constrained")


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def test_the_sets_and_shapes_the_issue_names_are_all_there():
    pairs = XC.pairs()
    assert {s for _, s in pairs} == set(XC.SET_NAMES)
    for u, s in pairs:
        c = u.sets[s]
        if s == "D":
            assert (c.no_repeat_ngram, c.min_words, len(c.banned), c.forced) == (1, 6, 2, ())
            emitted = {w for k, r in u.cells() for w in u.winner(None, k, r)}
            assert set(c.banned) <= emitted and START not in c.banned and u.end not in c.banned       # ids the plain search emits
        elif s == "B":
            assert (c.no_repeat_ngram, c.min_words, c.banned, c.forced) == (2, 0, (), ())
        else:
            assert len(c.forced) == 1 and (c.no_repeat_ngram, c.min_words, c.banned) == (0, 0, ())
    shapes = {u.shape for u, _ in pairs}
    assert shapes == set(XC.SHAPES) and any(XC.is_composed(u) for u, _ in pairs)
    assert {XC.SHAPES[x][5] for x in shapes} >= {"factual", "happy", "sad"}


@pytest.mark.parametrize("pair", XC.pairs(), ids=XC.pair_id)
def test_every_case_clears_the_rule_and_every_set_binds(pair):
    u, s = pair
    c = u.sets[s]
    c.check(u.case.V, u.end, max(u.case.ks), MAX_LEN + 1)
    margin, gap, bound, enc, enc_bound = u.check(s)
    print("%s: margin %.3g, completed gap %.3g > %.3g; encoder gap %.3g > %.3g" % (XC.pair_id(pair), margin, gap, bound, enc, enc_bound))
    assert bound == max(MARGIN, (MAX_LEN + 1) * need(u.scale(s)))
    assert margin > bound and gap > bound
    assert enc > enc_bound                                   # (inf for `factual`: the encoder's greedy pass is not run)
    # the constrained reference differs from the unconstrained one: in what completes and in what is returned
    assert u.changed(s) and u.moved(s), "the set changes nothing"
    # and what it returns has the properties, checked without the rule's own code
    for k, r in u.cells():
        for _, q in u.search(s, k, r).done:
            assert not violations(q, u.end, c) and not missing(q, c.forced), (k, r, q)
        assert u.winner(s, k, r)[-1] == u.end
    done = [len(u.winner(s, k, r)) > 1 for k, r in u.cells()]
    assert sum(done) >= len(done) - 1, "a search may end with nothing completed ([<end>]), but not most of a case's"
    if s in ("D", "F"):              # the plain search does break these sets
        plain = [u.winner(None, k, r) for k, r in u.cells()]
        assert any(violations(q, u.end, c) or missing(q, c.forced) for q in plain)


# ---- the front ends -----------------------------------------------------------------------------------------------------------
def test_parameter_order_is_pinned():
    for cls in (EncoderRNN, DecoderRNN):
        names = list(inspect.signature(cls.sample_beam).parameters)
        assert names[-3:] == ["constraints", "nbest", "length_penalty"], cls
        assert inspect.signature(cls.sample_beam).parameters["constraints"].default is None
    for cls in (EncoderRNN, DecoderRNN, Seq2Seq):
        names = list(inspect.signature(cls.sample_random).parameters)
        assert names[-2:] == ["exclude", "end_token"] and names[-3] == "top_p", cls
    # Seq2Seq.sample_beam / sample_beam_styles keep the signatures tests/test_constrained_beam_cpu.py pins (no `constraints`);
    # the constrained searches are methods of their own, the constraints required and directly behind end_token
    for plain, con in ((Seq2Seq.sample_beam, Seq2Seq.sample_beam_constrained),
                       (Seq2Seq.sample_beam_styles, Seq2Seq.sample_beam_styles_constrained)):
        old, new = list(inspect.signature(plain).parameters), list(inspect.signature(con).parameters)
        assert "constraints" not in old and old[-2:] == ["nbest", "length_penalty"]
        assert new == old[:4] + ["constraints"] + old[4:]
        assert inspect.signature(con).parameters["constraints"].default is inspect.Parameter.empty
        assert "diversity" not in new
    # ops: the new keyword stands behind the existing ones
    for fn in (ops.lstm_beam_decode, ops.lstm_beam_decode_groups):
        assert list(inspect.signature(fn).parameters)[-3:] == ["nbest", "length_penalty", "constraints"]
    for fn in (ops.vocab_topk, ops.vocab_topk_groups):
        assert list(inspect.signature(fn).parameters)[-2:] == ["mask", "select_only"]
        assert inspect.signature(fn).parameters["select_only"].default is False


def _model(V=37):
    return Seq2Seq(12, 64, V, 1, dropout=0.0, max_seq_length=MAX_LEN).eval()


def test_the_checks_raise_before_anything_runs():
    """On CPU tensors: a search or a decode that got past the check would fail for want of a GPU with another message."""
    m = _model()
    feats = torch.zeros(2, 12)
    END = 2
    bad = {"a banned id equal to end_token": Constraints(banned=(END,)), "a banned id outside the vocabulary": Constraints(banned=(37,)),
           "a forced id equal to end_token": Constraints(forced=(END,)), "min_words": Constraints(min_words=MAX_LEN + 1),
           "too many banned for the vocabulary": Constraints(banned=tuple(range(3, 3 + 18)))}        # 37 - 18 - 1 - 14 = 4 < 5
    for what, c in bad.items():
        for mode in ("factual", "happy"):
            with pytest.raises(ops.CapnetError, match="constraints"):
                m.sample_beam_constrained(feats, START, END, c, mode=mode, k=5)
        with pytest.raises(ops.CapnetError, match="constraints"):
            m.sample_beam_styles_constrained(feats, START, END, c, k=5)
        with pytest.raises(ops.CapnetError, match="constraints"):
            m.decoder_sad.sample_beam(START, END, (None, None), k=5, constraints=c)
    small = Seq2Seq(12, 64, 20, 1, dropout=0.0, max_seq_length=MAX_LEN).eval()                       # 20 - 0 - 1 - 14 = 5 < k = 6
    with pytest.raises(ops.CapnetError, match="vocab_size"):
        small.sample_beam_constrained(feats, START, END, Constraints(no_repeat_ngram=1), k=6)
    with pytest.raises(ops.CapnetError, match="capnet.beam.Constraints"):
        m.sample_beam_constrained(feats, START, END, {"no_repeat_ngram": 1})
    # sample_random: forced words, min_words without end_token, a banned <end>, not a Constraints
    for mode in ("factual", "happy"):
        with pytest.raises(ops.CapnetError, match="forced"):
            m.sample_random(feats, START, mode=mode, seed=0, exclude=Constraints(forced=(5,)), end_token=END)
        with pytest.raises(ops.CapnetError, match="end_token"):
            m.sample_random(feats, START, mode=mode, seed=0, exclude=Constraints(min_words=3))
        with pytest.raises(ops.CapnetError, match="exclude"):
            m.sample_random(feats, START, mode=mode, seed=0, exclude=Constraints(banned=(END,)), end_token=END)
        with pytest.raises(ops.CapnetError, match="vocab_size"):
            small.sample_random(feats, START, mode=mode, seed=0, top_k=6, exclude=Constraints(no_repeat_ngram=1), end_token=END)
        with pytest.raises(ops.CapnetError, match="capnet.beam.Constraints"):
            m.sample_random(feats, START, mode=mode, seed=0, exclude=(5,), end_token=END)
    with pytest.raises(ops.CapnetError, match="forced"):
        m.encoder.sample_random(feats, exclude=Constraints(forced=(5,)), end_token=END)
    with pytest.raises(ops.CapnetError, match="end_token"):
        m.decoder_happy.sample_random(START, (None, None), exclude=Constraints(min_words=1))


def test_forced_words_are_refused_on_the_fused_step_by_ops():
    with pytest.raises(ops.CapnetError, match="unfused"):
        ops._lstm_constrained("lstm_beam_decode", "capnet_lstm_beam_decode", Constraints(forced=(4,)), 1, "cpu")
    assert ops._lstm_constrained("x", "capnet_lstm_beam_decode", None, 1, "cpu") == ("capnet_lstm_beam_decode", ())
    name, args = ops._lstm_constrained("x", "capnet_lstm_beam_decode", Constraints(no_repeat_ngram=2, min_words=3), 1, "cpu")
    assert name == "capnet_lstm_beam_decode_constrained" and args[:2] == (2, 3) and args[3] == 0 and args[5] == 0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    lib = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "capnet.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_the_workspace_gains_the_mask_in_the_fused_form_only():
    L = _lib.lib()
    for nl, n, k, H, V, T in ((2, 3, 5, 64, 37, 13), (1, 1, 16, 128, 211, 13), (3, 12, 5, 512, 8192, 22)):
        plain = [L.capnet_lstm_beam_decode_ws_bytes(nl, n, k, H, V, T, f) for f in (0, 1)]
        con = [L.capnet_lstm_beam_decode_constrained_ws_bytes(nl, n, k, H, V, T, f) for f in (0, 1)]
        mask = (n * k * ((V + 31) // 32) * 4 + 15) // 16 * 16
        assert con[0] == plain[0] > 0 and con[1] == plain[1] + mask
        # the state lies where it lay: capnet_beam_nbest reads the same offset after either search
        for groups in (1, 3):
            gp = [L.capnet_lstm_beam_decode_groups_ws_bytes(nl, groups, n, k, H, V, T, f) for f in (0, 1)]
            gc = [L.capnet_lstm_beam_decode_groups_constrained_ws_bytes(nl, groups, n, k, H, V, T, f) for f in (0, 1)]
            gmask = (groups * n * k * ((V + 31) // 32) * 4 + 15) // 16 * 16
            assert gc[0] == gp[0] > 0 and gc[1] == gp[1] + gmask
            assert 0 < L.capnet_beam_decode_ws_beam_offset(nl, n, k, H, V, T, 1, groups) < gp[1]
    for bad in ((0, 3, 5, 64, 37, 13), (2, 0, 5, 64, 37, 13), (2, 3, 17, 64, 37, 13), (2, 3, 5, 64, 4, 13), (2, 3, 5, 64, 37, 0)):
        assert L.capnet_lstm_beam_decode_constrained_ws_bytes(*bad, 1) == 0 == L.capnet_lstm_beam_decode_constrained_ws_bytes(*bad, 0)
        assert L.capnet_lstm_beam_decode_groups_constrained_ws_bytes(bad[0], 2, *bad[1:], 1) == 0
    assert L.capnet_lstm_beam_decode_constrained_ws_bytes(2, 3, 5, 100, 37, 13, 1) == 0       # the fused top-k's hidden sizes
    assert L.capnet_lstm_beam_decode_groups_constrained_ws_bytes(2, 9, 3, 5, 64, 37, 13, 1) == 0


_BUF = (C.c_char * 4096)()
_P = C.cast(C.addressof(_BUF) + (-C.addressof(_BUF)) % 16, C.c_void_p)      # 16-B aligned host memory: never dereferenced
_ODD = C.c_void_p(_P.value + 2)


def _refused(L, rc, *words):
    msg = L.capnet_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg, words)


def test_the_mask_and_select_entries_refuse_bad_arguments():
    L = _lib.lib()

    def mask(beam=_P, n=3, k=5, T=7, step=1, V=37, g=1, mw=3, banned=_P, nb=1, out=_P):
        return L.capnet_beam_exclusion_mask(beam, n, k, T, step, V, 2, g, mw, banned, nb, out, None)
    for kw in (dict(beam=None), dict(beam=_ODD), dict(n=0), dict(k=0), dict(k=17), dict(T=0), dict(step=0), dict(step=8), dict(V=0),
               dict(V=(1 << 24) + 1), dict(g=5), dict(g=-1), dict(mw=-1), dict(nb=33), dict(nb=-1), dict(banned=None), dict(banned=_ODD),
               dict(out=None), dict(out=_ODD), dict(n=1 << 22, k=16)):
        _refused(L, mask(**kw), "beam_exclusion_mask")

    def select(rows=3, H=64, V=37, k=5, h=_P, w=_P, m=_P, ws=_P, values=_P, index=_P, lse=_P):
        return L.capnet_vocab_topk_select(h, w, None, rows, H, V, k, m, ws, values, index, lse, None)
    for kw in (dict(m=None), dict(m=_ODD), dict(k=0), dict(k=17), dict(k=5, V=4), dict(H=100), dict(rows=0), dict(h=None), dict(w=None),
               dict(ws=None), dict(values=None), dict(index=None), dict(lse=None)):
        _refused(L, select(**kw), "vocab_topk")
    two = (C.c_void_p * 2)(_P, _P)
    null2 = (C.c_void_p * 2)(_P, None)

    def grouped(groups=2, rpg=3, H=64, V=37, k=5, h=_P, w=two, m=_P, sel=1, ws=_P, values=_P, index=_P, lse=_P):
        return L.capnet_vocab_topk_groups_masked(h, w, None, groups, rpg, H, V, k, m, sel, ws, values, index, lse, None)
    for kw in (dict(m=None), dict(m=_ODD), dict(sel=2), dict(sel=-1), dict(groups=0), dict(groups=9), dict(rpg=0), dict(k=17), dict(H=100),
               dict(h=None), dict(w=None), dict(w=null2), dict(ws=None), dict(values=None), dict(index=None), dict(lse=None)):
        _refused(L, grouped(**kw), "vocab_topk")


def test_the_constrained_searches_refuse_bad_arguments():
    L = _lib.lib()
    two = (C.c_void_p * 2)(_P, _P)
    steps = C.c_int(-1)

    def single(k=3, H=64, V=37, fused=1, ws=_P, slab=_P, g=1, mw=2, banned=_P, nb=1, forced=None, nf=0, first=None):
        return L.capnet_lstm_beam_decode_constrained(1, 2, 2, k, 12, H, V, 5, 1, 2, first, _P, two, two, _P, None, None, ws, slab, 1 << 20,
                                                     fused, 0, _P, _P, C.byref(steps), _P, None, g, mw, banned, nb, forced, nf)

    def grouped(groups=2, k=3, H=64, V=37, fused=1, ws=_P, slab=_P, g=1, mw=2, banned=_P, nb=1, forced=None, nf=0):
        return L.capnet_lstm_beam_decode_groups_constrained(1, 2, groups, 2, k, 12, H, V, 5, 1, 2, two, two, two, two, None, None, ws, slab,
                                                            1 << 20, fused, 0, _P, _P, C.byref(steps), _P, None, g, mw, banned, nb,
                                                            forced, nf)
    for call, who in ((single, "lstm_beam_decode_constrained"), (grouped, "lstm_beam_decode_groups_constrained")):
        for kw in (dict(k=0), dict(k=17), dict(H=100), dict(ws=None), dict(fused=0, slab=None),           # the unconstrained entry's checks
                   dict(g=5), dict(g=-1), dict(mw=-1), dict(nb=33), dict(nb=-1), dict(banned=None), dict(banned=_ODD),   # beam_constraints_check
                   dict(fused=0, nf=5, forced=_P), dict(fused=0, nf=1, forced=None), dict(fused=0, nf=1, forced=_ODD), dict(nf=-1, forced=_P),
                   dict(fused=1, nf=1, forced=_P)):                                                        # forced: the unfused step only
            _refused(L, call(**kw), who)
    _refused(L, single(fused=1, nf=1, forced=_P), "forced words take the unfused step")
    _refused(L, grouped(groups=9), "groups")
    _refused(L, single(first=C.c_void_p(_P.value + 4)), "first_inputs")
