"""Sampled decoding with exclusions (sample_random(exclude=)) without a GPU: every case of
tests/excluded_sample_cases.py clears the margin rule and binds, Constraints.check_exclude, the keyword's place in every
signature, the new C symbols and their host-side refusals, and the mask rule against a hand-written table."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import capnet
import excluded_sample_cases as XC
import excluded_sample_ref as XR
import sample_random_ref as R
from capnet import _lib, decode, ops, train
from capnet.beam import Constraints

NEW = ("capnet_sample_exclusion_mask", "capnet_mask_logits", "capnet_vocab_sample_masked", "capnet_vocab_topk_masked",
       "capnet_sample_decode_excl_ws_bytes", "capnet_sample_decode_excl", "capnet_att_sample_decode_excl_ws_bytes",
       "capnet_att_sample_decode_excl")


# ---- the cases -----------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_families_at_both_top_k_with_both_sets():
    import sample_random_cases as SC
    fams = [c["family"] for c in SC.IMAGE_CASES if c["top_k"] == 0]
    plain = [c for c in XC.CASES if c["top_p"] == 1.0 and not c["greedy"]]
    assert sorted((c["family"], c["top_k"]) for c in plain) == sorted((f, k) for f in fams for k in (0, 5))
    assert {(c["set"], c["top_k"]) for c in plain} == {("A", 0), ("A", 5), ("D", 0), ("D", 5)}
    assert sum(c["top_p"] == 0.9 for c in XC.CASES) == 1 and sum(c["greedy"] for c in XC.CASES) == 1
    assert (XC.IMAGES, XC.SAMPLES, XC.MAX_LEN) == (2, 3, 12)
    assert len({c["id"] for c in XC.CASES}) == len(XC.CASES)
    for c in XC.CASES:                 # both sets pass the front end's check at every family's vocabulary
        V = SC.families()[c["family"]].V
        Constraints(no_repeat_ngram=1).check_exclude(V, 2, c["top_k"], XC.MAX_LEN)
        Constraints(no_repeat_ngram=2, min_words=6, banned=(3, 4)).check_exclude(V, 2, c["top_k"], XC.MAX_LEN)


@pytest.mark.parametrize("case", XC.CASES, ids=[c["id"] for c in XC.CASES])
def test_every_case_clears_the_margin_rule_and_binds(case):
    ref = XC.reference(case)
    ids, logp, tr = ref["excl"]
    inv_T = R.inv_temperature(case["T"])
    print("%s: key gap %.3g (need %.3g), k-th gap %.3g (need %.3g), end %d, %r"
          % (case["id"], tr.key_gap, R.need(tr.scale, inv_T), tr.kth_gap, R.need_kth(tr.scale), ref["end"], ref["c"]))
    # margin: the key gap above need; with top_k the k-th / (k + 1)-th gap among the allowed words above need_kth
    assert tr.key_gap > R.need(tr.scale, inv_T)
    if case["top_k"]:
        assert tr.kth_gap > R.need_kth(tr.scale)
    assert XR.clears(tr, case["T"], case["top_k"], case["top_p"]) == []
    assert ids.shape == (XC.IMAGES * XC.SAMPLES, XC.MAX_LEN) and np.isfinite(logp).all()
    # binding: the unexcluded restatement on the same seed violates the set in a cut caption, the excluded one does not
    before, after = XC.binding(ref)
    assert before and not after, (before, after)
    assert not np.array_equal(ids, ref["plain"][0])
    fam = XC.SC.families()[case["family"]]
    ref["c"].check_exclude(fam.V, ref["end"], case["top_k"], XC.MAX_LEN)
    if case["set"] == "D":
        assert ref["c"].min_words == 6 and len(ref["c"].banned) == 2 and ref["end"] not in ref["c"].banned
        first = R.cut(*ref["plain"][:2], XC.IMAGES, XC.SAMPLES, XC.START, ref["end"])[0][0][0]
        assert len(first) <= 5 and first[-1] == ref["end"]          # unexcluded, row 0 ends by its fourth word: within min_words


def test_the_greedy_case_completes_and_moves():
    """The greedy row under the set reaches <end> for both images (there the width-1 beam completes too), differs from the
    unexcluded greedy caption, obeys the set, and its argmax is never closer than need_kth to the runner-up."""
    case = [c for c in XC.CASES if c["greedy"]][0]
    ref = XC.reference(case)
    ref["c"].check_exclude(XC.SC.families()[case["family"]].V, ref["end"], case["top_k"], XC.MAX_LEN)
    for (tokens, gap, scale), (plain, _, _) in XC.greedy_captions(case, ref):
        assert tokens[-1] == ref["end"] and len(tokens) - 1 > ref["c"].min_words and tokens != plain
        assert not XR.violations(tokens, ref["end"], ref["c"]) and gap > R.need_kth(scale)


def test_seeds_are_the_first_that_are_admitted():
    """Every noted seed above 0 has its predecessors rejected (the cheap half: seed - 1 alone is rebuilt)."""
    for case in XC.CASES:
        if case["seed"] > 0:
            before = XC.build(case, case["seed"] - 1)
            before["c"].check_exclude(XC.SC.families()[case["family"]].V, before["end"], case["top_k"], XC.MAX_LEN)   # a valid set,
            assert XC.admitted(case, before), case["id"]                                                                 # yet rejected


# ---- check_exclude -------------------------------------------------------------------------------------------------------
def test_check_exclude_raises_on_each_condition_and_accepts_the_rest():
    E = capnet.CapnetError
    Constraints().check_exclude(37, 2, 0, 12)
    Constraints(no_repeat_ngram=2, min_words=11, banned=(3, 4)).check_exclude(37, 2, 5, 12)
    with pytest.raises(E, match="forced"):
        Constraints(forced=(5,)).check_exclude(37, 2, 0, 12)
    with pytest.raises(E, match="banned"):
        Constraints(banned=(2,)).check_exclude(37, 2, 0, 12)           # end_token
    with pytest.raises(E, match="banned"):
        Constraints(banned=(37,)).check_exclude(37, 2, 0, 12)          # outside the vocabulary
    with pytest.raises(E, match="min_words"):
        Constraints(min_words=12).check_exclude(37, 2, 0, 12)
    # V - len(banned) - 1 - (max_seq_length + 1) < max(top_k, 1)
    Constraints(banned=(3,)).check_exclude(20, 2, 5, 12)               # 20 - 1 - 1 - 13 = 5
    with pytest.raises(E, match="top_k"):
        Constraints(banned=(3, 4)).check_exclude(20, 2, 5, 12)         # 4 < 5
    Constraints().check_exclude(15, 2, 0, 12)                          # 1 word left for top_k = 0
    with pytest.raises(E, match="top_k"):
        Constraints().check_exclude(14, 2, 0, 12)


# ---- signatures ------------------------------------------------------------------------------------------------------------
def test_exclude_is_the_last_parameter_everywhere():
    from capnet.model import DecoderFactoredLSTM
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model import DecoderRNN
    from capnet.nic_model_att import DecoderRNNAtt
    from capnet.nic_stacked import StackedDecoderRNN, StackedDecoderRNNAtt
    from capnet.stacked import StackedFactoredLSTM
    from capnet.stacked_att import StackedFactoredLSTMAtt
    fns = [cls.sample_random for cls in (DecoderFactoredLSTM, DecoderRNN, StackedFactoredLSTM, StackedDecoderRNN,
                                         DecoderFactoredLSTMAtt, DecoderRNNAtt, StackedFactoredLSTMAtt, StackedDecoderRNNAtt)]
    fns += [decode.sample_random, decode.sample_random_device, train.self_critical_step]
    for fn in fns:
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "exclude" and params[-1].default is None, fn
        assert "constraints" not in [p.name for p in params], fn
    assert list(inspect.signature(decode.draw_step).parameters)[-1] == "mask"
    assert inspect.signature(Constraints.check_exclude).parameters.keys() == {"self", "vocab_size", "end_token", "top_k",
                                                                              "max_seq_length"}


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_check_their_arguments():
    lib = capnet.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "capnet.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    assert lib.capnet_abi_version() == 1
    one = C.c_void_p(16)           # never dereferenced: every call below is refused on the host
    bads = (((5, 0, None, 0), b"no_repeat_ngram"), ((-1, 0, None, 0), b"no_repeat_ngram"), ((1, -1, None, 0), b"min_words"),
            ((1, 0, one, 33), b"n_banned"), ((1, 0, one, -1), b"n_banned"), ((1, 0, None, 2), b"banned"),
            ((1, 0, C.c_void_p(18), 2), b"banned"))

    def mask(con=(1, 0, None, 0), ids=one, t=3, steps=12, out=one):
        return lib.capnet_sample_exclusion_mask(ids, 12, steps, one, 2, t, 37, 2, *con, out, None)

    def plain(con):
        return lib.capnet_sample_decode_excl(0, 1, 1, 16, 64, 37, 12, None, one, one, None, None, one, one, None, 1.0, 0, 1.0, 0,
                                             one, None, 0, one, one, None, one, 0, 2, *con, None)

    def att(con):
        return lib.capnet_att_sample_decode_excl(0, 1, 1, 1, 4, 16, 512, 16, 64, 37, 12, one, one, one, one, one, one, one, one,
                                                 None, None, one, one, one, 1.0, 0, 1.0, 0, one, one, 0, one, one, None, one, 0, 2,
                                                 *con, None)
    for bad, word in bads:
        for call in (lambda: mask(con=bad), lambda: plain(bad), lambda: att(bad)):
            assert call() != 0 and word in lib.capnet_last_error(), (bad, lib.capnet_last_error())
    for kw, word in ((dict(out=None), b"mask"), (dict(out=C.c_void_p(18)), b"mask"), (dict(ids=None), b"ids"),
                     (dict(t=13), b"steps"), (dict(t=-1), b"steps"), (dict(steps=0), b"steps")):
        assert mask(**kw) != 0 and word in lib.capnet_last_error(), (kw, lib.capnet_last_error())
    assert lib.capnet_mask_logits(one, 2, 37, 37, None, None) != 0 and b"mask" in lib.capnet_last_error()
    assert lib.capnet_mask_logits(None, 2, 37, 37, one, None) != 0 and b"logits" in lib.capnet_last_error()
    assert lib.capnet_mask_logits(one, 2, 36, 37, one, None) != 0 and b"ld" in lib.capnet_last_error()
    assert lib.capnet_vocab_sample_masked(one, one, None, 2, 64, 37, 1.0, 0, 0, 0, None, one, one, one, 0, None) != 0
    assert b"mask" in lib.capnet_last_error()
    assert lib.capnet_vocab_topk_masked(one, one, None, 2, 64, 37, 5, None, one, one, one, one, None) != 0
    assert b"mask" in lib.capnet_last_error()
    # the workspace of the new entries is the old one, 16-B aligned, and the mask: rows x ceil(V / 32) words
    for rows, V, top_k in ((6, 37, 0), (12, 8192, 5), (5, 7411, 0)):
        W = (V + 31) // 32
        grow = (rows * W * 4 + 15) // 16 * 16
        old = lib.capnet_sample_decode_ws_bytes(1, rows, 64, V, top_k)
        assert lib.capnet_sample_decode_excl_ws_bytes(1, rows, 64, V, top_k, 1.0) == (old + 15) // 16 * 16 + grow
        old = lib.capnet_sample_decode_nucleus_ws_bytes(1, rows, 64, V, top_k)
        assert lib.capnet_sample_decode_excl_ws_bytes(1, rows, 64, V, top_k, 0.9) == (old + 15) // 16 * 16 + grow
    old = lib.capnet_att_sample_decode_ws_bytes(1, 2, 3, 49, 32, 512, 24, 64, 97, 5)
    assert lib.capnet_att_sample_decode_excl_ws_bytes(1, 2, 3, 49, 32, 512, 24, 64, 97, 5, 1.0) == (old + 15) // 16 * 16 + 6 * 4 * 4
    assert lib.capnet_sample_decode_excl_ws_bytes(1, 6, 64, 37, 0, 0.0) == 0 and lib.capnet_sample_decode_excl_ws_bytes(1, 6, 64, 37, 0, 1.5) == 0


# ---- the mask rule on the host ---------------------------------------------------------------------------------------------
def test_the_mask_rule_agrees_with_a_hand_written_table():
    S, E = 1, 2           # <start>, <end>
    table = [
        # (c, tokens = [start, words so far], t, the excluded words)
        (Constraints(no_repeat_ngram=2), [S, 5, 6, 5, 7, 5], 5, {6, 7}),                 # the context `5` seen twice: two words
        (Constraints(no_repeat_ngram=3), [S, 5, 6, 9, 5, 6], 5, {9}),
        (Constraints(no_repeat_ngram=3), [S, 5], 1, set()),                              # a hypothesis shorter than g
        (Constraints(no_repeat_ngram=4), [S, 5, 6], 2, set()),
        (Constraints(no_repeat_ngram=2), [S], 0, set()),                                 # one token, g - 1 = 1 of context: nothing follows it yet
        (Constraints(no_repeat_ngram=1), [S, 5, 6, 5], 3, {S, 5, 6}),                    # g = 1: no word twice, <start> counts
        (Constraints(no_repeat_ngram=1), [S], 0, {S}),
        (Constraints(no_repeat_ngram=2), [S, S, 4], 2, set()),
        (Constraints(no_repeat_ngram=2), [S, 4, S], 2, {4}),                             # <start> is a token of the hypothesis
        (Constraints(min_words=3), [S, 5, 6], 2, {E}),                                   # t + 1 == min_words: banned
        (Constraints(min_words=3), [S, 5, 6, 7], 3, set()),                              # min_words + 1: not banned
        (Constraints(min_words=1), [S], 0, {E}),
        (Constraints(banned=(31, 32, 36)), [S], 0, {31, 32, 36}),
        (Constraints(no_repeat_ngram=2, min_words=6, banned=(8, 9)), [S, 5, E, 5], 3, {8, 9, E}),   # past <end>: the tokens as drawn
    ]
    for c, tokens, t, want in table:
        assert len(tokens) == t + 1
        assert XR.mask_bits(tokens, t, E, c) == want, (c, tokens)
        words = XR.mask_words([tokens], t, 37, E, c)
        assert words.shape == (1, ops.mask_words(37)) == (1, 2) and words.dtype == np.uint32
        assert {v for v in range(64) if (int(words[0, v >> 5]) >> (v & 31)) & 1} == want
    # the masked logits: -inf at the excluded words and nowhere else
    z = XR.masked(np.zeros((2, 37)), [[S, 5, 6, 5], [S, 7, 7, 7]], 3, E, Constraints(no_repeat_ngram=1))
    assert set(np.flatnonzero(np.isinf(z[0]))) == {S, 5, 6} and set(np.flatnonzero(np.isinf(z[1]))) == {S, 7}
    assert [ops.mask_words(V) for V in (1, 32, 33, 37, 97, 7411, 8192)] == [1, 1, 2, 2, 4, 232, 256]
