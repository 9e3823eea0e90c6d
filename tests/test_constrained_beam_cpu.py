"""Constrained beam search, the part that needs no GPU: the rule as code (capnet.beam.banned_words), the validation of
capnet.beam.Constraints and of the front end, the new symbols' host-side argument checks, and the two statements the GPU
tests rest on -- every case of tests/constrained_beam_cases.py is admitted (so nothing is skipped there) and every
constraint set changes what the unconstrained search returns, as the cases file lists."""
import ctypes as C
import inspect
import os

import pytest
import torch

import capnet
import constrained_beam_cases as CC
import constrained_beam_ref as R
import nbest_cases
from capnet import _lib, decode, ops
from capnet.beam import Constraints, banned_words

NEW = ("capnet_beam_advance_constrained", "capnet_beam_advance_constrained_traced", "capnet_beam_topk_banned",
       "capnet_beam_topk_batched_banned", "capnet_beam_decode_constrained", "capnet_att_beam_decode_constrained",
       "capnet_att_beam_decode_alphas_constrained")
END = 2


# ---- the rule ------------------------------------------------------------------------------------------------------------
def test_fewer_tokens_than_g_ban_nothing_by_ngram():
    for g in (2, 3, 4):
        c = Constraints(no_repeat_ngram=g)
        for n in range(1, g):
            assert banned_words([1, 5, 5, 5][:n], n, END, c) == []
    assert banned_words([1, 5, 5], 3, END, Constraints(no_repeat_ngram=3)) == []         # len == g: the context (5 5) was not seen
    assert banned_words([1, 5, 1, 5], 4, END, Constraints(no_repeat_ngram=3)) == [1]     # (1 5) was, followed by 1
    assert banned_words([1, 5], 2, END, Constraints(no_repeat_ngram=2)) == []


def test_a_context_seen_twice_bans_both_followers():
    c = Constraints(no_repeat_ngram=2)
    assert banned_words([1, 5, 6, 5, 7, 5], 6, END, c) == [6, 7]
    c3 = Constraints(no_repeat_ngram=3)
    assert banned_words([1, 5, 6, 8, 5, 6, 9, 5, 6], 9, END, c3) == [8, 9]
    assert banned_words([1, 5, 6, 8, 5, 7], 6, END, c3) == []
    # <start> is part of the hypothesis
    assert banned_words([1, 5, 1], 3, END, c) == [5]


def test_g_1_is_no_word_twice():
    assert banned_words([1, 7, 4, 7], 4, END, Constraints(no_repeat_ngram=1)) == [1, 4, 7]


def test_end_is_banned_exactly_up_to_min_words():
    c = Constraints(min_words=3)
    for step in range(1, 8):
        assert banned_words([1] + [4] * (step - 1), step, END, c) == ([END] if step <= 3 else [])
    assert banned_words([1], 1, END, Constraints()) == []
    assert banned_words([1, 4], 2, END, Constraints(no_repeat_ngram=1, min_words=6, banned=(0, 9))) == [0, 1, END, 4, 9]


def test_banned_words_is_the_reference_rule_on_random_sequences():
    g = torch.Generator().manual_seed(5)
    for _ in range(200):
        n = int(torch.randint(1, 10, (1,), generator=g))
        tokens = [1] + torch.randint(3, 7, (n - 1,), generator=g).tolist()
        for name, c in list(CC.SETS.items()) + [("g3", Constraints(no_repeat_ngram=3)), ("g4", Constraints(no_repeat_ngram=4))]:
            banned = set(banned_words(tokens, n, END, c))
            for v in range(8):
                broke = R.violations(tokens + [v], END, c)
                was = R.violations(tokens, END, c, completed=False)
                if was:
                    continue          # a sequence the search could not have reached
                assert (v in banned) == bool(broke), (name, tokens, v, broke)


# ---- validation ----------------------------------------------------------------------------------------------------------
def test_constraints_validation():
    c = Constraints()
    assert (c.no_repeat_ngram, c.min_words, c.banned, c.active) == (0, 0, (), False)
    assert Constraints(4, 0, range(32)).active and Constraints(banned=[3]).banned == (3,)
    for bad in (dict(no_repeat_ngram=5), dict(no_repeat_ngram=-1), dict(no_repeat_ngram=1.0), dict(no_repeat_ngram=True),
                dict(min_words=-1), dict(min_words="2"), dict(banned=(3, 3)), dict(banned=tuple(range(33))), dict(banned=(-1,)),
                dict(banned=(1.5,)), dict(banned=3), dict(banned="12")):
        with pytest.raises(capnet.CapnetError):
            Constraints(**bad)


class _Dec:
    vocab_size, max_seq_length = 37, 12


def _front(constraints, k=5, end=2, dec=_Dec):
    state = (torch.zeros(k, 4),)
    return decode.beam_decode(dec, None, state, None, k, 1, end, constraints=constraints)


def test_front_end_refuses_what_could_starve_a_step():
    with pytest.raises(capnet.CapnetError, match="end_token"):
        _front(Constraints(banned=(2,)))
    with pytest.raises(capnet.CapnetError, match="below 37"):
        _front(Constraints(banned=(37,)))
    with pytest.raises(capnet.CapnetError, match="min_words"):
        _front(Constraints(min_words=12))
    with pytest.raises(capnet.CapnetError, match="must be a capnet.beam.Constraints"):
        _front((1, 0, ()))

    class Small:
        vocab_size, max_seq_length = 21, 12        # 21 - 2 - 1 - 13 = 5 >= k = 5; one more banned word: 4
    Constraints(banned=(0, 3)).check(21, 2, 5, 12)
    with pytest.raises(capnet.CapnetError, match="fewer than k"):
        _front(Constraints(banned=(0, 3, 4)), dec=Small)
    with pytest.raises(capnet.CapnetError, match="fewer than k"):
        _front(Constraints(no_repeat_ngram=1), k=8, dec=Small)
    # a Constraints() that excludes nothing is not checked: the call runs as without the keyword, whatever the vocabulary
    # (here it goes on to the host loop, which calls the step function this test does not have)
    for nothing in (None, Constraints()):
        with pytest.raises(TypeError, match="NoneType"):
            _front(nothing, k=8, dec=Small)


def test_the_banned_arrays_cache_is_bounded(monkeypatch):
    made = []
    monkeypatch.setattr(ops.torch, "tensor", lambda v, dtype=None, device=None: made.append(tuple(v)) or torch.zeros(len(v), dtype=dtype))
    monkeypatch.setattr(ops, "_banned_dev", {})
    for r in range(3):
        for w in range(ops.BANNED_CACHE_MAX + 5):
            g, m, _, count = ops.constraint_args(Constraints(2, 3, banned=(w, w + 1)), "cpu")
            assert (g, m, count) == (2, 3, 2) and len(ops._banned_dev) <= ops.BANNED_CACHE_MAX
    assert ops.constraint_args(Constraints(), "cpu")[3] == 0 and made[-1] == (0,)
    n = len(made)
    ops.constraint_args(Constraints(), "cpu")                       # kept: not made again
    assert len(made) == n


def test_every_image_decoder_takes_the_keyword_and_the_others_do_not():
    from capnet.model import DecoderFactoredLSTM
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model import DecoderRNN
    from capnet.nic_model_att import DecoderRNNAtt
    from capnet.nic_stacked import StackedDecoderRNN, StackedDecoderRNNAtt
    from capnet.seq2seq import Seq2Seq
    from capnet.stacked import StackedFactoredLSTM
    from capnet.stacked_att import StackedFactoredLSTMAtt
    from capnet.train import evaluate
    for cls in (DecoderFactoredLSTM, DecoderRNN, StackedFactoredLSTM, StackedDecoderRNN, DecoderFactoredLSTMAtt, DecoderRNNAtt,
                StackedFactoredLSTMAtt, StackedDecoderRNNAtt):
        for name in ("sample", "sample_batch"):
            assert inspect.signature(getattr(cls, name)).parameters["constraints"].default is None, (cls, name)
        for name in ("sample_styles", "sample_random"):
            if hasattr(cls, name):
                assert "constraints" not in inspect.signature(getattr(cls, name)).parameters, (cls, name)
    assert inspect.signature(evaluate).parameters["constraints"].default is None
    assert inspect.signature(decode.beam_decode).parameters["constraints"].default is None
    for name in ("sample_beam", "sample_beam_styles"):
        assert "constraints" not in inspect.signature(getattr(Seq2Seq, name)).parameters


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_check_their_arguments():
    lib = capnet.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "capnet.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    assert lib.capnet_abi_version() == 1
    one = C.c_void_p(16)           # never dereferenced: every call below is refused on the host
    for bad, word in (((5, 0, None, 0), b"no_repeat_ngram"), ((-1, 0, None, 0), b"no_repeat_ngram"), ((1, -1, None, 0), b"min_words"),
                      ((1, 0, one, 33), b"n_banned"), ((1, 0, None, 2), b"banned"), ((1, 0, C.c_void_p(18), 2), b"banned")):
        rc = lib.capnet_beam_advance_constrained(one, one, 37, 37, 1, 3, 6, 1, 2, *bad, one, one, None)
        assert rc != 0 and word in lib.capnet_last_error(), (bad, lib.capnet_last_error())
        rc = lib.capnet_beam_advance_constrained_traced(one, one, one, 37, 37, 1, 3, 6, 1, 2, *bad, one, one, None)
        assert rc != 0 and word in lib.capnet_last_error(), (bad, lib.capnet_last_error())
    assert lib.capnet_beam_advance_constrained(one, None, 37, 37, 1, 3, 6, 1, 2, 1, 0, None, 0, one, one, None) != 0      # null logits
    assert lib.capnet_beam_advance_constrained(one, one, 37, 37, 1, 3, 6, 7, 2, 1, 0, None, 0, one, one, None) != 0       # step > max_steps
    assert lib.capnet_beam_advance_constrained_traced(one, None, one, 37, 37, 1, 3, 6, 1, 2, 1, 0, None, 0, one, one, None) != 0
    assert lib.capnet_beam_topk_banned(one, 37, 2, 37, one, 3, None, 4, one, one, None) != 0                             # null bans
    assert lib.capnet_beam_topk_banned(one, 37, 2, 37, one, 3, one, 0, one, one, None) != 0                              # cap 0
    assert lib.capnet_beam_topk_banned(one, 37, 17, 37, one, 3, one, 4, one, one, None) != 0                             # rows > 16
    assert lib.capnet_beam_topk_batched_banned(one, 37, 37, one, one, 2, None, 4, one, one, None) != 0
    assert lib.capnet_beam_topk_batched_banned(one, 37, 37, one, one, 2, one, 0, one, one, None) != 0


def test_ops_refuse_cpu_tensors_and_bad_bans():
    with pytest.raises(capnet.CapnetError):
        ops.beam_topk(torch.zeros(2, 37), torch.zeros(2), 2, 2, bans=torch.zeros(2, 3, dtype=torch.int32))


# ---- the cases -----------------------------------------------------------------------------------------------------------
def test_the_families_are_those_of_the_three_case_files():
    import att_beam_cases
    import beam_decode_cases
    import device_beam_cases
    names = [u.name for u in CC.units()]
    assert len(set(names)) == len(names)
    assert set(names) == {f.name for f in device_beam_cases.families() + att_beam_cases.families() + beam_decode_cases.families()}
    assert (CC.KS, CC.IMAGES, CC.MAX_LEN, CC.MARGIN) == ((3, 5), 3, 12, 1e-4)
    for c in CC.SETS.values():
        for u in CC.units():
            c.check(u.V, u.end, max(CC.KS), CC.MAX_LEN)


@pytest.mark.parametrize("u", CC.units(), ids=lambda u: u.name)
def test_every_case_is_admitted_and_every_set_bites(u):
    worst = float("inf")
    for s in CC.SETS:
        for k, i in u.cases():
            q = u.search(k, i, s)
            worst = min(worst, q.margin, q.gap(0.0))
            assert u.admitted(k, i, s), (u, s, k, i, q.margin, q.gap(0.0))
            for _, tokens in q.done:
                assert not R.violations(tokens, u.end, CC.SETS[s]), (u, s, k, i)
        changed = u.changed(s)
        print("%s set %s: %d of %d cases changed" % (u.name, s, len(changed), len(u.cases())))
        if s == "C" and u.name in CC.C_UNCHANGED:
            assert not changed
        else:
            assert changed, (u, s)
    # in at least one changed case of the family the caption returned is another one: what the GPU test calls the decoder on
    assert CC.other_winner(u) is not None
    print("%s: smallest margin / gap %.2e" % (u.name, worst))
    assert worst > CC.MARGIN


@pytest.mark.parametrize("k,V", CC.TABLE_CASES)
def test_the_tables_hold_their_scripts(k, V):
    tab = CC.table(k, V)
    free, _ = CC.model(k, V, None, tab, Constraints())
    # image 0 repeats word 3 forever without constraints; image 2 completes at step 1
    assert free.seqs[0][0] == [CC.TABLE_START] + [CC.FAR] * CC.TABLE_T
    assert k == 1 or free.done[2][0][2] == 1
    assert all(CC.BANNED in q for q in free.seqs[2][:free.live[2]] + [q for _, q in free.completed(2)][1:])
    for s, c in CC.TABLE_SETS.items():
        beam, gap = CC.model(k, V, s, tab)
        assert gap > CC.TABLE_GAP, (s, gap)
        for p in CC.PENALTIES:        # the rankings the kernel's n-best must reproduce rest on gaps as wide
            assert nbest_cases.table_rank_gap(beam, p) > CC.TABLE_GAP, (s, p)
        every = [q for i in range(CC.TABLE_N) for _, q in beam.completed(i)] + [q for i in range(CC.TABLE_N) for q in beam.seqs[i][:beam.live[i]]]
        for q in every:
            assert not R.violations(q, CC.TABLE_END, c), (s, q)
        far = [q.count(CC.FAR) for q in beam.seqs[0][:beam.live[0]]]
        assert max(far) <= 1 if s == "g1" else max(far) < CC.TABLE_T        # (g = 2: the pair 3 3 once, checked above)
        assert beam.seqs[0][0] != free.seqs[0][0]
        # image 2: every beam completes at step min_words + 1 exactly, the banned word never taken
        done2 = beam.done[2]
        assert len(done2) == k and all(step == CC.TABLE_MIN_WORDS + 1 for _, _, step in done2)
        # the log-sum-exp keeps the banned word: about 10 nats a step
        assert all(sc < -10.0 * (CC.TABLE_MIN_WORDS + 1) + 1.0 for sc, _, _ in done2)
        if s == "g2":            # image 1: a b a c a, then b and c are excluded behind a and 8 wins the tie that 6 would have won
            best = beam.seqs[1][0]
            assert best[:7] == [CC.TABLE_START, CC.A_, CC.B_, CC.A_, CC.C_, CC.A_, CC.TIE], best
            assert beam.excluded[6][(1, 0)] == sorted({CC.B_, CC.C_, CC.BANNED}), beam.excluded[6][(1, 0)]
            assert tab[5, k, CC.B_] == tab[5, k, CC.TIE] and CC.B_ < CC.TIE
