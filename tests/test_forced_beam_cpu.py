"""Forced words in beam search, the part that needs no GPU: the field of capnet.beam.Constraints and its checks, the rule as
code (capnet.beam.banned_words' new case, capnet.beam.forced_allocate on hand-worked pools and against the reference's own
walk), the unchanged signatures, the new symbols' host-side argument checks, and the statements the GPU tests rest on -- every
case of tests/forced_beam_cases.py is admitted and completes a hypothesis (so nothing is skipped there), in every family a
forced set changes the caption, and every table's model gap exceeds TABLE_GAP."""
import ctypes as C
import inspect
import os

import pytest
import torch

import capnet
import forced_beam_cases as FC
import forced_beam_ref as R
import nbest_cases
from capnet import _lib, decode, ops
from capnet.beam import Constraints, Diversity, banned_words, forced_allocate, met_mask

NEW = ("capnet_beam_advance_forced", "capnet_beam_topk_batched_forced", "capnet_beam_decode_forced", "capnet_att_beam_decode_forced")
END = 2


# ---- the field and its checks --------------------------------------------------------------------------------------------
def test_the_field_and_its_validation():
    c = Constraints()
    assert (c.no_repeat_ngram, c.min_words, c.banned, c.forced, c.active) == (0, 0, (), (), False)
    assert Constraints().active is False
    assert Constraints(forced=[5]).forced == (5,) and Constraints(forced=(5,)).active
    assert Constraints(1, 2, (3,), (4, 6)).forced == (4, 6) and Constraints.MAX_FORCED == 4
    assert list(inspect.signature(Constraints.__init__).parameters)[1:] == ["no_repeat_ngram", "min_words", "banned", "forced"]
    for bad in (dict(forced=(3, 3)), dict(forced=(1, 2, 3, 4, 5)), dict(forced=(-1,)), dict(forced=(1.5,)), dict(forced=(True,)),
                dict(forced=3), dict(forced="12"), dict(forced=(3,), banned=(4, 3))):
        with pytest.raises(capnet.CapnetError):
            Constraints(**bad)


def test_check_refuses_what_cannot_be_met():
    Constraints(forced=(3, 4)).check(37, END, 5, 12)
    with pytest.raises(capnet.CapnetError, match="below 37"):
        Constraints(forced=(37,)).check(37, END, 5, 12)
    with pytest.raises(capnet.CapnetError, match="end_token"):
        Constraints(forced=(END,)).check(37, END, 5, 12)
    with pytest.raises(capnet.CapnetError, match="fewer than max_seq_length"):
        Constraints(forced=(3, 4, 5)).check(37, END, 5, 3)
    Constraints(forced=(3, 4)).check(37, END, 5, 3)


class _Dec:
    vocab_size, max_seq_length = 37, 12


def _front(k=4, **kw):
    return decode.beam_decode(_Dec, None, (torch.zeros(k, 4),), None, k, 1, END, **kw)


def test_the_front_end_checks_and_refuses_diversity():
    with pytest.raises(capnet.CapnetError, match="end_token"):
        _front(constraints=Constraints(forced=(END,)))
    with pytest.raises(capnet.CapnetError, match="diversity"):
        _front(constraints=Constraints(forced=(5,)), diversity=Diversity(2, 0.5))
    # a Diversity that is not active is no diversity: the call goes on to the host loop, which calls the step this test lacks
    with pytest.raises(TypeError, match="NoneType"):
        _front(constraints=Constraints(forced=(5,)), diversity=Diversity(1, 0.5))


# ---- the rule ------------------------------------------------------------------------------------------------------------
def test_banned_words_with_and_without_forced():
    assert banned_words([1, 4, 7], 3, END, Constraints()) == []
    c = Constraints(forced=(7, 9))
    assert banned_words([1], 1, END, c) == [END]
    assert banned_words([1, 7, 4], 3, END, c) == [END]
    assert banned_words([1, 9, 4, 7], 4, END, c) == []
    assert banned_words([7, 9], 2, END, c) == [END]              # <start> does not count, whatever its id
    c = Constraints(no_repeat_ngram=1, min_words=1, banned=(0,), forced=(7,))
    assert banned_words([1, 7], 2, END, c) == [0, 1, 7]
    assert banned_words([1, 4], 2, END, c) == [0, 1, END, 4]
    assert met_mask([7, 9, 4], (7, 9)) == 2 and met_mask([1, 7, 9], (7, 9)) == 3 and met_mask([1], (7,)) == 0


def test_forced_allocate_on_hand_worked_pools():
    # F = 2, three banks; bank 1 is empty and is skipped; banks 2, 0, 2, 0, 0
    pool = [(-1.0, 10, 0), (-2.0, 11, 0), (-9.0, 12, 2), (-3.0, 13, 0), (-8.0, 14, 2), (-4.0, 15, 0)]
    assert [p[1] for p in forced_allocate(pool, 5, 2)] == [14, 10, 12, 11, 13]
    # fewer banks with candidates than slots: the walk comes round again; more slots than candidates: the pool, no more
    assert [p[1] for p in forced_allocate([(-5.0, 3, 1), (-1.0, 4, 0), (-2.0, 5, 0)], 3, 1)] == [3, 4, 5]
    assert [p[1] for p in forced_allocate([(-5.0, 3, 1), (-1.0, 4, 0)], 5, 1)] == [3, 4]
    # k = 1: the best of the highest bank that has a candidate, however bad
    assert forced_allocate([(-0.1, 4, 0), (-30.0, 9, 1), (-40.0, 8, 1)], 1, 2) == [(-30.0, 9, 1)]
    assert forced_allocate([(-0.1, 4, 0), (-0.2, 5, 0)], 1, 2) == [(-0.1, 4, 0)]
    # ties go to the lower flat index
    assert [p[1] for p in forced_allocate([(-1.0, 9, 1), (-1.0, 7, 1), (-1.0, 8, 0)], 2, 1)] == [7, 8]
    # a candidate that entered by several parts is in the pool once
    assert [p[1] for p in forced_allocate([(-1.0, 7, 1), (-1.0, 7, 1), (-2.0, 8, 1), (-1.0, 7, 1)], 3, 1)] == [7, 8]
    # F = 0: the plain order
    assert [p[1] for p in forced_allocate([(-2.0, 1, 0), (-1.0, 2, 0), (-3.0, 3, 0)], 2, 0)] == [2, 1]


def test_forced_allocate_is_the_references_walk_on_random_steps():
    g = torch.Generator().manual_seed(11)
    for trial in range(40):
        rows, V, F = int(torch.randint(1, 6, (1,), generator=g)), 23, 1 + trial % 4
        live = int(torch.randint(1, 7, (1,), generator=g))
        forced = tuple(range(3, 3 + F))
        toks = [[1] + torch.randint(3, 9, (trial % 5,), generator=g).tolist() for _ in range(rows)]
        block = torch.randn(rows, V, generator=g, dtype=torch.float64) * 6
        for r in range(rows):
            if R.missing(toks[r], forced):
                block[r, END] = float("-inf")
        taken, _ = R.select(block, toks, live, forced)
        # the pool by the rule's three parts, duplicates and all, through capnet.beam's code
        flat = block.reshape(-1)
        pool = [(float(flat[j]), int(j)) for j in torch.sort(flat, descending=True, stable=True)[1][:live].tolist()]
        for r in range(rows):
            pool += [(float(block[r, w]), r * V + w) for w in forced if w not in toks[r][1:]]
            pool.append((float(block[r].max()), r * V + int(block[r].argmax())))
        pool = [(sc, f, bin(met_mask(toks[f // V] + [f % V], forced)).count("1")) for sc, f in pool]
        assert [(sc, f) for sc, f, _ in forced_allocate(pool, live, F)] == taken, trial


# ---- signatures and the C ABI --------------------------------------------------------------------------------------------
def test_signatures_are_unchanged():
    from capnet.model import DecoderFactoredLSTM
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model import DecoderRNN
    from capnet.nic_model_att import DecoderRNNAtt
    from capnet.stacked import StackedFactoredLSTM
    from capnet.train import evaluate
    for cls in (DecoderFactoredLSTM, DecoderRNN, StackedFactoredLSTM, DecoderFactoredLSTMAtt, DecoderRNNAtt):
        for name in ("sample", "sample_batch"):
            assert list(inspect.signature(getattr(cls, name)).parameters)[-4:] == ["constraints", "diversity", "nbest", "length_penalty"]
            assert "forced" not in inspect.signature(getattr(cls, name)).parameters
    assert inspect.signature(evaluate).parameters["constraints"].default is None
    assert len(ops.constraint_args(Constraints(1, 2, (3,), (4,)), "cpu")) == 4
    arr, count = ops.forced_args(Constraints(forced=(4, 6)), "cpu")
    assert count == 2 and arr
    assert not ops.has_forced(None) and not ops.has_forced(Constraints(1)) and ops.has_forced(Constraints(forced=(4,)))


def test_new_symbols_are_declared_bound_and_check_their_arguments():
    lib = capnet.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "capnet.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    one = C.c_void_p(16)           # never dereferenced: every call below is refused on the host
    for bad, word in (((None, 1), b"forced"), ((one, 0), b"n_forced"), ((one, 5), b"n_forced"), ((C.c_void_p(18), 2), b"forced")):
        rc = lib.capnet_beam_advance_forced(one, None, one, 37, 37, 1, 3, 6, 1, 2, 0, 0, None, 0, *bad, one, one, None)
        assert rc != 0 and word in lib.capnet_last_error(), (bad, lib.capnet_last_error())
        rc = lib.capnet_beam_topk_batched_forced(one, 37, 37, one, one, 2, None, 0, one, *bad, 2, one, one, None)
        assert rc != 0 and word in lib.capnet_last_error(), (bad, lib.capnet_last_error())
    assert lib.capnet_beam_advance_forced(one, None, one, 37, 37, 1, 3, 6, 1, 2, 5, 0, None, 0, one, 1, one, one, None) != 0   # g = 5
    assert lib.capnet_beam_advance_forced(one, None, None, 37, 37, 1, 3, 6, 1, 2, 0, 0, None, 0, one, 1, one, one, None) != 0  # null logits
    assert lib.capnet_beam_advance_forced(one, None, one, 37, 37, 1, 3, 6, 7, 2, 0, 0, None, 0, one, 1, one, one, None) != 0   # step > max_steps
    assert lib.capnet_beam_advance_forced(one, None, one, 37, 37, 1, 17, 6, 1, 2, 0, 0, None, 0, one, 1, one, one, None) != 0  # k > 16
    assert lib.capnet_beam_topk_batched_forced(one, 37, 37, one, one, 2, None, 0, None, one, 1, 2, one, one, None) != 0        # null met
    assert lib.capnet_beam_topk_batched_forced(one, 37, 37, one, one, 2, one, 0, one, one, 1, 2, one, one, None) != 0          # cap 0


def test_ops_refuse_cpu_tensors():
    c = Constraints(forced=(4,))
    with pytest.raises(capnet.CapnetError):
        ops.beam_topk_batched(torch.zeros(2, 37), torch.zeros(2), torch.zeros(1, 3, dtype=torch.int32),
                              forced=(c, torch.zeros(2, dtype=torch.int32), END))


# ---- the cases -----------------------------------------------------------------------------------------------------------
def test_the_families_are_those_of_the_three_case_files():
    import att_beam_cases
    import beam_decode_cases
    import device_beam_cases
    names = [u.name for u in FC.units()]
    assert len(set(names)) == len(names)
    assert set(names) == {f.name for f in device_beam_cases.families() + att_beam_cases.families() + beam_decode_cases.families()}
    assert set(FC.FORCED) == set(names)
    assert (FC.KS, FC.IMAGES, FC.MAX_LEN, FC.MARGIN) == ((3, 5), 3, 12, 1e-4)
    for u in FC.units():
        assert len(u.sets) == 2
        for c in u.sets.values():
            c.check(u.V, u.end, max(FC.KS), FC.MAX_LEN)


@pytest.mark.parametrize("u", FC.units(), ids=lambda u: u.name)
def test_every_case_is_admitted_completes_and_the_sets_bite(u):
    worst = float("inf")
    for s, c in u.sets.items():
        for k, i in u.cases():
            q = u.search(k, i, s)
            worst = min(worst, q.margin, q.gap(0.0), q.gap(1.0))
            assert all(u.admitted(k, i, s, p) for p in FC.PENALTIES), (u, s, k, i, q.margin, q.gap(0.0), q.gap(1.0))
            assert q.done, (u, s, k, i)                  # at least one hypothesis completes within MAX_LEN
            for _, tokens in q.done:                     # the property, from the definition alone
                assert not R.missing(tokens, c.forced) and tokens[-1] == u.end, (u, s, k, i, tokens)
    hit = u.bites()
    assert hit is not None
    s, k, i = hit
    assert R.missing(u.winner(k, i, None), u.sets[s].forced) and u.winner(k, i, s) != u.winner(k, i, None)
    print("%s: smallest margin / gap %.2e; bites at %r" % (u.name, worst, hit))
    assert worst > FC.MARGIN


@pytest.mark.parametrize("k,V", FC.TABLE_CASES)
def test_the_tables_hold_their_scripts(k, V):
    tab = FC.table(k, V)
    T, n = FC.TABLE_T, FC.TABLE_N
    free, _ = FC.model(k, V, None, tab, Constraints())
    # image 0 without forced words: W0 is never emitted
    assert all(FC.W0 not in q for q in [p for _, p in free.completed(0)] + free.seqs[0][:free.live[0]])
    for s, c in FC.TABLE_SETS.items():
        F = len(c.forced)
        beam, gap = FC.model(k, V, s, tab)
        assert gap > FC.TABLE_GAP, (s, gap)
        for p in FC.PENALTIES:        # the rankings the kernel's n-best must reproduce rest on gaps as wide
            assert nbest_cases.table_rank_gap(beam, p) > FC.TABLE_GAP, (s, p)
        for i in range(n):
            for sc, q in beam.completed(i):
                assert not R.missing(q, c.forced), (s, i, q)
        # image 0: the forced word is emitted and paid in full -- the winner's score is the sum of its words' log-probabilities
        done0 = beam.completed(0)
        assert done0 and all(FC.W0 in q for _, q in done0)
        sc, q = max(done0, key=lambda p: p[0])
        logp = torch.log_softmax(tab.double(), dim=2)
        rows = beam.done_paths[0][[p for _, p in done0].index(q)][1:]
        want = sum(float(logp[e, r, q[e + 1]]) for e, r in enumerate(rows))
        assert abs(sc - want) < 1e-9 and sc < -30.0, (s, sc, want)
        # image 3: nothing completes before every forced word is in, then <end>, far ahead, at once (min_words permitting)
        first = min(len(q) for _, q in beam.completed(3))
        assert first == max(F, c.min_words) + 2, (s, first)
        if F >= 2:            # image 1: W1 is taken once at step 2 by the best hypothesis
            assert all(q.count(FC.W1) <= 1 for q in beam.seqs[1][:beam.live[1]]) or c.no_repeat_ngram == 0
            assert k == 1 or any(len(q) > 2 and q[2] == FC.W1 for q in beam.seqs[1][:beam.live[1]] + [p for _, p in beam.completed(1)])
        # image 2: the exact tie at TIE_STEP goes to the lower flat index
        assert tab[FC.TIE_STEP - 1, 2 * k, FC.TIE_A] == tab[FC.TIE_STEP - 1, 2 * k, FC.TIE_B]
        words, rows, competing = beam.outputs[FC.TIE_STEP]
        picks = list(zip(rows[2 * k:3 * k], words[2 * k:3 * k]))[:beam.live[2] if FC.TIE_STEP == T else k]
        tied = [(p, w) for p, w in picks if w in (FC.TIE_A, FC.TIE_B)]
        assert competing[2] and tied, (s, picks)
        for p, w in tied:
            if w == FC.TIE_B and FC.TIE_A not in beam.excluded[FC.TIE_STEP][(2, p - 2 * k)]:     # (g = 1 excludes a word already in)
                assert (p, FC.TIE_A) in tied[:tied.index((p, w))], (s, picks)
