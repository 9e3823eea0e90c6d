"""Diverse beam search without a GPU: capnet.beam.Diversity and the merge rules, the keyword's presence, position and absence,
capnet.metrics.distinct_n, the host-side refusals of the new C entries, and the admission of every case
tests/test_diverse_beam_gpu.py runs (tests/diverse_beam_cases.py: nothing is skipped there)."""
import ctypes as C
import inspect
import os

import pytest

import capnet
import diverse_beam_cases as DC
import diverse_beam_ref as R
from capnet import _lib, decode, metrics, ops
from capnet.beam import Diversity, dedupe_completed, merge_groups, rank_completed

NEW = ("capnet_beam_advance_diverse", "capnet_beam_topk_batched_diverse", "capnet_beam_decode_diverse",
       "capnet_att_beam_decode_diverse")


# ---- Diversity -------------------------------------------------------------------------------------------------------
def test_diversity_validation():
    d = Diversity(groups=3, strength=0.5)
    assert (d.groups, d.strength, d.per_group, d.active) == (3, 0.5, False, True)
    assert Diversity(2, 1).strength == 1.0 and isinstance(Diversity(2, 1).strength, float)
    assert Diversity(16, 0.0).active and Diversity(2, 0.0, True).per_group
    assert "groups=3" in repr(d) and "0.5" in repr(d) and "per_group=False" in repr(d)
    for bad in (dict(groups=0), dict(groups=17), dict(groups=2.0), dict(groups=True), dict(groups="2"),
                dict(strength=-0.1), dict(strength=float("inf")), dict(strength=float("nan")), dict(strength="1"),
                dict(strength=None), dict(strength=True), dict(per_group=1), dict(per_group=None)):
        with pytest.raises(capnet.CapnetError):
            Diversity(**bad)


def test_one_group_is_not_active():
    assert not Diversity(1, 0.5).active and not Diversity(1, 0.0, per_group=True).active


def test_check_wants_the_groups_to_divide_k():
    Diversity(2, 1.0).check(4)
    Diversity(3, 1.0).check(6)
    Diversity(16, 1.0).check(16)
    for D, k in ((2, 5), (3, 4), (4, 6), (4, 2), (2, 0)):
        with pytest.raises(capnet.CapnetError, match="divide"):
            Diversity(D, 1.0).check(k)


# ---- rank, dedupe, merge on hand-made lists --------------------------------------------------------------------------------
G0 = [(-3.0, [1, 7, 2]), (-2.0, [1, 7, 8, 2])]
G1 = [(-2.5, [1, 9, 2]), (-2.0000002, [1, 7, 8, 2]), (-9.0, [1, 4, 4, 4, 4, 2])]


def test_dedupe_keeps_the_first():
    flat = G0 + G1
    assert dedupe_completed(flat) == [G0[0], G0[1], G1[0], G1[2]]
    assert R.dedupe(flat) == [G0[0], G0[1], G1[0], G1[2]]
    assert dedupe_completed([]) == []


def test_merge_without_nbest_is_the_first_maximum_in_group_order():
    d = Diversity(2, 1.0)
    assert merge_groups([G0, G1], 2, d) == [1, 7, 8, 2]
    assert merge_groups([[], G1], 2, d) == [1, 7, 8, 2] == R.winner([[], G1], 2)
    assert merge_groups([[], [G1[0], G1[2]]], 2, d) == [1, 9, 2] == R.winner([[], [G1[0], G1[2]]], 2)
    assert merge_groups([[], []], 2, d) == [2] == R.winner([[], []], 2)
    tie = [[(-1.0, [1, 5, 2])], [(-1.0, [1, 6, 2])]]
    assert merge_groups(tie, 2, d) == [1, 5, 2] == R.winner(tie, 2)                          # ties: the lower group
    assert merge_groups([[(-1.0, [1, 5, 2]), (-1.0, [1, 6, 2])], []], 2, d) == [1, 5, 2]     # then the earlier completion


def test_merge_nbest_dedupes_then_ranks():
    d = Diversity(2, 1.0)
    got = merge_groups([G0, G1], 2, d, nbest=True)
    assert got == [([1, 7, 8, 2], -2.0), ([1, 9, 2], -2.5), ([1, 7, 2], -3.0), ([1, 4, 4, 4, 4, 2], -9.0)]
    assert got == R.nbest([G0, G1], 0.0)
    # length_penalty 1: score / generated words
    got = merge_groups([G0, G1], 2, d, nbest=True, length_penalty=1.0)
    assert [q for q, _ in got] == [[1, 7, 8, 2], [1, 9, 2], [1, 7, 2], [1, 4, 4, 4, 4, 2]]
    assert got == R.nbest([G0, G1], 1.0) == rank_completed(dedupe_completed(G0 + G1), 1.0)
    assert merge_groups([[], []], 2, d, nbest=True) == []


def test_merge_per_group():
    d = Diversity(3, 1.0, per_group=True)
    assert merge_groups([G0, G1, []], 2, d, nbest=True) == [([1, 7, 8, 2], -2.0), ([1, 7, 8, 2], -2.0000002), None]
    long_ = [(-2.0, [1, 7, 2]), (-2.5, [1, 7, 8, 9, 2])]
    assert merge_groups([long_, [], []], 2, d, nbest=True, length_penalty=1.0)[0] == ([1, 7, 8, 9, 2], -2.5)
    assert merge_groups([long_, [], []], 2, d, nbest=True, length_penalty=1.0) == R.per_group([long_, [], []], 1.0)


# ---- distinct_n --------------------------------------------------------------------------------------------------------
def test_distinct_n_on_worked_cases():
    assert metrics.distinct_n([[1, 2, 3], [1, 2, 4]], 1) == 4 / 6.0
    assert metrics.distinct_n([[1, 2, 3], [1, 2, 4]], 2) == 3 / 4.0
    assert metrics.distinct_n([[1, 2, 3], [1, 2, 3]], 2) == 0.5
    assert metrics.distinct_n([[1, 1, 1, 1]], 2) == 1 / 3.0
    assert metrics.distinct_n([[1, 2], [3]], 3) == 0.0 and metrics.distinct_n([], 1) == 0.0
    assert metrics.distinct_n([(5, 6), [7, 8]], 2) == 1.0
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError):
            metrics.distinct_n([[1, 2]], bad)


# ---- the keyword ---------------------------------------------------------------------------------------------------------
def test_every_image_decoder_takes_the_keyword_in_front_of_nbest_and_the_others_do_not():
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
            params = list(inspect.signature(getattr(cls, name)).parameters)
            assert inspect.signature(getattr(cls, name)).parameters["diversity"].default is None, (cls, name)
            assert params[-4:] == ["constraints", "diversity", "nbest", "length_penalty"], (cls, name, params)
        for name in ("sample_styles", "sample_styles_nbest", "sample_random"):
            if hasattr(cls, name):
                assert "diversity" not in inspect.signature(getattr(cls, name)).parameters, (cls, name)
    assert inspect.signature(evaluate).parameters["diversity"].default is None
    assert inspect.signature(decode.beam_decode).parameters["diversity"].default is None
    for name in dir(Seq2Seq):
        if name.startswith("sample_beam") or name == "sample_random":
            assert "diversity" not in inspect.signature(getattr(Seq2Seq, name)).parameters, name
    assert "diversity" not in inspect.signature(decode.sample_random).parameters


class _Dec:
    vocab_size, max_seq_length = 37, 6


def test_the_front_end_checks_before_anything_runs():
    import torch
    state = (torch.zeros(4, 8),)
    with pytest.raises(capnet.CapnetError, match="per_group"):
        decode.beam_decode(_Dec(), None, state, None, 4, 1, 2, diversity=Diversity(2, 1.0, per_group=True))
    with pytest.raises(capnet.CapnetError, match="divide"):
        decode.beam_decode(_Dec(), None, state, None, 5, 1, 2, diversity=Diversity(2, 1.0))
    with pytest.raises(capnet.CapnetError, match="Diversity"):
        decode.beam_decode(_Dec(), None, state, None, 4, 1, 2, diversity=(2, 1.0))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_check_their_arguments():
    lib = capnet.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "capnet.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    one = C.c_void_p(16)           # never dereferenced: every call below is refused on the host
    none = (0, 0, None, 0)

    def advance(k=4, D=2, strength=1.0, step=1, con=none, logits=one, trace=None):
        return lib.capnet_beam_advance_diverse(one, trace, logits, 37, 37, 1, k, D, strength, 6, step, 2, *con, one, one, None)
    for kw, word in ((dict(k=5), b"teams"), (dict(D=0), b"teams"), (dict(D=17, k=17), b"teams"), (dict(k=32, D=2), b"teams"),
                     (dict(strength=-1.0), b"strength"), (dict(strength=float("inf")), b"strength"),
                     (dict(strength=float("nan")), b"strength"), (dict(con=(5, 0, None, 0)), b"no_repeat_ngram"),
                     (dict(con=(1, 0, None, 2)), b"banned"), (dict(step=7), b"step"), (dict(logits=None), b"null"),
                     (dict(trace=C.c_void_p(18)), b"trace")):
        assert advance(**kw) != 0 and word in lib.capnet_last_error(), (kw, lib.capnet_last_error())

    def topk(D=2, strength=1.0, bans=None, cap=0, meta=one):
        return lib.capnet_beam_topk_batched_diverse(one, 37, 37, one, meta, 2, D, strength, bans, cap, one, one, None)
    for kw, word in ((dict(D=0), b"teams"), (dict(D=17), b"teams"), (dict(strength=-0.5), b"strength"),
                     (dict(bans=one, cap=0), b"cap"), (dict(bans=C.c_void_p(18), cap=3), b"bans"), (dict(meta=None), b"bad argument")):
        assert topk(**kw) != 0 and word in lib.capnet_last_error(), (kw, lib.capnet_last_error())


def test_ops_refuse_cpu_tensors():
    import torch
    with pytest.raises(capnet.CapnetError):
        ops.beam_topk_batched(torch.zeros(4, 37), torch.zeros(4), torch.zeros(2, 3, dtype=torch.int32), diversity=Diversity(2, 1.0))


# ---- the cases -----------------------------------------------------------------------------------------------------------
def test_the_families_are_those_of_the_three_case_files():
    import att_beam_cases
    import beam_decode_cases
    import device_beam_cases
    names = [f.name for f in device_beam_cases.families() + att_beam_cases.families() + beam_decode_cases.families()]
    assert [u.name for u in DC.units()] == list(dict.fromkeys(names))
    assert DC.SHAPES == ((4, 2), (6, 2), (6, 3)) and DC.STRENGTH == 1.0 and DC.MARGIN == 1e-4


_seen = {"D distinct winners": 0, "a group completes nothing": 0}


@pytest.mark.parametrize("u", DC.units(), ids=lambda u: u.name)
def test_every_case_is_admitted_and_diversity_bites(u):
    differs = False
    for k, D, i in u.cases():
        assert u.admitted(k, D, i), (u, k, D, i, u.smallest(k, D, i))
        q = u.search(k, D, i)
        assert len(q.groups) == D and all(len(d) <= k // D for d in q.groups)
        wins = q.per_group(0.0)
        _seen["D distinct winners"] += len({tuple(w[0]) for w in wins if w is not None}) == D
        _seen["a group completes nothing"] += any(w is None for w in wins)
        plain = u.search(k, 1, i)
        differs |= [t for t, _ in q.nbest(0.0)] != [t for t, _ in plain.nbest(0.0)]
        # the n-best holds every token list once, and the winner is its entry 0
        tokens = [tuple(t) for t, _ in q.nbest(0.0)]
        assert len(set(tokens)) == len(tokens)
        assert q.winner() == (list(tokens[0]) if tokens else [u.end])
    assert differs, u


def test_the_rejected_case_is_rejected_and_both_situations_occur():
    for (name, k, D), other in DC.STRENGTH_OTHER.items():
        u = [u for u in DC.units() if u.name == name][0]
        assert not all(u.admitted(k, D, i, strength=DC.STRENGTH) for i in range(DC.IMAGES))
        assert other != DC.STRENGTH
    for u in DC.units():            # (parametrised tests may have been deselected: count here)
        for k, D, i in u.cases():
            wins = u.search(k, D, i).per_group(0.0)
            _seen["D distinct winners"] += len({tuple(w[0]) for w in wins if w is not None}) == D
            _seen["a group completes nothing"] += any(w is None for w in wins)
    assert all(_seen.values()), _seen


def test_the_constrained_and_the_parity_cases_are_admitted():
    for name, k, D in DC.CON_CASES:
        u = DC.unit(name)
        assert all(u.admitted(k, D, i, constraints=DC.con_set()) for i in range(DC.IMAGES)), (name, k, D)
        assert any([t for t, _ in u.search(k, D, i, constraints=DC.con_set()).nbest(0.0)] != [t for t, _ in u.search(k, D, i).nbest(0.0)]
                   for i in range(DC.IMAGES))
    # the plain searches of k / D beams the strength-0 parity test compares with
    for u in DC.units():
        for k, D in DC.SHAPES:
            assert all(u.admitted(k // D, 1, i) for i in range(DC.IMAGES)), (u, k, D)


def test_one_group_is_the_plain_search():
    import nbest_ref
    u = DC.units()[0]
    step_fn, state = u.family.initial(4, 0)
    plain = nbest_ref.nbest_search(step_fn, state, u.V, DC.START, u.end, 4, DC.MAX_LEN)
    assert u.search(4, 1, 0).groups == [plain.done]


@pytest.mark.parametrize("k,D,V", DC.TABLE_CASES)
def test_the_tables_hold_their_scripts(k, D, V):
    kp, tab = k // D, DC.table(k, D, V)
    assert V - 1 >= k
    for strength in (0.0,) + DC.TABLE_STRENGTHS:
        for con in (None, DC.TABLE_CONSTRAINTS):
            m, gap = DC.model(k, D, V, strength, tab, con)
            assert gap > DC.TABLE_GAP, (strength, con, gap)
            # image 2: group 0 dies at step END_FROM (one step later under min_words = 3)
            first = DC.END_FROM + (1 if con is not None else 0)
            ends = [[len(q) - 1 for _, q in d] for d in m.group_done(2)]
            assert ends[0] == [first] * kp
            if strength == 1e4:         # group g cannot end while an earlier group does: one step later each
                assert ends[:2] == [[first] * kp, [first + 1] * kp]
                for step in range(1, DC.TABLE_T + 1):
                    for i in range(DC.TABLE_N):
                        assert not R.shared_words(R.group_words(m, step, i)), (step, i)
            else:
                assert ends[1] == [first] * kp or strength * kp > 60
            if con is None:             # image 1: the exact tie on group 1's rows
                got = m.selected[DC.TIE_STEP][1 * D + 1][1][0] % V
                assert got == (DC.A_ if strength == 0.0 else DC.B_), (strength, got)
            # image 0: at 0 and 0.5 every group takes the word that is 60 ahead, at 1e4 only group 0 does
            took = [DC.FAR in s for s in R.group_words(m, 1, 0)]
            assert took == ([True] + [False] * (D - 1) if strength == 1e4 else [True] * D)
