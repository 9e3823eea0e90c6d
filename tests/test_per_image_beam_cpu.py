"""Per-image constraints in batched beam search, the part that needs no GPU: capnet.beam.PerImage (validation, uniform(),
slicing, check), the rule table's layout word for word, the four new C entries (declared, bound, exported, and refusing a NULL
or misaligned table on the host), what the front ends refuse, the host loops' rule as code (_bans / _met under a mixed set), and
the statements the GPU tests rest on -- every (family, k, image, entry) of tests/per_image_cases.py is admitted by the existing
margin rule, every family has a k at which the two assignments and the three uniform sets all return different captions, and
every stored-logits expectation rests on gaps above TABLE_GAP."""
import ctypes as C
import os

import pytest
import torch

import capnet
import per_image_cases as PC
from capnet import _lib, beam, decode, ops
from capnet.beam import MIXED, Constraints, Diversity, PerImage, banned_words, met_mask

NEW = ("capnet_beam_advance_rules", "capnet_beam_topk_batched_rules", "capnet_beam_decode_rules", "capnet_att_beam_decode_rules")
END = 2


# ---- PerImage --------------------------------------------------------------------------------------------------------
def test_per_image_is_a_sequence_of_entries_and_no_constraints():
    a, b = Constraints(forced=(5,)), Constraints(no_repeat_ngram=2)
    p = PerImage([a, None, b])
    assert not isinstance(p, Constraints) and not hasattr(p, "forced")
    assert len(p) == 3 and p[0] is a and p[1] is None and p[-1] is b and list(p) == [a, None, b]
    tail = p[1:]
    assert isinstance(tail, PerImage) and len(tail) == 2 and tail[0] is None and tail[1] is b
    assert isinstance(p[0:0], PerImage) and len(p[0:0]) == 0
    assert p.active and not PerImage([None, Constraints()]).active and not PerImage([]).active
    for bad in (3, "ab", a, [a, (1, 0, ())], [a, 5]):
        with pytest.raises(capnet.CapnetError, match="PerImage"):
            PerImage(bad)


def test_uniform_collapses_equal_entries():
    a = Constraints(1, 2, (3,), (4,))
    assert PerImage([a, Constraints(1, 2, (3,), (4,)), a]).uniform() is a
    assert PerImage([None, None]).uniform() is None
    assert PerImage([Constraints(), Constraints()]).uniform() is None
    assert PerImage([None, Constraints(), None]).uniform() is None          # an inactive Constraints() and None are equal
    assert PerImage([a, None]).uniform() is MIXED
    assert PerImage([a, Constraints()]).uniform() is MIXED
    assert PerImage([a, Constraints(1, 2, (3,), (5,))]).uniform() is MIXED
    assert PerImage([Constraints(banned=(3, 4)), Constraints(banned=(4, 3))]).uniform() is MIXED     # the fields, as given
    assert MIXED is not None and not isinstance(MIXED, Constraints)


def test_check_counts_the_entries_and_runs_every_active_entrys_own():
    p = PerImage([Constraints(forced=(3, 4)), None, Constraints()])
    p.check(37, END, 5, 12, 3)
    for n in (2, 4):
        with pytest.raises(capnet.CapnetError, match="3 entries for %d images" % n):
            p.check(37, END, 5, 12, n)
    with pytest.raises(capnet.CapnetError, match="end_token"):
        PerImage([None, Constraints(forced=(END,))]).check(37, END, 5, 12, 2)
    with pytest.raises(capnet.CapnetError, match="below 37"):
        PerImage([Constraints(banned=(37,)), None]).check(37, END, 5, 12, 2)
    with pytest.raises(capnet.CapnetError, match="min_words"):
        PerImage([None, None, Constraints(min_words=12)]).check(37, END, 5, 12, 3)


# ---- the table -------------------------------------------------------------------------------------------------------
def test_the_table_holds_the_exact_words():
    p = PerImage([Constraints(2, 3, (9, 7, 30), (4, 6)), None, Constraints(), Constraints(forced=(11, 12, 13, 14)),
                  Constraints(banned=tuple(range(40, 72)))])
    t = p.table("cpu")
    assert t.dtype == torch.int32 and tuple(t.shape) == (5, 40) and t.is_contiguous()
    assert PerImage.RULE_WORDS == ops.RULE_WORDS == 40
    assert t[0].tolist() == [2, 3, 3, 2, 9, 7, 30] + [0] * 29 + [4, 6, 0, 0]
    assert t[1].tolist() == [0] * 40 and t[2].tolist() == [0] * 40
    assert t[3].tolist() == [0, 0, 0, 4] + [0] * 32 + [11, 12, 13, 14]
    assert t[4].tolist() == [0, 0, 32, 0] + list(range(40, 72)) + [0] * 4
    assert p.table("cpu") is t                       # made once per device
    assert p[3:].table("cpu").tolist() == t[3:].tolist()


def test_the_header_states_the_layout():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "capnet.h")).read()
    assert "#define CAPNET_BEAM_RULE_WORDS 40" in header
    for line in ("word 0        no_repeat_ngram", "word 1        min_words", "word 2        n_banned", "word 3        n_forced",
                 "words 4..35   banned", "words 36..39  forced"):
        assert line in header, line


# ---- the C entries ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_refuse_a_bad_table():
    lib = capnet.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "capnet.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
        assert "sample" not in name and "nucleus" not in name
    assert lib.capnet_abi_version() == 1
    one = C.c_void_p(16)           # never dereferenced: every call below is refused on the host
    ptrs = (C.c_void_p * 2)(16, 16)
    steps = C.c_int(0)
    for bad in (None, C.c_void_p(20), C.c_void_p(24)):       # NULL; 4- and 8-byte aligned only
        calls = {
            "capnet_beam_advance_rules": lambda: lib.capnet_beam_advance_rules(one, None, one, 37, 37, 1, 3, 6, 1, 2, bad, one, one, None),
            "capnet_beam_topk_batched_rules": lambda: lib.capnet_beam_topk_batched_rules(one, 37, 37, one, one, 2, None, 0, one, bad, 2, one, one, None),
            "capnet_beam_decode_rules": lambda: lib.capnet_beam_decode_rules(0, 1, 2, 3, 16, 64, 37, 6, 1, 2, one, ptrs, ptrs, one, one, None, one, one,
                                                                             1024, 0, one, one, C.byref(steps), one, None, bad),
            "capnet_att_beam_decode_rules": lambda: lib.capnet_att_beam_decode_rules(0, 1, 2, 3, 49, 32, 64, 16, 64, 37, 6, 1, 2, one, one, one, one, one,
                                                                                     one, one, ptrs, ptrs, one, one, one, one, one, 1024, 0, one, one,
                                                                                     C.byref(steps), one, None, None, bad),
        }
        for name in NEW:
            rc = calls[name]()
            assert rc != 0 and b"rules" in lib.capnet_last_error(), (name, bad, lib.capnet_last_error())
    # with a good table the other host checks are the forced entries': null logits, step > max_steps, k > 16, null met, cap 0
    assert lib.capnet_beam_advance_rules(one, None, None, 37, 37, 1, 3, 6, 1, 2, one, one, one, None) != 0
    assert lib.capnet_beam_advance_rules(one, None, one, 37, 37, 1, 3, 6, 7, 2, one, one, one, None) != 0
    assert lib.capnet_beam_advance_rules(one, None, one, 37, 37, 1, 17, 6, 1, 2, one, one, one, None) != 0
    assert lib.capnet_beam_topk_batched_rules(one, 37, 37, one, one, 2, None, 0, None, one, 2, one, one, None) != 0
    assert lib.capnet_beam_topk_batched_rules(one, 37, 37, one, one, 2, one, 0, one, one, 2, one, one, None) != 0


def test_ops_refuse_cpu_tensors_and_a_wrong_count():
    p = PerImage([Constraints(forced=(4,)), None])
    with pytest.raises(capnet.CapnetError):
        ops.beam_topk_batched(torch.zeros(2, 37), torch.zeros(2), torch.zeros(2, 3, dtype=torch.int32),
                              forced=(p, torch.zeros(2, dtype=torch.int32), END))
    assert ops.is_per_image(p) and not ops.is_per_image(Constraints()) and not ops.is_per_image(None) and not ops.has_forced(p)
    with pytest.raises(capnet.CapnetError, match="2 entries for 3 images"):
        ops.rules_arg("here", p, 3, "cpu")


# ---- what the front ends refuse ----------------------------------------------------------------------------------------
class _Dec:
    vocab_size, max_seq_length = 37, 12


def _front(n, k=4, **kw):
    rows = k * (1 if n is None else n)
    return decode.beam_decode(_Dec, None, (torch.zeros(rows, 4),), n, k, 1, END, **kw)


def test_the_front_end_refuses_one_image_and_diversity_and_checks():
    mixed = PerImage([Constraints(forced=(5,)), None])
    with pytest.raises(capnet.CapnetError, match="sample_batch"):
        _front(None, constraints=mixed)
    with pytest.raises(capnet.CapnetError, match="sample_batch"):
        _front(None, constraints=PerImage([None]))
    with pytest.raises(capnet.CapnetError, match="diversity"):
        _front(2, constraints=mixed, diversity=Diversity(2, 0.5))
    with pytest.raises(capnet.CapnetError, match="2 entries for 3 images"):
        _front(3, constraints=mixed)
    with pytest.raises(capnet.CapnetError, match="end_token"):
        _front(2, constraints=PerImage([None, Constraints(forced=(END,))]))
    # a Diversity that is not active is none; the call then reaches the host loop, which calls the step this test lacks -- with a
    # mixed set, with a uniform one and with one that says nothing
    for p in (mixed, PerImage([Constraints(forced=(5,))] * 2), PerImage([None, Constraints()])):
        with pytest.raises(TypeError, match="NoneType"):
            _front(2, constraints=p, diversity=Diversity(1, 0.5))
    # a plain tuple of Constraints is still no Constraints
    with pytest.raises(capnet.CapnetError, match="must be a capnet.beam.Constraints"):
        _front(2, constraints=(Constraints(forced=(5,)), Constraints()))
    with pytest.raises(capnet.CapnetError, match="must be a capnet.beam.Constraints"):
        _front(2, constraints=[Constraints(forced=(5,)), None])


def test_uniform_sets_reach_the_loops_as_the_one_rule(monkeypatch):
    seen = []
    monkeypatch.setattr(decode, "beam_search_batched", lambda *a, **kw: seen.append(kw) or [[END]] * 2)
    c = Constraints(forced=(5,))
    mixed = PerImage([c, None])
    _front(2, constraints=PerImage([c, Constraints(forced=(5,))]))
    _front(2, constraints=PerImage([None, Constraints()]))
    _front(2, constraints=mixed)
    _front(2, constraints=c)
    _front(2)
    assert seen[0] == {"constraints": c} == seen[3] and seen[1] == {} == seen[4] and seen[2] == {"constraints": mixed}


def test_what_takes_only_a_constraints_still_says_so():
    from capnet import seq2seq, train
    mixed = PerImage([Constraints(no_repeat_ngram=1), None])
    with pytest.raises(capnet.CapnetError, match="exclude must be a capnet.beam.Constraints"):
        decode.sample_random(_Dec, None, (torch.zeros(4, 4),), 2, 2, 1, END, exclude=mixed)
    with pytest.raises(capnet.CapnetError, match="exclude must be a capnet.beam.Constraints"):
        train.self_critical_step(None, None, None, None, 1, END, 5.0, exclude=mixed)
    m = seq2seq.Seq2Seq(12, 64, 37, 1, dropout=0.0, max_seq_length=12).eval()
    feats = torch.zeros(2, 12)
    with pytest.raises(capnet.CapnetError, match="constraints must be a capnet.beam.Constraints"):
        m.sample_beam_constrained(feats, 1, END, mixed, k=5)
    with pytest.raises(capnet.CapnetError, match="constraints must be a capnet.beam.Constraints"):
        m.sample_beam_styles_constrained(feats, 1, END, mixed, k=5)
    with pytest.raises(capnet.CapnetError, match="constraints must be a capnet.beam.Constraints"):
        m.decoder_sad.sample_beam(1, END, (None, None), k=5, constraints=mixed)
    with pytest.raises(capnet.CapnetError, match="exclude must be a capnet.beam.Constraints"):
        m.sample_random(feats, 1, seed=0, exclude=mixed, end_token=END)


# ---- the host loops' rule as code ------------------------------------------------------------------------------------
def test_bans_and_met_take_each_rows_own_images_entry():
    entries = [Constraints(no_repeat_ngram=1, min_words=3, banned=(0,), forced=(7, 9)), None, Constraints(no_repeat_ngram=2),
               Constraints(forced=(4,))]
    p = PerImage(entries)
    rows = [[1, 7, 4], [1, 9, 7], [1, 4, 4], [1, 5, 6, 5], [1, 5, 5], [1, 4, 8]]
    images = [0, 0, 1, 2, 2, 3]
    step = 3
    bans = beam._bans(rows[:3] + [rows[3][:3]] + rows[4:], step, END, p, "cpu", images)
    met = beam._met(rows, p, "cpu", images)
    for r, (tokens, i) in enumerate(zip(rows[:3] + [rows[3][:3]] + rows[4:], images)):
        c = entries[i] or Constraints()
        want = banned_words(tokens, step, END, c)
        assert bans[r, 0] == len(want) and bans[r, 1:1 + len(want)].tolist() == want, (r, bans[r].tolist(), want)
    assert bans[2].tolist()[0] == 0                               # the image without a rule: an empty list
    assert met.tolist() == [met_mask(t, (entries[i] or Constraints()).forced) for t, i in zip(rows, images)]
    assert met.tolist() == [1, 3, 0, 0, 0, 1]
    assert beam.entry_of(p, 1).active is False and beam.entry_of(p, 3) is entries[3] and beam.entry_of(entries[0], None) is entries[0]
    # one Constraints for all rows: as before there was a PerImage
    one = entries[0]
    assert beam._bans(rows, 4, END, one, "cpu").tolist() == beam._bans(rows, 4, END, PerImage([one] * 6), "cpu", list(range(6))).tolist()


# ---- the cases -------------------------------------------------------------------------------------------------------
def test_the_assignments_are_the_issues():
    names = [fu.name for fu, _ in PC.units()]
    assert names == [u.name for u in PC.FC.units()] and all(fu.name == cu.name for fu, cu in PC.units())
    assert (PC.KS, PC.IMAGES, PC.MARGIN) == ((3, 5), 3, 1e-4)
    for name in names:
        a, b = PC.keys(name, "A"), PC.keys(name, "B")
        assert a[0] == ("forced", "one") and a[1][0] == "con" and a[1][1] in PC.CC.SETS and a[2] is None
        assert b == [a[2], a[0], a[1]]                            # A rotated by one image
    fu = PC.units()[0][0]
    p = PC.per_image(fu, "A")
    assert p[0] is fu.sets["one"] and not p[1].forced and p[1].active and p[2] is None and p.uniform() is MIXED
    assert PC.TABLE_ASSIGNMENTS == {"first": ("F1", "F2", "g1", "F4"), "second": ("F4", "F2", None, "F1")}
    assert PC.TABLE_ENTRIES["g1"] is PC.CC.TABLE_SETS["g1"] and PC.TABLE_ENTRIES["F4"] is PC.FC.TABLE_SETS["F4"]
    assert (PC.TABLE_N, PC.TABLE_T, PC.TABLE_GAP) == (4, 7, 1e-3)
    assert PC.TABLE_CASES == [(1, 37), (3, 37), (5, 37), (16, 37), (5, 1500)]


@pytest.mark.parametrize("fu,cu", PC.units(), ids=lambda u: u.name)
def test_every_case_is_admitted_and_the_assignments_tell(fu, cu):
    worst = float("inf")
    for which in PC.ASSIGNMENTS:
        PC.per_image(fu, which).check(fu.V, fu.end, max(PC.KS), PC.MAX_LEN, PC.IMAGES)
        for k in PC.KS:
            for i, key in enumerate(PC.keys(fu.name, which)):
                q = PC.search(fu, cu, k, i, key)
                worst = min(worst, q.margin, q.gap(0.0), q.gap(1.0))
                assert all(PC.admitted(fu, cu, k, i, key, p) for p in PC.PENALTIES), (fu, which, k, i, key, q.margin, q.gap(0.0), q.gap(1.0))
                assert q.done, (fu, which, k, i, key)
    k = PC.telling_k(fu, cu)
    assert k is not None, fu
    a, b = PC.keys(fu.name, "A"), PC.keys(fu.name, "B")
    wa, wb = PC.winners(fu, cu, k, a), PC.winners(fu, cu, k, b)
    assert wa != wb
    for key in a:                      # no single entry for all images returns either
        same = PC.winners(fu, cu, k, [key] * PC.IMAGES)
        assert same != wa and same != wb, (fu, k, key)
    print("%s: smallest margin / gap %.2e; the assignments tell at k = %d" % (fu.name, worst, k))
    assert worst > PC.MARGIN


@pytest.mark.parametrize("k,V", PC.TABLE_CASES)
def test_the_composed_models_rest_on_gaps_above_the_tables(k, V):
    for which, names in PC.TABLE_ASSIGNMENTS.items():
        want = PC.Composed(k, V, which)
        assert want.gap > PC.TABLE_GAP, (which, want.gap)
        for i, key in enumerate(names):
            model, gap = PC.table_model(k, V, key, i)
            assert gap > PC.TABLE_GAP, (which, i, key, gap)
            # image i of the model driven alone is image i of the whole model under that entry: the images are independent
            whole, _ = PC.FC.model(k, V, None, PC.FC.table(k, V), PC.TABLE_ENTRIES[key] or Constraints())
            assert model.completed(i) == whole.completed(i) and model.finish()[i] == whole.finish()[i]
            for step in range(1, PC.TABLE_T + 1):
                for part in (0, 1):
                    assert model.outputs[step][part][i * k:(i + 1) * k] == whole.outputs[step][part][i * k:(i + 1) * k]
            c = PC.TABLE_ENTRIES[key]
            if c is not None and c.forced:
                assert all(w in q for _, q in model.completed(i) for w in c.forced)
        # the two assignments ask different things of images 0, 2 and 3
    first, second = PC.Composed(k, V, "first"), PC.Composed(k, V, "second")
    assert [first.completed(i) != second.completed(i) for i in (0, 3)] == [True, True] or k == 1
    assert first.outputs(PC.TABLE_T) != second.outputs(PC.TABLE_T) or first.finish() != second.finish()
