"""The margin rule of tests/greedy_row_cases.py, on the CPU: every case's recorded stream seed is the first from 0 upwards
whose fp64 restatement clears the rule at every row and step (the rejected seeds are printed with what failed), the greedy
rows clear theirs, the drawn rows of the restatement are those of the restatement without a greedy row, and what is left
after dropping still covers every family, shape and option."""
import numpy as np
import pytest
import torch

import greedy_row_cases as GC
import greedy_row_ref as G
import nucleus_ref as N
import sample_random_ref as R
from device_beam_cases import START


@pytest.mark.parametrize("case", GC.CASES, ids=[c["id"] for c in GC.CASES])
def test_recorded_seed_is_the_first_that_clears_the_rule(case):
    seed, rejected = GC.first_seed(case)
    for s, fails in sorted(rejected.items()):
        print("%s: seed %d rejected: %s" % (case["id"], s, "; ".join(fails)))
    if case["id"] in GC.DROPPED:
        assert seed is None, "a dropped case has a seed that clears the rule: %r" % (seed,)
        return
    assert seed == GC.SEEDS[case["id"]]
    ids, logp, tr = GC.reference(case)
    inv_T = R.inv_temperature(case["T"])
    assert G.clears(tr, inv_T, case["top_k"], case["top_p"]) == []
    assert tr.greedy_gap > G.need_greedy(tr.scale, inv_T) and tr.key_gap > R.need(tr.scale, inv_T)
    assert ids.shape == (case["n"] * (case["m"] + 1), GC.STEPS) and np.isfinite(logp).all() and (logp <= 0).all()


def test_what_is_left_covers_every_family_shape_and_option():
    live = GC.live_cases()
    cov = GC.coverage(live)
    assert cov["family"] == set(GC.FAMILIES) and cov["shape"] == set(GC.SHAPES)
    assert cov["top_k"] == {0, 5} and cov["top_p"] == {1.0, 0.9} and cov["T"] == {1.0, 0.7}
    for fam in GC.FAMILIES:
        for opt, values in (("top_k", (0, 5)), ("top_p", (1.0, 0.9)), ("T", (1.0, 0.7))):
            for v in values:
                assert (fam, opt, v) in cov["family_options"], (fam, opt, v)
    for shape in GC.SHAPES:
        for opt, values in (("top_k", (0, 5)), ("top_p", (1.0, 0.9)), ("T", (1.0, 0.7))):
            assert {c[opt] for c in live if (c["n"], c["m"]) == shape} == set(values), (shape, opt)
    assert set(GC.DROPPED) <= {c["id"] for c in GC.CASES}


@pytest.mark.parametrize("case", GC.live_cases(), ids=[c["id"] for c in GC.live_cases()])
def test_drawn_rows_are_those_of_the_decode_without_a_greedy_row(case):
    """The restatement's layout: physical row i (m + 1) + j on noise row i m + j."""
    ids, logp, _ = GC.reference(case)
    fam = GC.families()[case["family"]]
    n, m = case["n"], case["m"]
    seed = GC.SEEDS[case["id"]]
    if case["top_p"] < 1.0:
        ids0, logp0, _ = N.family_sampled(fam.initial, n, m, GC.STEPS, START, case["T"], seed, case["top_k"], case["top_p"])
    else:
        ids0, logp0, _ = R.family_sampled(fam.initial, n, m, GC.STEPS, START, case["T"], seed, case["top_k"])
    drawn = [i * (m + 1) + j for i in range(n) for j in range(m)]
    assert np.array_equal(ids[drawn], ids0) and np.allclose(logp[drawn], logp0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", GC.live_cases(), ids=[c["id"] for c in GC.live_cases()])
def test_greedy_rows_are_the_argmax_decode(case):
    """The greedy row against a plain argmax loop over the same restated step; its end token is reached by image 0."""
    ids, _, _ = GC.reference(case)
    fam = GC.families()[case["family"]]
    for i, row in enumerate(GC.greedy_rows(case)):
        step_fn, state = fam.initial(1, i)
        words = torch.LongTensor([[START]])
        for t in range(GC.STEPS):
            logits, state = step_fn(words, state)
            words = logits.argmax(1, keepdim=True)
            assert int(words) == int(ids[row][t]), (i, t)
    assert GC.end_token(case) in ids[GC.greedy_rows(case)[0]].tolist()
