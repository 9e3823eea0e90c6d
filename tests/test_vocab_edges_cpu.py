"""The inputs of the vocabulary kernels' edge tests (tests/vocab_edge_cases.py) in fp64 alone: every launch keeps to the cap
of at most one row set aside as not clear, and the wide cases put winners into both passes of the last arriver's loop."""
import pytest

import sample_random_ref as R
import vocab_edge_cases as VC


@pytest.mark.parametrize("case", VC.ARGMAX, ids=VC.case_id)
def test_argmax_inputs_keep_to_the_cap(case):
    name, H, V, rows, groups = case
    _, _, _, logits = VC.argmax_inputs(*case)
    assert len(logits) == groups
    for z in logits:
        assert tuple(z.shape) == (rows, V) and int(VC.argmax_clear(z).sum()) >= rows - 1
    if name == "wide":
        want = logits[0].argmax(1).tolist()
        assert want[0] == VC.WIDE_COLS[0]                                       # workgroup 257: the second pass
        if rows > 2:
            assert want[1] == VC.WIDE_COLS[1] and any(w < 8192 for w in want)   # workgroup 256, and the first pass


@pytest.mark.parametrize("case", VC.SAMPLE, ids=VC.case_id)
def test_sample_inputs_keep_to_the_cap(case):
    name, H, V, rows = case
    _, _, _, z = VC.sample_inputs(*case)
    drawn = []
    for T, inv_T, seed, step in VC.sample_launches(*case):
        d = R.draw(z, inv_T, seed, step)
        assert int(VC.sample_clear(d, inv_T).sum()) >= rows - 1, (T, step)
        drawn += d["tokens"].tolist()
    if name == "wide":
        assert any(t >= 8192 for t in drawn) and any(t < 8192 for t in drawn)   # winners in both passes of the merge
