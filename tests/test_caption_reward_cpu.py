"""capnet.metrics.sentence_bleu and capnet.train.DeviceBleuReward's packing, on the CPU."""
import math

import pytest
import torch

import caption_reward_cases as CC
from capnet import metrics, train


@pytest.mark.parametrize("name", sorted(CC.NAMED))
def test_unsmoothed_sentence_bleu_is_corpus_bleu_of_one_sentence(name):
    ids, refs = CC.NAMED[name]
    hyp = CC.hypothesis(ids)
    for w in (CC.WEIGHTS, (1, 0, 0, 0), (0.5, 0.5, 0, 0), (0.33, 0.33, 0.33, 0)):
        assert metrics.sentence_bleu(refs, hyp, w) == metrics.corpus_bleu([refs], [hyp], w)
        assert metrics.sentence_bleu(refs, hyp, w, smooth=0) == metrics.corpus_bleu([refs], [hyp], w)
    st = metrics.sentence_stats(refs, hyp)
    assert len(st) == 10 and st[8] == len(hyp) and st[4:8] == [max(1, len(hyp) - n) for n in range(4)]
    # add-one can only raise a score, and leaves 0 only where no word matches
    s1 = metrics.sentence_bleu(refs, hyp, smooth=1)
    assert s1 >= metrics.sentence_bleu(refs, hyp) and (s1 == 0.0) == (st[0] == 0)


def test_sweep_rows_agree_with_corpus_bleu():
    ids, refs = CC.sweep(per_image=3)
    zeros = 0
    for r, row in enumerate(ids):
        hyp = CC.hypothesis(row)
        b = metrics.sentence_bleu(refs[r // 3], hyp)
        assert b == metrics.corpus_bleu([refs[r // 3]], [hyp])
        zeros += b == 0.0
    assert 0 < zeros < len(ids)


def test_known_values():
    ids, refs = CC.NAMED["copy"]
    assert metrics.sentence_bleu(refs, CC.hypothesis(ids)) == 1.0 and metrics.sentence_bleu(refs, CC.hypothesis(ids), smooth=1) == 1.0
    ids, refs = CC.NAMED["clipped"]
    assert metrics.sentence_stats(refs, CC.hypothesis(ids))[:4] == [4, 2, 1, 0]       # <start> 5 5 <end>; (<start> 5), (5 5); (<start> 5 5)
    ids, refs = CC.NAMED["max_not_sum"]
    assert metrics.sentence_stats(refs, CC.hypothesis(ids))[0] == 3                   # <start>, ONE 5, <end>
    ids, refs = CC.NAMED["length_tie"]
    assert metrics.sentence_stats(refs, CC.hypothesis(ids))[8:] == [6, 5]


def test_add_one_by_hand():
    """hyp = <start> 3 4 5 9 <end> (6 words) against <start> 3 4 5 6 <end> (6 words):
    unigrams: <start> 3 4 5 <end> match, 9 does not -> 5 / 6
    bigrams: (<start> 3) (3 4) (4 5) match, (5 9) (9 <end>) do not -> 3 / 5, smoothed (3 + 1) / (5 + 1)
    trigrams: (<start> 3 4) (3 4 5) -> 2 / 4, smoothed 3 / 5
    4-grams: (<start> 3 4 5) -> 1 / 3, smoothed 2 / 4
    equal lengths: bp = exp(1 - 6 / 6) = 1."""
    refs, hyp = [[1, 3, 4, 5, 6, 2]], [1, 3, 4, 5, 9, 2]
    assert metrics.sentence_stats(refs, hyp) == [5, 3, 2, 1, 6, 5, 4, 3, 6, 6]
    want = ((5 / 6) * (4 / 6) * (3 / 5) * (2 / 4)) ** 0.25
    assert metrics.sentence_bleu(refs, hyp, smooth=1) == pytest.approx(want, rel=1e-14)
    plain = ((5 / 6) * (3 / 5) * (2 / 4) * (1 / 3)) ** 0.25
    assert metrics.sentence_bleu(refs, hyp) == pytest.approx(plain, rel=1e-14)
    # no matching 4-gram: 0.0 unsmoothed, a score with add-one
    hyp2 = [1, 3, 4, 9, 5, 2]
    assert metrics.sentence_bleu(refs, hyp2) == 0.0
    st = metrics.sentence_stats(refs, hyp2)
    assert st[:4] == [5, 2, 1, 0]
    assert metrics.sentence_bleu(refs, hyp2, smooth=1) == pytest.approx(math.exp(0.25 * sum(math.log(x) for x in (5 / 6, 3 / 6, 2 / 5, 1 / 4))),
                                                                      rel=1e-14)
    with pytest.raises(ValueError):
        metrics.sentence_bleu(refs, hyp, smooth=2)


def test_device_reward_packs_ragged_references():
    refs = [[[1, 3, 4, 2], [1, 5, 2], []],            # three slots, one of them empty
            [[1, 9, 9, 9, 9, 9, 2]],                  # one reference, the longest
            [[1, 2], [1, 3, 2], [1, 3, 4, 2], [1, 3, 4, 5, 2]]]
    rw = train.DeviceBleuReward(refs, smooth=1)
    assert rw.refs.dtype == torch.int32 and rw.ref_len.dtype == torch.int32
    assert tuple(rw.refs.shape) == (3, 4, 7) and tuple(rw.ref_len.shape) == (3, 4)
    assert rw.ref_len.tolist() == [[4, 3, 0, 0], [7, 0, 0, 0], [2, 3, 4, 5]]
    for i, rr in enumerate(refs):
        for j in range(4):
            r = rr[j] if j < len(rr) else []
            assert rw.refs[i, j].tolist() == r + [0] * (7 - len(r))
    # the host call: metrics.sentence_bleu against the image's references (an empty slot is not a reference)
    assert rw(0, [1, 3, 4, 2]) == metrics.sentence_bleu(refs[0], [1, 3, 4, 2], smooth=1)
    assert rw(1, torch.tensor([1, 9, 2])) == metrics.sentence_bleu(refs[1], [1, 9, 2], smooth=1)
    plain = train.DeviceBleuReward(refs)
    assert plain(2, [1, 3, 4, 5, 2]) == train.bleu_reward(refs)(2, [1, 3, 4, 5, 2]) == 1.0
    for bad in ([], [[[1, 2]], []], [[[1, 2]], [[]]], [[[1, 2]] * 17], [[[3] * 300] * 16]):
        with pytest.raises(ValueError):
            train.DeviceBleuReward(bad)
    with pytest.raises(ValueError):
        train.DeviceBleuReward(refs, weights=(0.5, 0.5))
    with pytest.raises(ValueError):
        train.DeviceBleuReward(refs, smooth=3)
