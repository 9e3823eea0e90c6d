"""ops.bleu_rows on the GPU against capnet.metrics.sentence_bleu (fp64, pure Python): the ten integers exactly, the reward
within 2^-23 relative -- one float32 rounding (2^-24) of an fp64 result whose own error is negligible, with twice the margin
-- and an exact 0.0 as exact 0.0."""
import pytest
import torch

import caption_reward_cases as CC
from capnet import CapnetError, metrics, ops, train

pytestmark = pytest.mark.gpu

REL = 2.0 ** -23


def _check(dev, ids, refs, per_image, smooth, weights=CC.WEIGHTS, steps=None, pad_columns=0):
    """bleu_rows of the rows `ids` (lists) against the oracle, row by row -> the rewards (a list)."""
    rw = train.DeviceBleuReward(refs, weights, smooth)
    t = torch.tensor(ids, dtype=torch.int64)
    if pad_columns:                                         # a wider block, as a sampler's with more steps: ld > steps
        t = torch.cat([t, torch.full((t.shape[0], pad_columns), CC.END, dtype=torch.int64)], 1)
    t = t.to(dev)
    r_dev, s_dev = ops.bleu_rows(t, CC.START, CC.END, per_image, *rw.on(dev), weights=weights, smooth=smooth, steps=steps)
    assert r_dev.dtype == torch.float32 and s_dev.dtype == torch.int32 and tuple(s_dev.shape) == (len(ids), 10)
    reward, stats = r_dev.cpu().tolist(), s_dev.cpu().tolist()
    for r, row in enumerate(ids):
        hyp = CC.hypothesis(row, steps)
        rr = [x for x in refs[r // per_image] if len(x)]
        assert stats[r] == metrics.sentence_stats(rr, hyp), (r, row, stats[r])
        want = metrics.sentence_bleu(rr, hyp, weights, smooth)
        assert rw(r // per_image, hyp) == want
        if want == 0.0:
            assert reward[r] == 0.0, (r, reward[r])
        else:
            assert abs(reward[r] - want) <= REL * want, (r, reward[r], want)
    return reward


@pytest.mark.parametrize("smooth", [0, 1])
def test_named_rows(dev, smooth):
    names = sorted(CC.NAMED)
    ids, refs = [CC.NAMED[k][0] for k in names], [CC.NAMED[k][1] for k in names]
    assert {len(r) for r in refs} >= {1, 2, 4}              # an image with one reference beside an image with four
    reward = dict(zip(names, _check(dev, ids, refs, 1, smooth)))
    print({k: round(v, 6) for k, v in reward.items()})
    assert reward["copy"] == 1.0
    if smooth:
        assert all(v > 0 for v in reward.values())
    else:
        assert reward["clipped"] == 0.0 and reward["start_end"] == 0.0 and reward["length_tie"] > 0
    # the other weightings of capnet.train.evaluate, and the same rows in a wider block
    for w in ((1, 0, 0, 0), (0.5, 0.5, 0, 0), (0.33, 0.33, 0.33, 0)):
        _check(dev, ids, refs, 1, smooth, weights=w)
    assert _check(dev, ids, refs, 1, smooth, steps=CC.STEPS, pad_columns=3) == list(reward.values())
    ops.check_device_errors()


@pytest.mark.parametrize("smooth", [0, 1])
def test_128_steps(dev, smooth):
    g = torch.Generator().manual_seed(5)
    body = torch.randint(3, 9, (3, 128), generator=g).tolist()          # no <end> among the words 3 .. 8
    body[1][100] = CC.END                                               # one row ends at column 100
    body[2][127] = CC.END                                               # one at the last column
    refs = [[[CC.START] + body[0][:90] + [CC.END], [CC.START] + body[0][20:60] + [CC.END]],
            [[CC.START] + body[1][:100] + [CC.END]],
            [[CC.START] + body[2][:50] + body[0][:70] + [CC.END]]]
    reward = _check(dev, body, refs, 1, smooth)
    assert all(v > 0 for v in reward) and reward[1] == pytest.approx(1.0, abs=1e-6)
    with pytest.raises(CapnetError):                                    # 129 columns: beyond the kernel's limit
        ops.bleu_rows(torch.zeros((1, 129), dtype=torch.int64, device=dev), CC.START, CC.END, 1,
                      *train.DeviceBleuReward(refs).on(dev))
    ops.check_device_errors()


@pytest.mark.parametrize("per_image", [1, 3, 6])
@pytest.mark.parametrize("smooth", [0, 1])
def test_sweep(dev, per_image, smooth):
    ids, refs = CC.sweep(256, per_image)
    reward = _check(dev, ids, refs, per_image, smooth)
    zeros = sum(1 for v in reward if v == 0.0)
    print("per_image %d smooth %d: %d of 256 rewards are 0, the largest %.4f" % (per_image, smooth, zeros, max(reward)))
    assert zeros < 256 and len(set(reward)) > (16 if smooth else 4)      # (unsmoothed, most random rows have no matching 4-gram)
    ops.check_device_errors()


def test_rows_take_the_references_of_their_image(dev):
    """The same row six times over two images of three rows: rows 0 .. 2 score against image 0, rows 3 .. 5 against image 1."""
    row = [3, 4, 5, 6, CC.END, 0, 0, 0]
    refs = [[[CC.START, 3, 4, 5, 6, CC.END]], [[CC.START, 3, 4, 7, 7, 7, 7, CC.END], [CC.START, 9, CC.END]]]
    reward = _check(dev, [row] * 6, refs, 3, 1)
    assert reward[0] == reward[1] == reward[2] == 1.0 and reward[3] == reward[4] == reward[5] and 0 < reward[3] < 1
    rw = train.DeviceBleuReward(refs, smooth=1)
    ids = torch.tensor([row] * 6, dtype=torch.int64, device=dev)
    assert rw.rows(ids, CC.START, CC.END, 3)[0].cpu().tolist() == reward
    with pytest.raises(CapnetError):
        rw.rows(ids, CC.START, CC.END, 2)                   # six rows are not two images x 2
    with pytest.raises(CapnetError):
        ops.bleu_rows(ids, CC.START, CC.END, 2, *rw.on(dev))              # rows beyond the references' images
    with pytest.raises(CapnetError):
        ops.bleu_rows(ids.int(), CC.START, CC.END, 3, *rw.on(dev))
    ops.check_device_errors()
