"""ops.cider_rows on the GPU against capnet.metrics.cider_d_parts / sentence_cider_d (fp64, pure Python), row by row:
  stats   exact (the length, the distinct n-grams per order, and how many of them the table holds: a lookup error shows here);
  parts   within 1e-12 relative, and exactly 0.0 where the oracle's part is 0.0. Every term is non-negative, so nothing
          cancels; a part takes fewer than 600 fp64 roundings (up to 129 terms of about 3 each, a square root, a division
          and an exponential): at most 600 x 2^-53 = 7e-14, so 1e-12 leaves an order of magnitude;
  reward  within 2^-23 relative of the fp64 score -- one float32 rounding (2^-24) of an fp64 result whose own error is
          negligible, with twice the margin, as tests/test_caption_reward_gpu.py -- and exactly 0.0 where the score is 0.0."""
import pytest
import torch

import cider_cases as KC
from capnet import CapnetError, metrics, ops, train

pytestmark = pytest.mark.gpu

REL, PART_REL = 2.0 ** -23, 1e-12


def _check(dev, corpus, ids, refs, per_image, steps=None, pad_columns=0, sigma=6.0):
    """cider_rows of the rows `ids` (lists) against the oracle, row by row -> (rewards, stats) as lists."""
    rw = train.DeviceCiderReward(refs, corpus, sigma)
    t = torch.tensor(ids, dtype=torch.int64)
    if pad_columns:                                         # a wider block, as a sampler's with more steps: ld > steps
        t = torch.cat([t, torch.full((t.shape[0], pad_columns), KC.END, dtype=torch.int64)], 1)
    t = t.to(dev)
    r_dev, p_dev, s_dev = ops.cider_rows(t, KC.START, KC.END, per_image, *rw.on(dev), corpus.log_n, sigma, steps=steps)
    assert r_dev.dtype == torch.float32 and p_dev.dtype == torch.float64 and s_dev.dtype == torch.int32
    assert tuple(r_dev.shape) == (len(ids),) and tuple(p_dev.shape) == (len(ids), 4) and tuple(s_dev.shape) == (len(ids), 9)
    reward, parts, stats = r_dev.cpu().tolist(), p_dev.cpu().tolist(), s_dev.cpu().tolist()
    for r, row in enumerate(ids):
        hyp = KC.hypothesis(row, steps)
        rr = refs[r // per_image]
        assert stats[r] == KC.oracle_stats(corpus, hyp), (r, row, stats[r])
        want_parts = metrics.cider_d_parts(corpus, rr, hyp, sigma)
        for n in range(4):
            if want_parts[n] == 0.0:
                assert parts[r][n] == 0.0, (r, n, parts[r])
            else:
                assert abs(parts[r][n] - want_parts[n]) <= PART_REL * want_parts[n], (r, n, parts[r][n], want_parts[n])
        want = metrics.sentence_cider_d(corpus, rr, hyp, sigma)
        assert rw(r // per_image, hyp) == want
        if want == 0.0:
            assert reward[r] == 0.0, (r, reward[r])
        else:
            assert abs(reward[r] - want) <= REL * want, (r, reward[r], want)
    return reward, stats


def test_worked_cases(dev):
    corpus = metrics.CiderCorpus(KC.WORKED_CORPUS)
    ids = [KC.row(hyp[1:-1]) for hyp, _, _, _ in KC.WORKED]
    refs = [r for _, r, _, _ in KC.WORKED]
    reward, _ = _check(dev, corpus, ids, refs, 1)
    for got, want in zip(reward, KC.WORKED_VALUES):
        assert abs(got - want) <= REL * want
    assert reward[2] == reward[3] == 10.0 and reward[4] == 5.0
    # a one-image corpus scores everything 0
    assert _check(dev, metrics.CiderCorpus([KC.A]), ids[:3], [KC.A] * 3, 1)[0] == [0.0, 0.0, 0.0]
    ops.check_device_errors()


def test_named_rows(dev):
    names = sorted(KC.NAMED)
    ids, refs = [KC.NAMED[k][0] for k in names], [KC.NAMED[k][1] for k in names]
    assert {len(r) for r in refs} >= {1, 2, 4}              # an image with one reference beside an image with four
    corpus = metrics.CiderCorpus(refs)
    reward = dict(zip(names, _check(dev, corpus, ids, refs, 1)[0]))
    print({k: round(v, 6) for k, v in reward.items()})
    assert reward["copy"] == 10.0 and reward["no_match"] == 0.0 and reward["end_first"] == 0.0
    assert _check(dev, corpus, ids, refs, 1, steps=KC.STEPS, pad_columns=3)[0] == list(reward.values())
    ops.check_device_errors()


def test_128_steps(dev):
    g = torch.Generator().manual_seed(5)
    body = torch.randint(3, 9, (3, 128), generator=g).tolist()          # no <end> among the words 3 .. 8
    body[1][100] = KC.END                                               # one row ends at column 100
    body[2][127] = KC.END                                               # one at the last column
    refs = [[[KC.START] + body[0][:90] + [KC.END], [KC.START] + body[0][20:60] + [KC.END]],
            [[KC.START] + body[1][:100] + [KC.END]],
            [[KC.START] + body[2][:50] + body[0][:70] + [KC.END]]]
    # (13 short random reference sets: some lack a word, so that the unigrams 3 .. 8 keep a non-zero idf)
    corpus = metrics.CiderCorpus(refs + KC.random_corpus(13, 9, seed=11, lo=3, hi=6))
    reward, stats = _check(dev, corpus, body, refs, 1)
    assert [s[0] for s in stats] == [129, 102, 129] and all(v > 0 for v in reward) and reward[1] == 10.0
    with pytest.raises(CapnetError):                                    # 129 columns: beyond the kernel's limit
        ops.cider_rows(torch.zeros((1, 129), dtype=torch.int64, device=dev), KC.START, KC.END, 1,
                       *train.DeviceCiderReward(refs, corpus).on(dev), corpus.log_n)
    ops.check_device_errors()


def _sweep(dev, per_image, V, corpus_of):
    ids, refs = KC.sweep(256, per_image, V=V)
    corpus = metrics.CiderCorpus(corpus_of(refs))
    reward, stats = _check(dev, corpus, ids, refs, per_image)
    distinct, known = sum(sum(s[1:5]) for s in stats), sum(sum(s[5:9]) for s in stats)
    zeros = sum(1 for v in reward if v == 0.0)
    print("per_image %d V %d: %d of %d n-grams in the table, %d of 256 rewards are 0, %d distinct, the largest %.4f"
          % (per_image, V, known, distinct, zeros, len(set(reward)), max(reward)))
    assert 0 < known < distinct
    assert zeros < 32 and len(set(reward)) > 200
    return ids, refs, corpus


@pytest.mark.parametrize("per_image", [1, 3, 6])
def test_sweep(dev, per_image):
    _sweep(dev, per_image, 6, lambda refs: refs)
    ops.check_device_errors()


def test_sweep_with_half_the_corpus(dev):
    """V = 40 and a corpus of every second image's references: many of the hypotheses' (and references') n-grams miss the table."""
    _sweep(dev, 3, 40, lambda refs: refs[::2])
    ops.check_device_errors()


@pytest.mark.parametrize("K", KC.EDGE_KEYS)
def test_lookup_edges(dev, K):
    corpus = metrics.CiderCorpus(KC.edge_corpus(K))
    assert [k.shape[0] for k, _ in corpus.tables()] == [K] * 4
    ids = KC.edge_rows(corpus)
    refs = [KC.edge_corpus(K)[0]]
    _, stats = _check(dev, corpus, ids, refs, len(ids))
    for n in range(4):                                      # every order: some row finds a key, some row misses one
        assert any(s[5 + n] >= 1 for s in stats) and any(s[5 + n] < s[1 + n] for s in stats)
    ops.check_device_errors()


def test_no_four_grams(dev):
    corpus = metrics.CiderCorpus(KC.three_word_corpus())
    assert [k.shape[0] for k, _ in corpus.tables()][3] == 0
    ids = [KC.row([3]), KC.row([3, 4, 5]), KC.row([1, 3, 2, 1, 4, 2]), KC.row([9, 9, 9, 9, 9])]
    refs = [KC.three_word_corpus()[0], KC.three_word_corpus()[2]]
    _, stats = _check(dev, corpus, ids, refs, 2)
    assert all(s[8] == 0 for s in stats) and any(s[4] > 0 for s in stats)
    ops.check_device_errors()


def test_rows_take_the_references_of_their_image(dev):
    """The same row six times over two images of three rows: rows 0 .. 2 score against image 0, rows 3 .. 5 against image 1."""
    row = [3, 4, 5, 6, KC.END, 0, 0, 0]
    refs = [[[KC.START, 3, 4, 5, 6, KC.END]], [[KC.START, 3, 4, 7, 7, 7, 7, KC.END], [KC.START, 9, KC.END]]]
    corpus = metrics.CiderCorpus(refs + KC.random_corpus(6, 10, seed=2))
    reward, _ = _check(dev, corpus, [row] * 6, refs, 3)
    assert reward[0] == reward[1] == reward[2] == 10.0 and reward[3] == reward[4] == reward[5] and 0 < reward[3] < 10
    rw = train.DeviceCiderReward(refs, corpus)
    ids = torch.tensor([row] * 6, dtype=torch.int64, device=dev)
    out = rw.rows(ids, KC.START, KC.END, 3)
    assert len(out) == 3 and out[0].cpu().tolist() == reward
    ops.check_device_errors()


def test_raised_errors(dev):
    row = [3, 4, 5, 6, KC.END, 0, 0, 0]
    refs = [[[KC.START, 3, 4, 5, 6, KC.END]], [[KC.START, 3, 4, 7, KC.END], [KC.START, 9, KC.END]]]
    rw = train.DeviceCiderReward(refs)
    ids = torch.tensor([row] * 6, dtype=torch.int64, device=dev)
    log_n = rw.corpus.log_n
    with pytest.raises(CapnetError):
        rw.rows(ids, KC.START, KC.END, 2)                   # six rows are not two images x 2
    with pytest.raises(CapnetError):
        ops.cider_rows(ids, KC.START, KC.END, 2, *rw.on(dev), log_n)      # rows beyond the references' images
    with pytest.raises(CapnetError):
        ops.cider_rows(ids.int(), KC.START, KC.END, 3, *rw.on(dev), log_n)
    for sigma in (0.0, -6.0):
        with pytest.raises(CapnetError):
            ops.cider_rows(ids, KC.START, KC.END, 3, *rw.on(dev), log_n, sigma=sigma)
    with pytest.raises(CapnetError):
        ops.cider_rows(ids, KC.START, KC.END, 3, *rw.on(dev)[:3], rw.on(dev)[3][:3], log_n)          # three tables
    ops.check_device_errors()


def test_two_launches_agree_bit_for_bit(dev):
    ids, refs = KC.sweep(256, 3)
    rw = train.DeviceCiderReward(refs)
    t = torch.tensor(ids, dtype=torch.int64, device=dev)
    r1, p1, s1 = ops.cider_rows(t, KC.START, KC.END, 3, *rw.on(dev), rw.corpus.log_n)       # (256 rows: the last image has one)
    r2, p2, s2 = ops.cider_rows(t, KC.START, KC.END, 3, *rw.on(dev), rw.corpus.log_n)
    assert torch.equal(r1, r2) and torch.equal(p1, p2) and torch.equal(s1, s2)
    assert float(p1.sum()) > 0
    ops.check_device_errors()
