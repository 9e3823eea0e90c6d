"""capnet.metrics' CIDEr-D (CiderCorpus, cider_d_parts, sentence_cider_d, corpus_cider_d), capnet.train.cider_reward /
DeviceCiderReward's host side and evaluate(cider=True), on the CPU. The pin is the published definition and the worked cases
of cider_cases (closed forms, restated there)."""
import math

import pytest
import torch

import cider_cases as KC
from capnet import metrics, train


def test_worked_cases():
    corpus = metrics.CiderCorpus(KC.WORKED_CORPUS)
    assert corpus.N == 2 and corpus.log_n == math.log(2.0)
    for (hyp, refs, score, parts), decimal in zip(KC.WORKED, KC.WORKED_VALUES):
        got = metrics.sentence_cider_d(corpus, refs, hyp)
        assert got == pytest.approx(score, rel=1e-12) and got == pytest.approx(decimal, rel=1e-12), (hyp, got)
        if parts is not None:
            got_parts = metrics.cider_d_parts(corpus, refs, hyp)
            for g, w in zip(got_parts, parts):
                assert g == (0.0 if w == 0.0 else pytest.approx(w, rel=1e-12)), (hyp, got_parts)
            assert got == 2.5 * (got_parts[0] + got_parts[1] + got_parts[2] + got_parts[3])
    for (hyp, refs, _, _), decimals in zip(KC.WORKED, KC.WORKED_PARTS):      # the parts as decimals, to the digits written
        assert metrics.cider_d_parts(corpus, refs, hyp) == pytest.approx(decimals, rel=2e-10, abs=0.0)
    # a one-image corpus: ln 1 = 0, so everything scores 0
    one = metrics.CiderCorpus([KC.A])
    assert metrics.sentence_cider_d(one, KC.A, [1, 3, 4, 2]) == 0.0 and metrics.sentence_cider_d(one, KC.A, [1, 9, 2]) == 0.0
    with pytest.raises(ValueError):
        metrics.cider_d_parts(corpus, KC.A, [1, 3, 2], sigma=0.0)


def test_idf_and_tables():
    corpus = metrics.CiderCorpus(KC.WORKED_CORPUS)
    assert corpus.idf((1,)) == 0.0 and corpus.idf((3,)) == math.log(2.0)
    for g in ((9,), (3, 5), (1, 3, 5), (9, 9, 9, 9)):                    # never seen: ln N
        assert corpus.idf(g) == corpus.log_n
    for refs in (KC.WORKED_CORPUS, KC.random_corpus(40, 9, seed=3), KC.edge_corpus(7), KC.three_word_corpus()):
        c = metrics.CiderCorpus(refs)
        tables = c.tables()
        assert len(tables) == 4
        for n, (keys, idf) in enumerate(tables, 1):
            assert keys.dtype == torch.int32 and idf.dtype == torch.float64 and not keys.is_cuda
            assert tuple(keys.shape) == (len(c.df[n - 1]), n) and tuple(idf.shape) == (len(c.df[n - 1]),)
            rows = [tuple(k) for k in keys.tolist()]
            assert all(a < b for a, b in zip(rows, rows[1:]))            # strictly ascending, as tuples compare
            assert idf.tolist() == [c.idf(k) for k in rows]
            assert all(0.0 <= v <= c.log_n for v in idf.tolist())
    assert metrics.CiderCorpus(KC.three_word_corpus()).tables()[3][0].shape == (0, 4)
    for K in KC.EDGE_KEYS:
        assert [len(d) for d in metrics.CiderCorpus(KC.edge_corpus(K)).df] == [K] * 4
    for bad in ([[[1, -3, 2]]], [[[1, 2 ** 31, 2]]], []):
        with pytest.raises(ValueError):
            metrics.CiderCorpus(bad)
    # empty references are skipped
    assert metrics.CiderCorpus([KC.A + [[]], KC.B]).df == corpus.df


def test_named_rows_with_their_own_corpus():
    names = sorted(KC.NAMED)
    refs = [KC.NAMED[k][1] for k in names]
    corpus = metrics.CiderCorpus(refs)
    score = {k: metrics.sentence_cider_d(corpus, KC.NAMED[k][1], KC.hypothesis(KC.NAMED[k][0])) for k in names}
    print({k: round(v, 4) for k, v in score.items()})
    assert score["no_match"] == 0.0 and score["end_first"] == 0.0
    assert score["copy"] == pytest.approx(10.0, rel=1e-12)
    assert all(0.0 < v < 10.0 for k, v in score.items() if k not in ("no_match", "end_first", "copy"))


@pytest.mark.parametrize("V", [6, 12, 40])
@pytest.mark.parametrize("per_image", [1, 3, 6])
def test_sweep_rewards_are_spread(per_image, V):
    ids, refs = KC.sweep(256, per_image, V=V)
    corpus = metrics.CiderCorpus(refs)
    score = [metrics.sentence_cider_d(corpus, refs[r // per_image], KC.hypothesis(row)) for r, row in enumerate(ids)]
    assert all(0.0 <= s <= 10.0 for s in score)
    assert sum(1 for s in score if s == 0.0) <= 14 and len(set(score)) >= 243


def test_device_reward_host_side():
    refs = [[[1, 3, 4, 2], [1, 5, 2], []], [[1, 9, 9, 9, 9, 9, 2]], [[1, 2], [1, 3, 2], [1, 3, 4, 2], [1, 3, 4, 5, 2]]]
    corpus = metrics.CiderCorpus(refs + KC.random_corpus(20, 10, seed=1))
    rw = train.DeviceCiderReward(refs, corpus)
    assert rw.corpus is corpus and tuple(rw.refs.shape) == (3, 4, 7) and rw.ref_len.tolist() == [[4, 3, 0, 0], [7, 0, 0, 0], [2, 3, 4, 5]]
    bleu = train.DeviceBleuReward(refs)                                  # one packing for both
    assert torch.equal(rw.refs, bleu.refs) and torch.equal(rw.ref_len, bleu.ref_len)
    assert torch.equal(train.DeviceBleuReward.pack(refs)[0], train.pack_references(refs)[0])
    for i, hyp in ((0, [1, 3, 4, 2]), (1, torch.tensor([1, 9, 2])), (2, [1, 3, 4, 5, 2]), (2, [7, 7])):
        want = metrics.sentence_cider_d(corpus, refs[i], [int(w) for w in hyp])
        assert rw(i, hyp) == want == train.cider_reward(refs, corpus)(i, hyp)
    # ref_norm: the norms of cider_d_parts' own vectors, 0 in the absent slots
    assert rw.ref_norm.dtype == torch.float64 and tuple(rw.ref_norm.shape) == (3, 4, 4)
    for i in range(3):
        for j in range(4):
            r = refs[i][j] if j < len(refs[i]) else []
            vecs, norms = corpus.vectors(r)
            want = [math.sqrt(sum(v * v for v in vec.values())) for vec in vecs] if r else [0.0] * 4
            assert rw.ref_norm[i, j].tolist() == want and (not r or norms == want)
    # corpus=None: the batch's own references
    own = train.DeviceCiderReward(refs)
    assert own.corpus.N == 3 and own(0, [1, 3, 4, 2]) == metrics.sentence_cider_d(metrics.CiderCorpus(refs), refs[0], [1, 3, 4, 2])
    for bad in ([], [[[1, 2]], []], [[[1, 2]], [[]]], [[[1, 2]] * 17], [[[3] * 300] * 16]):
        with pytest.raises(ValueError):
            train.DeviceCiderReward(bad)
    with pytest.raises(ValueError):
        train.DeviceCiderReward(refs, sigma=0.0)


def test_corpus_cider_d():
    ids, refs = KC.sweep(48, 1, V=9)
    hyps = [KC.hypothesis(row) for row in ids]
    mean, each = metrics.corpus_cider_d(refs, hyps)
    assert (mean, each) == metrics.corpus_cider_d(refs, hyps, corpus=metrics.CiderCorpus(refs))
    assert len(each) == 48 and mean == sum(each) / 48 and 0.0 < mean < 10.0
    assert each == [metrics.sentence_cider_d(metrics.CiderCorpus(refs), r, h) for r, h in zip(refs, hyps)]
    other = metrics.corpus_cider_d(refs, hyps, corpus=metrics.CiderCorpus(refs[::2]))[0]
    assert other != mean


class _Encoder(torch.nn.Module):
    def forward(self, images):
        return images


class _Decoder(torch.nn.Module):
    """A decoder that "decodes" image i to the caption its feature row names."""

    def __init__(self, captions):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.captions = captions

    def sample_batch(self, features, start_token, end_token, k, **kw):
        return [self.captions[int(i)] for i in features.tolist()]

    def sample_styles(self, features, start_token, end_token, k, modes):
        return {m: self.sample_batch(features, start_token, end_token, k) for m in modes}


class _Vocab(object):
    word2idx = {"<start>": KC.START, "<end>": KC.END}


def test_evaluate_gains_a_fifth_entry():
    ids, refs = KC.sweep(12, 1, V=7)
    hyps = [KC.hypothesis(row) for row in ids]
    hyps[0] = list(refs[0][0])
    loader = [(torch.arange(0, 6), None, None, refs[:6]), (torch.arange(6, 12), None, None, refs[6:])]
    dec = _Decoder(hyps)
    four = train.evaluate(_Encoder(), dec, _Vocab(), loader, k=3)
    five = train.evaluate(_Encoder(), dec, _Vocab(), loader, k=3, cider=True)
    assert len(four) == 4 and len(five) == 5 and five[:4] == four
    assert five[4] == metrics.corpus_cider_d(refs, hyps)[0] and five[4] > 0.0
    assert train.evaluate_styles(_Encoder(), dec, _Vocab(), loader, modes=("sad",), k=3) == {"sad": four}     # (unchanged)
