"""self_critical_step with a CIDEr-D reward: the device route (capnet.train.DeviceCiderReward, ops.cider_rows) against the same
step with the host reward (capnet.train.cider_reward), on tests/test_self_critical_device_gpu.py's CASE -- two copies of one
tiny attention decoder at one seed, whose decode the fp64 restatement reproduces token for token, so that references and
rewards can be restated on the CPU -- and the learning test with the CIDEr-D reward never on the host."""
import pytest
import torch

import cider_cases as KC
import greedy_row_cases as GC
import sample_random_ref as R
from capnet import metrics, ops, synthetic, train

CASE = [c for c in GC.CASES if c["family"] == "StackedFactoredLSTMAtt-2-v37" and (c["n"], c["m"]) == (3, 5)][0]
SAMPLING = dict(temperature=CASE["T"], top_k=CASE["top_k"], top_p=CASE["top_p"])
N_IMG, M = CASE["n"], CASE["m"]
START = GC.START
REL = 2.0 ** -23
gpu = pytest.mark.gpu


def _restated():
    """test_self_critical_device_gpu's: (the restated captions per image -- M drawn and the greedy one --, the end token, the
    references: per image the first drawn caption itself and the first words of two more and of the greedy one)."""
    ids, logp, _ = GC.reference(CASE)
    end = GC.end_token(CASE)
    caps = [[q for q, _ in img] for img in R.cut(ids, logp, N_IMG, M + 1, START, end)]
    refs = [[img[0], img[1][:4] + [end], img[2][:5] + [end], img[M][:3] + [end]] for img in caps]
    return caps, end, refs


def test_references_spread_the_rewards():
    """On the CPU, from the restatement, with the corpus being the three images' references: the rewards are neither all 0
    nor all equal, and under the greedy baseline an advantage is 0 only where a drawn caption IS the greedy caption."""
    caps, end, refs = _restated()
    ids = GC.reference(CASE)[0]
    assert all(end in ids[row].tolist() for row in GC.greedy_rows(CASE))
    corpus = metrics.CiderCorpus(refs)
    r = [[metrics.sentence_cider_d(corpus, refs[i], q) for q in img] for i, img in enumerate(caps)]
    flat = [x for img in r for x in img[:M]]
    print("rewards %s" % [[round(x, 3) for x in img] for img in r])
    assert min(flat) >= 0.0 and max(flat) > 1.0 and len(set(flat)) >= 10
    for i, img in enumerate(caps):
        for j in range(M):
            assert (r[i][j] - r[i][M] == 0.0) == (img[j] == img[M]), (i, j)
    assert any(x != img[M] for img in r for x in img[:M])


def _pair(dev):
    fam = GC.families()[CASE["family"]]
    decs = [GC.make(fam, dev).train() for _ in range(2)]
    return fam, decs, fam.features()[:N_IMG].to(dev)


@gpu
@pytest.mark.parametrize("baseline", ["greedy", "mean"])
def test_device_route_is_the_host_route(dev, monkeypatch, baseline):
    caps, end, refs = _restated()
    fam, (dec_h, dec_d), f = _pair(dev)
    seed = GC.SEEDS[CASE["id"]]
    corpus = metrics.CiderCorpus(refs)
    dev_reward = train.DeviceCiderReward(refs, corpus)
    host_reward = train.cider_reward(refs, corpus)
    kw = dict(samples=M, baseline=baseline, seed=seed, **SAMPLING, **fam.kw)
    res_h = train.self_critical_step(dec_h, torch.optim.SGD(dec_h.parameters(), lr=0.0), f, host_reward, START, end, 5.0, **kw)

    def never(self, i, tokens):
        raise AssertionError("the host reward was called on the device route")
    monkeypatch.setattr(train.DeviceCiderReward, "__call__", never)
    res_d = train.self_critical_step(dec_d, torch.optim.SGD(dec_d.parameters(), lr=0.0), f, dev_reward, START, end, 5.0, **kw)
    ops.check_device_errors()
    assert set(res_d) == set(res_h)
    assert all(torch.is_tensor(res_d[k]) and res_d[k].is_cuda and res_d[k].dim() == 0 for k in res_d)
    print("%s: host %s" % (baseline, {k: float(v) for k, v in res_h.items()}))
    print("%s: device %s" % (baseline, {k: float(v) for k, v in res_d.items()}))
    assert int(res_d["zero_rows"]) == res_h["zero_rows"]
    for k in ("reward_mean", "baseline_mean"):
        assert abs(float(res_d[k]) - res_h[k]) <= REL * abs(res_h[k]), k
    # the drawn captions are the restatement's, so the host's rewards and advantages can be restated here
    r = [[metrics.sentence_cider_d(corpus, refs[i], q) for q in img] for i, img in enumerate(caps)]
    assert res_h["reward_mean"] == pytest.approx(sum(x for img in r for x in img[:M]) / (N_IMG * M), rel=1e-12)
    if baseline == "greedy":
        adv = [x - img[M] for img in r for x in img[:M]]
    else:
        adv = [x - (sum(img[:M]) - x) / (M - 1) for img in r for x in img[:M]]
    # The loss is -(1 / W) sum_r adv_r logp_r over the W words of the captions. Both routes run the same kernels on the same
    # captions; what differs is adv. A CIDEr-D reward lies in [0, 10], so in float32 its ulp is at most 2^-20 (that of [8, 16))
    # and its rounding on the device is off by at most 2^-21 -- not the 2^-25 of a BLEU in [0, 1]. So is the baseline's (a
    # rounded reward, or an fp64 mean of rounded rewards); the host rounds r - b to float32 once (|r - b| <= 10: 2^-21), the
    # device too: |delta adv_r| <= 4 2^-21 = 2^-19 per caption, hence |delta loss| <= 2^-19 sum_r |logp_r| / W. The float32
    # accumulation of either route adds at most (rows + 2) 2^-24 sum_r |adv_r logp_r| / W (a sum of W terms and a division).
    drawn = [img[:M] for img in caps]
    logp = dec_h.score_captions(f, drawn, **fam.kw).double().abs().cpu().tolist()
    words = sum(len(q) - 1 for img in drawn for q in img)
    bound = (2.0 ** -19 * sum(logp) + 2 * (words + 2) * 2.0 ** -24 * sum(abs(a) * l for a, l in zip(adv, logp))) / words
    diff = abs(res_d["loss"].item() - res_h["loss"].item())
    print("loss host %.9g device %.9g: difference %.3g, bound %.3g" % (res_h["loss"].item(), res_d["loss"].item(), diff, bound))
    assert diff <= bound


LEARN_V, LEARN_START, LEARN_END = 11, 1, 2
LEARN_REF = [LEARN_START, 5, 5, 7, 5, LEARN_END]


def _learning_corpus():
    """The four images of the learning test (one shared reference) and 28 seeded random reference sets over the same 11
    words, so that the reference's n-grams have a non-zero idf."""
    return metrics.CiderCorpus([[LEARN_REF]] * 4 + KC.random_corpus(28, LEARN_V, seed=4, lo=4, hi=8, max_refs=2))


def test_the_learning_reference_scores_ten():
    corpus = _learning_corpus()
    assert corpus.N == 32 and all(corpus.idf(tuple(LEARN_REF[i:i + 2])) > 0 for i in range(5))
    assert metrics.sentence_cider_d(corpus, [LEARN_REF], LEARN_REF) == pytest.approx(10.0, rel=1e-12)
    assert train.DeviceCiderReward([[LEARN_REF]] * 4, corpus)(2, LEARN_REF) == pytest.approx(10.0, rel=1e-12)
    assert metrics.sentence_cider_d(corpus, [LEARN_REF], [LEARN_START, 5, 7, LEARN_END]) < 10.0


@gpu
def test_self_critical_training_on_the_device_route_raises_cider(dev):
    """tests/test_self_critical_device_gpu.py's learning test with DeviceCiderReward: 40 steps of Adam at lr 0.01,
    baseline='mean', 4 samples of 4 images, seeds 0..39. The mean CIDEr-D of 256 captions drawn with one fixed evaluation
    seed rises (the values are printed)."""
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.optim import Adam
    V, start, end = LEARN_V, LEARN_START, LEARN_END
    dec = DecoderFactoredLSTMAtt(32, 24, 64, 32, V, 1, feature_size=512, dropout=0.0, max_seq_length=8)
    dec.load_state_dict(synthetic.decoder_state(dec.state_dict(), seed=6, bias_range=0.05))
    dec.to(dev).train()
    f = (torch.randn(4, 4, 512, generator=torch.Generator().manual_seed(6)).abs() * 0.5).to(dev)
    reward = train.DeviceCiderReward([[LEARN_REF]] * 4, _learning_corpus())

    def mean_reward():
        _, ids, _ = dec.sample_random(f, start, end, samples=64, seed=12345, device=True)
        return reward.rows(ids, start, end, 64)[0].double().mean().item()

    before = mean_reward()
    opt = Adam(dec.parameters(), lr=0.01)
    for seed in range(40):
        train.self_critical_step(dec, opt, f, reward, start, end, 5.0, samples=4, baseline="mean", seed=seed)
    ops.check_device_errors()
    after = mean_reward()
    print("mean CIDEr-D of 256 captions: %.4f before, %.4f after 40 steps" % (before, after))
    assert after > before
