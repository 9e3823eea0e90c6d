"""self_critical_step with its reward and advantages on the device (capnet.train.DeviceBleuReward) against the same step with
a host reward (capnet.train.bleu_reward), on two copies of one tiny attention decoder at one seed: greedy_row_cases'
two-layer attention family at 3 images x 5 samples, whose decode the fp64 restatement reproduces token for token
(tests/test_greedy_row_cpu.py), so the references can be built from the restatement's rows on the CPU. Its end token is
one that the greedy caption of EVERY image reaches within max_seq_length: only there is the host route's baseline, the
width-1 beam, the greedy caption (asserted on the CPU)."""
import pytest
import torch

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
    """(the restated captions per image -- M drawn and the greedy one --, the end token, the references): per image the
    first drawn caption itself and the first words of two more and of the greedy one, closed by <end>: a sample scores 1.0,
    those that share four words in a row with a reference something, the others 0 unless smoothed."""
    ids, logp, _ = GC.reference(CASE)
    end = GC.end_token(CASE)
    caps = [[q for q, _ in img] for img in R.cut(ids, logp, N_IMG, M + 1, START, end)]
    refs = [[img[0], img[1][:4] + [end], img[2][:5] + [end], img[M][:3] + [end]] for img in caps]
    return caps, end, refs


def test_references_spread_the_rewards():
    """On the CPU, from the restatement: per smoothing the rewards are neither all 0 nor all equal, and under the greedy
    baseline some advantage is 0 and some is not."""
    caps, end, refs = _restated()
    ids = GC.reference(CASE)[0]
    assert all(end in ids[row].tolist() for row in GC.greedy_rows(CASE))
    for smooth in (0, 1):
        r = [[metrics.sentence_bleu(refs[i], q, smooth=smooth) for q in img] for i, img in enumerate(caps)]
        flat = [x for img in r for x in img[:M]]
        print("smooth %d rewards %s" % (smooth, [[round(x, 3) for x in img] for img in r]))
        assert any(x > 0 for x in flat) and len(set(flat)) > 3
        adv = [x - img[M] for img in r for x in img[:M]]
        assert any(a != 0 for a in adv)


def _pair(dev):
    fam = GC.families()[CASE["family"]]
    decs = [GC.make(fam, dev).train() for _ in range(2)]
    return fam, decs, fam.features()[:N_IMG].to(dev)


@gpu
@pytest.mark.parametrize("baseline", ["greedy", "mean"])
@pytest.mark.parametrize("smooth", [0, 1])
def test_device_route_is_the_host_route(dev, monkeypatch, baseline, smooth):
    caps, end, refs = _restated()
    fam, (dec_h, dec_d), f = _pair(dev)
    seed = GC.SEEDS[CASE["id"]]
    dev_reward = train.DeviceBleuReward(refs, smooth=smooth)
    host_reward = train.bleu_reward(refs) if smooth == 0 else (lambda i, tokens: metrics.sentence_bleu(refs[i], tokens, smooth=1))
    kw = dict(samples=M, baseline=baseline, seed=seed, **SAMPLING, **fam.kw)
    res_h = train.self_critical_step(dec_h, torch.optim.SGD(dec_h.parameters(), lr=0.0), f, host_reward, START, end, 5.0, **kw)

    def never(self, i, tokens):
        raise AssertionError("the host reward was called on the device route")
    monkeypatch.setattr(train.DeviceBleuReward, "__call__", never)
    res_d = train.self_critical_step(dec_d, torch.optim.SGD(dec_d.parameters(), lr=0.0), f, dev_reward, START, end, 5.0, **kw)
    ops.check_device_errors()
    assert set(res_d) == set(res_h)
    assert all(torch.is_tensor(res_d[k]) and res_d[k].is_cuda and res_d[k].dim() == 0 for k in res_d)
    print("%s smooth %d: host %s" % (baseline, smooth, {k: float(v) for k, v in res_h.items()}))
    print("%s smooth %d: device %s" % (baseline, smooth, {k: float(v) for k, v in res_d.items()}))
    assert int(res_d["zero_rows"]) == res_h["zero_rows"]
    for k in ("reward_mean", "baseline_mean"):
        assert abs(float(res_d[k]) - res_h[k]) <= REL * abs(res_h[k]), k
    # the drawn captions are the restatement's, so the host's rewards and advantages can be restated here
    r = [[metrics.sentence_bleu(refs[i], q, smooth=smooth) for q in img] for i, img in enumerate(caps)]
    assert res_h["reward_mean"] == pytest.approx(sum(x for img in r for x in img[:M]) / (N_IMG * M), rel=1e-12)
    if baseline == "greedy":
        adv = [x - img[M] for img in r for x in img[:M]]
    else:
        adv = [x - (sum(img[:M]) - x) / (M - 1) for img in r for x in img[:M]]
    # The loss is -(1 / W) sum_r adv_r logp_r over the W words of the captions. Both routes run the same kernels on the same
    # captions; what differs is adv. A reward is at most 1, so its float32 rounding on the device is off by at most 2^-25, and
    # so is the baseline's (a reward, or a mean of rewards); the host rounds r - b to float32 once (|r - b| <= 1: 2^-25), the
    # device too: |delta adv_r| <= 4 2^-25 = 2^-23 per caption, hence |delta loss| <= 2^-23 sum_r |logp_r| / W. The float32
    # accumulation of either route adds at most (rows + 2) 2^-24 sum_r |adv_r logp_r| / W (a sum of W terms and a division).
    drawn = [img[:M] for img in caps]
    logp = dec_h.score_captions(f, drawn, **fam.kw).double().abs().cpu().tolist()
    words = sum(len(q) - 1 for img in drawn for q in img)
    bound = (REL * sum(logp) + 2 * (words + 2) * 2.0 ** -24 * sum(abs(a) * l for a, l in zip(adv, logp))) / words
    diff = abs(res_d["loss"].item() - res_h["loss"].item())
    print("loss host %.9g device %.9g: difference %.3g, bound %.3g" % (res_h["loss"].item(), res_d["loss"].item(), diff, bound))
    assert diff <= bound


@gpu
def test_policy_step_takes_device_advantages_bit_for_bit(dev):
    caps, end, _ = _restated()
    fam, (dec_a, dec_b), f = _pair(dev)
    drawn = [img[:M] for img in caps]
    adv = torch.randn(N_IMG * M, generator=torch.Generator().manual_seed(2))
    adv[3] = 0.0
    la, pa = train.policy_step(dec_a, torch.optim.SGD(dec_a.parameters(), lr=0.0), f, drawn, adv.tolist(), 5.0, **fam.kw)
    lb, pb = train.policy_step(dec_b, torch.optim.SGD(dec_b.parameters(), lr=0.0), f, drawn, adv.to(dev), 5.0, **fam.kw)
    lc, pc = train.policy_step(dec_b, torch.optim.SGD(dec_b.parameters(), lr=0.0), f, drawn, adv, 5.0, **fam.kw)     # a host tensor
    ops.check_device_errors()
    assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(la, lc) and torch.equal(pa, pc)
    for (ka, a), (kb, b) in zip(dec_a.named_parameters(), dec_b.named_parameters()):
        assert (a.grad is None) == (b.grad is None) and (a.grad is None or torch.equal(a.grad, b.grad)), ka
    with pytest.raises(ops.CapnetError):
        train.policy_step(dec_b, torch.optim.SGD(dec_b.parameters(), lr=0.0), f, drawn, adv[:-1].to(dev), 5.0, **fam.kw)


@gpu
def test_self_critical_training_on_the_device_route_raises_bleu(dev):
    """tests/test_policy_gpu.py's learning test with its toy reward swapped for add-one BLEU against one fixed reference, the
    rewards and advantages never on the host: 40 steps of Adam at lr 0.01, baseline='mean', 4 samples of 4 images, seeds
    0..39. The mean reward of 256 captions drawn with one fixed evaluation seed rises (the values are printed)."""
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.optim import Adam
    V, start, end = 11, 1, 2
    dec = DecoderFactoredLSTMAtt(32, 24, 64, 32, V, 1, feature_size=512, dropout=0.0, max_seq_length=8)
    dec.load_state_dict(synthetic.decoder_state(dec.state_dict(), seed=6, bias_range=0.05))
    dec.to(dev).train()
    f = (torch.randn(4, 4, 512, generator=torch.Generator().manual_seed(6)).abs() * 0.5).to(dev)
    reward = train.DeviceBleuReward([[[start, 5, 5, 7, 5, end]]] * 4, smooth=1)

    def mean_reward():
        _, ids, _ = dec.sample_random(f, start, end, samples=64, seed=12345, device=True)
        return reward.rows(ids, start, end, 64)[0].double().mean().item()

    before = mean_reward()
    opt = Adam(dec.parameters(), lr=0.01)
    for seed in range(40):
        train.self_critical_step(dec, opt, f, reward, start, end, 5.0, samples=4, baseline="mean", seed=seed)
    ops.check_device_errors()
    after = mean_reward()
    print("mean add-one BLEU of 256 captions: %.4f before, %.4f after 40 steps" % (before, after))
    assert after > before
