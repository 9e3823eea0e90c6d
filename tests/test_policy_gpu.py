"""The policy-gradient step on sampled captions, on the GPU (tests/policy_ref.py restates the loss in fp64):

  T1  every advantage 1.0: ops.policy_loss is ops.cross_entropy, loss and dlogits, bit for bit
  T2  the loss kernels against fp64: both signs, exact zeros (written as zeros, their logits never read), a caption of one word
  T3  capnet.train.policy_step against the fp64 oracles of all eight image decoders
  T4  score_captions against the sampler: the sequence kernels against the one-call decode step
  T5  self_critical_step is sample_random + the baseline + policy_step
  T6  forty steps raise the reward they are given
"""
import random

import pytest
import torch

import policy_cases as PC
import policy_ref as PR
import sample_random_cases as C
import sample_random_ref as R
from capnet import CapnetError, decode, ops, synthetic, train
from helpers import rel_err
from oracle import decoders_ref as D

pytestmark = pytest.mark.gpu


def _run_loss(dev, logits, targets, adv, lengths):
    """(loss, caption_logp, dlogits) of ops.policy_loss on the device."""
    x = logits.to(dev).requires_grad_(True)
    loss, logp = ops.policy_loss(x, targets.to(dev), torch.tensor(adv, dtype=torch.float32, device=dev), D.batch_sizes(lengths))
    assert not logp.requires_grad and tuple(logp.shape) == (len(lengths),) and loss.dim() == 0
    loss.backward()
    return loss.detach(), logp, x.grad


def _logp_close(logp, ref):
    err = (logp.double().cpu() - ref).abs()
    return bool((err <= 1e-6 * (1 + ref.abs())).all()), err.max().item()


# ---- T1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.IDENTITY)
def test_unit_advantages_give_the_cross_entropy_bit_for_bit(dev, name):
    logits, targets, lengths = PC.kernel_inputs(name)
    loss, logp, grad = _run_loss(dev, logits, targets, [1.0] * len(lengths), lengths)
    y = logits.to(dev).requires_grad_(True)
    ce = ops.cross_entropy(y, targets.to(dev))
    ce.backward()
    ops.check_device_errors()
    assert torch.equal(loss, ce.detach()), (loss.item(), ce.item())
    assert torch.equal(grad, y.grad)
    ok, err = _logp_close(logp, PR.caption_logp(logits, targets, lengths))
    print("%s: caption_logp error %.3g" % (name, err))
    assert ok, err


# ---- T2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.KERNEL))
def test_policy_loss_matches_fp64(dev, name):
    logits, targets, lengths = PC.kernel_inputs(name)
    adv = PC.advantages(len(lengths))
    loss, logp, grad = _run_loss(dev, logits, targets, adv, lengths)
    ops.check_device_errors()
    ref = PR.policy_loss(logits, targets, adv, lengths).item()
    ok, lerr = _logp_close(logp, PR.caption_logp(logits, targets, lengths))
    gerr = (grad.double().cpu() - PR.dlogits(logits, targets, adv, lengths)).abs().max().item()
    print("%s: loss %.9g (fp64 %.9g, rel %.3g), caption_logp error %.3g, dlogits error %.3g"
          % (name, loss.item(), ref, abs(loss.item() - ref) / max(abs(ref), 1e-30), lerr, gerr))
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref)
    assert ok, lerr
    assert gerr <= 1e-6
    # rows of advantage 0 are exactly 0.0 -- and their logits are not read: NaN there changes nothing
    cap = PR.row_captions(lengths)
    zero = torch.tensor([adv[c] == 0.0 for c in cap.tolist()])
    assert bool((grad.cpu()[zero] == 0.0).all())
    if zero.any():
        poisoned = logits.clone()
        poisoned[zero] = float("nan")
        loss2, logp2, grad2 = _run_loss(dev, poisoned, targets, adv, lengths)
        ops.check_device_errors()
        assert bool((grad2.cpu()[zero] == 0.0).all())
        assert torch.equal(grad2.cpu()[~zero], grad.cpu()[~zero]) and torch.equal(loss2, loss)
        live = torch.tensor([a != 0.0 for a in adv])
        assert torch.equal(logp2.cpu()[live], logp.cpu()[live])


@pytest.mark.parametrize("bad", [-1, 203])
def test_policy_loss_flags_a_target_out_of_range(dev, bad):
    logits, targets, lengths = PC.kernel_inputs("n7_v203")
    ops.check_device_errors()
    targets = targets.clone()
    targets[3] = bad
    ops.policy_loss(logits.to(dev), targets.to(dev), torch.ones(len(lengths), device=dev), D.batch_sizes(lengths))
    with pytest.raises(CapnetError, match="target out of range"):
        ops.check_device_errors()
    ops.check_device_errors()           # the word is cleared


def test_policy_loss_refuses_mismatched_operands(dev):
    logits, targets, lengths = PC.kernel_inputs("n7_v203")
    x, t, ones = logits.to(dev), targets.to(dev), torch.ones(3, device=dev)
    for args in ((x, t, ones[:2], [3, 2, 1, 1]), (x, t, ones, [3, 2, 1]), (x, t[:6], ones, [3, 2, 1, 1]), (x, t, ones, [3, 1, 2, 1]),
                 (x, t.int(), ones, [3, 2, 1, 1])):
        with pytest.raises(CapnetError):
            ops.policy_loss(*args)


# ---- T3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", PC.STEP_CASES, ids=["%s-%s" % c for c in PC.STEP_CASES])
def test_policy_step_matches_oracle(dev, name, size):
    dec, p64, forward, att, mode, tokens, feats, adv = PC.decoder_case(name, size)
    dec.to(dev).train()
    # the oracle: the fp64 forward on the sorted batch, every step teacher forced, then the restated loss
    order, inputs, lengths, targets = PR.sorted_batch(tokens)
    adv_sorted = [adv[r] for r in order]
    pr = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
    logits_r = forward(pr, inputs, lengths, feats.double()[order] if att else None, [True] * lengths[0])
    loss_r = PR.policy_loss(logits_r, targets, adv_sorted, lengths)
    loss_abs = PR.policy_loss(logits_r, targets, [abs(a) for a in adv_sorted], lengths)
    names = [k for k, _ in dec.named_parameters()]
    g_ref = dict(zip(names, torch.autograd.grad(loss_r, [pr[k] for k in names], retain_graph=True, allow_unused=True)))
    g_abs = dict(zip(names, torch.autograd.grad(loss_abs, [pr[k] for k in names], allow_unused=True)))
    # the device
    fd = feats.to(dev) if att else None                 # a plain decoder does not read the features
    state = random.getstate()
    with torch.no_grad():
        i_d, l_d, t_d, o_d, f_d = decode.policy_batch(dec, fd, tokens)
        logits = decode.policy_logits(dec, i_d, l_d, f_d, mode)
    assert o_d == order and l_d == lengths and torch.equal(t_d.cpu(), targets)
    assert rel_err(logits, logits_r) < 1e-4
    opt = torch.optim.SGD(dec.parameters(), lr=0.0)
    loss, logp = train.policy_step(dec, opt, fd, tokens, adv, 1e6, mode=mode)
    ops.check_device_errors()
    assert random.getstate() == state
    print("%s %s: loss %.9g (fp64 %.9g, |adv| %.9g)" % (name, size, loss.item(), loss_r.item(), loss_abs.item()))
    assert abs(loss.item() - loss_r.item()) <= 1e-5 * abs(loss_abs.item())
    # caption_logp, in the caller's order: a word's log-probability is a logit minus the lse, each within 1e-4 of the scale
    logp_r = PR.caption_logp(logits_r, targets, lengths)
    scale = logits_r.detach().abs().max().item()
    assert not logp.requires_grad and tuple(logp.shape) == (len(tokens),)
    for i, r in enumerate(order):
        assert abs(logp[r].item() - logp_r[i].item()) <= (2e-4 * scale + 2e-6) * lengths[i], (r, logp[r].item(), logp_r[i].item())
    n = 0
    for k, prm in dec.named_parameters():
        if g_ref[k] is None:
            assert prm.grad is None, k
            continue
        assert prm.grad is not None, k
        S = g_abs[k].abs().max().item()
        err = (prm.grad.double().cpu() - g_ref[k]).abs().max().item()
        assert err <= 5e-4 * S + 1e-6, (k, err, S)
        n += 1
    assert n >= 6


# ---- T4 ---------------------------------------------------------------------------------------------------------------------
T4_CASES = [c for c in C.IMAGE_CASES if c["T"] == 1.0 and c["top_k"] == 0]


def test_t4_cases_cover_the_decoder_kinds():
    fams = {c["family"] for c in T4_CASES}
    assert "DecoderFactoredLSTM" in fams                                    # a plain factored decoder
    assert any(f.startswith("DecoderRNNAtt") for f in fams)                 # an LSTM decoder
    assert any(f.startswith("DecoderFactoredLSTMAtt") for f in fams)        # an attention decoder
    assert any(f.startswith("StackedFactoredLSTMAtt-2") for f in fams)      # a 2-layer stack


@pytest.mark.parametrize("case", T4_CASES, ids=[c["id"] for c in T4_CASES])
def test_score_captions_matches_the_sampler(dev, case):
    ids_r, logp_r, tr = C.image_reference(case)
    fam = C.families()[case["family"]]
    dec = fam.make().to(dev).eval()
    f = fam.features()[:C.IMAGES].to(dev)
    tol = R.logp_tol(tr.scale, 1.0)
    for end in (fam.V, C.early_end(ids_r)):              # never drawn: equal lengths; drawn early: unequal ones, a sort
        drawn = dec.sample_random(f, C.START, end, samples=C.SAMPLES, seed=case["seed"], **fam.kw)
        want = [s for img in R.cut(ids_r, logp_r, C.IMAGES, C.SAMPLES, C.START, end) for s in img]
        flat = [s for img in drawn for s in img]
        score = dec.score_captions(f, drawn, **fam.kw)
        assert score.dtype == torch.float32 and tuple(score.shape) == (len(flat),) and not score.requires_grad
        got = score.double().cpu().tolist()
        for r, ((q, lp), (qr, lpr)) in enumerate(zip(flat, want)):
            assert q == qr
            words = len(q) - 1
            print("%s end %d caption %d: %d words, score %.7g, sampler %.7g, fp64 %.7g" % (case["id"], end, r, words, got[r], lp, lpr))
            assert abs(got[r] - lp) <= 2 * tol * words
            assert abs(got[r] - lpr) <= tol * words
        # the flat form, caption r on row r of the features: the same tensor, in the caller's order
        tokens = [q for q, _ in flat]
        assert torch.equal(dec.score_captions(f.repeat_interleave(C.SAMPLES, 0), tokens, **fam.kw), score)
        back = list(reversed(range(len(tokens))))
        again = dec.score_captions(f.repeat_interleave(C.SAMPLES, 0)[back], [tokens[r] for r in back], **fam.kw)
        assert (again.double().cpu() - score.double().cpu()[back]).abs().max().item() <= 2 * tol * dec.max_seq_length
    ops.check_device_errors()


# ---- T5 ---------------------------------------------------------------------------------------------------------------------
def _stub_reward(i, tokens):
    """A fixed function of the image and the tokens, different for different captions of an image."""
    return ((sum((k + 3) * (w + 1) for k, w in enumerate(tokens)) * 7919 + 131 * i) % 1000003) / 1000003.0


def _grads(dec):
    return {k: (None if p.grad is None else p.grad.clone()) for k, p in dec.named_parameters()}


def _same_grads(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        assert a[k] is None or torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("family", ["DecoderFactoredLSTMAtt-p4-happy", "DecoderRNN"])
@pytest.mark.parametrize("baseline", ["greedy", "mean"])
def test_self_critical_step_is_sampling_plus_policy_step(dev, family, baseline):
    fam = C.families()[family]
    dec = fam.make().to(dev).train()
    dec.dropout.p = 0.0                                      # (DecoderRNN's family keeps the default): calls are compared bit for bit
    f = fam.features()[:C.IMAGES].to(dev)
    mode = fam.kw.get("mode")
    opt = torch.optim.SGD(dec.parameters(), lr=0.0)          # the parameters stay: every call starts from the same ones
    # temperature 0.125, seed 3: in the fp64 restatement 2 (3 for DecoderRNN) of the 8 samples are the greedy caption, every
    # draw's key gap (1.5e-2, 3.7e-2) far above sample_random_ref.need's 2e-3 -- zero rows and live rows in one batch
    kw = dict(samples=4, baseline=baseline, mode=mode, temperature=0.125, seed=3)
    res = train.self_critical_step(dec, opt, f, _stub_reward, C.START, fam.end, 5.0, **kw)
    g1 = _grads(dec)
    # the same, put together here
    drawn = dec.sample_random(f, C.START, fam.end, samples=4, temperature=0.125, seed=3, **fam.kw)
    rewards = [[_stub_reward(i, q) for q, _ in row] for i, row in enumerate(drawn)]
    if baseline == "greedy":
        greedy = dec.sample_batch(f, C.START, fam.end, k=1, **fam.kw)
        base = [[_stub_reward(i, list(g))] * 4 for i, g in enumerate(greedy)]
        same = sum(1 for i, row in enumerate(drawn) for q, _ in row if q == [int(w) for w in greedy[i]])
        print("%s: %d of %d samples are the greedy caption" % (family, same, 4 * len(drawn)))
        assert res["zero_rows"] == same and 0 < same < 4 * len(drawn)
    else:
        base = PR.mean_baseline(rewards)
    adv = [r - b for rr, bb in zip(rewards, base) for r, b in zip(rr, bb)]
    loss, _ = train.policy_step(dec, opt, f, drawn, adv, 5.0, mode=mode)
    assert torch.equal(loss, res["loss"])
    _same_grads(_grads(dec), g1)
    n = float(len(adv))
    assert res["reward_mean"] == pytest.approx(sum(map(sum, rewards)) / n) and res["baseline_mean"] == pytest.approx(sum(map(sum, base)) / n)
    assert res["advantage_abs_mean"] == pytest.approx(sum(abs(a) for a in adv) / n)
    # the same seed from the same parameters: the same step; another seed: another
    res2 = train.self_critical_step(dec, opt, f, _stub_reward, C.START, fam.end, 5.0, **kw)
    assert torch.equal(res2["loss"], res["loss"]) and {k: v for k, v in res2.items() if k != "loss"} == {k: v for k, v in res.items() if k != "loss"}
    _same_grads(_grads(dec), g1)
    res3 = train.self_critical_step(dec, opt, f, _stub_reward, C.START, fam.end, 5.0, **dict(kw, seed=12))
    assert not torch.equal(res3["loss"], res["loss"])
    ops.check_device_errors()


def test_greedy_samples_are_zero_rows(dev):
    """top_k = 1 draws the argmax: every sample is the greedy caption, every advantage 0, the loss and every gradient 0."""
    fam = C.families()["DecoderFactoredLSTMAtt-p4-happy"]
    dec = fam.make().to(dev).train()
    f = fam.features()[:1].to(dev)                           # image 0: its greedy caption ends at fam.end, by the family's construction
    opt = torch.optim.SGD(dec.parameters(), lr=0.0)
    res = train.self_critical_step(dec, opt, f, _stub_reward, C.START, fam.end, 5.0, samples=3, baseline="greedy", top_k=1, seed=0,
                                   **fam.kw)
    assert res["zero_rows"] == 3 and res["advantage_abs_mean"] == 0.0 and res["loss"].item() == 0.0
    grads = [p.grad for p in dec.parameters() if p.grad is not None]
    assert grads and all(bool((g == 0).all()) for g in grads)
    ops.check_device_errors()


# ---- T6 ---------------------------------------------------------------------------------------------------------------------
def test_self_critical_training_raises_the_reward(dev):
    """A tiny attention decoder, V = 11, reward = the share of a caption's words equal to one chosen token; Adam at lr 0.01, 40
    steps with baseline='mean', 4 samples of 4 images, seeds 0..39. The mean reward of 256 captions drawn with one fixed
    evaluation seed is strictly greater after the steps than before (no margin fixed in advance: DESIGN records the values)."""
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.optim import Adam
    V, token, start, end = 11, 5, 1, 2
    dec = DecoderFactoredLSTMAtt(32, 24, 64, 32, V, 1, feature_size=512, dropout=0.0, max_seq_length=8)
    dec.load_state_dict(synthetic.decoder_state(dec.state_dict(), seed=6, bias_range=0.05))
    dec.to(dev).train()
    f = (torch.randn(4, 4, 512, generator=torch.Generator().manual_seed(6)).abs() * 0.5).to(dev)

    def reward(i, tokens):
        return sum(1 for w in tokens[1:] if w == token) / float(len(tokens) - 1)

    def mean_reward():
        drawn = dec.sample_random(f, start, end, samples=64, seed=12345)
        return sum(reward(i, q) for i, row in enumerate(drawn) for q, _ in row) / 256.0

    before = mean_reward()
    opt = Adam(dec.parameters(), lr=0.01)
    for seed in range(40):
        train.self_critical_step(dec, opt, f, reward, start, end, 5.0, samples=4, baseline="mean", seed=seed)
    ops.check_device_errors()
    after = mean_reward()
    print("mean reward of 256 captions: %.4f before, %.4f after 40 steps" % (before, after))
    assert after > before
