"""The host half of the policy-gradient step (no GPU): the fp64 restatement of the loss against a hand computation,
pack_samples, the ready-made BLEU reward, the 'mean' baseline, and the new symbols of the C ABI."""
import math
import os
import re

import pytest
import torch

import capnet
import policy_cases as PC
import policy_ref as PR
from capnet import _lib, decode, train
from oracle import decoders_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_policy_ref_matches_hand_computation():
    # captions of 2 and 1 words: packed rows (step 0: caption 0, caption 1), (step 1: caption 0); V = 3
    logits = torch.tensor([[0.0, math.log(2.0), 0.0],          # caption 0, word 1: softmax = (1/4, 1/2, 1/4)
                           [math.log(3.0), 0.0, 0.0],          # caption 1, word 1: softmax = (3/5, 1/5, 1/5)
                           [0.0, 0.0, 0.0]], dtype=torch.float64)   # caption 0, word 2: softmax = (1/3, 1/3, 1/3)
    targets = torch.tensor([1, 2, 0])
    adv, lengths = [2.0, -0.5], [2, 1]
    assert PR.row_captions(lengths).tolist() == [0, 1, 0]
    want = -(2.0 * math.log(1 / 2) - 0.5 * math.log(1 / 5) + 2.0 * math.log(1 / 3)) / 3
    assert PR.policy_loss(logits, targets, adv, lengths).item() == pytest.approx(want, rel=1e-14)
    logp = PR.caption_logp(logits, targets, lengths)
    assert logp.tolist() == pytest.approx([math.log(1 / 2) + math.log(1 / 3), math.log(1 / 5)], rel=1e-14)
    # d loss / d logits[i] = (softmax_i - onehot_i) * adv[cap(i)] / N
    g = PR.dlogits(logits, targets, adv, lengths)
    want_g = torch.tensor([[1 / 4, 1 / 2 - 1, 1 / 4], [3 / 5, 1 / 5, 1 / 5 - 1], [1 / 3 - 1, 1 / 3, 1 / 3]], dtype=torch.float64)
    want_g = want_g * torch.tensor([[2.0], [-0.5], [2.0]], dtype=torch.float64) / 3
    assert (g - want_g).abs().max().item() < 1e-15
    # every advantage 1: the mean cross entropy
    ce = torch.nn.functional.cross_entropy(logits, targets)
    assert PR.policy_loss(logits, targets, [1.0, 1.0], lengths).item() == pytest.approx(ce.item(), rel=1e-14)


def test_pack_samples_hand_cases():
    S, E = 1, 2
    # equal lengths keep their order; a caption of one word [start, end]; one without <end>
    caps = [[S, 5, E], [S, E], [S, 7, 8, 9], [S, 6, E]]
    inputs, lengths, targets, order = decode.pack_samples(caps)
    assert order == [2, 0, 3, 1] and lengths == [3, 2, 2, 1]
    assert inputs.dtype == torch.int64 and inputs.tolist() == [[S, 7, 8], [S, 5, 0], [S, 6, 0], [S, 0, 0]]
    assert targets.dtype == torch.int64 and targets.tolist() == [7, 5, 6, E, 8, E, E, 9]
    # a single caption
    inputs, lengths, targets, order = decode.pack_samples([[S, 4, 3, E]])
    assert order == [0] and lengths == [3] and inputs.tolist() == [[S, 4, 3]] and targets.tolist() == [4, 3, E]
    # all equal: the identity
    assert decode.pack_samples([[S, 4, E], [S, 5, E], [S, 6, E]])[3] == [0, 1, 2]
    for bad in ([], [[S]], [[S, 4, E], []]):
        with pytest.raises(capnet.CapnetError):
            decode.pack_samples(bad)


def test_pack_samples_matches_the_oracles_packing():
    g = torch.Generator().manual_seed(5)
    for trial in range(20):
        B = int(torch.randint(1, 9, (1,), generator=g))
        caps = [[1] + torch.randint(2, 50, (int(torch.randint(1, 7, (1,), generator=g)),), generator=g).tolist() for _ in range(B)]
        inputs, lengths, targets, order = decode.pack_samples(caps)
        assert sorted(order) == list(range(B)) and lengths == sorted(lengths, reverse=True)
        assert all(order[i] < order[i + 1] for i in range(B - 1) if lengths[i] == lengths[i + 1])      # stable
        full = torch.zeros(B, lengths[0] + 1, dtype=torch.long)
        for i, r in enumerate(order):
            full[i, :len(caps[r])] = torch.tensor(caps[r])
        assert torch.equal(targets, D.packed_targets(full[:, 1:], lengths))
        o2, i2, l2, t2 = PR.sorted_batch(caps)
        assert o2 == order and l2 == lengths and torch.equal(t2, targets)
        for i, l in enumerate(lengths):     # tokens[:-1], then padding (the restatement's rows keep their last token there:
            assert torch.equal(inputs[i, :l], full[i, :l]) and not inputs[i, l:].any()      # a column no step reads)
            assert torch.equal(i2[i, :l], inputs[i, :l])


def test_flat_captions_takes_both_forms():
    nested = [[([1, 4, 2], -0.5), ([1, 5, 6, 2], -1.5)], [([1, 7, 2], -0.1), ([1, 2], -0.2)]]
    tokens, image = decode.flat_captions(nested)
    assert tokens == [[1, 4, 2], [1, 5, 6, 2], [1, 7, 2], [1, 2]] and image == [0, 0, 1, 1]
    assert decode.flat_captions([[q for q, _ in row] for row in nested]) == (tokens, image)     # nested, without the logprobs
    assert decode.flat_captions(tokens) == (tokens, [0, 1, 2, 3])                               # flat: caption r on row r


def test_bleu_reward_is_corpus_bleu_of_one_sentence():
    from capnet.metrics import corpus_bleu
    ref = [[1, 2, 3, 4, 5, 6, 7]]                                   # the example of tests/test_oracle_cpu.py
    hyp = [1, 2, 3, 4, 5, 9, 7]
    reward = train.bleu_reward([[[9, 9]], ref])
    assert reward(1, hyp) == corpus_bleu([ref], [hyp]) == pytest.approx((6 / 7 * 4 / 6 * 3 / 5 * 2 / 4) ** 0.25)
    assert reward(1, ref[0]) == pytest.approx(1.0) and reward(0, hyp) == corpus_bleu([[[9, 9]]], [hyp])
    refs = [[1, 5, 6, 7, 1, 8, 9], [10, 6, 11, 5, 7, 1, 8]]
    assert train.bleu_reward([refs], weights=(1.0,))(0, [1] * 7) == pytest.approx(2 / 7)


def test_mean_baseline_hand_case():
    rewards = [[1.0, 2.0, 6.0], [0.5, 0.5, 0.5], [3.0, -1.0]]
    base = train.mean_baseline(rewards)
    assert base == [[4.0, 3.5, 1.5], [0.5, 0.5, 0.5], [-1.0, 3.0]]
    assert base == PR.mean_baseline(rewards)
    # advantages r - mean(others) = (m r - total) / (m - 1): they sum to 0 per image
    for rr, bb in zip(rewards, base):
        assert sum(r - b for r, b in zip(rr, bb)) == pytest.approx(0.0, abs=1e-15)
    with pytest.raises(ValueError):
        train.mean_baseline([[1.0]])


def test_mean_baseline_needs_two_samples():
    # raised before anything is decoded: no decoder, no GPU
    with pytest.raises(ValueError):
        train.self_critical_step(None, None, None, lambda i, q: 0.0, 1, 2, 5.0, samples=1, baseline="mean")
    with pytest.raises(ValueError):
        train.self_critical_step(None, None, None, lambda i, q: 0.0, 1, 2, 5.0, baseline="median")


def test_abi_declares_the_policy_loss_symbols():
    src = open(os.path.join(ROOT, "include", "capnet.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = capnet.lib()
    for name, nargs in (("capnet_policy_xent_fwd", 15), ("capnet_policy_xent_bwd", 14)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert lib.capnet_abi_version() == 1
    # the host-side argument checks need no GPU: more steps than the step table holds, batch_sizes that do not sum to N
    import ctypes as C
    one = C.c_float()
    p = C.cast(C.pointer(one), C.c_void_p)
    bs = _lib.int_array([1] * 129)
    assert lib.capnet_policy_xent_fwd(p, 4, 129, 4, p, p, 1, bs, 129, p, p, p, p, p, None) != 0
    assert b"steps" in lib.capnet_last_error()
    assert lib.capnet_policy_xent_fwd(p, 4, 5, 4, p, p, 2, _lib.int_array([2, 1]), 2, p, p, p, p, p, None) != 0
    assert b"batch_sizes" in lib.capnet_last_error()


def test_kernel_cases_cover_what_they_claim():
    for name, (lengths, V) in PC.KERNEL.items():
        assert lengths == sorted(lengths, reverse=True) and min(lengths) >= 1
        adv = PC.advantages(len(lengths))
        if len(lengths) > 1:
            assert any(a == 0.0 for a in adv) and any(a < 0 for a in adv) and any(a > 0 for a in adv)
            assert lengths[-1] == 1                                   # a caption of one word
    assert sum(PC.KERNEL["n300_v8192"][0]) == 300 and sum(PC.KERNEL["n40_v1000"][0]) == 40
