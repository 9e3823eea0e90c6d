"""fp64 restatement of the policy-gradient loss on sampled captions (csrc/policy_loss.hip, capnet.ops.policy_loss,
capnet.train.policy_step / self_critical_step). TEST INFRASTRUCTURE. The reference project has no reward-based training:
nothing here is reference-pinned; the decoder forwards underneath are (oracle.decoders_ref and the restatements of the
stacked decoders under tests/).

  loss = -(1/N) sum over packed rows i of adv[cap(i)] * log_softmax(logits)[i, target_i]      N = sum(lengths)
Rows are in pack_padded_sequence order: step t holds the captions longer than t, in the batch's (descending-length) order.
"""
import torch

from oracle import decoders_ref as D


def row_captions(lengths):
    """LongTensor [N]: the caption of every packed row."""
    return torch.tensor([b for n in D.batch_sizes(lengths) for b in range(n)], dtype=torch.long)


def row_logp(logits, targets):
    """fp64 log-probability of every packed row's target."""
    return torch.log_softmax(logits.double(), dim=1).gather(1, targets.view(-1, 1)).squeeze(1)


def policy_loss(logits, targets, adv, lengths):
    """-(adv[cap] * log_softmax(logits)[target]).sum() / N in fp64 (differentiable in logits)."""
    adv = torch.as_tensor(adv, dtype=torch.float64)
    return -(adv[row_captions(lengths)] * row_logp(logits, targets)).sum() / logits.shape[0]


def caption_logp(logits, targets, lengths):
    """fp64 [B]: every caption's log-probability, the sum of its rows."""
    out = torch.zeros(len(lengths), dtype=torch.float64)
    return out.index_add(0, row_captions(lengths), row_logp(logits, targets).detach())


def dlogits(logits, targets, adv, lengths):
    """fp64 gradient of policy_loss in the logits."""
    x = logits.double().clone().requires_grad_(True)
    policy_loss(x, targets, adv, lengths).backward()
    return x.grad


def sorted_batch(captions):
    """Token lists [start, w_1 .. w_j] -> (order, inputs [B, T], lengths, targets): the teacher-forced batch restated on
    torch -- a stable descending sort by length, padded rows, oracle.decoders_ref.packed_targets."""
    order = sorted(range(len(captions)), key=lambda r: len(captions[r]), reverse=True)
    lengths = [len(captions[r]) - 1 for r in order]
    full = torch.zeros(len(captions), lengths[0] + 1, dtype=torch.long)
    for i, r in enumerate(order):
        full[i, :len(captions[r])] = torch.tensor(captions[r], dtype=torch.long)
    return order, full[:, :-1].contiguous(), lengths, D.packed_targets(full[:, 1:], lengths)


def mean_baseline(rewards):
    """rewards [image][sample] -> for every sample the mean reward of the image's other samples."""
    return [[sum(r for k, r in enumerate(row) if k != j) / (len(row) - 1) for j in range(len(row))] for row in rewards]
