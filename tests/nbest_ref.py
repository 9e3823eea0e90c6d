"""The reference side of the n-best tests (tests/test_nbest_cpu.py, tests/test_nbest_gpu.py). TEST INFRASTRUCTURE.

  * key / rank / min_gap / reordered: the rule itself, on a completed list [(score, tokens)] in completion order. The key
    is score / (len(tokens) - 1)^penalty (len - 1: the generated words, <end> included), at penalty 0 the score itself;
    best first, ties to the earlier completion.
  * nbest_search: device_beam_ref.beam_margin's fp64 loop keeping (score, sequence) of every completion, the margin as
    beam_margin computes it, and the largest |logit| it met.
  * NBestBeam: att_alpha_ref.TracedBeam (the fixed-slot model with row histories) with nbest(length_penalty) and
    nbest_rows(max_steps, length_penalty): what capnet_beam_nbest / capnet_beam_nbest_traced write.
"""
import torch
import torch.nn.functional as Fn

from att_alpha_ref import TracedBeam


def key(score, tokens, penalty):
    return score if penalty == 0 else score / float(len(tokens) - 1) ** penalty


def order(done, penalty):
    """Indices into `done`, best first."""
    keys = [key(s, q, penalty) for s, q in done]
    return sorted(range(len(done)), key=lambda j: (-keys[j], j))


def rank(done, penalty):
    """[(tokens, score)] best first."""
    return [(list(done[j][1]), done[j][0]) for j in order(done, penalty)]


def min_gap(done, penalty):
    """The smallest gap in the key between neighbours of the ranked list (inf for fewer than two)."""
    keys = sorted((key(s, q, penalty) for s, q in done), reverse=True)
    return min((a - b for a, b in zip(keys, keys[1:])), default=float("inf"))


def reordered(done, penalty):
    return order(done, penalty) != list(range(len(done)))


class Search:
    """done: [(score, tokens)] in completion order (by step, then rank); margin: beam_margin's; scale: the largest |logit|."""

    def __init__(self, done, margin, scale):
        self.done, self.margin, self.scale = done, margin, scale

    def gap(self, penalty):
        return min_gap(self.done, penalty)

    def nbest(self, penalty):
        return rank(self.done, penalty)


def nbest_search(step_fn, state, vocab_size, start_token, end_token, k, max_seq_length):
    """device_beam_ref.beam_margin's loop (oracle.beam_ref._beam's search) -> Search."""
    V = vocab_size
    words = torch.LongTensor([[start_token]] * k)
    seqs = [[int(start_token)] for _ in range(k)]
    top = torch.zeros(k, 1, dtype=torch.float64)
    margin, done, step, scale = float("inf"), [], 1, 0.0
    while True:
        out, state = step_fn(words, state)
        scale = max(scale, float(out.abs().max()))
        scores = top.expand_as(out) + Fn.log_softmax(out, dim=1)
        flat = scores[0] if step == 1 else scores.view(-1)
        best, idx = flat.topk(min(k + 1, flat.numel()), 0, True, True)
        if best.numel() > k:
            margin = min(margin, float(best[k - 1] - best[k]))
        best, idx = best[:k], idx[:k]
        prev, nxt = (idx // V).tolist(), (idx % V).tolist()
        seqs = [seqs[p] + [w] for p, w in zip(prev, nxt)]
        keep = [i for i, w in enumerate(nxt) if w != end_token]
        done += [(float(best[i]), seqs[i]) for i in range(k) if i not in keep]
        k = len(keep)
        if k == 0 or step > max_seq_length:
            break
        seqs = [seqs[i] for i in keep]
        state = tuple(s[torch.tensor(prev)[keep]] for s in state)
        top = best[keep].unsqueeze(1)
        words = torch.tensor(nxt)[keep].unsqueeze(1)
        step += 1
    by_score = sorted((s for s, _ in done), reverse=True)
    if len(by_score) > 1:
        margin = min(margin, by_score[0] - by_score[1])
    return Search(done, margin, scale)


class NBestBeam(TracedBeam):
    def completed(self, i):
        """Image i's (score, tokens) in completion order."""
        return [(s, q) for s, q, _ in self.done[i]]

    def nbest(self, length_penalty):
        """Per image [(tokens, score)], best first."""
        return [rank(self.completed(i), length_penalty) for i in range(self.n)]

    def nbest_rows(self, max_steps, length_penalty):
        """capnet_beam_nbest_traced's rows [n][k][max_steps]: i k + slot, -1 past length - 1 and past the count."""
        out = []
        for i in range(self.n):
            rows = []
            for j in order(self.completed(i), length_penalty):
                path = self.done_paths[i][j][1:]
                rows.append([i * self.k + s for s in path] + [-1] * (max_steps - len(path)))
            out.append(rows + [[-1] * max_steps] * (self.k - len(rows)))
        return out

    def events(self, max_steps):
        """DeviceBeam.events and what the n-best tests need of their tables."""
        ev = super().events(max_steps)
        for i in range(self.n):
            d = self.completed(i)
            scores = [s for s, _ in d]
            if len(d) == self.k:
                ev.add("all k completed")
            if reordered(d, 0.0):
                ev.add("completion order differs from score order")
            if any(a == b for j, a in enumerate(scores) for b in scores[j + 1:]):
                ev.add("two equal scores")
            if d and order(d, 0.0)[0] != order(d, 1.0)[0]:
                ev.add("the penalty changes rank 0")
        return ev
