"""The fp64 side of the constrained-beam-search tests (tests/test_constrained_beam_cpu.py, tests/test_constrained_beam_gpu.py).
TEST INFRASTRUCTURE.

  * constrained_search: nbest_ref.nbest_search's loop with capnet.beam.Constraints' rule applied to top + log_softmax(out)
    before topk -- the excluded candidates become -inf AFTER the log-softmax, so every surviving score is the model's own
    summed log-probability. It keeps the completed list, the largest |logit| and the margin: the gap between the k-th and
    the (k+1)-th FINITE candidate at every step, and between the two best completed scores -> nbest_ref.Search.
  * ConstrainedBeam / drive: the fixed-slot model with stored logits (nbest_ref.NBestBeam: sequences, row histories,
    completed lists) whose top-k, in fp64 with ties to the lower flat index, leaves out what the rule excludes for the
    sequence in each competing slot -- what capnet_beam_advance_constrained must select. It keeps every step's outputs and
    what every competing slot was forbidden.
  * violations: the properties of a returned caption, checked without the rule's own code.
"""
import torch
import torch.nn.functional as Fn

from capnet.beam import banned_words
from nbest_ref import NBestBeam, Search


def constrained_search(step_fn, state, vocab_size, start_token, end_token, k, max_seq_length, constraints):
    V = vocab_size
    words = torch.LongTensor([[start_token]] * k)
    seqs = [[int(start_token)] for _ in range(k)]
    top = torch.zeros(k, 1, dtype=torch.float64)
    margin, done, step, scale = float("inf"), [], 1, 0.0
    while True:
        out, state = step_fn(words, state)
        scale = max(scale, float(out.abs().max()))
        scores = top.expand_as(out) + Fn.log_softmax(out, dim=1)
        for r, q in enumerate(seqs):
            scores[r, banned_words(q, step, end_token, constraints)] = float("-inf")
        flat = scores[0] if step == 1 else scores.view(-1)
        best, idx = flat.topk(min(k + 1, flat.numel()), 0, True, True)
        assert bool(torch.isfinite(best[:k]).all()), "a step with fewer than k finite candidates"
        if best.numel() > k and bool(torch.isfinite(best[k])):
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


class ConstrainedBeam(NBestBeam):
    """NBestBeam that also remembers, per step, what every competing slot was forbidden: excluded[step] = {(image, slot):
    sorted word ids}."""

    def __init__(self, n, k, vocab_size, start_token, end_token, constraints):
        super().__init__(n, k, vocab_size, start_token, end_token)
        self.constraints, self.excluded = constraints, {}
        self.outputs = {}           # step -> (next_words [n k], parent_rows [n k], the rows that competed per image)

    def advance(self, step, topk):
        competing = [(1 if step == 1 else live) if live else 0 for live in self.live]
        words, rows = super().advance(step, topk)
        self.outputs[step] = (words, rows, competing)
        return words, rows

    def bans(self, step, i, rows):
        """The lists of image i's first `rows` slots at `step`."""
        out = [banned_words(self.seqs[i][r], step, self.end, self.constraints) for r in range(rows)]
        self.excluded.setdefault(step, {}).update({(i, r): b for r, b in enumerate(out)})
        return out


def drive(beam, tab, steps=None):
    """`beam` (a ConstrainedBeam) over the stored logits tab [T][n k][V] -> the smallest non-zero gap between neighbours
    among the finite candidates taken and the first finite one left out, over all steps and images."""
    k, T = beam.k, tab.shape[0] if steps is None else steps
    gap = [float("inf")]
    for step in range(1, T + 1):
        logp = Fn.log_softmax(tab[step - 1].double(), dim=1)        # over the whole, unmodified rows

        def topk(i, nrows, kk, logp=logp, step=step):
            prev = torch.tensor(beam.scores[i], dtype=torch.float64)
            block = (prev[:nrows, None] + logp[i * k:i * k + nrows]).clone()
            for r, b in enumerate(beam.bans(step, i, nrows)):
                block[r, b] = float("-inf")
            flat = block.reshape(-1).tolist()
            best = sorted(range(len(flat)), key=lambda j: (-flat[j], j))[:kk + 1]
            assert all(flat[j] > float("-inf") for j in best[:kk])
            for p, q in zip(best, best[1:]):
                if flat[p] != flat[q] and flat[q] > float("-inf"):
                    gap[0] = min(gap[0], flat[p] - flat[q])
            return [flat[j] for j in best[:kk]], best[:kk]
        beam.advance(step, topk)
    return gap[0]


def violations(tokens, end_token, constraints, completed=True):
    """What a caption [start, w_1 ..] breaks, as a list of strings (empty: nothing), from the definitions alone: a g-gram
    that occurs twice, a banned id, fewer than min_words words before <end>."""
    out = []
    g = constraints.no_repeat_ngram
    if g:
        grams = [tuple(tokens[e:e + g]) for e in range(len(tokens) - g + 1)]
        if len(set(grams)) != len(grams):
            out.append("a %d-gram twice in %r" % (g, tokens))
    if set(tokens) & set(constraints.banned):
        out.append("a banned word in %r" % (tokens,))
    if completed and tokens[-1] == end_token and len(tokens) - 2 < constraints.min_words:
        out.append("%d words, fewer than %d, in %r" % (len(tokens) - 2, constraints.min_words, tokens))
    return out
