"""The fp64 side of the forced-word beam-search tests (tests/test_forced_beam_cpu.py, tests/test_forced_beam_gpu.py).
TEST INFRASTRUCTURE.

  * select: one image's step under capnet.beam.Constraints(forced=...) on an fp64 block of scores whose excluded entries are
    -inf -- the pool (the plain selection, every row's missing forced ids, every row's best word; a flat index once), the banks
    by met count and the round-robin walk F, F - 1 .. 0, F .., written out here WITHOUT capnet.beam.forced_allocate. It also
    returns the smallest gap its decisions rest on: the live-th against the next finite candidate of the plain selection,
    every row's best against its second, neighbours inside every bank up to and including the first entry left untaken.
    Exact ties are excepted on request (the tables have one on purpose); they go to the lower flat index.
  * forced_search: constrained_beam_ref.constrained_search's loop with `select` in topk's place -> nbest_ref.Search, its
    margin the smallest of those gaps and the gap between the two best completed scores.
  * ForcedBeam / drive: constrained_beam_ref.ConstrainedBeam / drive extended likewise: what capnet_beam_advance_forced and
    capnet_beam_topk_batched_forced must select on stored logits.
  * missing: the property, from the definition alone -- the forced ids a caption lacks.
The exclusions: capnet.beam.banned_words for the part that exists without forced words (on a Constraints without them), the
new one -- <end> on a row that lacks a forced id -- written out here.
"""
import torch
import torch.nn.functional as Fn

from capnet.beam import Constraints, banned_words
from constrained_beam_ref import ConstrainedBeam
from nbest_ref import Search

NEG = float("-inf")


def missing(tokens, forced):
    """The forced ids that do not occur behind <start> in `tokens`."""
    return [w for w in forced if w not in tokens[1:]]


def without_forced(c):
    return Constraints(c.no_repeat_ngram, c.min_words, c.banned)


def excluded(tokens, step, end_token, constraints):
    """The sorted word ids the row `tokens` may not take at `step`: the old rule, and <end> while a forced id is missing."""
    out = set(banned_words(tokens, step, end_token, without_forced(constraints)))
    if missing(tokens, constraints.forced):
        out.add(int(end_token))
    return sorted(out)


def _gap(a, b, ties_ok):
    """The gap a decision between neighbours a >= b rests on (inf for an excepted exact tie or a -inf neighbour)."""
    if b == NEG or (ties_ok and a == b):
        return float("inf")
    return a - b


def select(block, rows_tokens, live, forced, ties_ok=False):
    """block: fp64 [rows, V] = running score + log-softmax, -inf where excluded; rows_tokens: the competing rows' hypotheses.
    -> ([(score, flat)] in taking order, the smallest gap)."""
    rows, V = block.shape
    F = len(forced)
    gap = float("inf")
    flat = block.reshape(-1)
    vals, idx = torch.sort(flat, descending=True, stable=True)          # ties: the lower flat index first
    vals, idx = vals[:live + 1].tolist(), idx[:live + 1].tolist()
    pool = {}
    for j in range(min(live, len(vals))):                               # 1. the plain selection
        if vals[j] > NEG:
            pool[idx[j]] = vals[j]
    if len(vals) > live and vals[live - 1] > NEG:
        gap = min(gap, _gap(vals[live - 1], vals[live], ties_ok))
    for r in range(rows):
        have = set(rows_tokens[r][1:])
        for w in forced:                                                # 2. the row's missing forced ids
            if w not in have and float(block[r, w]) > NEG:
                pool[r * V + w] = float(block[r, w])
        v2, i2 = torch.sort(block[r], descending=True, stable=True)     # 3. the row's best word
        if float(v2[0]) > NEG:
            pool[r * V + int(i2[0])] = float(v2[0])
            if V > 1:
                gap = min(gap, _gap(float(v2[0]), float(v2[1]), ties_ok))
    banks = [[] for _ in range(F + 1)]
    for f, sc in pool.items():
        have = set(rows_tokens[f // V][1:]) | {f % V}
        banks[sum(1 for w in forced if w in have)].append((sc, f))
    for b in banks:
        b.sort(key=lambda p: (-p[0], p[1]))
    taken, at, b = [], [0] * (F + 1), F
    while len(taken) < min(live, len(pool)):
        if at[b] < len(banks[b]):
            taken.append(banks[b][at[b]])
            at[b] += 1
        b = F if b == 0 else b - 1
    for b in range(F + 1):                                              # up to and including the first entry left untaken
        for j in range(min(at[b], len(banks[b]) - 1)):
            gap = min(gap, _gap(banks[b][j][0], banks[b][j + 1][0], ties_ok))
    return taken, gap


def forced_search(step_fn, state, vocab_size, start_token, end_token, k, max_seq_length, constraints):
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
            scores[r, excluded(q, step, end_token, constraints)] = NEG
        rows = 1 if step == 1 else k
        taken, gap = select(scores[:rows], seqs[:rows], k, constraints.forced)
        assert len(taken) == k, "a step with fewer than k candidates"
        margin = min(margin, gap)
        best = torch.tensor([sc for sc, _ in taken], dtype=torch.float64)
        prev, nxt = [f // V for _, f in taken], [f % V for _, f in taken]
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


class ForcedBeam(ConstrainedBeam):
    """ConstrainedBeam whose exclusions are `excluded`'s and which remembers every competing slot's met ids."""

    def bans(self, step, i, rows):
        out = [excluded(self.seqs[i][r], step, self.end, self.constraints) for r in range(rows)]
        self.excluded.setdefault(step, {}).update({(i, r): b for r, b in enumerate(out)})
        return out

    def met(self, i, rows):
        """The met masks of image i's first `rows` slots: bit f for forced[f]."""
        return [sum(1 << f for f, w in enumerate(self.constraints.forced) if w in self.seqs[i][r][1:]) for r in range(rows)]


def drive(beam, tab, steps=None):
    """`beam` (a ForcedBeam) over the stored logits tab [T][n k][V] -> the smallest non-zero gap its selections rest on."""
    k, T = beam.k, tab.shape[0] if steps is None else steps
    gap = [float("inf")]
    for step in range(1, T + 1):
        logp = Fn.log_softmax(tab[step - 1].double(), dim=1)        # over the whole, unmodified rows

        def topk(i, nrows, kk, logp=logp, step=step):
            prev = torch.tensor(beam.scores[i], dtype=torch.float64)
            block = (prev[:nrows, None] + logp[i * k:i * k + nrows]).clone()
            for r, b in enumerate(beam.bans(step, i, nrows)):
                block[r, b] = NEG
            taken, g = select(block, beam.seqs[i][:nrows], kk, beam.constraints.forced, ties_ok=True)
            assert len(taken) == kk
            gap[0] = min(gap[0], g)
            return [sc for sc, _ in taken], [f for _, f in taken]
        beam.advance(step, topk)
    return gap[0]
