"""The fp64 side of the diverse-beam-search tests (tests/test_diverse_beam_cpu.py, tests/test_diverse_beam_gpu.py).
TEST INFRASTRUCTURE.

  * diverse_search: nbest_ref.nbest_search's loop once per group, the groups of an image advancing in order at every step;
    group g ranks its candidates by key = score - strength * c_g(v), c_g(v) the number of candidates groups 0 .. g - 1
    selected at this step with word v (<end> counted like any word; a group with no live beam selects and counts nothing),
    and carries the unpenalised score forward. With constraints the exclusions (-inf) come first. It keeps every group's
    completed list, the largest |logit| and the margin: the gap between the live-th key and the next FINITE key, in any
    group at any step -> DSearch, whose gap(penalty) is the smallest gap between the ranking keys of completed hypotheses
    with distinct token lists, over all groups.
  * rank / dedupe / winner / nbest / per_group: what the calls return, written here on plain lists.
  * DiverseBeam / drive: the fixed-slot model over stored logits -- an nbest_ref.NBestBeam of n D state-images of k / D slots
    (state-image i D + g = group g of image i, rows (i D + g) k / D ..) whose top-k, in fp64 with ties to the lower flat
    index, ranks by the key -- what capnet_beam_advance_diverse must select and capnet_beam_topk_batched_diverse return.
  * shared_words / group_words: the property checks, written without the rule's own code.
"""
import torch
import torch.nn.functional as Fn

import nbest_ref
from capnet.beam import banned_words
from nbest_ref import NBestBeam

NEG = float("-inf")


# ---- what the calls return, on plain lists -----------------------------------------------------------------------------
def dedupe(done):
    """[(score, tokens)] with every token list once, the first kept."""
    out, seen = [], []
    for sc, q in done:
        if list(q) not in seen:
            seen.append(list(q))
            out.append((sc, list(q)))
    return out


def nbest(groups_done, penalty):
    """[(tokens, score)]: all groups' completed lists in group order, deduplicated, ranked by nbest_ref's rule."""
    return nbest_ref.rank(dedupe([p for d in groups_done for p in d]), penalty)


def per_group(groups_done, penalty):
    return [nbest_ref.rank(d, penalty)[0] if d else None for d in groups_done]


def winner(groups_done, end_token):
    """The first maximum of the scores in group order, then completion order; [<end>] for none."""
    flat = [p for d in groups_done for p in d]
    if not flat:
        return [int(end_token)]
    best = 0
    for j in range(1, len(flat)):
        if flat[j][0] > flat[best][0]:
            best = j
    return list(flat[best][1])


class DSearch:
    """groups: per group [(score, tokens)] in completion order; margin: the smallest selection gap; scale: the largest
    |logit|."""

    def __init__(self, groups, margin, scale, end_token):
        self.groups, self.margin, self.scale, self.end = groups, margin, scale, int(end_token)

    def gap(self, penalty):
        return nbest_ref.min_gap(dedupe([p for d in self.groups for p in d]), penalty)

    def nbest(self, penalty):
        return nbest(self.groups, penalty)

    def per_group(self, penalty):
        return per_group(self.groups, penalty)

    def winner(self):
        return winner(self.groups, self.end)


# ---- the fp64 search ---------------------------------------------------------------------------------------------------
def diverse_search(initial, vocab_size, start_token, end_token, k, D, strength, max_seq_length, constraints=None):
    """initial(rows) -> (step_fn, state) of a search of `rows` beams (called once per group, with k / D)."""
    V, kp = vocab_size, k // D
    assert kp * D == k
    G = []
    for _ in range(D):
        step_fn, state = initial(kp)
        G.append(dict(step_fn=step_fn, state=state, words=torch.LongTensor([[start_token]] * kp), live=kp,
                      seqs=[[int(start_token)] for _ in range(kp)], top=torch.zeros(kp, 1, dtype=torch.float64), done=[]))
    margin, scale, step = float("inf"), 0.0, 1
    while any(g["live"] for g in G):
        counts = {}
        for g in G:
            live = g["live"]
            if not live:
                continue
            out, state = g["step_fn"](g["words"], g["state"])
            scale = max(scale, float(out.abs().max()))
            scores = g["top"].expand_as(out) + Fn.log_softmax(out, dim=1)
            key = scores.clone()
            if constraints is not None:
                for r, q in enumerate(g["seqs"]):
                    key[r, banned_words(q, step, end_token, constraints)] = NEG
            for v, c in counts.items():
                key[:, v] -= strength * c
            flat, plain = (key[0], scores[0]) if step == 1 else (key.view(-1), scores.view(-1))
            best, idx = flat.topk(min(live + 1, flat.numel()), 0, True, True)
            assert bool(torch.isfinite(best[:live]).all()), "a step with fewer than `live` finite candidates"
            if best.numel() > live and bool(torch.isfinite(best[live])):
                margin = min(margin, float(best[live - 1] - best[live]))
            idx = idx[:live]
            carried = plain[idx]                               # the unpenalised scores
            prev, nxt = (idx // V).tolist(), (idx % V).tolist()
            for w in nxt:
                counts[w] = counts.get(w, 0) + 1
            seqs = [g["seqs"][p] + [w] for p, w in zip(prev, nxt)]
            keep = [i for i, w in enumerate(nxt) if w != end_token]
            g["done"] += [(float(carried[i]), seqs[i]) for i in range(live) if i not in keep]
            g["live"] = len(keep)
            if not keep:
                continue
            g["seqs"] = [seqs[i] for i in keep]
            g["state"] = tuple(s[torch.tensor(prev)[keep]] for s in state)
            g["top"] = carried[keep].unsqueeze(1)
            g["words"] = torch.tensor(nxt)[keep].unsqueeze(1)
        if step > max_seq_length:
            break
        step += 1
    return DSearch([g["done"] for g in G], margin, scale, end_token)


# ---- the fixed-slot model over stored logits ---------------------------------------------------------------------------
class DiverseBeam(NBestBeam):
    """NBestBeam of n D state-images of k / D slots that remembers per step what it put out and selected:
    outputs[step] = (next_words [n k], parent_rows [n k], per state-image the rows that competed and its live count);
    selected[step][state-image] = (scores, flat indices local to the group); excluded[step][(state-image, slot)]."""

    def __init__(self, n, k, D, strength, vocab_size, start_token, end_token, constraints=None):
        assert k % D == 0
        super().__init__(n * D, k // D, vocab_size, start_token, end_token)
        self.images, self.D, self.strength, self.constraints = n, D, float(strength), constraints
        self.outputs, self.selected, self.excluded, self.states = {}, {}, {}, {}

    def advance(self, step, topk):
        competing = [(1 if step == 1 else live) if live else 0 for live in self.live]
        before = list(self.live)
        picked = {}

        def spy(q, rows, live):
            picked[q] = topk(q, rows, live)
            return picked[q]
        words, rows = super().advance(step, spy)
        self.outputs[step] = (words, rows, competing, before)
        self.selected[step] = picked
        # the state after the step: live counts, the live slots' scores, every completed list so far
        self.states[step] = (list(self.live), [list(s[:l]) for s, l in zip(self.scores, self.live)],
                             [self.completed(q) for q in range(self.n)])
        return words, rows

    def bans(self, step, q, rows):
        if self.constraints is None:
            return [[] for _ in range(rows)]
        out = [banned_words(self.seqs[q][r], step, self.end, self.constraints) for r in range(rows)]
        self.excluded.setdefault(step, {}).update({(q, r): b for r, b in enumerate(out)})
        return out

    def group_done(self, i):
        """Image i's completed lists, per group."""
        return [self.completed(i * self.D + g) for g in range(self.D)]


def drive(beam, tab, steps=None):
    """`beam` (a DiverseBeam) over the stored logits tab [T][n k][V] -> the smallest non-zero gap between neighbouring keys
    among the finite candidates taken and the first finite one left out, over all steps, images and groups."""
    kp, D, T = beam.k, beam.D, tab.shape[0] if steps is None else steps
    gap = [float("inf")]
    for step in range(1, T + 1):
        logp = Fn.log_softmax(tab[step - 1].double(), dim=1)        # over the whole, unmodified rows
        counts = {}                                                  # image -> {word: count}, this step

        def topk(q, nrows, kk, logp=logp, step=step, counts=counts):
            prev = torch.tensor(beam.scores[q], dtype=torch.float64)
            block = prev[:nrows, None] + logp[q * kp:q * kp + nrows]
            key = block.clone()
            for r, b in enumerate(beam.bans(step, q, nrows)):
                key[r, b] = NEG
            mine = counts.setdefault(q // D, {})
            for v, c in mine.items():
                key[:, v] -= beam.strength * c
            flat, plain = key.reshape(-1).tolist(), block.reshape(-1).tolist()
            best = sorted(range(len(flat)), key=lambda j: (-flat[j], j))[:kk + 1]
            assert all(flat[j] > NEG for j in best[:kk])
            for p, r in zip(best, best[1:]):
                if flat[p] != flat[r] and flat[r] > NEG:
                    gap[0] = min(gap[0], flat[p] - flat[r])
            for j in best[:kk]:
                mine[j % beam.V] = mine.get(j % beam.V, 0) + 1
            return [plain[j] for j in best[:kk]], best[:kk]
        beam.advance(step, topk)
    return gap[0]


# ---- properties, without the rule's own code ---------------------------------------------------------------------------
def group_words(beam, step, i):
    """Per LIVE group of image i, the set of words it selected at `step` (from the model's or a device's outputs alike:
    the flat indices of `selected`)."""
    out = []
    for g in range(beam.D):
        q = i * beam.D + g
        if q in beam.selected[step]:
            out.append({int(f) % beam.V for f in beam.selected[step][q][1]})
    return out


def shared_words(sets):
    """The words that occur in more than one of the given sets."""
    seen, twice = set(), set()
    for s in sets:
        twice |= seen & s
        seen |= s
    return twice
