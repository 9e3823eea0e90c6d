"""The fp64 side of the attention-map tests (tests/test_att_alphas_cpu.py, tests/test_att_alphas_gpu.py). TEST INFRASTRUCTURE.

  * replay(family, image, tokens): the contract itself. The token list is fed through the family's initial(1, image) step
    function; before step e the softmax over the pixels is taken from the layer-0 h with oracle.decoders_ref.attention_step.
    Row e - 1 is the map that preceded word e.
  * TracedBeam: device_beam_ref.DeviceBeam with a row history next to each sequence -- entry e of a hypothesis is the slot
    it occupied when the decoder ran step e (entry 0 is -1), what capnet_beam_advance_traced records. winner_rows() is
    capnet_beam_finish_traced's `rows`.
  * fixed_slot_search(family, k, image): the whole search on the fixed-slot model in fp64, all k rows taking every step,
    with every step's per-slot maps kept: the winner's tokens, its path, the maps read along the path, and two WRONG
    readings of the same history (decoys) that a trace which ignored parents, or was off by one step, would produce.
"""
import torch
import torch.nn.functional as Fn

from device_beam_ref import DeviceBeam
from oracle import decoders_ref as D


def att_prefix(family):
    """The Attention module a family's sample() uses: the mode's (factored decoders) or `attention`."""
    return D.MODE_ATT[family.kw.get("mode", "factual")]


def state_alpha(family, state):
    """The maps [rows, P] of the step about to be taken on `state` (hs + cs + (feat,)): from layer 0's h."""
    return D.attention_step(family.params, att_prefix(family), state[-1], state[0])[1]


def replay(family, image, tokens):
    """fp64 maps [len(tokens) - 1, P] of one caption of one image."""
    step_fn, state = family.initial(1, image)
    maps = []
    for e in range(1, len(tokens)):
        maps.append(state_alpha(family, state)[0])
        _, state = step_fn(torch.LongTensor([[tokens[e - 1]]]), state)
    P = state[-1].shape[1]
    return torch.stack(maps) if maps else torch.zeros(0, P, dtype=torch.float64)


class TracedBeam(DeviceBeam):
    def __init__(self, n, k, vocab_size, start_token, end_token):
        super().__init__(n, k, vocab_size, start_token, end_token)
        self.paths = [[[-1] for _ in range(k)] for _ in range(n)]
        self.done_paths = [[] for _ in range(n)]               # in completion order, beside self.done

    def advance(self, step, topk):
        picked, before = {}, list(self.live)

        def spy(i, rows, live):
            scores, flat = topk(i, rows, live)
            picked[i] = [int(f) for f in flat[:live]]
            return scores, flat
        out = super().advance(step, spy)
        for i, flat in picked.items():
            kept = []
            for j in range(before[i]):
                p, w = flat[j] // self.V, flat[j] % self.V
                path = self.paths[i][p] + [p]
                (self.done_paths[i] if w == self.end else kept).append(path)
            self.paths[i] = kept + self.paths[i][len(kept):]
        return out

    def best(self, i):
        """Index of image i's winner in its completed list (finish()'s rule), None where nothing completed."""
        d = self.done[i]
        if not d:
            return None
        best = 0
        for q in range(1, len(d)):
            if d[q][0] > d[best][0]:
                best = q
        return best

    def winner_path(self, i):
        """The winner's slots at steps 1 .. len - 1 ([] where nothing completed)."""
        b = self.best(i)
        return [] if b is None else self.done_paths[i][b][1:]

    def winner_rows(self, max_steps):
        """capnet_beam_finish_traced's rows [n][max_steps]: i k + slot, -1 past length - 1."""
        out = []
        for i in range(self.n):
            path = self.winner_path(i)
            out.append([i * self.k + s for s in path] + [-1] * (max_steps - len(path)))
        return out


class Search:
    """What fixed_slot_search returns: tokens (the winner's, [<end>] where nothing completed); path (its slot at steps
    1 .. len - 1); maps [len - 1, P] read along the path; final_slot / late: the two decoys, [len - 1, P] each; events
    (DeviceBeam.events)."""

    def __init__(self, tokens, path, hist, events):
        self.tokens, self.path, self.events = tokens, path, events
        P = hist[1].shape[1]
        rows = lambda slots: (torch.stack([hist[e + 1][s] for e, s in enumerate(slots)]) if slots   # noqa: E731
                              else torch.zeros(0, P, dtype=torch.float64))
        self.maps = rows(path)
        self.final_slot = rows([path[-1]] * len(path) if path else [])       # the winner's last slot at every step
        self.late = rows(path[:1] + path[:-1])                               # the right path, one step late

    @property
    def leaves_slot_0(self):
        return sum(1 for s in self.path if s != 0)


def fixed_slot_search(family, k, image, start, max_len):
    """The search of family.reference(k, image) on the fixed-slot model in fp64 -> Search."""
    step_fn, state = family.initial(k, image)
    V, end, steps = family.V, family.end, max_len + 1
    beam = TracedBeam(1, k, V, start, end)
    hist, words, rows = [None], None, None
    for step in range(1, steps + 1):
        if step > 1:
            idx = torch.tensor(rows)
            state = tuple(t[idx] for t in state)
        hist.append(state_alpha(family, state))
        prev = torch.LongTensor([[start]] * k if words is None else [[w] for w in words])
        logits, state = step_fn(prev, state)
        logp = Fn.log_softmax(logits, dim=1)
        prev_scores = torch.tensor(beam.scores[0], dtype=torch.float64)

        def topk(i, nrows, kk, logp=logp, prev_scores=prev_scores):
            flat = (prev_scores[:nrows, None] + logp[:nrows]).reshape(-1)
            s, ix = flat.topk(kk, 0, True, True)
            return s.tolist(), ix.tolist()
        words, rows = beam.advance(step, topk)
        if not beam.live_total:
            break
    return Search(beam.finish()[0], beam.winner_path(0), hist, beam.events(steps))
