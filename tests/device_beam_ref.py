"""A pure-Python model of the fixed-slot beam search of capnet_beam_advance / capnet_beam_finish. TEST INFRASTRUCTURE.

Image i owns slots i k .. i k + k - 1 for the whole search; its live beams are its first live[i] slots, in the rank order
of the survivors. A step asks topk(image, rows, k) -> (scores [k], flat indices [k], flat = slot * V + word) for the
image's live[i] best over its first `rows` slots (row 0 alone at step 1). <end> completes a beam (appended to the image's
completed list, by step then rank); any other word survives into the image's next free slot. Dead slots report <end>
and their own row. finish(): the first maximum of the completed scores, [<end>] where nothing completed.

It also records what the tests assert their cases contain: `events`.
"""


class DeviceBeam:
    def __init__(self, n, k, vocab_size, start_token, end_token):
        self.n, self.k, self.V, self.end = n, k, vocab_size, int(end_token)
        self.live = [k] * n
        self.seqs = [[[int(start_token)] for _ in range(k)] for _ in range(n)]
        self.scores = [[0.0] * k for _ in range(n)]
        self.done = [[] for _ in range(n)]                 # (score, sequence, step) in completion order
        self.steps = 0

    @property
    def live_total(self):
        return sum(self.live)

    def advance(self, step, topk):
        """One step of every image -> (next_words [n k], parent_rows [n k])."""
        n, k, V = self.n, self.k, self.V
        next_words, parent_rows = [self.end] * (n * k), list(range(n * k))
        for i in range(n):
            live = self.live[i]
            if not live:
                continue
            scores, flat = topk(i, 1 if step == 1 else live, live)
            seqs, kept = [], []
            for j in range(live):
                p, w = int(flat[j]) // V, int(flat[j]) % V
                sq = self.seqs[i][p] + [w]
                if w == self.end:
                    self.done[i].append((scores[j], sq, step))
                else:
                    s = len(seqs)
                    seqs.append(sq)
                    kept.append(scores[j])
                    next_words[i * k + s] = w
                    parent_rows[i * k + s] = i * k + p
            self.live[i] = len(seqs)
            self.seqs[i] = seqs + self.seqs[i][len(seqs):]          # (dead slots keep stale sequences, never read)
            self.scores[i] = kept + self.scores[i][len(kept):]
        self.steps = step
        return next_words, parent_rows

    def finish(self):
        """-> a list of n token lists."""
        out = []
        for d in self.done:
            if not d:
                out.append([self.end])
                continue
            best = 0
            for q in range(1, len(d)):
                if d[q][0] > d[best][0]:
                    best = q
            out.append(list(d[best][1]))
        return out

    def events(self, max_steps):
        """The situations this search went through, as a set of names (over all images)."""
        ev = set()
        for d in self.done:
            steps = [s for _, _, s in d]
            if any(steps.count(s) > 1 for s in steps):
                ev.add("several completions in one step")
            if not d and self.steps == max_steps:
                ev.add("nothing completed")
            if len(d) == self.k and max(steps) < max_steps:
                ev.add("all beams complete before the last step")
            if d:
                best = max(range(len(d)), key=lambda q: (d[q][0], -q))
                if best != 0:
                    ev.add("the winner is not the first completion")
        return ev


def run(beam, max_steps, step_topk, stop_when_dead=True):
    """Drive `beam` for up to max_steps steps: step_topk(step, next_words, parent_rows) -> topk callback for that step
    (next_words / parent_rows: the previous step's, None at step 1). Returns finish()."""
    words = rows = None
    for step in range(1, max_steps + 1):
        words, rows = beam.advance(step, step_topk(step, words, rows))
        if stop_when_dead and not beam.live_total:
            break
    return beam.finish()


def beam_margin(step_fn, state, vocab_size, start_token, end_token, k, max_seq_length):
    """The smallest gap, over the steps of oracle.beam_ref._beam on this (step_fn, state), between the k-th and the
    (k+1)-th best candidate score, and between the best and the second-best completed sequence (the rule of
    tests/stacked_decode_ref.py, for any decoder). Where it is well above f32 rounding, every correct f32 beam search
    picks the same sequence, whatever rows its products ran on."""
    import torch
    import torch.nn.functional as Fn
    V = vocab_size
    words = torch.LongTensor([[start_token]] * k)
    top = torch.zeros(k, 1, dtype=torch.float64)
    margin, done, step = float("inf"), [], 1
    while True:
        out, state = step_fn(words, state)
        scores = top.expand_as(out) + Fn.log_softmax(out, dim=1)
        flat = scores[0] if step == 1 else scores.view(-1)
        best, idx = flat.topk(min(k + 1, flat.numel()), 0, True, True)
        if best.numel() > k:
            margin = min(margin, float(best[k - 1] - best[k]))
        best, idx = best[:k], idx[:k]
        prev, nxt = idx // V, idx % V
        keep = [i for i, w in enumerate(nxt.tolist()) if w != end_token]
        done += [float(best[i]) for i in range(k) if i not in keep]
        k = len(keep)
        if k == 0 or step > max_seq_length:
            break
        state = tuple(s[prev[keep]] for s in state)
        top = best[keep].unsqueeze(1)
        words = nxt[keep].unsqueeze(1)
        step += 1
    done.sort(reverse=True)
    if len(done) > 1:
        margin = min(margin, done[0] - done[1])
    return margin
