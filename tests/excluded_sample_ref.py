"""fp64 restatement of sampled decoding with exclusions (capnet.decode.sample_random(exclude=), csrc/sample_exclude.hip).
TEST INFRASTRUCTURE; the reference project has no sampler, nothing here is reference-pinned.

The loop is sample_random_ref.family_sampled's (nucleus_ref.family_sampled's where top_p < 1) with one addition before each
draw: row r's logits get -inf at capnet.beam.banned_words([start] + its words so far, t + 1, end, c). Both draws already treat
-inf as unpickable and normalise over the rest, which is the meaning of `exclude=`. Gaps, need, need_kth, logp_tol and the
nucleus' margin rule are sample_random_ref's and nucleus_ref's own: no tolerance is introduced here.

  * mask_bits: the rule as the set of excluded words of one row (what the mask kernel's bits must be).
  * mask_words: those sets packed as the kernel packs them, [rows][ceil(V / 32)] uint32.
  * family_sampled: the loop.  violations: what a cut caption does against a Constraints.
"""
import numpy as np
import torch

import nucleus_ref as N
import sample_random_ref as R
from capnet.beam import banned_words


def mask_bits(tokens, t, end_token, c):
    """The words row `tokens` = [start, w_0 .. w_{t-1}] may not draw at stream step t (0-based): banned_words at step t + 1."""
    return set(banned_words([int(w) for w in tokens], t + 1, end_token, c))


def mask_words(rows_tokens, t, V, end_token, c):
    """The exclusion mask of the rows' hypotheses at stream step t -> uint32 [rows, ceil(V / 32)]: bit v & 31 of word v >> 5."""
    out = np.zeros((len(rows_tokens), (V + 31) // 32), dtype=np.uint32)
    for r, tokens in enumerate(rows_tokens):
        for v in mask_bits(tokens, t, end_token, c):
            if 0 <= v < V:
                out[r, v >> 5] |= np.uint32(1 << (v & 31))
    return out


def masked(logits, rows_tokens, t, end_token, c):
    """fp64 copy of logits [rows, V] with -inf at every row's excluded words."""
    z = np.array(torch.as_tensor(logits, dtype=torch.float64).numpy() if isinstance(logits, torch.Tensor) else logits,
                 dtype=np.float64)
    for r, tokens in enumerate(rows_tokens):
        for v in mask_bits(tokens, t, end_token, c):
            if 0 <= v < z.shape[1]:
                z[r, v] = -np.inf
    return z


def family_sampled(initial, n, m, steps, start_token, end_token, T, seed, top_k, c, top_p=1.0):
    """capnet.decode.sample_random(exclude=c) on a restated decoder (c None: no exclusions) -> (ids [n m, steps], logp
    [n m, steps], Trace -- nucleus_ref's where top_p < 1)."""
    inv_T = R.inv_temperature(T)
    nucleus = top_p < 1.0
    tr = N.Trace() if nucleus else R.Trace()
    ids, logp = [], []
    for i in range(n):
        step_fn, state = initial(m, i)
        words = torch.full((m, 1), int(start_token), dtype=torch.long)
        wi, li = [], []
        for t in range(steps):
            logits, state = step_fn(words, state)
            z = logits.detach()
            if c is not None:
                z = masked(z, [[int(start_token)] + [int(w[r]) for w in wi] for r in range(m)], t, end_token, c)
            d = N.draw(z, inv_T, seed, t, i * m, top_k, N.top_p32(top_p)) if nucleus else R.draw(z, inv_T, seed, t, i * m, top_k)
            tr.add(d)
            wi.append(d["tokens"])
            li.append(d["logp"])
            words = torch.from_numpy(d["tokens"]).view(m, 1)
        ids.append(np.stack(wi, 1))
        logp.append(np.stack(li, 1))
    return np.concatenate(ids, 0), np.concatenate(logp, 0), tr


def clears(tr, T, top_k, top_p=1.0):
    """The margin rule on a Trace -> the list of what fails (empty: admitted)."""
    inv_T = R.inv_temperature(T)
    if top_p < 1.0:
        return N.clears(tr, inv_T, top_k)
    fails = []
    if not tr.key_gap > R.need(tr.scale, inv_T):
        fails.append("key gap %.3g <= %.3g" % (tr.key_gap, R.need(tr.scale, inv_T)))
    if top_k and not tr.kth_gap > R.need_kth(tr.scale):
        fails.append("k-th gap %.3g <= %.3g" % (tr.kth_gap, R.need_kth(tr.scale)))
    return fails


def violations(tokens, end_token, c):
    """What the cut caption `tokens` = [start, w_1 .. w_j] does against c: a list of strings (empty: it obeys). A word at
    position p (1-based behind <start>) was drawn at step p from the hypothesis tokens[:p]."""
    out = []
    for p in range(1, len(tokens)):
        if int(tokens[p]) in banned_words([int(w) for w in tokens[:p]], p, end_token, c):
            out.append("word %d at step %d" % (int(tokens[p]), p))
    return out


def greedy_caption(initial, image, steps, start_token, end_token, c):
    """The greedy row of sample_random(greedy=True, exclude=c) for one image: argmax over the allowed words at every step (ties
    to the lower index), cut after the first end_token -> (tokens, the smallest gap between the two best allowed logits, the
    largest |logit|)."""
    step_fn, state = initial(1, image)
    words = torch.full((1, 1), int(start_token), dtype=torch.long)
    tokens, gap, scale = [int(start_token)], np.inf, 0.0
    for t in range(steps):
        logits, state = step_fn(words, state)
        z = logits.detach() if c is None else masked(logits.detach(), [tokens], t, end_token, c)
        z = np.asarray(torch.as_tensor(z, dtype=torch.float64).numpy() if isinstance(z, torch.Tensor) else z)[0]
        order = np.lexsort((np.arange(z.shape[0]), -z))
        gap, scale = min(gap, float(z[order[0]] - z[order[1]])), max(scale, float(np.abs(z[np.isfinite(z)]).max()))
        tokens.append(int(order[0]))
        words = torch.tensor([[int(order[0])]])
        if tokens[-1] == end_token:
            break
    return tokens, gap, scale
