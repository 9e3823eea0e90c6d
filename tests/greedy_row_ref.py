"""fp64 restatement of a sampled decode that carries greedy rows (capnet.decode.sample_random(greedy=True),
csrc/sample_key.h's vs_row_key) on top of sample_random_ref / nucleus_ref. TEST INFRASTRUCTURE; nothing here is
reference-pinned.

Per image the decode has m + 1 physical rows: rows 0 .. m - 1 draw on the noise rows i m + j -- what the decode of m rows
without a greedy row draws -- and row m takes argmax_v logit_v at every step (ties to the lower index). Its logp is taken
under the distribution the drawn rows' is taken under: softmax(z / T) renormalised over the top_k candidates and over the
nucleus where those are set, so the greedy row passes through the same truncation (its k-th gap, edge gap and mass ratio
enter the margin rule; the gap of its noised keys does not: it has no noise).

The margin rule of a greedy row: the best two scaled logits are more than 2 TOL_STEP max|logit| / T apart.
"""
import numpy as np
import torch

import nucleus_ref as N
import sample_random_ref as R


class Trace(N.Trace):
    """nucleus_ref.Trace (the drawn rows' and the truncations' quantities) and the greedy rows' smallest top-two gap."""

    def __init__(self):
        super().__init__()
        self.greedy_gap = np.inf


def need_greedy(scale, inv_T):
    return 2 * R.TOL_STEP * scale * inv_T


def _draw(logits, inv_T, seed, step, row0, top_k, top_p):
    if top_p < 1.0:
        return N.draw(logits, inv_T, seed, step, row0, top_k, top_p)
    return R.draw(logits, inv_T, seed, step, row0, top_k)


def greedy_pick(z_row, inv_T, d):
    """The greedy row's (token, logp, top-two gap of the scaled logits) from its logits and d, a draw of the same row on any
    noise: the drawn token's s - logp is the log-normaliser of the truncated distribution, whatever was drawn."""
    s = np.asarray(z_row, dtype=np.float64) * inv_T
    order = np.lexsort((np.arange(s.size), -s))
    lse = s[int(d["tokens"][0])] - d["logp"][0]
    gap = float(s[order[0]] - s[order[1]]) if s.size > 1 else np.inf
    return int(order[0]), float(s[order[0]] - lse), gap


def family_sampled(initial, n, m, steps, start_token, T, seed, top_k, top_p):
    """sample_random(greedy=True) on a restated decoder: initial(m + 1, image) -> (step_fn, state of m + 1 rows).
    -> (ids [n (m + 1), steps], logp [n (m + 1), steps], Trace): physical row i (m + 1) + j is sample j of image i, row
    i (m + 1) + m the greedy one."""
    inv_T = R.inv_temperature(T)
    top_p = N.top_p32(top_p) if top_p < 1.0 else 1.0
    ids, logp, tr = [], [], Trace()
    for i in range(n):
        step_fn, state = initial(m + 1, i)
        words = torch.full((m + 1, 1), int(start_token), dtype=torch.long)
        wi, li = [], []
        for t in range(steps):
            logits, state = step_fn(words, state)
            logits = logits.detach()
            d = _draw(logits[:m], inv_T, seed, t, i * m, top_k, top_p)
            g = _draw(logits[m:], inv_T, seed, t, 0, top_k, top_p)
            tok, lp, gap = greedy_pick(logits[m].numpy(), inv_T, g)
            g["key_gap"], g["key_gaps"] = np.inf, np.full(1, np.inf)      # no noise on a greedy row
            if top_p == 1.0:                                              # sample_random_ref.draw's dict: nothing truncated by mass
                for dd in (d, g):
                    rows = dd["tokens"].shape[0]
                    dd.update(size=np.ones(rows, dtype=np.int64), edge_gap=np.full(rows, np.inf), mass_ratio=np.full(rows, np.inf),
                              below=np.full(rows, np.inf), above=np.full(rows, np.inf))
            tr.add(d)
            tr.add(g)
            tr.greedy_gap = min(tr.greedy_gap, gap)
            wi.append(np.concatenate([d["tokens"], [tok]]))
            li.append(np.concatenate([d["logp"], [lp]]))
            words = torch.from_numpy(wi[-1]).view(m + 1, 1)
        ids.append(np.stack(wi, 1))
        logp.append(np.stack(li, 1))
    return np.concatenate(ids, 0), np.concatenate(logp, 0), tr


def clears(tr, inv_T, top_k, top_p):
    """The margin rule on a Trace -> the list of what fails (empty: admitted): sample_random_ref's (key gap, k-th gap),
    nucleus_ref's where top_p < 1 (edge gap, mass ratio), and the greedy rows' top-two gap."""
    if top_p < 1.0:
        fails = N.clears(tr, inv_T, top_k)
    else:
        fails = []
        if not tr.key_gap > R.need(tr.scale, inv_T):
            fails.append("key gap %.3g <= %.3g" % (tr.key_gap, R.need(tr.scale, inv_T)))
        if top_k and not tr.kth_gap > R.need_kth(tr.scale):
            fails.append("k-th gap %.3g <= %.3g" % (tr.kth_gap, R.need_kth(tr.scale)))
    if not tr.greedy_gap > need_greedy(tr.scale, inv_T):
        fails.append("greedy gap %.3g <= %.3g" % (tr.greedy_gap, need_greedy(tr.scale, inv_T)))
    return fails
