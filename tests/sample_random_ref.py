"""fp64 restatement of sampled decoding (csrc/sample_rng.h, csrc/vocab_sample.hip, capnet.decode.sample_random,
capnet.seq2seq's sample_random). TEST INFRASTRUCTURE. The reference project has no sampler: nothing here is reference-pinned;
the decode steps underneath are (seq2seq_ref, oracle.decoders_ref through the families of device_beam_cases).

  * sample_uniform: the stream in Python integers, bit for bit the C function's; uniform_np: the same on numpy uint64 arrays.
  * draw: one step's draw of every row of a logits block -- the Gumbel noise and the keys in fp64 -- with what the margin
    rule needs: the gap between the best and second-best key, the gap between the k-th and (k + 1)-th logit, max |logit|.
  * the loops: seq2seq_sampled / seq2seq_sample_random over seq2seq_ref's step, family_sampled over a (step_fn, state) pair.
"""
import numpy as np
import torch

import seq2seq_ref as SR

MASK = (1 << 64) - 1
TOL_STEP = 3e-5      # a decode step's relative error bound (tests/seq2seq_cases.py)
TOL_G = 4e-6         # the device Gumbel's absolute error bound (logf to 1 ulp: 2.2e-6; confirmed for numpy's fp32 log on the CPU)


def sample_uniform(seed, step, row, v):
    """u(seed, step, row, v) in Python integers: (2 b + 1) / 2^24, exact as a float."""
    c = (step << 48) | (row << 24) | v
    z = (seed + 0x9E3779B97F4A7C15 * (c + 1)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z = z ^ (z >> 31)
    b = z >> 41
    return (2 * b + 1) / 16777216.0


def uniform_np(seed, step, row, v):
    """sample_uniform on broadcastable integer arrays -> float64 (exact)."""
    with np.errstate(over="ignore"):
        step, row, v = (np.asarray(a).astype(np.uint64) for a in (step, row, v))
        c = (step << np.uint64(48)) | (row << np.uint64(24)) | v
        z = np.uint64(seed & MASK) + np.uint64(0x9E3779B97F4A7C15) * (c + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        b = z >> np.uint64(41)
    return (2.0 * b.astype(np.float64) + 1.0) / 16777216.0


def gumbel(u):
    return -np.log(-np.log(u))


def inv_temperature(T):
    """1 / T as the C entry forms it (fp32)."""
    return float(np.float32(1.0) / np.float32(T))


def need(scale, inv_T):
    """The margin rule's bound on the gap of the two best keys: twice the error a key may carry."""
    return 2 * (TOL_STEP * scale * inv_T + TOL_G)


def need_kth(scale):
    """top_k > 0: the bound on the gap between the k-th and the (k + 1)-th logit."""
    return 2 * TOL_STEP * scale


def logp_tol(scale, inv_T):
    return 2 * TOL_STEP * scale * inv_T + 1e-6


def draw(logits, inv_T, seed, step, row0=0, top_k=0):
    """One step's draw for every row of logits [rows, V] (anything array-like, taken as fp64): row r on stream row row0 + r.
    A NaN or -inf logit is never drawn. -> dict(tokens [rows], logp [rows], key_gap, kth_gap, scale, key_gaps [rows],
    kth_gaps [rows]): the gaps per row (inf where there is no second key / no (k + 1)-th logit) and their smallest, scale
    the largest finite |logit|."""
    z = np.asarray(torch.as_tensor(logits, dtype=torch.float64).numpy() if isinstance(logits, torch.Tensor) else logits,
                   dtype=np.float64)
    rows, V = z.shape
    tokens, logp, scale = [], [], 0.0
    key_gaps, kth_gaps = np.full(rows, np.inf), np.full(rows, np.inf)
    cols = np.arange(V)
    for r in range(rows):
        ok = z[r] > -np.inf                     # NaN fails
        cand = cols[ok]
        if cand.size == 0:
            tokens.append(0)
            logp.append(-np.inf)
            continue
        zr = z[r][cand]
        scale = max(scale, float(np.abs(zr[np.isfinite(zr)]).max()) if np.isfinite(zr).any() else 0.0)
        if top_k:
            order = np.lexsort((cand, -zr))      # logit descending, index ascending
            if cand.size > top_k:
                kth_gaps[r] = float(zr[order[top_k - 1]] - zr[order[top_k]])
            cand, zr = cand[order[:top_k]], zr[order[:top_k]]
        s = zr * inv_T
        key = s + gumbel(uniform_np(seed, step, row0 + r, cand))
        order = np.lexsort((cand, -key))         # key descending, index ascending
        w = order[0]
        if cand.size > 1:
            key_gaps[r] = float(key[w] - key[order[1]])
        m = s.max()
        tokens.append(int(cand[w]))
        logp.append(float(s[w] - (m + np.log(np.exp(s - m).sum()))))
    return dict(tokens=np.array(tokens, dtype=np.int64), logp=np.array(logp), key_gap=float(key_gaps.min()),
                kth_gap=float(kth_gaps.min()), scale=scale, key_gaps=key_gaps, kth_gaps=kth_gaps)


class Trace:
    """What a sampled decode accumulates for the margin rule."""

    def __init__(self):
        self.key_gap, self.kth_gap, self.scale = np.inf, np.inf, 0.0

    def add(self, d):
        self.key_gap, self.kth_gap = min(self.key_gap, d["key_gap"]), min(self.kth_gap, d["kth_gap"])
        self.scale = max(self.scale, d["scale"])


def seq2seq_sampled(p, prefix, num_layers, steps, inv_T, seed, top_k, features=None, start_token=None, states=None):
    """EncoderRNN.sample_random (features) / DecoderRNN.sample_random (start_token broadcast to the states' rows) ->
    (ids [rows, steps], logp [rows, steps], (h, c) [num_layers, rows, H], Trace)."""
    emb_w = p[prefix + ".embed.weight"]
    H = p[prefix + ".lstm.weight_hh_l0"].shape[1]
    rows = features.size(0) if features is not None else states[0].size(1)
    zeros = torch.zeros(num_layers, rows, H, dtype=emb_w.dtype)
    h, c = (zeros, zeros) if states is None else (zeros if s is None else s.to(emb_w.dtype) for s in states)
    hs, cs = list(h), list(c)
    x = features if features is not None else emb_w[torch.full((rows,), int(start_token), dtype=torch.long)]
    ids, logp, tr = [], [], Trace()
    for t in range(steps):
        top, hs, cs = SR.step(p, prefix, num_layers, x, hs, cs)
        d = draw(SR._logits(p, prefix, top), inv_T, seed, t, 0, top_k)
        tr.add(d)
        ids.append(d["tokens"])
        logp.append(d["logp"])
        x = emb_w[torch.from_numpy(d["tokens"])]
    return np.stack(ids, 1), np.stack(logp, 1), (torch.stack(hs), torch.stack(cs)), tr


def seq2seq_sample_random(p, num_layers, steps, features, start_token, mode, T, seed, top_k):
    """Seq2Seq.sample_random -> (ids, logp, the sampler's final (h, c), Trace, the encoder's greedy (margin, scale) or None)."""
    inv_T = inv_temperature(T)
    if mode == "factual":
        return seq2seq_sampled(p, "encoder", num_layers, steps, inv_T, seed, top_k, features=features) + (None,)
    _, states, margin, scale = SR.greedy(p, "encoder", num_layers, steps, features=features)
    return seq2seq_sampled(p, "decoder_" + mode, num_layers, steps, inv_T, seed, top_k, start_token=start_token,
                           states=states) + ((margin, scale),)


def family_sampled(initial, n, m, steps, start_token, T, seed, top_k):
    """capnet.decode.sample_random on a restated decoder: initial(m, image) -> (step_fn, state of m rows), as the families
    of device_beam_cases give it; row i m + j is sample j of image i. -> (ids [n m, steps], logp [n m, steps], Trace)."""
    inv_T = inv_temperature(T)
    ids, logp, tr = [], [], Trace()
    for i in range(n):
        step_fn, state = initial(m, i)
        words = torch.full((m, 1), int(start_token), dtype=torch.long)
        wi, li = [], []
        for t in range(steps):
            logits, state = step_fn(words, state)
            d = draw(logits.detach(), inv_T, seed, t, i * m, top_k)
            tr.add(d)
            wi.append(d["tokens"])
            li.append(d["logp"])
            words = torch.from_numpy(d["tokens"]).view(m, 1)
        ids.append(np.stack(wi, 1))
        logp.append(np.stack(li, 1))
    return np.concatenate(ids, 0), np.concatenate(logp, 0), tr


def cut(ids, logp, n, m, start_token, end_token):
    """capnet.decode.cut_samples on the restatement's arrays."""
    out = []
    for i in range(n):
        rows = []
        for r in range(i * m, (i + 1) * m):
            q = [int(v) for v in ids[r]]
            keep = q.index(end_token) + 1 if end_token in q else len(q)
            rows.append(([int(start_token)] + q[:keep], float(np.sum(logp[r][:keep]))))
        out.append(rows)
    return out
