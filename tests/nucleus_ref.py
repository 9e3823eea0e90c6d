"""fp64 restatement of nucleus (top-p) sampling (csrc/vocab_nucleus.hip, capnet.decode.sample_random(top_p=),
capnet.seq2seq's sample_random(top_p=)) on top of sample_random_ref's stream, Gumbel noise and Trace. TEST INFRASTRUCTURE;
the reference project has no sampler, nothing here is reference-pinned.

  per row and step:  s_v = z_v / T over the pickable entries (not NaN, not -inf), p = softmax(s), the entries ordered by s
  descending then index ascending, before(v) = the sum of p_u over the entries strictly better than v,
  N = { v : before(v) < top_p }, the draw Gumbel-max over N on the stream keyed by the vocabulary index,
  logp = s_tok - log sum_{v in N} exp(s_v). top_k > 0: all of it among the k best entries, renormalised over them.

  * nucleus / nucleus_by_definition: N by sort + cumulative sum, and straight from the definition (tests compare the two).
  * draw: one step's draw of every row, with what the margin rule needs (below).
  * kernel_sum32 / kernel_mass_error: the kernel's fixed-order fp32 sum restated in numpy, and the error of the normalised
    mass it compares with top_p -- the measurement behind SUM_ERR.
  * the loops: seq2seq_sample_random, family_sampled (sample_random_ref's with this draw).

The margin rule -- when a GPU run must return the restatement's tokens exactly. At every row and step:
  (a) the two best keys AMONG THE KEPT entries are further apart than R.need(scale, 1 / T);
  (b) the last kept and the first dropped scaled logit are further apart than R.need_kth(scale) / T, or the two sides may
      order them differently;
  (c) every cumulative mass C_j along the order is further from top_p than the error a device may carry in it:
      2 (2 TOL_STEP scale / T) C_j -- the logits' error through numerator and normaliser -- plus SUM_ERR, the fp32 error of
      the kernel's sums;
  top_k > 0: also sample_random_ref's k-th / (k + 1)-th rule.
"""
import numpy as np
import torch

import sample_random_ref as R
import seq2seq_ref as SR

# Twice the largest |fp32 kernel-order mass - fp64 mass| (normalised, at the entries around the edge, the rounding of the
# product top_p S and numpy's fp32 exp included) seen over every row and step of tests/nucleus_cases.py: 1.91e-7
# (DecoderRNNAtt-p4 at top_p 0.9; test_nucleus_cpu.py re-measures it with every case).
SUM_ERR = 4.0e-7


def top_p32(top_p):
    """top_p as the kernels compare it: rounded once to fp32."""
    return float(np.float32(top_p))


def _pickable(z_row):
    cols = np.arange(z_row.shape[0])
    ok = z_row > -np.inf                      # NaN fails
    return cols[ok], z_row[ok]


def nucleus(s, idx, top_p):
    """-> (order, n, C): the entries' positions in the total order (s descending, idx ascending), the nucleus size n (the
    nucleus is order[:n]) and the cumulative masses C along the order, C[j] = before(order[j + 1])."""
    order = np.lexsort((idx, -s))
    e = np.exp(s[order] - s.max())
    C = np.cumsum(e / e.sum())
    before = np.concatenate(([0.0], C[:-1]))
    keep = before < top_p
    n = int(keep.sum())
    assert keep[:n].all()
    return order, n, C


def nucleus_by_definition(s, idx, top_p):
    """The set { j : before(j) < top_p } straight from the definition: before(j) sums p over the entries strictly better
    than j, found by comparing every pair. O(n^2): small rows only."""
    e = np.exp(s - s.max())
    p = e / e.sum()
    better = (s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (idx[None, :] < idx[:, None]))   # [j, u]: u better than j
    before = np.array([p[better[j]].sum() for j in range(len(s))])
    return set(int(i) for i in idx[before < top_p])


def draw(logits, inv_T, seed, step, row0=0, top_k=0, top_p=1.0, exact32=False):
    """One step's nucleus draw for every row of logits [rows, V] (taken as fp64): row r on stream row row0 + r. top_p is
    compared as given (pass top_p32's value). exact32: the logits are the very fp32 numbers a kernel reads, and s is formed
    as the kernel forms it, fl32(z fl32(1 / T)) -- the order and the ties are then the kernel's, exactly.
    -> sample_random_ref.draw's dict (key gaps AMONG THE KEPT entries) and, per row: size (the nucleus size), edge_gap (last kept s - first dropped s; inf where nothing is dropped), mass_ratio
    (min over j of (|C_j - top_p| - SUM_ERR) / C_j: rule (c) asks it to exceed 4 TOL_STEP scale / T), below / above (the
    distances from top_p of the cumulative masses on both sides of the edge), lse (log sum exp over the kept entries) and
    lse_less / lse_more (the same with one entry fewer / one more kept: what a wrong nucleus size would give)."""
    z = np.asarray(torch.as_tensor(logits, dtype=torch.float64).numpy() if isinstance(logits, torch.Tensor) else logits,
                   dtype=np.float64)
    rows = z.shape[0]
    out = dict(tokens=np.zeros(rows, dtype=np.int64), logp=np.full(rows, -np.inf), key_gaps=np.full(rows, np.inf),
               kth_gaps=np.full(rows, np.inf), size=np.zeros(rows, dtype=np.int64), edge_gap=np.full(rows, np.inf),
               mass_ratio=np.full(rows, np.inf), below=np.full(rows, np.inf), above=np.full(rows, np.inf),
               lse=np.full(rows, -np.inf), lse_less=np.full(rows, -np.inf), lse_more=np.full(rows, np.inf))
    scale = 0.0
    for r in range(rows):
        cand, zr = _pickable(z[r])
        if cand.size == 0:
            continue
        scale = max(scale, float(np.abs(zr[np.isfinite(zr)]).max()) if np.isfinite(zr).any() else 0.0)
        if top_k:
            order = np.lexsort((cand, -zr))
            if cand.size > top_k:
                out["kth_gaps"][r] = float(zr[order[top_k - 1]] - zr[order[top_k]])
            cand, zr = cand[order[:top_k]], zr[order[:top_k]]
        s = (zr.astype(np.float32) * np.float32(inv_T)).astype(np.float64) if exact32 else zr * inv_T
        order, n, C = nucleus(s, cand, top_p)
        so = s[order]
        out["size"][r] = n
        if n < cand.size:
            out["edge_gap"][r] = float(so[n - 1] - so[n])
        out["mass_ratio"][r] = float(((np.abs(C - top_p) - SUM_ERR) / C).min())
        out["below"][r] = float(top_p - C[n - 2]) if n >= 2 else float(top_p)
        out["above"][r] = float(C[n - 1] - top_p)
        m = so[0]
        lse = lambda q: float(m + np.log(np.exp(so[:q] - m).sum())) if q >= 1 else -np.inf
        out["lse"][r], out["lse_less"][r] = lse(n), lse(n - 1)
        out["lse_more"][r] = lse(n + 1) if n < cand.size else np.inf
        kept, sk = cand[order[:n]], so[:n]
        key = sk + R.gumbel(R.uniform_np(seed, step, row0 + r, kept))
        ko = np.lexsort((kept, -key))
        if n > 1:
            out["key_gaps"][r] = float(key[ko[0]] - key[ko[1]])
        out["tokens"][r] = int(kept[ko[0]])
        out["logp"][r] = float(sk[ko[0]] - out["lse"][r])
    out.update(key_gap=float(out["key_gaps"].min()), kth_gap=float(out["kth_gaps"].min()), scale=scale)
    return out


class Trace(R.Trace):
    """sample_random_ref.Trace with the nucleus' quantities: the smallest and largest nucleus, the smallest edge gap, the
    smallest mass ratio and the smallest distances from top_p on both sides of the edge."""

    def __init__(self):
        super().__init__()
        self.min_size, self.max_size = np.inf, 0
        self.edge_gap = self.mass_ratio = self.below = self.above = np.inf

    def add(self, d):
        super().add(d)
        live = d["size"] > 0
        if live.any():
            self.min_size, self.max_size = min(self.min_size, int(d["size"][live].min())), max(self.max_size, int(d["size"].max()))
        for name in ("edge_gap", "mass_ratio", "below", "above"):
            setattr(self, name, min(getattr(self, name), float(d[name].min())))


def clears(tr, inv_T, top_k):
    """The margin rule on a Trace -> the list of what fails (empty: admitted)."""
    fails = []
    if not tr.key_gap > R.need(tr.scale, inv_T):
        fails.append("key gap %.3g <= %.3g" % (tr.key_gap, R.need(tr.scale, inv_T)))
    if not tr.edge_gap > R.need_kth(tr.scale) * inv_T:
        fails.append("edge gap %.3g <= %.3g" % (tr.edge_gap, R.need_kth(tr.scale) * inv_T))
    if not tr.mass_ratio > 4 * R.TOL_STEP * tr.scale * inv_T:
        fails.append("mass ratio %.3g <= %.3g" % (tr.mass_ratio, 4 * R.TOL_STEP * tr.scale * inv_T))
    if top_k and not tr.kth_gap > R.need_kth(tr.scale):
        fails.append("k-th gap %.3g <= %.3g" % (tr.kth_gap, R.need_kth(tr.scale)))
    return fails


# ---- the kernel's sums, restated in fp32 --------------------------------------------------------------------------------
def kernel_sum32(e):
    """nucleus_rows_kernel's sum of the fp32 array e (entries outside the set already zero): thread t adds entries t, t + 256,
    ... in that order, a wave's 64 partials meet in the xor tree (offsets 32 .. 1), the four waves' sums are added in order."""
    e = np.asarray(e, dtype=np.float32)
    pad = (-e.size) % 256
    a = np.concatenate([e, np.zeros(pad, dtype=np.float32)]).reshape(-1, 256)
    acc = np.zeros(256, dtype=np.float32)
    for chunk in a:
        acc = acc + chunk
    lanes = acc.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(64) ^ o]
    t = lanes[0, 0]
    for w in (1, 2, 3):
        t = np.float32(t + lanes[w, 0])
    return np.float32(t)


def kernel_mass_error(z_row, inv_T, top_p, top_k=0):
    """The largest |fp32 mass - fp64 mass| at the entries around the edge of one row, both on the fp32 roundings of the row:
    the fp32 side is what the kernel compares, before(v) / (fl32(top_p S) / top_p) from kernel_sum32 (top_k > 0:
    nucleus_pick_kernel's sums in the total order), the fp64 side the exact normalised mass."""
    cand, zr = _pickable(np.asarray(z_row, dtype=np.float64))
    if cand.size == 0:
        return 0.0
    z32 = zr.astype(np.float32)
    if top_k:
        o = np.lexsort((cand, -z32))[:top_k]
        cand, z32 = cand[o], z32[o]
    s32 = (z32 * np.float32(inv_T)).astype(np.float32)
    order, n, C = nucleus(s32.astype(np.float64), cand, top_p)
    e32 = np.exp((s32 - s32.max()).astype(np.float32)).astype(np.float32)
    rank = np.empty(cand.size, dtype=np.int64)
    rank[order] = np.arange(cand.size)
    if top_k:
        total = lambda mask: np.cumsum(np.where(mask, e32, np.float32(0))[order], dtype=np.float32)[-1]
    else:
        full = np.zeros(int(cand.max()) + 1, dtype=np.float32)

        def total(mask):
            full[:] = 0
            full[cand] = np.where(mask, e32, np.float32(0))
            return kernel_sum32(full)
    S = total(np.ones(cand.size, dtype=bool))
    edge = np.float32(np.float32(top_p) * S)
    worst = 0.0
    for j in range(max(n - 1, 1), min(n + 2, cand.size)):          # before(order[j]) = C[j - 1]
        got = float(total(rank < j)) / (float(edge) / top_p)
        worst = max(worst, abs(got - float(C[j - 1])))
    return worst


# ---- the loops (sample_random_ref's, with the nucleus draw) -------------------------------------------------------------
def seq2seq_sampled(p, prefix, num_layers, steps, inv_T, seed, top_k, top_p, features=None, start_token=None, states=None,
                    on_logits=None):
    """sample_random_ref.seq2seq_sampled with the nucleus draw. on_logits(t, logits): called with every step's logits."""
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
        logits = SR._logits(p, prefix, top)
        if on_logits:
            on_logits(t, logits)
        d = draw(logits, inv_T, seed, t, 0, top_k, top_p)
        tr.add(d)
        ids.append(d["tokens"])
        logp.append(d["logp"])
        x = emb_w[torch.from_numpy(d["tokens"])]
    return np.stack(ids, 1), np.stack(logp, 1), (torch.stack(hs), torch.stack(cs)), tr


def seq2seq_sample_random(p, num_layers, steps, features, start_token, mode, T, seed, top_k, top_p, on_logits=None):
    """Seq2Seq.sample_random(top_p=) -> (ids, logp, the sampler's final (h, c), Trace, the encoder's greedy (margin, scale) or
    None)."""
    inv_T, top_p = R.inv_temperature(T), top_p32(top_p)
    if mode == "factual":
        return seq2seq_sampled(p, "encoder", num_layers, steps, inv_T, seed, top_k, top_p, features=features,
                               on_logits=on_logits) + (None,)
    _, states, margin, scale = SR.greedy(p, "encoder", num_layers, steps, features=features)
    return seq2seq_sampled(p, "decoder_" + mode, num_layers, steps, inv_T, seed, top_k, top_p, start_token=start_token,
                           states=states, on_logits=on_logits) + ((margin, scale),)


def family_sampled(initial, n, m, steps, start_token, T, seed, top_k, top_p, on_logits=None):
    """sample_random_ref.family_sampled with the nucleus draw -> (ids [n m, steps], logp [n m, steps], Trace)."""
    inv_T, top_p = R.inv_temperature(T), top_p32(top_p)
    ids, logp, tr = [], [], Trace()
    for i in range(n):
        step_fn, state = initial(m, i)
        words = torch.full((m, 1), int(start_token), dtype=torch.long)
        wi, li = [], []
        for t in range(steps):
            logits, state = step_fn(words, state)
            if on_logits:
                on_logits(t, logits.detach())
            d = draw(logits.detach(), inv_T, seed, t, i * m, top_k, top_p)
            tr.add(d)
            wi.append(d["tokens"])
            li.append(d["logp"])
            words = torch.from_numpy(d["tokens"]).view(m, 1)
        ids.append(np.stack(wi, 1))
        logp.append(np.stack(li, 1))
    return np.concatenate(ids, 0), np.concatenate(logp, 0), tr
