"""Nucleus (top-p) sampling on the GPU against the fp64 restatement (tests/nucleus_ref.py): the kernels of
csrc/vocab_nucleus.hip one by one, the one-call loops and the composed loops behind every sample_random(top_p=), route
equality, determinism and top_p = 1.0 as today's path.

Ids are compared exactly and nothing is skipped: tests/test_nucleus_cpu.py asserts the margin rule for every case of
tests/nucleus_cases.py, and the kernel tests choose their stream step on the CPU, the first at which every row of the launch
clears the rule for logits that are exact (the kernel reads the very fp32 numbers the restatement reads: what is left is
the Gumbel's error, 2 TOL_G on the key gap, and SUM_ERR on every cumulative mass). logp: within
sample_random_ref.logp_tol per word. The nucleus size: the normaliser implied by the returned logp, s_tok - logp, lies
nearer the restatement's log-sum over its nucleus than what one entry fewer or one more would give."""
import numpy as np
import pytest
import torch

import nucleus_cases as C
import nucleus_ref as N
import sample_random_ref as R
import test_sample_random_gpu as TS
from capnet import decode, ops

pytestmark = pytest.mark.gpu

ROWS = 3
KEY_NEED = 2 * R.TOL_G + 4e-6      # exact logits: the Gumbel's error on both keys and the rounding of the keys (|key| < 32)
_rows = {}


def _logits(V):
    """[ROWS, V] fp32 logits, a peaked row, a flatter one and one in between -- computed once."""
    if V not in _rows:
        g = torch.Generator().manual_seed(7 * V + 1)
        _rows[V] = torch.randn(ROWS, V, generator=g) * torch.tensor([[4.0], [1.5], [2.5]])
    return _rows[V]


def _admit(z, inv_T, top_p, seed, row0=0):
    """The first stream step at which every row of the fp32 block z clears the rule for exact logits -> (step, draw dict)."""
    for step in range(64):
        d = N.draw(z.double().numpy(), inv_T, seed, step, row0, 0, top_p, exact32=True)
        gap_ok = d["key_gaps"] > KEY_NEED
        mass_ok = d["mass_ratio"] > 0          # every cumulative mass further than SUM_ERR from top_p
        if (gap_ok & mass_ok)[d["size"] > 0].all():
            return step, d
    raise AssertionError("no step clears the rule")


def _check(tokens, logp, z, d, inv_T, what):
    """A launch against the restatement's dict: tokens exact, logp within tolerance, the nucleus size through the implied
    normaliser."""
    tokens, logp = tokens.cpu().numpy(), logp.double().cpu().numpy()
    assert tokens.dtype == np.int64 and tokens.shape == d["tokens"].shape
    assert np.array_equal(tokens, d["tokens"]), (what, tokens, d["tokens"], d["size"])
    live = d["size"] > 0
    tol = R.logp_tol(d["scale"], inv_T)
    assert np.abs(logp[live] - d["logp"][live]).max(initial=0.0) <= tol, (what, logp, d["logp"])
    assert (logp[~live] == -np.inf).all() and (tokens[~live] == 0).all()
    s = (z.numpy().astype(np.float32) * np.float32(inv_T)).astype(np.float64)
    for r in np.nonzero(live)[0]:
        implied = s[r, tokens[r]] - logp[r]
        off = abs(implied - d["lse"][r])
        assert off < abs(implied - d["lse_less"][r]) and off < abs(implied - d["lse_more"][r]), (what, r, d["size"][r])


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 31, 33, 257, 8191, 12289])      # 12289: one entry past the LDS-resident bound
def test_nucleus_rows_matches_restatement(dev, V):
    z = _logits(V)
    zd = z.to(dev)
    for T, top_p in ((1.0, 0.9), (0.5, 0.5), (2.0, 0.9), (1.0, 0.5)):
        inv_T, p32 = R.inv_temperature(T), N.top_p32(top_p)
        step, d = _admit(z, inv_T, p32, seed=V)
        tok, lp = ops.nucleus_rows(zd, temperature=T, top_p=top_p, seed=V, step=step)
        _check(tok, lp, z, d, inv_T, (V, T, top_p))
        print("V %d T %.1f top_p %.1f: nucleus sizes %s" % (V, T, top_p, d["size"].tolist()))
        # a padded block (ld > V) and one row split over two launches by row0: the same bits
        wide = torch.full((ROWS, V + 5), 9.0e9, device=dev)
        wide[:, :V] = zd
        tw, lw = ops.nucleus_rows(wide[:, :V], temperature=T, top_p=top_p, seed=V, step=step)
        assert torch.equal(tw, tok) and torch.equal(lw, lp)
        t0, l0 = ops.nucleus_rows(zd[:1], temperature=T, top_p=top_p, seed=V, step=step)
        t1, l1 = ops.nucleus_rows(zd[1:], temperature=T, top_p=top_p, seed=V, step=step, row0=1)
        assert torch.equal(torch.cat([t0, t1]), tok) and torch.equal(torch.cat([l0, l1]), lp)
        # the same call again: the same bits
        t2, l2 = ops.nucleus_rows(zd, temperature=T, top_p=top_p, seed=V, step=step)
        assert torch.equal(t2, tok) and torch.equal(l2, lp)


def test_nucleus_rows_edge_rows(dev):
    V = 70
    ninf, nan = float("-inf"), float("nan")
    z = torch.full((6, V), -30.0)
    z[0, 41] = 2.0                                       # all mass on one word
    z[1, [5, 66]] = torch.tensor([1.5, 1.0])             # mass 0.26 + 0.16 ...
    tie = [69, 8, 33, 12, 50, 21, 2, 44]                 # ... then eight equal logits, 0.072 each: top_p 0.85 keeps six of them
    z[1, tie] = 0.2
    z[2] = ninf                                          # NaN / -inf entries among a few pickable ones
    z[2, [3, 17, 40, 64]] = torch.tensor([0.3, 0.1, -0.2, 0.0])
    z[2, [0, 18, 69]] = nan
    z[3] = ninf                                          # nothing pickable
    z[3, 7] = nan
    z[4] = torch.linspace(-1, 1, V)                      # top_p tiny: the best word only
    z[5] = 1.25                                          # every logit equal: the lowest indices stay
    zd = z.to(dev)
    seen = [set() for _ in range(6)]
    for step in range(24):
        for top_p in (0.85, 1e-6):
            p32 = N.top_p32(top_p)
            d = N.draw(z.double().numpy(), 1.0, 11, step, 0, 0, p32, exact32=True)
            tok, lp = ops.nucleus_rows(zd, temperature=1.0, top_p=top_p, seed=11, step=step)
            tok, lp = tok.cpu(), lp.cpu()
            clear = (d["key_gaps"] > KEY_NEED) & (d["mass_ratio"] > 0) & (d["size"] > 0)
            assert (tok.numpy()[clear] == d["tokens"][clear]).all(), (step, top_p)
            assert np.abs(lp.double().numpy()[clear] - d["logp"][clear]).max() <= R.logp_tol(d["scale"], 1.0)
            assert int(tok[0]) == 41 and float(lp[0]) == 0.0 and d["size"][0] == 1
            assert int(tok[3]) == 0 and float(lp[3]) == ninf
            if top_p == 1e-6:                            # only the best word stays, logp exactly 0
                assert (d["size"][[0, 1, 2, 4, 5]] == 1).all()
                assert tok.tolist() == [41, 5, 3, 0, V - 1, 0] and (lp[[0, 1, 2, 4, 5]] == 0).all()
            else:
                for r in range(6):
                    seen[r].add(int(tok[r]))
    kept1 = {5, 66} | set(sorted(tie)[:N.draw(z.double().numpy(), 1.0, 11, 0, 0, 0, N.top_p32(0.85), exact32=True)["size"][1] - 2])
    assert len(kept1) == 8 and seen[1] <= kept1 and len(seen[1]) > 4       # the tie group is cut by index
    assert seen[2] <= {3, 17, 40, 64} and len(seen[2]) > 1
    n5 = int(np.ceil(N.top_p32(0.85) * V))                                    # before(j) = j / V < top_p
    assert seen[5] <= set(range(n5)) and len(seen[5]) > 5


@pytest.mark.parametrize("H,V", [(64, 37), (512, 7411)])
def test_nucleus_pick_matches_restatement(dev, H, V):
    h, W, b, _ = TS._kernel_inputs(H, V)
    hd, Wd, bd = h[:5].to(dev), W.to(dev), b.to(dev)
    for k in (1, 5, 16):
        values, index, _ = ops.vocab_topk(hd, Wd, bd, k=k)
        dense = torch.full((5, V), float("-inf"))
        dense.scatter_(1, index.long().cpu(), values.cpu())
        for T, top_p in ((1.0, 0.9), (0.5, 0.5), (2.0, 0.5)):
            inv_T, p32 = R.inv_temperature(T), N.top_p32(top_p)
            step, d = _admit(dense, inv_T, p32, seed=k)
            tok, lp = ops.nucleus_pick(values, index, V, temperature=T, top_p=top_p, seed=k, step=step)
            _check(tok, lp, dense, d, inv_T, ("pick", V, k, T, top_p))
            # the order of the list does not matter, padding slots are never picked
            perm = torch.randperm(k, generator=torch.Generator().manual_seed(k))
            pv = torch.cat([values[:, perm], torch.full_like(values[:, :1], float("-inf"))], 1).contiguous() if k < 16 else values[:, perm].contiguous()
            pi = torch.cat([index[:, perm], torch.full_like(index[:, :1], -1)], 1).contiguous() if k < 16 else index[:, perm].contiguous()
            t2, l2 = ops.nucleus_pick(pv, pi, V, temperature=T, top_p=top_p, seed=k, step=step)
            assert torch.equal(t2, tok) and torch.equal(l2, lp)
    # top_p so small that only the best candidate stays: the argmax, logp exactly 0; a row of padding gives (0, -inf)
    values, index, _ = ops.vocab_topk(hd, Wd, bd, k=5)
    tok, lp = ops.nucleus_pick(values, index, V, temperature=0.7, top_p=1e-6, seed=3, step=1)
    assert torch.equal(tok, ops.vocab_argmax(hd, Wd, bd)) and bool((lp == 0).all())
    values[2], index[2] = float("-inf"), -1
    tok, lp = ops.nucleus_pick(values, index, V, temperature=0.7, top_p=0.5, seed=3, step=1)
    assert int(tok[2]) == 0 and float(lp[2]) == float("-inf")


def test_top_p_one_is_todays_draw(dev):
    z = _logits(257).to(dev)
    a = ops.nucleus_rows(z, temperature=0.5, top_p=1.0, seed=4, step=2)
    b = ops.sample_rows(z, temperature=0.5, seed=4, step=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    values, index = torch.topk(z, 5, dim=1)
    a = ops.nucleus_pick(values.contiguous(), index.int().contiguous(), 257, temperature=0.5, top_p=1.0, seed=4, step=2)
    b = ops.sample_pick(values.contiguous(), index.int().contiguous(), 257, temperature=0.5, seed=4, step=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 2. capnet.seq2seq ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SEQ2SEQ))
def test_seq2seq_nucleus_matches_restatement(dev, monkeypatch, name):
    c, p, feats, s, (ids_r, logp_r, states_r, tr, _) = C.seq2seq_reference(name)
    inv_T = R.inv_temperature(s["T"])
    m = TS._seq_model(p, c, dev)
    f = feats.float().to(dev)
    kw = dict(temperature=s["T"], top_k=s["top_k"], top_p=s["top_p"], seed=s["seed"])
    calls = TS._count_calls(monkeypatch, "sample_decode")
    runs = TS._routes(monkeypatch, lambda: m.sample_random(f, 1, mode=c["mode"], **kw), calls)
    tol = R.logp_tol(tr.scale, inv_T)
    for route, (ids, logp) in runs.items():
        assert ids.dtype == torch.int64 and tuple(ids.shape) == (c["rows"], 40) and tuple(logp.shape) == (c["rows"], 40)
        assert np.array_equal(ids.cpu().numpy(), ids_r), (name, route)
        err = np.abs(logp.double().cpu().numpy() - logp_r).max()
        print("%s %s: logp error %.3g (tolerance %.3g), nucleus %s..%s" % (name, route, err, tol, tr.min_size, tr.max_size))
        assert err <= tol, (name, route)


def test_seq2seq_nucleus_rows_routes_agree_at_12_rows(dev, monkeypatch):
    """V 7411 at 12 rows without top_k, where no stream seed clears the margin rule (tests/nucleus_cases.py): the one call
    and the composed loop on the fused step run the same kernels on the same logits, so they return the same bits; the
    same seed twice returns the same bits; top_p = 1.0 is the call without the keyword."""
    c, p, feats = TS.SC.greedy_case("r12_l2_v7411")
    m = TS._seq_model(p, c, dev)
    f = feats.float().to(dev)
    kw = dict(temperature=0.5, top_p=0.5, seed=9)
    monkeypatch.setattr(decode, "FUSED_NUCLEUS_MAX_ROWS", 12)       # the one call at 12 rows, whatever the threshold is
    calls = TS._count_calls(monkeypatch, "sample_decode")
    runs = TS._routes(monkeypatch, lambda: m.sample_random(f, 1, **kw), calls)
    a, b = runs["one_call"], runs["no_fused_sample"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    again = m.sample_random(f, 1, **kw)
    assert torch.equal(again[0], a[0]) and torch.equal(again[1], a[1])
    assert bool(torch.isfinite(a[1]).all()) and bool((a[1] <= 0).all())
    off = m.sample_random(f, 1, temperature=0.5, seed=9)
    assert not torch.equal(off[0], a[0])
    one = m.sample_random(f, 1, temperature=0.5, top_p=1.0, seed=9)
    assert torch.equal(one[0], off[0]) and torch.equal(one[1], off[1])
    # top_k too: top_p = 1.0 against the call without the keyword
    x = m.sample_random(f, 1, temperature=2.0, top_k=5, seed=9)
    y = m.sample_random(f, 1, temperature=2.0, top_k=5, top_p=1.0, seed=9)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


# ---- 3. the image decoders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.IMAGE_CASES, ids=[c["id"] for c in C.IMAGE_CASES])
def test_image_decoder_nucleus_matches_restatement(dev, monkeypatch, case):
    ids_r, logp_r, tr = C.image_reference(case)
    fam, dec, f = TS._decoder(case, dev)
    tol = R.logp_tol(tr.scale, R.inv_temperature(case["T"]))
    kw = dict(samples=C.SAMPLES, temperature=case["T"], top_k=case["top_k"], top_p=case["top_p"], seed=case["seed"], **fam.kw)
    monkeypatch.setattr(decode, "FUSED_NUCLEUS_MAX_ROWS", 12)       # the one call without top_k too, whatever the threshold is
    calls = TS._count_calls(monkeypatch, "sample_decode", "att_sample_decode")
    no_end = fam.V                                           # never drawn: all MAX_LEN words
    runs = TS._routes(monkeypatch, lambda: dec.sample_random(f, C.START, no_end, **kw), calls)
    want = R.cut(ids_r, logp_r, C.IMAGES, C.SAMPLES, C.START, no_end)
    for route, got in runs.items():
        assert all(len(q) == C.MAX_LEN + 1 for img in got for q, _ in img), route
        TS._same_lists(got, want, tol)
    # the same seed again: the same lists
    assert dec.sample_random(f, C.START, no_end, **kw) == runs["one_call"]


def test_image_decoder_top_p_one_is_todays_path(dev):
    for cid in ("DecoderRNNAtt-p4-k0-p0.9", "DecoderFactoredLSTM-k5-p0.9"):
        case = [c for c in C.IMAGE_CASES if c["id"] == cid][0]
        fam, dec, f = TS._decoder(case, dev)
        kw = dict(samples=3, temperature=case["T"], top_k=case["top_k"], seed=31, **fam.kw)
        assert dec.sample_random(f, C.START, fam.V, top_p=1.0, **kw) == dec.sample_random(f, C.START, fam.V, **kw)
        assert dec.sample_random(f, C.START, fam.V, top_p=0.5, **kw) != dec.sample_random(f, C.START, fam.V, **kw)
    # more rows than the one-call route takes: the composed loop, the same lists
    want = dec.sample_random(f, C.START, fam.V, top_p=0.5, **kw)
    old = decode.FUSED_NUCLEUS_TOPK_MAX_ROWS
    try:
        decode.FUSED_NUCLEUS_TOPK_MAX_ROWS = 5
        assert [q for img in dec.sample_random(f, C.START, fam.V, top_p=0.5, **kw) for q, _ in img] == \
            [q for img in want for q, _ in img]
    finally:
        decode.FUSED_NUCLEUS_TOPK_MAX_ROWS = old
