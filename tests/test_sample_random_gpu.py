"""Sampled decoding on the GPU against the fp64 restatement (tests/sample_random_ref.py): the kernels of
csrc/vocab_sample.hip one by one, the one-call loops and the composed loops behind every sample_random, route equality,
determinism and truncation.

Ids are compared exactly: tests/test_sample_random_cpu.py asserts the margin rule for every case of
tests/sample_random_cases.py. In the kernel tests, whose inputs are plain random rows, a row is compared where ITS gap
clears the rule (the form of test_vocab_argmax_matches_composed_and_fp64), and all but at most one row of a launch must.
logp: within 2 TOL_STEP max|logit| / T + 1e-6 per word (sample_random_ref.logp_tol)."""
import numpy as np
import pytest
import torch

import sample_random_cases as C
import sample_random_ref as R
import seq2seq_cases as SC
import vocab_edge_cases as VC
from capnet import decode, ops
from capnet.decode import FUSED_DECODE_OFF, FUSED_SAMPLE_OFF
from capnet.seq2seq import Seq2Seq

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 16, 17, 32, 33)      # one tile, a partial tile, the pass boundaries of TM = 2 (32 rows) and TM = 1 (16 rows)
TEMPS = (0.5, 1.0, 2.0)
_inputs = {}


def _kernel_inputs(H, V):
    """(h [33, H], W [V, H], b [V]) fp32 on the CPU and the fp64 logits with and without the bias -- computed once."""
    if (H, V) not in _inputs:
        g = torch.Generator().manual_seed(3 * V + H)
        W = torch.randn(V, H, generator=g) * (2.0 / H ** 0.5)
        b = torch.randn(V, generator=g) * 0.1
        h = torch.rand(max(ROWS), H, generator=g) * 2 - 1
        nb = h.double() @ W.double().t()
        _inputs[(H, V)] = (h, W, b, {True: (nb + b.double()).numpy(), False: nb.numpy()})
    return _inputs[(H, V)]


def _check(tokens, logp, d, inv_T, top_k=0, what=""):
    """tokens / logp of a launch against draw()'s dict `d`, on the rows whose gaps clear the rule."""
    clear = d["key_gaps"] > R.need(d["scale"], inv_T)
    if top_k:
        clear &= d["kth_gaps"] > R.need_kth(d["scale"])
    rows = len(clear)
    assert clear.sum() >= rows - 1, what
    tokens, logp = tokens.cpu().numpy(), logp.double().cpu().numpy()
    assert tokens.dtype == np.int64 and tokens.shape == (rows,) and logp.shape == (rows,)
    assert (tokens[clear] == d["tokens"][clear]).all(), what
    err = np.abs(logp[clear] - d["logp"][clear]).max() if clear.any() else 0.0
    assert err <= R.logp_tol(d["scale"], inv_T), (what, err)
    return err


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 512, 1024])
@pytest.mark.parametrize("V", [37, 7411, 8192])
def test_vocab_sample_matches_restatement(dev, H, V):
    h, W, b, z = _kernel_inputs(H, V)
    hd, Wd, bd = h.to(dev), W.to(dev), b.to(dev)
    worst, step = 0.0, 0
    for rows in ROWS:
        for bias in (True, False):
            for T in TEMPS:
                step += 1
                inv_T = R.inv_temperature(T)
                tok, lp = ops.vocab_sample(hd[:rows], Wd, bd if bias else None, temperature=T, seed=V + rows, step=step)
                d = R.draw(z[bias][:rows], inv_T, V + rows, step)
                worst = max(worst, _check(tok, lp, d, inv_T, what=(rows, bias, T)))
    print("vocab_sample H %d V %d: worst logp error %.3g" % (H, V, worst))


@pytest.mark.parametrize("H,V", [(64, 37), (512, 7411), (1024, 8192)])
def test_vocab_sample_row0_and_counter_rearm(dev, H, V):
    h, W, b, z = _kernel_inputs(H, V)
    hd, Wd, bd = h.to(dev), W.to(dev), b.to(dev)
    tok, lp = ops.vocab_sample(hd, Wd, bd, temperature=0.5, seed=77, step=3)
    for r0, r1 in ((5, 17), (16, 33), (32, 33)):       # a slice of the rows on its own launch draws the same stream
        t2, l2 = ops.vocab_sample(hd[r0:r1], Wd, bd, temperature=0.5, seed=77, step=3, row0=r0)
        assert torch.equal(t2, tok[r0:r1]) and torch.equal(l2, lp[r0:r1]), (r0, r1)
    t0, _ = ops.vocab_sample(hd[5:17], Wd, bd, temperature=0.5, seed=77, step=3)      # ... and another without the offset
    assert not torch.equal(t0, tok[5:17])
    # launches back to back on one workspace: the counter re-arms, the results are those of fresh workspaces, bit for bit
    ws = ops.vocab_sample_workspace(33, V, dev)
    outs = [ops.vocab_sample(hd, Wd, bd, temperature=1.0, seed=s, step=s, workspace=ws) for s in range(6)]
    torch.cuda.synchronize()
    assert int(ws[0].item()) & 0xffffffff == 0
    for s, (a, la) in enumerate(outs):
        f, lf = ops.vocab_sample(hd, Wd, bd, temperature=1.0, seed=s, step=s)
        assert torch.equal(a, f) and torch.equal(la, lf)
    assert len({tuple(a.tolist()) for a, _ in outs}) > 1


@pytest.mark.parametrize("case", VC.SAMPLE, ids=VC.case_id)
def test_vocab_sample_edges_of_the_shared_front(dev, case):
    """258 workgroups (the second pass of the last arriver's loops: winners and a fifth of the sum lie there) and one
    workgroup (the only arriver is the last): tests/vocab_edge_cases.py, _check's rule."""
    h, W, b, z = VC.sample_inputs(*case)
    hd, Wd, bd = h.to(dev), W.to(dev), b.to(dev)
    for T, inv_T, seed, step in VC.sample_launches(*case):
        tok, lp = ops.vocab_sample(hd, Wd, bd, temperature=T, seed=seed, step=step)
        _check(tok, lp, R.draw(z, inv_T, seed, step), inv_T, what=(case, T, step))


def test_vocab_sample_never_draws_nan_or_minus_inf(dev):
    H, V, rows = 64, 200, 19
    g = torch.Generator().manual_seed(4)
    W = torch.randn(V, H, generator=g) * 0.25
    h = torch.rand(rows, H, generator=g) * 2 - 1
    b = torch.full((V,), float("-inf"))
    b[3] = float("nan")
    b[150] = float("nan")
    pick = [7, 40, 41, 77, 199]
    b[pick] = torch.tensor([0.1, -0.2, 0.3, 0.0, 0.2])
    h[11] = float("nan")                                   # a row with nothing to pick
    z = (h.double() @ W.double().t() + b.double()).numpy()
    hd, Wd, bd = h.to(dev), W.to(dev), b.to(dev)
    seen = set()
    for step in range(40):
        tok, lp = ops.vocab_sample(hd, Wd, bd, temperature=1.0, seed=1, step=step)
        rws, _ = ops.sample_rows(ops.linear(hd, Wd, bd), temperature=1.0, seed=1, step=step)
        tok, lp, rws = tok.cpu(), lp.cpu(), rws.cpu()
        d = R.draw(z, 1.0, 1, step)
        assert int(tok[11]) == 0 and float(lp[11]) == float("-inf") and int(rws[11]) == 0
        live = [r for r in range(rows) if r != 11]
        assert all(int(tok[r]) in pick for r in live) and torch.isfinite(lp[live]).all()
        clear = d["key_gaps"] > R.need(d["scale"], 1.0)
        clear[11] = False
        assert (tok.numpy()[clear] == d["tokens"][clear]).all() and (rws.numpy()[clear] == d["tokens"][clear]).all()
        assert np.abs(lp.double().numpy()[clear] - d["logp"][clear]).max() <= R.logp_tol(d["scale"], 1.0)
        seen |= set(tok[live].tolist())
    assert seen == set(pick)                               # over 40 steps x 18 rows every pickable entry is drawn


@pytest.mark.parametrize("H,V", [(64, 37), (512, 7411), (1024, 8192)])
def test_sample_rows_and_sample_pick_match_restatement(dev, H, V):
    h, W, b, z = _kernel_inputs(H, V)
    hd, Wd, bd = h.to(dev), W.to(dev), b.to(dev)
    for rows in ROWS:
        for T in TEMPS:
            inv_T, seed, step = R.inv_temperature(T), 5 * rows, rows
            logits = ops.linear(hd[:rows], Wd, bd)
            tok, lp = ops.sample_rows(logits, temperature=T, seed=seed, step=step)
            d = R.draw(z[True][:rows], inv_T, seed, step)
            _check(tok, lp, d, inv_T, what=("rows", rows, T))
            # on the logits of the same inputs sample_rows draws the tokens vocab_sample drew
            vt, _ = ops.vocab_sample(hd[:rows], Wd, bd, temperature=T, seed=seed, step=step)
            clear = torch.from_numpy(d["key_gaps"] > R.need(d["scale"], inv_T))
            assert torch.equal(vt.cpu()[clear], tok.cpu()[clear])
            # a padded block (ld > V)
            wide = torch.full((rows, V + 3), 9.0e9, device=dev)
            wide[:, :V] = logits
            tw, lw = ops.sample_rows(wide[:, :V], temperature=T, seed=seed, step=step)
            assert torch.equal(tw, tok) and torch.equal(lw, lp)
            for k in (1, 5, 16):
                values, index, _ = ops.vocab_topk(hd[:rows], Wd, bd, k=k)
                pt, pl = ops.sample_pick(values, index, V, temperature=T, seed=seed, step=step)
                dk = R.draw(z[True][:rows], inv_T, seed, step, 0, k)
                _check(pt, pl, dk, inv_T, top_k=k, what=("pick", rows, T, k))
    # top_k = 1 is the argmax with log-probability 0
    values, index, _ = ops.vocab_topk(hd, Wd, bd, k=1)
    pt, pl = ops.sample_pick(values, index, V, temperature=0.5, seed=3, step=1)
    assert torch.equal(pt, ops.vocab_argmax(hd, Wd, bd)) and bool((pl == 0).all())
    # padding slots (-inf, -1) are never picked; a row of padding gives (0, -inf)
    values, index = values.repeat(1, 3).contiguous(), index.repeat(1, 3).contiguous()
    values[:, 1:], index[:, 1:] = float("-inf"), -1
    values[2], index[2] = float("-inf"), -1
    pt2, pl2 = ops.sample_pick(values, index, V, temperature=0.5, seed=3, step=1)
    keep = torch.arange(pt.numel(), device=dev) != 2
    assert torch.equal(pt2[keep], pt[keep]) and bool((pl2[keep] == 0).all())
    assert int(pt2[2]) == 0 and float(pl2[2]) == float("-inf")


# ---- 2. capnet.seq2seq ------------------------------------------------------------------------------------------------------
def _seq_model(p, c, dev):
    m = Seq2Seq(c["E"], c["H"], c["V"], c["layers"], dropout=0.0)
    m.load_state_dict({k: v.float() for k, v in p.items()}, strict=True)
    return m.to(dev).eval()


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _routes(monkeypatch, run, calls=None):
    """run() on the one-call route, with CAPNET_NO_FUSED_SAMPLE=1 and with CAPNET_NO_FUSED_DECODE_STEP=1."""
    out = {}
    for name, env in (("one_call", None), ("no_fused_sample", FUSED_SAMPLE_OFF), ("no_fused_step", FUSED_DECODE_OFF)):
        monkeypatch.delenv(FUSED_SAMPLE_OFF, raising=False)
        monkeypatch.delenv(FUSED_DECODE_OFF, raising=False)
        if env:
            monkeypatch.setenv(env, "1")
        before = None if calls is None else calls[0]
        out[name] = run()
        if calls is not None:          # the one C call runs on the default route and only there
            assert (calls[0] - before == 1) == (env is None), name
    monkeypatch.delenv(FUSED_SAMPLE_OFF, raising=False)
    monkeypatch.delenv(FUSED_DECODE_OFF, raising=False)
    return out


def _count_calls(monkeypatch, *names):
    calls = [0]
    for name in names:
        real = getattr(ops, name)

        def counted(*a, _real=real, **kw):
            calls[0] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls


@pytest.mark.parametrize("name", sorted(C.SEQ2SEQ))
def test_seq2seq_sample_random_matches_restatement(dev, monkeypatch, name):
    c, p, feats, s, (ids_r, logp_r, states_r, tr, _) = C.seq2seq_reference(name)
    inv_T = R.inv_temperature(s["T"])
    m = _seq_model(p, c, dev)
    f = feats.float().to(dev)
    kw = dict(temperature=s["T"], top_k=s["top_k"], seed=s["seed"])
    calls = _count_calls(monkeypatch, "sample_decode")
    runs = _routes(monkeypatch, lambda: m.sample_random(f, 1, mode=c["mode"], **kw), calls)
    tol = R.logp_tol(tr.scale, inv_T)
    for route, (ids, logp) in runs.items():
        assert ids.dtype == torch.int64 and tuple(ids.shape) == (c["rows"], 40) and tuple(logp.shape) == (c["rows"], 40)
        assert np.array_equal(ids.cpu().numpy(), ids_r), (name, route)
        err = np.abs(logp.double().cpu().numpy() - logp_r).max()
        print("%s %s: logp error %.3g (tolerance %.3g)" % (name, route, err, tol))
        assert err <= tol, (name, route)
    if c["mode"] == "factual":          # the encoder's own method also returns the final states
        for route, (ids, logp, (h, cc)) in _routes(monkeypatch, lambda: m.encoder.sample_random(f, **kw)).items():
            assert np.array_equal(ids.cpu().numpy(), ids_r)
            assert _rel(h, states_r[0]) < R.TOL_STEP and _rel(cc, states_r[1]) < R.TOL_STEP, route
    else:                               # a call numbers its rows from 0: row 0 of the batch is the one-row call's row
        one = m.sample_random(f[:1], 1, mode=c["mode"], **kw)[0]
        assert torch.equal(one[0], runs["one_call"][0][0])


def test_seq2seq_top_k_1_is_greedy(dev):
    c, p, feats = SC.greedy_case("r12_l1_v8192")
    m = _seq_model(p, c, dev)
    f = feats.float().to(dev)
    ids, logp = m.sample_random(f, 1, temperature=0.7, top_k=1, seed=5)
    assert torch.equal(ids, m.sample(f, 1)) and bool((logp == 0).all())
    c, p, feats = SC.greedy_case("sad_r1_l2_v7411")
    m = _seq_model(p, c, dev)
    ids, logp = m.sample_random(feats.float().to(dev), 1, mode="sad", top_k=1, seed=6)
    assert torch.equal(ids, m.sample(feats.float().to(dev), 1, mode="sad")) and bool((logp == 0).all())


def test_seq2seq_determinism(dev):
    c, p, feats, s, _ = C.seq2seq_reference("r12_l2_v7411")
    m = _seq_model(p, c, dev)
    f = feats.float().to(dev)
    a = m.sample_random(f, 1, temperature=1.0, seed=123)
    b = m.sample_random(f, 1, temperature=1.0, seed=123)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], m.sample_random(f, 1, temperature=1.0, seed=124)[0])
    torch.manual_seed(9)
    x = m.sample_random(f, 1)
    y = m.sample_random(f, 1)
    torch.manual_seed(9)
    x2 = m.sample_random(f, 1)
    assert torch.equal(x[0], x2[0]) and torch.equal(x[1], x2[1]) and not torch.equal(x[0], y[0])


# ---- 3. the image decoders ----------------------------------------------------------------------------------------------------
def _decoder(case, dev):
    fam = C.families()[case["family"]]
    dec = fam.make().to(dev).eval()
    return fam, dec, fam.features()[:C.IMAGES].to(dev)


def _same_lists(got, want, tol_word):
    assert len(got) == len(want)
    for gi, wi in zip(got, want):
        assert len(gi) == len(wi)
        for (gt, gl), (wt, wl) in zip(gi, wi):
            assert gt == wt, (gt, wt)
            assert abs(gl - wl) <= tol_word * (len(wt) - 1), (gl, wl)


@pytest.mark.parametrize("case", C.IMAGE_CASES, ids=[c["id"] for c in C.IMAGE_CASES])
def test_image_decoder_sample_random_matches_restatement(dev, monkeypatch, case):
    ids_r, logp_r, tr = C.image_reference(case)
    fam, dec, f = _decoder(case, dev)
    tol = R.logp_tol(tr.scale, R.inv_temperature(case["T"]))
    kw = dict(samples=C.SAMPLES, temperature=case["T"], top_k=case["top_k"], seed=case["seed"], **fam.kw)
    calls = _count_calls(monkeypatch, "sample_decode", "att_sample_decode")
    no_end = fam.V                                           # never drawn: all MAX_LEN words
    runs = _routes(monkeypatch, lambda: dec.sample_random(f, C.START, no_end, **kw), calls)
    want = R.cut(ids_r, logp_r, C.IMAGES, C.SAMPLES, C.START, no_end)
    for route, got in runs.items():
        assert all(len(q) == C.MAX_LEN + 1 for img in got for q, _ in img), route
        _same_lists(got, want, tol)
    # truncation: an end token the restatement draws early cuts the lists after it; logprob sums the kept words only
    end = C.early_end(ids_r)
    cut = dec.sample_random(f, C.START, end, **kw)
    _same_lists(cut, R.cut(ids_r, logp_r, C.IMAGES, C.SAMPLES, C.START, end), tol)
    assert len(cut[0][0][0]) <= 5 and cut[0][0][0][-1] == end
    # the samples of one image are not all equal
    assert any(len({tuple(q) for q, _ in img}) > 1 for img in runs["one_call"])


def test_image_decoder_determinism(dev):
    case = [c for c in C.IMAGE_CASES if c["id"] == "DecoderRNNAtt-p4-k0"][0]
    fam, dec, f = _decoder(case, dev)
    a = dec.sample_random(f, C.START, fam.V, samples=3, seed=31)
    assert a == dec.sample_random(f, C.START, fam.V, samples=3, seed=31)
    assert [q for img in a for q, _ in img] != [q for img in dec.sample_random(f, C.START, fam.V, samples=3, seed=32) for q, _ in img]
    torch.manual_seed(3)
    x = dec.sample_random(f, C.START, fam.V, samples=3)
    y = dec.sample_random(f, C.START, fam.V, samples=3)
    torch.manual_seed(3)
    assert x == dec.sample_random(f, C.START, fam.V, samples=3) and x != y
    # more rows than the one-call route takes: the composed loop, the same lists
    want = dec.sample_random(f, C.START, fam.V, samples=3, seed=31)
    old = decode.FUSED_ATT_SAMPLE_MAX_ROWS
    try:
        decode.FUSED_ATT_SAMPLE_MAX_ROWS = 5
        assert [q for img in dec.sample_random(f, C.START, fam.V, samples=3, seed=31) for q, _ in img] == \
            [q for img in want for q, _ in img]
    finally:
        decode.FUSED_ATT_SAMPLE_MAX_ROWS = old
