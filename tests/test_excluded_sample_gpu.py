"""Sampled decoding with exclusions on the GPU (sample_random(exclude=); csrc/sample_exclude.hip): the mask
kernel against capnet.beam.banned_words bit for bit, the masked vocabulary kernels and the -inf writer against the fp64
restatement on masked logits, every image-decoder case of tests/excluded_sample_cases.py on all three routes, and
self_critical_step(exclude=).

Ids are compared exactly: tests/test_excluded_sample_cpu.py asserts the margin rule for every case. In the kernel tests a
row is compared where ITS gap clears the rule and all but at most one row of a launch must (test_sample_random_gpu's rule).
logp: within sample_random_ref.logp_tol per word."""
import numpy as np
import pytest
import torch

import excluded_sample_cases as XC
import excluded_sample_ref as XR
import nucleus_ref as N
import sample_random_ref as R
from capnet import metrics, ops, train
from capnet.beam import Constraints, banned_words
from capnet.decode import FUSED_DECODE_OFF, FUSED_SAMPLE_OFF

pytestmark = pytest.mark.gpu

START, END = 1, 2
ROWS = (1, 5, 16, 17, 32, 33)      # test_sample_random_gpu's: one tile, a partial tile, the pass boundaries of TM = 2 and TM = 1
_inputs = {}


def _kernel_inputs(H, V):
    """test_sample_random_gpu._kernel_inputs, rebuilt: (h [33, H], W [V, H], b [V]) fp32 on the CPU and the fp64 logits with
    the bias -- computed once."""
    if (H, V) not in _inputs:
        g = torch.Generator().manual_seed(3 * V + H)
        W = torch.randn(V, H, generator=g) * (2.0 / H ** 0.5)
        b = torch.randn(V, generator=g) * 0.1
        h = torch.rand(max(ROWS), H, generator=g) * 2 - 1
        _inputs[(H, V)] = (h, W, b, (h.double() @ W.double().t() + b.double()).numpy())
    return _inputs[(H, V)]


def _dev_mask(bits, dev):
    """bool [rows, V] -> the int32 [rows, ceil(V / 32)] mask on the device."""
    rows, V = bits.shape
    padded = np.zeros((rows, (V + 31) // 32 * 32), dtype=bool)
    padded[:, :V] = bits
    words = (padded.reshape(rows, -1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32)).to(dev)


def _check(tokens, logp, d, inv_T, top_k=0, what=""):
    """test_sample_random_gpu._check: a launch against draw()'s dict on the rows whose gaps clear the rule."""
    clear = d["key_gaps"] > R.need(d["scale"], inv_T)
    if top_k:
        clear &= d["kth_gaps"] > R.need_kth(d["scale"])
    rows = len(clear)
    assert clear.sum() >= rows - 1, what
    tokens, logp = tokens.cpu().numpy(), logp.double().cpu().numpy()
    assert tokens.dtype == np.int64 and tokens.shape == (rows,) and logp.shape == (rows,)
    assert (tokens[clear] == d["tokens"][clear]).all(), what
    both = clear & np.isfinite(d["logp"])
    err = np.abs(logp[both] - d["logp"][both]).max() if both.any() else 0.0
    assert err <= R.logp_tol(d["scale"], inv_T), (what, err)
    assert (logp[clear & ~np.isfinite(d["logp"])] == -np.inf).all(), what
    return clear


# ---- 1. the mask kernel against banned_words ----------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [37, 97, 7411, 8192])
def test_mask_kernel_is_banned_words_bit_for_bit(dev, V):
    steps = 40
    full = tuple(range(3, 31)) + (31, 32, 33, V - 1)          # 32 ids with 31, 32 (a word boundary) and V - 1
    assert len(set(full)) == 32 and END not in full
    g = torch.Generator().manual_seed(V)
    launches = 0
    for rows in (1, 12):
        ids = torch.tensor([5, 6, 9])[torch.randint(0, 3, (rows, steps), generator=g)]       # three words: contexts recur
        start = torch.where(torch.arange(rows) % 2 == 1, 5, START)                               # <start> inside the alphabet too
        ids_d, start_d = ids.to(dev), start.to(dev)
        out = None
        for gram in (0, 1, 2, 3, 4):
            for t in sorted({0, 1, max(gram - 1, 0), 11, 39}):
                for banned in ((), full):
                    for min_words in (t + 1, t):              # <end> banned at the boundary, not one past it
                        c = Constraints(no_repeat_ngram=gram, min_words=min_words, banned=banned)
                        out = ops.sample_exclusion_mask(ids_d, start_d, t, V, END, c, out=out)     # one buffer: every word is rewritten
                        hyps = [[int(start[r])] + ids[r, :t].tolist() for r in range(rows)]
                        want = XR.mask_words(hyps, t, V, END, c)
                        got = out.cpu().numpy().view(np.uint32)
                        assert got.shape == (rows, (V + 31) // 32) and np.array_equal(got, want), (rows, gram, t, banned, min_words)
                        assert (((got[:, 0] >> END) & 1) == (1 if min_words == t + 1 else 0)).all()
                        launches += 1
        # without start tokens the hypotheses are the words alone
        c = Constraints(no_repeat_ngram=2, min_words=3)
        got = ops.sample_exclusion_mask(ids_d, None, 11, V, END, c).cpu().numpy().view(np.uint32)
        for r in range(rows):
            want = set(banned_words(ids[r, :11].tolist(), 12, END, c))
            assert {v for v in range(64) if (int(got[r, v >> 5]) >> (v & 31)) & 1} == want
    ops.check_device_errors()
    print("V %d: %d masks equal" % (V, launches))
    with pytest.raises(ops.CapnetError):
        ops.sample_exclusion_mask(ids_d, start_d, 41, V, END, Constraints(no_repeat_ngram=1))
    with pytest.raises(ops.CapnetError):
        ops.sample_exclusion_mask(ids_d, start_d, 3, V, END, Constraints(forced=(4,)))


# ---- 2. the masked vocabulary kernels ---------------------------------------------------------------------------------------
def _kernel_masks(winner, V, seed):
    """name -> bool [rows, V], each excluding every row's unmasked winner `winner` [rows]; and the one word all_but_one keeps."""
    rows = len(winner)
    rng = np.random.RandomState(seed)
    r = np.arange(rows)
    out = {}
    m = np.zeros((rows, V), dtype=bool)                       # all 32 columns of the winner's workgroup
    for i in r:
        m[i, (winner[i] >> 5) * 32:min((winner[i] >> 5) * 32 + 32, V)] = True
    out["workgroup"] = m
    m = np.zeros((rows, V), dtype=bool)                       # all columns of the last workgroup (partial where V % 32)
    m[:, (V - 1) // 32 * 32:] = True
    m[r, winner] = True
    out["last_workgroup"] = m
    keep = (winner + 1 + rng.randint(0, V - 1, rows)) % V     # every word but one, which is not the winner
    assert (keep != winner).all()
    m = np.ones((rows, V), dtype=bool)
    m[r, keep] = False
    out["all_but_one"] = m
    out["all"] = np.ones((rows, V), dtype=bool)
    m = rng.rand(rows, V) < 0.5                               # a different mask on every row
    m[r, winner] = True
    out["per_row"] = m
    return out, keep


@pytest.mark.parametrize("H,V", [(64, 37), (512, 7411), (1024, 8192)])
def test_masked_vocab_sample_and_topk_match_restatement_on_masked_logits(dev, H, V):
    h, W, b, z = _kernel_inputs(H, V)
    hd, Wd, bd = h.to(dev), W.to(dev), b.to(dev)
    for rows, T in ((5, 1.0), (33, 0.5)):
        inv_T, seed, step = R.inv_temperature(T), 7 * rows + V, rows
        plain_tok, plain_lp = ops.vocab_sample(hd[:rows], Wd, bd, temperature=T, seed=seed, step=step)
        d0 = R.draw(z[:rows], inv_T, seed, step)
        masks, keep = _kernel_masks(d0["tokens"], V, seed)
        # a null mask is the unmasked call, and so, bit for bit, is a mask that excludes nothing
        nt, nl = ops.vocab_sample(hd[:rows], Wd, bd, temperature=T, seed=seed, step=step, mask=None)
        zt, zl = ops.vocab_sample(hd[:rows], Wd, bd, temperature=T, seed=seed, step=step, mask=_dev_mask(np.zeros((rows, V), bool), dev))
        assert torch.equal(nt, plain_tok) and torch.equal(nl, plain_lp) and torch.equal(zt, plain_tok) and torch.equal(zl, plain_lp)
        v0 = ops.vocab_topk(hd[:rows], Wd, bd, k=5)
        v1 = ops.vocab_topk(hd[:rows], Wd, bd, k=5, mask=None)
        v2 = ops.vocab_topk(hd[:rows], Wd, bd, k=5, mask=_dev_mask(np.zeros((rows, V), bool), dev))
        assert all(torch.equal(a, b_) and torch.equal(a, c_) for a, b_, c_ in zip(v0, v1, v2))
        for name, bits in masks.items():
            zm = np.where(bits, -np.inf, z[:rows])
            md = _dev_mask(bits, dev)
            tok, lp = ops.vocab_sample(hd[:rows], Wd, bd, temperature=T, seed=seed, step=step, mask=md)
            d = R.draw(zm, inv_T, seed, step)
            clear = _check(tok, lp, d, inv_T, what=(name, rows))
            tok_c = tok.cpu().numpy()
            if name == "all":
                assert (tok_c == 0).all() and bool((lp == float("-inf")).all())
            else:
                assert not bits[np.arange(rows), tok_c].any(), name                    # never an excluded word
                assert (tok_c[clear] != d0["tokens"][clear]).all(), name               # the unmasked winner is gone
            if name == "all_but_one":
                assert (tok_c == keep).all() and bool((lp == 0).all())                 # logp exactly 0
            # top_k 5 of the allowed words, then the pick
            values, index, lse = ops.vocab_topk(hd[:rows], Wd, bd, k=5, mask=md)
            pt, pl = ops.sample_pick(values, index, V, temperature=T, seed=seed, step=step)
            dk = R.draw(zm, inv_T, seed, step, 0, 5)
            cleark = _check(pt, pl, dk, inv_T, top_k=5, what=("topk", name, rows))
            idx = index.cpu().numpy()
            live = idx >= 0
            assert not bits[np.arange(rows)[:, None].repeat(5, 1)[live], idx[live]].any(), name
            if name != "all":
                want_lse = np.array([np.logaddexp.reduce(zm[r][np.isfinite(zm[r])]) for r in range(rows)])
                assert np.abs(lse.double().cpu().numpy() - want_lse).max() <= R.logp_tol(d["scale"], 1.0), name     # over the allowed words
                for r in np.nonzero(cleark)[0]:
                    order = np.lexsort((np.arange(V), -zm[r]))[:5]
                    n_ok = int(np.isfinite(zm[r][order]).sum())
                    assert idx[r, :n_ok].tolist() == order[:n_ok].tolist() and (idx[r, n_ok:] == -1).all(), (name, r)
            else:
                assert (idx == -1).all()
    # two masked launches back to back on one workspace agree with fresh workspaces (the counter re-arms)
    rows = 33
    md = _dev_mask(masks["per_row"], dev)
    ws = ops.vocab_sample_workspace(rows, V, dev)
    a = [ops.vocab_sample(hd, Wd, bd, temperature=1.0, seed=s, step=s, workspace=ws, mask=md) for s in range(2)]
    wk = ops.vocab_topk_workspace(rows, 5, V, dev)
    ak = [ops.vocab_topk(hd, Wd, bd, k=5, workspace=wk, mask=md) for _ in range(2)]
    torch.cuda.synchronize()
    assert int(ws[0].item()) & 0xffffffff == 0 and int(wk[0].item()) & 0xffffffff == 0
    for s, (t, l) in enumerate(a):
        ft, fl = ops.vocab_sample(hd, Wd, bd, temperature=1.0, seed=s, step=s, mask=md)
        assert torch.equal(t, ft) and torch.equal(l, fl)
    fk = ops.vocab_topk(hd, Wd, bd, k=5, mask=md)
    assert all(torch.equal(x, y) and torch.equal(x, w) for x, y, w in zip(ak[0], ak[1], fk))
    ops.check_device_errors()


@pytest.mark.parametrize("H,V", [(64, 37), (512, 7411), (1024, 8192)])
def test_mask_logits_then_the_draws_from_memory(dev, H, V):
    h, W, b, z = _kernel_inputs(H, V)
    hd, Wd, bd = h.to(dev), W.to(dev), b.to(dev)
    rows, T, seed, step = 33, 1.0, 11 + V, 4
    inv_T = R.inv_temperature(T)
    d0 = R.draw(z, inv_T, seed, step)
    masks, _ = _kernel_masks(d0["tokens"], V, seed)
    logits = ops.linear(hd, Wd, bd)
    for name in ("workgroup", "last_workgroup", "per_row"):
        bits = masks[name]
        md = _dev_mask(bits, dev)
        wide = torch.full((rows, V + 3), 7.0, device=dev)           # a padded block: nothing is written past V
        wide[:, :V] = logits
        out = ops.mask_logits(wide[:, :V], md)
        got = wide.cpu().numpy()
        assert (got[:, V:] == 7.0).all()
        assert np.array_equal(np.isneginf(got[:, :V]), bits) and np.array_equal(got[:, :V][~bits], logits.cpu().numpy()[~bits])
        zm = np.where(bits, -np.inf, z)
        d = R.draw(zm, inv_T, seed, step)
        st, sl = ops.sample_rows(out, temperature=T, seed=seed, step=step)
        clear = _check(st, sl, d, inv_T, what=("sample_rows", name))
        vt, vl = ops.vocab_sample(hd, Wd, bd, temperature=T, seed=seed, step=step, mask=md)
        c = torch.from_numpy(clear)
        assert torch.equal(st.cpu()[c], vt.cpu()[c]), name                   # the masked vocab_sample's tokens
        assert (sl.cpu()[c] - vl.cpu()[c]).abs().max().item() <= 2 * R.logp_tol(d["scale"], inv_T)
        # the nucleus of the allowed words: exact logits (the kernel reads the numbers the restatement reads)
        top_p = N.top_p32(0.9)
        z32 = wide[:, :V].cpu().double().numpy()
        dn = N.draw(z32, inv_T, seed, step, 0, 0, top_p, exact32=True)
        nt, nl = ops.nucleus_rows(out, temperature=T, top_p=0.9, seed=seed, step=step)
        ok = (dn["key_gaps"] > 2 * R.TOL_G + 4e-6) & (dn["mass_ratio"] > 0) & (dn["size"] > 0)
        assert ok.sum() >= rows - 3, (name, int(ok.sum()))
        nt, nl = nt.cpu().numpy(), nl.double().cpu().numpy()
        assert (nt[ok] == dn["tokens"][ok]).all() and not bits[np.arange(rows), nt].any(), name
        assert np.abs(nl[ok] - dn["logp"][ok]).max() <= R.logp_tol(dn["scale"], inv_T)
    ops.check_device_errors()


# ---- 3. the image decoders on every route -----------------------------------------------------------------------------------
def _routes(monkeypatch, run, calls=None):
    """run() on the one-call route, with CAPNET_NO_FUSED_SAMPLE=1 and with CAPNET_NO_FUSED_DECODE_STEP=1 (the form of
    test_sample_random_gpu._routes)."""
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
    calls, seen = [0], []
    for name in names:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **kw):
            calls[0] += 1
            seen.append((_name, sorted(kw)))
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls, seen


def _decoder(case, dev):
    fam = XC.SC.families()[case["family"]]
    return fam, fam.make().to(dev).eval(), fam.features()[:XC.IMAGES].to(dev)


def _same_lists(got, want, tol_word):
    assert len(got) == len(want)
    for gi, wi in zip(got, want):
        assert len(gi) == len(wi)
        for (gt, gl), (wt, wl) in zip(gi, wi):
            assert gt == wt, (gt, wt)
            assert abs(gl - wl) <= tol_word * (len(wt) - 1), (gl, wl)


def _kw(case, fam):
    kw = dict(samples=XC.SAMPLES, temperature=case["T"], top_k=case["top_k"], seed=case["seed"], **fam.kw)
    if case["top_p"] < 1.0:
        kw["top_p"] = case["top_p"]
    return kw


PLAIN_ONE_CALL = {c["id"] for c in XC.CASES if "Att" in c["family"] or c["top_p"] == 1.0}      # (a plain stack's nucleus without top_k: composed)


@pytest.mark.parametrize("case", [c for c in XC.CASES if not c["greedy"]], ids=[c["id"] for c in XC.CASES if not c["greedy"]])
def test_image_decoder_excluded_sample_matches_restatement_on_every_route(dev, monkeypatch, case):
    ref = XC.reference(case)
    ids_r, logp_r, tr = ref["excl"]
    end, c = ref["end"], ref["c"]
    fam, dec, f = _decoder(case, dev)
    tol = R.logp_tol(tr.scale, R.inv_temperature(case["T"]))
    kw = _kw(case, fam)
    calls, seen = _count_calls(monkeypatch, "sample_decode", "att_sample_decode")
    runs = _routes(monkeypatch, lambda: dec.sample_random(f, XC.START, end, device=True, exclude=c, **kw),
                   calls if case["id"] in PLAIN_ONE_CALL else None)
    assert all("exclude" in k for _, k in seen)
    want = R.cut(ids_r, logp_r, XC.IMAGES, XC.SAMPLES, XC.START, end)
    for route, (got, ids, logp) in runs.items():
        assert np.array_equal(ids.cpu().numpy(), ids_r), (case["id"], route)          # the raw rows: past <end> too
        err = np.abs(logp.double().cpu().numpy() - logp_r).max()
        assert err <= tol, (route, err)
        _same_lists(got, want, tol)
        _same_lists(got, runs["one_call"][0], 2 * tol)                                 # every route returns the same lists
        assert not [v for img in got for q, _ in img for v in XR.violations(q, end, c)]
    # exclude=None and an inactive Constraints() are the call without the keyword, and make the calls it makes
    del seen[:]
    base = dec.sample_random(f, XC.START, end, **kw)
    made = list(seen)
    for off in (None, Constraints()):
        del seen[:]
        assert dec.sample_random(f, XC.START, end, exclude=off, **kw) == base and seen == made
    assert all("exclude" not in k and "end_token" not in k for _, k in made)
    assert base != runs["one_call"][0]                                                 # and the set binds on the device as on the CPU
    ops.check_device_errors()


def test_greedy_row_under_exclusions(dev, monkeypatch):
    case = [c for c in XC.CASES if c["greedy"]][0]
    ref = XC.reference(case)
    end, c = ref["end"], ref["c"]
    fam, dec, f = _decoder(case, dev)
    kw = _kw(case, fam)
    m = XC.SAMPLES
    want = R.cut(*ref["excl"][:2], XC.IMAGES, m, XC.START, end)
    tol = R.logp_tol(ref["excl"][2].scale, R.inv_temperature(case["T"]))
    runs = _routes(monkeypatch, lambda: dec.sample_random(f, XC.START, end, greedy=True, exclude=c, **kw))
    beam = dec.sample_batch(f, XC.START, end, k=1, constraints=c, **fam.kw)
    restated = [g[0] for g, _ in XC.greedy_captions(case, ref)]                        # complete, by the choice of the case
    for route, got in runs.items():
        assert all(len(img) == m + 1 for img in got)
        _same_lists([img[:m] for img in got], want, tol)                              # the first m pairs: the call without greedy
        _same_lists(got, runs["one_call"], 2 * tol)
        for i, img in enumerate(got):
            g = img[m][0]
            assert g == restated[i] and g[-1] == end and not XR.violations(g, end, c), (route, i)
            assert [int(w) for w in beam[i]] == g, (route, i)                          # the width-1 beam under the same set
    plain = dec.sample_random(f, XC.START, end, greedy=True, **kw)
    assert [img[m][0] for img in plain] != [img[m][0] for img in runs["one_call"]]     # the exclusions move the greedy caption
    ops.check_device_errors()


def test_exclude_is_checked_before_anything_runs(dev):
    case = XC.CASES[0]
    fam, dec, f = _decoder(case, dev)
    assert fam.V == 37                 # 37 - 19 banned - 1 - 13 = 4 < top_k = 5
    for bad in (Constraints(forced=(5,)), Constraints(banned=(END,)), Constraints(banned=(fam.V,)), Constraints(min_words=XC.MAX_LEN),
                Constraints(banned=tuple(range(3, 22)))):
        with pytest.raises(ops.CapnetError):
            dec.sample_random(f, XC.START, END, samples=2, top_k=5, seed=0, exclude=bad, **fam.kw)


# ---- 4. self_critical_step(exclude=) ----------------------------------------------------------------------------------------
def _sc_setup(dev):
    """tests/test_self_critical_device_gpu.py's pair: two copies of greedy_row_cases' two-layer attention decoder at 3 images x
    5 samples, with the end token that the greedy caption of every image reaches within max_seq_length (asserted on the CPU
    there), so the host route's width-1 beam is the greedy caption."""
    import greedy_row_cases as GC
    case = [c for c in GC.CASES if c["family"] == "StackedFactoredLSTMAtt-2-v37" and (c["n"], c["m"]) == (3, 5)][0]
    fam = GC.families()[case["family"]]
    decs = [GC.make(fam, dev).train() for _ in range(2)]
    sampling = dict(temperature=case["T"], top_k=case["top_k"], top_p=case["top_p"], seed=GC.SEEDS[case["id"]], **fam.kw)
    return decs, fam.features()[:case["n"]].to(dev), case["m"], GC.end_token(case), sampling, fam.kw


@pytest.mark.parametrize("baseline", ["greedy", "mean"])
def test_self_critical_step_excludes_on_both_routes(dev, baseline):
    (dec_h, dec_d), f, m, end, sampling, fkw = _sc_setup(dev)
    plain = dec_h.sample_random(f, START, end, samples=m, greedy=True, **sampling)
    drawn_words = [w for img in plain for q, _ in img[:m] for w in q[1:] if w != end]
    greedy_words = {w for img in plain for w in img[m][0]}
    # a word the unexcluded step draws; outside the greedy captions, so that those stay what they are and the host route's
    # width-1 beam completes exactly where it does without the keyword
    w = [x for x in drawn_words if x not in greedy_words][0]
    c = Constraints(banned=(w,))
    caps = dec_h.sample_random(f, START, end, samples=m, greedy=True, exclude=c, **sampling)
    assert all(w not in q for img in caps for q, _ in img)
    assert [img[m][0] for img in caps] == [img[m][0] for img in plain]
    if baseline == "greedy":           # the host's baseline is the greedy row only where the width-1 beam completes
        beam = dec_h.sample_batch(f, START, end, k=1, constraints=c, **fkw)
        assert [[int(x) for x in b] for b in beam] == [img[m][0] for img in caps]
    refs = [[img[0][0], img[1][0][:3] + [end], img[m][0][:3] + [end]] for img in caps]
    kw = dict(samples=m, baseline=baseline, exclude=c, **sampling)
    before = [p.detach().clone() for p in dec_d.parameters()]
    seen = []
    host_reward = lambda i, tokens: (seen.append(list(tokens)), metrics.sentence_bleu(refs[i], tokens, smooth=1))[1]
    res_h = train.self_critical_step(dec_h, torch.optim.SGD(dec_h.parameters(), lr=0.0), f, host_reward, START, end, 5.0, **kw)
    res_d = train.self_critical_step(dec_d, torch.optim.SGD(dec_d.parameters(), lr=0.0), f, train.DeviceBleuReward(refs, smooth=1),
                                     START, end, 5.0, **kw)
    ops.check_device_errors()
    assert seen and all(w not in q for q in seen)                                        # no drawn caption holds w
    assert [q for q in seen[:3 * m]] == [q for img in caps for q, _ in img[:m]]
    rel = 2.0 ** -23
    assert int(res_d["zero_rows"]) == res_h["zero_rows"]
    for k in ("reward_mean", "baseline_mean"):
        assert abs(float(res_d[k]) - res_h[k]) <= rel * abs(res_h[k]), k
    # test_self_critical_device_gpu's bound on the two losses
    r = [[metrics.sentence_bleu(refs[i], q, smooth=1) for q, _ in img] for i, img in enumerate(caps)]
    adv = [x - img[m] for img in r for x in img[:m]] if baseline == "greedy" else \
        [x - (sum(img[:m]) - x) / (m - 1) for img in r for x in img[:m]]
    drawn = [[q for q, _ in img[:m]] for img in caps]
    logp = dec_h.score_captions(f, drawn, **fkw).double().abs().cpu().tolist()
    words = sum(len(q) - 1 for img in drawn for q in img)
    bound = (rel * sum(logp) + 2 * (words + 2) * 2.0 ** -24 * sum(abs(a) * l for a, l in zip(adv, logp))) / words
    diff = abs(res_d["loss"].item() - res_h["loss"].item())
    print("%s: loss host %.9g device %.9g: difference %.3g, bound %.3g" % (baseline, res_h["loss"].item(), res_d["loss"].item(), diff, bound))
    assert diff <= bound
    assert any(a != 0 for a in adv)
    # lr = 0 leaves the parameters, Adam moves them
    assert all(torch.equal(a, b) for a, b in zip(before, dec_d.parameters()))
    from capnet.optim import Adam
    train.self_critical_step(dec_d, Adam(dec_d.parameters(), lr=0.01), f, train.DeviceBleuReward(refs, smooth=1), START, end, 5.0, **kw)
    ops.check_device_errors()
    assert any(not torch.equal(a, b) for a, b in zip(before, dec_d.parameters()))
