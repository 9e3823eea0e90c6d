"""capnet.seq2seq under constraints on the GPU: csrc/vocab_topk.hip's select-only instance and the beam-state
mask kernel on their own, then Seq2Seq.sample_beam_constrained / sample_beam_styles_constrained (EncoderRNN /
DecoderRNN.sample_beam(constraints=) underneath) on every route against the fp64
constrained search of every (case, set) of tests/seq2seq_constrained_cases.py (tests/test_seq2seq_constrained_cpu.py asserts
that all clear the rule: nothing is skipped here), and sample_random(exclude=) on both routes.

Tolerances. The kernel checks are exact (torch.equal): select-only shares lse with the unmasked launch and the candidates with
the sampler's masked launch by construction. Token lists end to end: exact, under the margin rule. Scores:
tests/test_nbest_gpu.py's for seq2seq, (len - 1) x seq2seq_cases.need(scale) of the fp64 score. logp of sample_random:
tests/test_excluded_sample_gpu.py's, sample_random_ref.logp_tol per word."""
import numpy as np
import pytest
import torch

import constrained_beam_cases as CC
import excluded_sample_ref as XR
import sample_random_ref as SR
import seq2seq_constrained_cases as XC
from capnet import ops
from capnet.beam import Constraints, banned_words
from capnet.decode import FUSED_DECODE_OFF, FUSED_SAMPLE_OFF
from constrained_beam_ref import violations
from device_beam_cases import MAX_LEN, START
from seq2seq_cases import need

pytestmark = pytest.mark.gpu

ROWS = (1, 8, 9, 15, 33)            # the merge at 64, 32 and 16 lanes per row; 33: a second pass of the row walk
SHAPES = ((64, 37, (5, 16)), (128, 211, (5,)))      # (H, V, ks): two workgroups, the last ragged; seven


@pytest.fixture(autouse=True)
def _clean(dev, monkeypatch):
    for name in (FUSED_DECODE_OFF, FUSED_SAMPLE_OFF, "CAPNET_NO_FUSED_TOPK"):
        monkeypatch.delenv(name, raising=False)
    yield
    ops.check_device_errors()


# ---- 1. the select-only instance of vocab_topk -------------------------------------------------------------------------------
def _inputs(H, V, dev):
    g = torch.Generator().manual_seed(3 * V + H)
    W = torch.randn(V, H, generator=g) * (2.0 / H ** 0.5)
    b = torch.randn(V, generator=g) * 0.1
    h = torch.rand(max(ROWS), H, generator=g) * 2 - 1
    return h.to(dev), W.to(dev), b.to(dev)


def _dev_mask(bits, dev):
    """bool [rows, V] -> the int32 [rows, ceil(V / 32)] mask on the device (tests/test_excluded_sample_gpu.py's)."""
    rows, V = bits.shape
    padded = np.zeros((rows, (V + 31) // 32 * 32), dtype=bool)
    padded[:, :V] = bits
    words = (padded.reshape(rows, -1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32)).to(dev)


def _masks(winner, V, seed):
    """tests/test_excluded_sample_gpu.py's masks, each excluding every row's unmasked winner: a different mask on every row,
    all 32 columns of the winner's workgroup, all but one word (and the word kept)."""
    rows = len(winner)
    rng = np.random.RandomState(seed)
    r = np.arange(rows)
    out = {}
    m = rng.rand(rows, V) < 0.5
    m[r, winner] = True
    out["per_row"] = m
    m = np.zeros((rows, V), dtype=bool)
    for i in r:
        m[i, (winner[i] >> 5) * 32:min((winner[i] >> 5) * 32 + 32, V)] = True
    out["workgroup"] = m
    keep = (winner + 1 + rng.randint(0, V - 1, rows)) % V
    assert (keep != winner).all()
    m = np.ones((rows, V), dtype=bool)
    m[r, keep] = False
    out["all_but_one"] = m
    return out, keep


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("H,V,ks", SHAPES, ids=["h64-v37", "h128-v211"])
def test_select_only_keeps_the_unmasked_lse_and_the_masked_candidates(dev, H, V, ks):
    hd, Wd, bd = _inputs(H, V, dev)
    for k in ks:
        for rows in ROWS:
            h = hd[:rows]
            plain = ops.vocab_topk(h, Wd, bd, k=k)
            zero = _dev_mask(np.zeros((rows, V), bool), dev)
            assert _equal(ops.vocab_topk(h, Wd, bd, k=k, mask=zero, select_only=True), plain), (k, rows)     # nothing set
            winner = plain[1][:, 0].cpu().numpy().astype(np.int64)
            masks, keep = _masks(winner, V, 7 * rows + V + k)
            for name, bits in masks.items():
                md = _dev_mask(bits, dev)
                values, index, lse = ops.vocab_topk(h, Wd, bd, k=k, mask=md, select_only=True)
                pv, pi, plse = ops.vocab_topk(h, Wd, bd, k=k, mask=md)                  # the sampler's meaning
                assert torch.equal(lse, plain[2]), (name, k, rows)                      # lse: every word still counts
                assert torch.equal(values, pv) and torch.equal(index, pi), (name, k, rows)
                idx = index.cpu().numpy()
                live = idx >= 0
                assert not bits[np.arange(rows)[:, None].repeat(k, 1)[live], idx[live]].any(), name
                allowed = (~bits).sum(1)
                assert (live.sum(1) == np.minimum(allowed, k)).all(), name            # a short row ends in (-inf, -1)
                assert bool((values[torch.from_numpy(~live)] == float("-inf")).all())
                if name == "all_but_one":
                    assert (idx[:, 0] == keep).all() and (idx[:, 1:] == -1).all()
                    if k > 1:
                        assert not torch.equal(plse, lse)                               # and the two meanings do differ
    # two launches back to back on one workspace agree with fresh workspaces, and the counter is zero afterwards
    rows, k = 33, 5
    md = _dev_mask(masks["per_row"], dev)
    ws = ops.vocab_topk_workspace(rows, k, V, dev)
    twice = [ops.vocab_topk(hd, Wd, bd, k=k, workspace=ws, mask=md, select_only=True) for _ in range(2)]
    torch.cuda.synchronize()
    assert int(ws[0].item()) & 0xffffffff == 0
    fresh = ops.vocab_topk(hd, Wd, bd, k=k, mask=md, select_only=True)
    assert _equal(twice[0], fresh) and _equal(twice[1], fresh)
    with pytest.raises(ops.CapnetError):
        ops.vocab_topk(hd, Wd, bd, k=k, select_only=True)                               # select_only without a mask


@pytest.mark.parametrize("H,V,ks", SHAPES, ids=["h64-v37", "h128-v211"])
def test_grouped_select_only_equals_each_groups_single_launch(dev, H, V, ks):
    groups, k = 3, 5
    g = torch.Generator().manual_seed(V + H)
    Ws = [(torch.randn(V, H, generator=g) * (2.0 / H ** 0.5)).to(dev) for _ in range(groups)]
    bs = [(torch.randn(V, generator=g) * 0.1).to(dev) for _ in range(groups)]
    for rpg in (1, 9, 15, 33):
        h = (torch.rand(groups * rpg, H, generator=g) * 2 - 1).to(dev)
        bits = np.random.RandomState(rpg).rand(groups * rpg, V) < 0.5
        md = _dev_mask(bits, dev)
        ws = ops.vocab_topk_groups_workspace(groups, rpg, k, V, dev)
        for select in (True, False):
            for _ in range(2):                                                           # the counters re-arm
                got = ops.vocab_topk_groups(h, Ws, bs, k=k, workspace=ws, mask=md, select_only=select)
                for q in range(groups):
                    rows = slice(q * rpg, (q + 1) * rpg)
                    one = ops.vocab_topk(h[rows], Ws[q], bs[q], k=k, mask=md[rows].contiguous(), select_only=select)
                    assert all(torch.equal(x[rows], y) for x, y in zip(got, one)), (rpg, select, q)
        torch.cuda.synchronize()
        assert all(int(ws.view(torch.int32)[4 * q].item()) == 0 for q in range(groups))


# ---- 2. the mask of a device beam's rows -------------------------------------------------------------------------------------
def _hypotheses(beam, step):
    """[n k] token lists: what step `step` reads of the state's words -- [4] | live[n] | n_done[n] | scores[n k] |
    done_score[n k] | done_len[n k] | seq[2][n k][max_steps + 2] -- and live [n]."""
    n, k, L = beam.n, beam.k, beam.max_steps + 2
    w = beam.words.cpu()
    seq = w[4 + 2 * n + 3 * n * k:][:2 * n * k * L].view(2, n * k, L)
    return seq[(step - 1) & 1][:, :step].tolist(), w[4:4 + n].tolist()


@pytest.mark.parametrize("k,V", [(5, 37), (3, 1500), (16, 37)])
def test_beam_exclusion_mask_is_banned_words_on_the_states_rows(dev, k, V):
    n, T, END = CC.TABLE_N, CC.TABLE_T, CC.TABLE_END
    tab = CC.table(k, V).clone()
    tab[:, 0, END] = 65.0              # image 0, slot 0: <end> ahead of everything, so once min_words allows it a beam completes
    sets = dict(CC.TABLE_SETS, wide=Constraints(no_repeat_ngram=3, min_words=2, banned=(4, 31, 32, V - 1)))
    partly_live = 0
    for s, c in sets.items():
        words = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(2)]
        parent = torch.empty(n * k, dtype=torch.long, device=dev)
        beam = ops.beam_init(n, k, T, CC.TABLE_START, words[0])
        mask = None
        for step in range(1, T + 1):
            mask = ops.beam_exclusion_mask(beam, step, V, END, c, out=mask)            # one buffer: every word is rewritten
            hyps, live = _hypotheses(beam, step)
            got = mask.cpu().numpy().view(np.uint32)
            assert got.shape == (n * k, (V + 31) // 32)
            for i in range(n):
                partly_live += 0 < live[i] < k
                for r in range(k if step == 1 else live[i]):                          # (dead slots: a mask nobody reads)
                    row = i * k + r
                    want = XR.mask_words([hyps[row]], step - 1, V, END, c)[0]
                    assert np.array_equal(got[row], want), (s, step, i, r)
                    assert {v for v in range(V) if (int(got[row, v >> 5]) >> (v & 31)) & 1} == \
                        set(banned_words(hyps[row], step, END, c)), (s, step, i, r)
            ops.beam_advance(beam, tab[step - 1].to(dev), step, END, words[step & 1], parent, constraints=c)
    assert partly_live                 # an image with 0 < live < k was among them
    with pytest.raises(ops.CapnetError):
        ops.beam_exclusion_mask(beam, T + 1, V, END, c)
    with pytest.raises(ops.CapnetError):
        ops.beam_exclusion_mask(beam, 1, V, END, Constraints(forced=(4,)))


# ---- 3. the constrained searches on every route -----------------------------------------------------------------------------
def _routes(monkeypatch, run, composed):
    """run(**kw) with fused_topk=True, with fused_topk=False and under CAPNET_NO_FUSED_DECODE_STEP=1. (A shape the decode
    kernel does not take runs the composed step whatever is asked.)"""
    out = {}
    for name, kw, env in (("fused", dict(fused_topk=True), None), ("unfused", dict(fused_topk=False), None),
                          ("composed", {}, FUSED_DECODE_OFF)):
        if env:
            monkeypatch.setenv(env, "1")
        out[name] = run(**kw)
        monkeypatch.delenv(FUSED_DECODE_OFF, raising=False)
    return out


def _captions(got, mode, end):
    """The completed captions among a call's lists, START first ([<end>] alone: nothing completed there)."""
    return [q if mode != "factual" else [START] + q for q in got if q != [end]]


def _count(monkeypatch, name):
    seen = []
    real = getattr(ops, name)

    def counted(*a, **kw):
        seen.append({key: v for key, v in kw.items() if not torch.is_tensor(v)})      # (the keywords; of the values, the plain ones)
        return real(*a, **kw)
    monkeypatch.setattr(ops, name, counted)
    return seen


@pytest.mark.parametrize("pair", XC.pairs(), ids=XC.pair_id)
def test_sample_beam_returns_the_constrained_search_on_every_route(dev, monkeypatch, pair):
    u, s = pair
    case, c, end = u.case, u.sets[pair[1]], u.end
    model = case.module().to(dev)
    feats = case.features.float().to(dev)
    seen = _count(monkeypatch, "lstm_beam_decode")
    for k in case.ks:
        want = [u.reference(s, k, r) for r in range(case.rows)]
        runs = _routes(monkeypatch, lambda **kw: model.sample_beam_constrained(feats, START, end, c, mode=case.mode, k=k, **kw),
                       XC.is_composed(u))
        for route, got in runs.items():
            assert got == want, (route, k, got, want)
            full = _captions(got, case.mode, end)
            assert not [v for q in full for v in violations(q, end, c)], route
            assert all(q[-1] == end and set(c.forced) <= set(q) for q in full), route
        # n-best: the same hypotheses on the three routes, the scores within (len - 1) x need(scale)
        lists = _routes(monkeypatch, lambda **kw: model.sample_beam_constrained(feats, START, end, c, mode=case.mode, k=k,
                                                                                nbest=True, **kw), XC.is_composed(u))
        scale, worst = u.scale(s), 0.0
        for route, got in lists.items():
            for r in range(case.rows):
                ref = u.nbest(s, k, r)
                assert [q for q, _ in got[r]] == [q for q, _ in ref], (route, k, r)
                for (q, sc), (_, rs) in zip(got[r], ref):
                    words = len(q) - (0 if case.mode == "factual" else 1)
                    worst = max(worst, abs(sc - rs) / (words * need(scale)))
                    assert abs(sc - rs) <= words * need(scale), (route, k, r, sc, rs)
            assert [h[0][0] if h else [end] for h in got] == runs[route], route
        print("%s k=%d: worst score error %.3g of its bound" % (XC.pair_id(pair), k, worst))
        # poll_every composes
        assert model.sample_beam_constrained(feats, START, end, c, mode=case.mode, k=k, poll_every=3) == want
    if not XC.is_composed(u):
        # the one C call took the constraints; forced words went to the unfused step even where the fused one was asked for
        assert seen and all("constraints" in kw for kw in seen)
        assert all(not kw["fused_topk"] for kw in seen if c.forced)
        assert any(kw["fused_topk"] for kw in seen) == (not c.forced)
    # constraints=None and a Constraints() that excludes nothing: the call without the keyword, and the calls it makes
    del seen[:]
    k = case.ks[-1]
    base = model.sample_beam(feats, START, end, mode=case.mode, k=k)
    made = list(seen)
    def stack(off):       # the searching stack's own sample_beam, which takes the keyword (Seq2Seq.sample_beam does not)
        if case.mode == "factual":
            return model.encoder.sample_beam(feats, START, end, k=k, constraints=off)
        return model._decoder(case.mode).sample_beam(START, end, model.encoder.sample(feats)[1], k=k, constraints=off)
    for run in (lambda: stack(None), lambda: stack(Constraints()),
                lambda: model.sample_beam_constrained(feats, START, end, Constraints(), mode=case.mode, k=k)):
        del seen[:]
        assert run() == base and seen == made
    assert all("constraints" not in kw for kw in made)
    assert base != [u.reference(s, k, r) for r in range(case.rows)] or not [x for x in u.moved(s) if x[0] == k]


@pytest.mark.parametrize("shape", ["small-happy", "h16-happy"])
def test_sample_beam_styles_equals_sample_beam_under_constraints(dev, monkeypatch, shape):
    pairs = [p for p in XC.pairs() if p[0].shape == shape]
    modes = ("factual", "happy", "sad", "angry")
    for u, s in pairs:
        case, c, end = u.case, u.sets[s], u.end
        model = case.module().to(dev)
        feats = case.features.float().to(dev)
        k = case.ks[-1]
        grouped = _count(monkeypatch, "lstm_beam_decode_groups")
        for what, kw, env in (("fused", dict(fused_topk=True), None), ("unfused", dict(fused_topk=False), None),
                              ("loop", {}, FUSED_DECODE_OFF)):
            if env:
                monkeypatch.setenv(env, "1")
            for nb in (dict(), dict(nbest=True)):
                got = model.sample_beam_styles_constrained(feats, START, end, c, modes=modes, k=k, **kw, **nb)
                assert tuple(got) == modes
                for m in modes:
                    assert got[m] == model.sample_beam_constrained(feats, START, end, c, mode=m, k=k, **kw, **nb), (what, s, m)
                if not nb:
                    assert got[case.mode] == [u.reference(s, k, r) for r in range(case.rows)], (what, s)
                    for m in modes:
                        full = _captions(got[m], m, end)
                        assert not [v for q in full for v in violations(q, end, c)], (what, s, m)
                        assert all(set(c.forced) <= set(q) for q in full), (what, s, m)
            monkeypatch.delenv(FUSED_DECODE_OFF, raising=False)
        if not XC.is_composed(u):
            assert grouped and all("constraints" in kw for kw in grouped)
            assert any(kw["fused_topk"] for kw in grouped) == (not c.forced)
        monkeypatch.undo()


# ---- 4. sample_random(exclude=) ---------------------------------------------------------------------------------------------
def _sample_routes(monkeypatch, run):
    out = {}
    for name, env in (("one_call", None), ("composed", FUSED_SAMPLE_OFF)):
        if env:
            monkeypatch.setenv(env, "1")
        out[name] = run()
        monkeypatch.delenv(FUSED_SAMPLE_OFF, raising=False)
    return out


@pytest.mark.parametrize("mode,top_k", [("happy", 0), ("happy", 5), ("factual", 0)])
def test_sample_random_excludes_on_both_routes(dev, monkeypatch, mode, top_k):
    import seq2seq_ref as S2
    u = [p[0] for p in XC.pairs() if p[0].shape == "small-happy"][0]
    case, end = u.case, u.end
    model = case.module().to(dev)
    feats = case.features.float().to(dev)
    T, seed, steps = 1.3, 11, MAX_LEN
    plain_ids, _ = model.sample_random(feats, START, mode=mode, temperature=T, top_k=top_k, seed=seed)
    drawn = [w for w in plain_ids[0].tolist() if w != end]
    c = Constraints(no_repeat_ngram=1, min_words=6, banned=tuple(dict.fromkeys(drawn))[:2])       # two words the plain call draws
    seen = _count(monkeypatch, "sample_decode")
    runs = _sample_routes(monkeypatch, lambda: model.sample_random(feats, START, mode=mode, temperature=T, top_k=top_k, seed=seed,
                                                                    exclude=c, end_token=end))
    # the one call where the hypotheses begin with start tokens; from the feature column the composed loop
    assert [("exclude" in kw) for kw in seen] == ([True] if mode != "factual" else [])
    ids, logp = runs["one_call"]
    assert torch.equal(ids, runs["composed"][0])                                                  # the same tokens
    assert ids.shape == (case.rows, steps) and not torch.equal(ids, plain_ids)
    lead = [] if mode == "factual" else [START]
    for row in ids.tolist():
        assert not violations(lead + row, end, c, completed=False), row
        assert end not in row[:c.min_words]
    # logp against the fp64 restatement of the same draws: the model's logits along the drawn ids, the excluded words at -inf
    p, prefix = case.params, "encoder" if mode == "factual" else "decoder_" + mode
    if mode == "factual":
        hs = [torch.zeros(case.rows, case.H, dtype=torch.float64) for _ in range(case.L)]
        cs = [torch.zeros(case.rows, case.H, dtype=torch.float64) for _ in range(case.L)]
    else:
        _, (h, cc), _, _ = S2.greedy(p, "encoder", case.L, MAX_LEN, features=case.features)
        hs, cs = [h[l].clone() for l in range(case.L)], [cc[l].clone() for l in range(case.L)]
    inv_T = SR.inv_temperature(T)
    prev = torch.full((case.rows,), START, dtype=torch.long)
    ids_c, want, scale = ids.cpu(), np.zeros((case.rows, steps)), 0.0
    for t in range(steps):
        x = case.features if (t == 0 and mode == "factual") else p[prefix + ".embed.weight"][prev]
        top, hs, cs = S2.step(p, prefix, case.L, x, hs, cs)
        z = S2._logits(p, prefix, top).numpy().copy()
        scale = max(scale, float(np.abs(z).max()))
        for r in range(case.rows):
            z[r, banned_words(lead + ids_c[r, :t].tolist(), t + 1, end, c)] = -np.inf
        d = SR.draw(z, inv_T, seed, t, 0, top_k)
        clear = d["key_gaps"] > SR.need(d["scale"], inv_T)
        if top_k:
            clear &= d["kth_gaps"] > SR.need_kth(d["scale"])
        assert (ids_c[:, t].numpy()[clear] == d["tokens"][clear]).all(), t
        # the log-probability of the token the device drew, under the restated distribution of this step
        zt = z * inv_T
        if top_k:
            kth = np.sort(zt, 1)[:, -top_k][:, None]
            zt = np.where(zt >= kth, zt, -np.inf)
        lse = np.logaddexp.reduce(np.where(np.isfinite(zt), zt, -np.inf), axis=1)
        want[:, t] = zt[np.arange(case.rows), ids_c[:, t].numpy()] - lse
        prev = ids_c[:, t]
    tol = SR.logp_tol(scale, inv_T)
    for route, (_, lp) in runs.items():
        err = np.abs(lp.double().cpu().numpy() - want).max()
        assert err <= tol, (route, err, tol)
    # exclude=None and a Constraints() that excludes nothing: the call without the keyword
    for off in (None, Constraints()):
        a, b = model.sample_random(feats, START, mode=mode, temperature=T, top_k=top_k, seed=seed, exclude=off, end_token=end)
        assert torch.equal(a, plain_ids)
