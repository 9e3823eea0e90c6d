"""N-best lists with scores from every beam search, on the GPU: capnet_beam_nbest / capnet_beam_nbest_traced against the Python
model on stored logits (tests/nbest_cases.py's tables: ties, re-ordering, nothing completed, all completed); every route
of every front end against the fp64 n-best of every admitted case (tests/test_nbest_cpu.py asserts that all are: nothing
is skipped here); the maps of every hypothesis against the fp64 replay of its tokens.

Tolerances. Token lists, their order, lengths, counts and rows: exact. Scores on stored logits: exactly the state's
done_score. Scores end to end: (len - 1) x seq2seq_cases.need(scale) of the fp64 score, scale the largest |logit| the fp64
search met -- the project's per-step logits bound summed over the steps. Maps: tests/att_alpha_cases.BOUND of max|alpha| of
the row, tests/test_att_alphas_gpu.py's bound for a search's maps."""
import pytest
import torch

import nbest_cases as NC
from att_alpha_cases import BOUND, row_error
from att_alpha_ref import replay
from capnet import decode, ops
from nbest_cases import IMAGES, KS, MAX_LEN, PENALTIES, START, TABLE_END, TABLE_KS, TABLE_N, TABLE_START, TABLE_T
from nbest_ref import order
from seq2seq_cases import need

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _clean(dev, monkeypatch):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    monkeypatch.delenv("CAPNET_NO_FUSED_TOPK", raising=False)
    yield
    ops.check_device_errors()


# ---- 1. the kernel on stored logits ----------------------------------------------------------------------------------
def _state_lists(beam):
    """(n_done [n], done_score [n, k]) out of the state's words: [4] | live[n] | n_done[n] | scores[n k] | done_score[n k]."""
    n, k = beam.n, beam.k
    w = beam.words
    return w[4 + n:4 + 2 * n].tolist(), w[4 + 2 * n + n * k:4 + 2 * n + 2 * n * k].view(torch.float32).view(n, k)


@pytest.mark.parametrize("k", TABLE_KS)
def test_kernel_equals_the_model_on_stored_logits(dev, k):
    n, T, L = TABLE_N, TABLE_T, TABLE_T + 2
    tab = NC.table(k)
    model, _ = NC.drive_model(k, tab)
    if k >= 3:
        assert NC.SITUATIONS <= model.events(T)
    words = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(2)]
    parent = torch.empty(n * k, dtype=torch.long, device=dev)
    beam = ops.beam_init(n, k, T, TABLE_START, words[0])
    trace = ops.beam_trace(beam)
    trace.fill_(0x7fffffff)
    for step in range(1, T + 1):
        ops.beam_advance_traced(beam, trace, tab[step - 1].to(dev), step, TABLE_END, words[step & 1], parent)
    n_done, done_score = _state_lists(beam)
    assert n_done == [len(model.completed(i)) for i in range(n)] == [k, k, 0]
    before = beam.words.clone()
    fin = ops.beam_finish_traced(beam, trace, TABLE_END)
    scale = float(tab.abs().max())
    for penalty in (0.0, 0.7, 1.0):
        seqs, lengths, scores, counts, packed = ops.beam_nbest(beam, TABLE_END, penalty)
        seqs_t, lengths_t, scores_t, counts_t, rows = ops.beam_nbest_traced(beam, trace, TABLE_END, penalty)
        assert torch.equal(seqs, seqs_t) and torch.equal(lengths, lengths_t) and torch.equal(scores, scores_t)
        assert torch.equal(counts, counts_t)
        assert seqs.dtype == torch.int64 and tuple(seqs.shape) == (n, k, L) and lengths.dtype == torch.int32
        assert scores.dtype == torch.float32 and counts.dtype == torch.int32 and rows.dtype == torch.int32
        want = model.nbest(penalty)
        assert counts.tolist() == [len(w) for w in want]
        for i in range(n):
            src = order(model.completed(i), penalty)
            for r in range(k):
                row, ln = seqs[i, r].tolist(), int(lengths[i, r])
                if r < len(want[i]):
                    assert row[:ln] == want[i][r][0] and row[ln:] == [0] * (L - ln), (penalty, i, r)
                    assert float(scores[i, r]) == float(done_score[i, src[r]]), (penalty, i, r)       # the raw score, bit for bit
                    assert abs(float(scores[i, r]) - want[i][r][1]) <= (ln - 1) * need(scale)
                else:
                    assert row == [0] * L and ln == 0 and float(scores[i, r]) == 0.0, (penalty, i, r)
        assert rows.tolist() == model.nbest_rows(T, penalty)
        # the one copy: ops.nbest_lists of the packed buffer
        lists = ops.nbest_lists(packed, n, k, L)[0]
        assert [[q for q, _ in hyps] for hyps in lists] == [[q for q, _ in hyps] for hyps in want]
        assert all(isinstance(s, float) for hyps in lists for _, s in hyps)
        if penalty == 0.0:        # entry 0 is beam_finish's winner bit for bit, its rows beam_finish_traced's
            for i in range(n):
                if counts[i]:
                    assert torch.equal(seqs[i, 0], fin[0][i]) and int(lengths[i, 0]) == int(fin[1][i])
                    assert torch.equal(rows[i, 0], fin[2][i])
                else:
                    assert fin[0][i].tolist() == [TABLE_END] + [0] * (L - 1) and rows[i].tolist() == [[-1] * T] * k
    if k >= 3:
        assert float(scores[1, 0]) == float(scores[1, 1])                    # the tie, in fp32, the earlier completion first
    # the state is only read
    assert torch.equal(beam.words, before)
    again = ops.beam_finish_traced(beam, trace, TABLE_END)
    assert all(torch.equal(a, b) for a, b in zip(fin, again))


def test_alpha_gather_reads_the_rows_it_is_given(dev):
    nk, T, P, caps = 6, 4, 260, 5
    g = torch.Generator().manual_seed(3)
    hist = torch.rand(T, nk, P, generator=g).to(dev)
    rows = torch.tensor([[0, 5, 2, -1], [-1, -1, -1, -1], [3, 3, 6, 1], [5, 4, -7, 0], [1, 2, 3, 4]], dtype=torch.int32, device=dev)
    out = torch.full((caps, T, P), float("nan"), device=dev)
    from capnet._lib import check, current_stream, lib, ptr
    check(lib().capnet_alpha_gather(ptr(hist), ptr(rows), caps, nk, T, P, ptr(out), current_stream()))
    for c in range(caps):
        for e in range(T):
            r = int(rows[c, e])
            want = hist[e, r] if 0 <= r < nk else torch.zeros(P, device=dev)
            assert torch.equal(out[c, e], want), (c, e)


# ---- 2. every route end to end ---------------------------------------------------------------------------------------
def _compare(u, k, got, penalty, what, images=None):
    """got: per image [(tokens, score)] -> the worst score error over its bound."""
    worst = 0.0
    images = range(u.images) if images is None else images
    assert len(got) == len(images), what
    for hyps, i in zip(got, images):
        want = u.nbest(k, i, penalty)
        assert [q for q, _ in hyps] == [q for q, _ in want], (u, what, k, i, penalty)
        full = u.search(k, i).nbest(penalty)
        for (q, s), (_, sw), (fq, _) in zip(hyps, want, full):
            assert isinstance(s, float), (what, type(s))
            bound = u.score_bound(k, i, len(fq) - 1)
            assert abs(s - sw) <= bound, (u, what, k, i, penalty, s, sw, bound)
            worst = max(worst, abs(s - sw) / bound)
    return worst


IMAGE_ROUTES = (("host", {}), ("on_device", dict(on_device=True)), ("on_device poll 3", dict(on_device=True, poll_every=3)),
                ("one_call", dict(one_call=True)), ("one_call poll 3", dict(one_call=True, poll_every=3)))


@pytest.mark.parametrize("u", NC.of_kind("image"), ids=lambda u: u.name)
def test_sample_batch_on_every_route(dev, monkeypatch, u):
    family = u.source
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    worst = 0.0
    for k in KS:
        plain = dec.sample_batch(feats, START, end, k=k, one_call=True, **kw)
        assert plain == [family.reference(k, i) for i in range(IMAGES)]
        for what, route in IMAGE_ROUTES:
            for p in PENALTIES:
                got = dec.sample_batch(feats, START, end, k=k, nbest=True, length_penalty=p, **route, **kw)
                worst = max(worst, _compare(u, k, got, p, what))
                if p == 0.0:         # entry 0 is the call without the keyword
                    assert [hyps[0][0] if hyps else [end] for hyps in got] == dec.sample_batch(feats, START, end, k=k, **route, **kw)
        # sample() on one image agrees with sample_batch
        i = k % IMAGES
        for what, route in (IMAGE_ROUTES[0], IMAGE_ROUTES[1], IMAGE_ROUTES[3]):
            one = dec.sample(feats[i:i + 1], START, end, k=k, nbest=True, length_penalty=1.0, **route, **kw)
            assert all(t.dtype == torch.long and t.dim() == 2 and t.shape[0] == 1 and t.device.type == "cuda" for t, _ in one)
            worst = max(worst, _compare(u, k, [[(t[0].tolist(), s) for t, s in one]], 1.0, "sample " + what, images=[i]))
        # the fallback of one_call: the composed step under the device bookkeeping
        monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
        for p in PENALTIES:
            got = dec.sample_batch(feats, START, end, k=k, one_call=True, nbest=True, length_penalty=p, **kw)
            worst = max(worst, _compare(u, k, got, p, "composed"))
        monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP")
    print("%s: worst score error %.3f of its bound" % (u.name, worst))
    with pytest.raises(ops.CapnetError, match="nbest=True"):
        dec.sample_batch(feats, START, end, k=3, length_penalty=1.0, **kw)


@pytest.mark.parametrize("name", list(NC.STYLES))
def test_sample_styles_nbest(dev, monkeypatch, name):
    import style_decode_cases
    family, modes = style_decode_cases.family(name), NC.STYLES[name]
    units = {m: NC.units()["%s/%s" % (name, m)] for m in modes}
    dec = family.make().to(dev).eval()
    feats, end = family.features().to(dev), family.end
    for k in KS:
        plain = dec.sample_styles(feats, START, end, k=k, modes=modes)
        for fallback in (False, True):
            if fallback:
                monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
            for p in PENALTIES:
                got = dec.sample_styles_nbest(feats, START, end, k=k, modes=modes, length_penalty=p, poll_every=3 if p else 0)
                assert set(got) == set(modes)
                for m in modes:
                    _compare(units[m], k, got[m], p, "styles %s%s" % (m, " composed" if fallback else ""))
                    if p == 0.0:
                        assert [hyps[0][0] if hyps else [end] for hyps in got[m]] == plain[m]
            monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)


@pytest.mark.parametrize("u", NC.of_kind("seq2seq"), ids=lambda u: u.name)
def test_seq2seq_sample_beam_on_both_top_k_routes(dev, monkeypatch, u):
    case = u.source
    model = case.module().to(dev)
    feats, end = case.features.float().to(dev), case.end
    for k in case.ks:
        for what, kw in (("fused", dict(fused_topk=True)), ("unfused", dict(fused_topk=False)),
                         ("fused poll 3", dict(fused_topk=True, poll_every=3)), ("composed", {})):
            if what == "composed":
                monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
            plain = model.sample_beam(feats, START, end, mode=case.mode, k=k, **kw)
            assert plain == [case.reference(k, r) for r in range(case.rows)]
            for p in PENALTIES:
                got = model.sample_beam(feats, START, end, mode=case.mode, k=k, nbest=True, length_penalty=p, **kw)
                _compare(u, k, got, p, what)
                if p == 0.0:
                    assert [hyps[0][0] if hyps else [end] for hyps in got] == plain
        monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    with pytest.raises(ops.CapnetError, match="nbest=True"):
        model.sample_beam(feats, START, end, mode=case.mode, k=3, length_penalty=0.5)


def test_seq2seq_sample_beam_styles(dev, monkeypatch):
    import seq2seq_beam_style_cases
    sc = seq2seq_beam_style_cases.case(NC.SEQ2SEQ_STYLE_CASE)
    modes = NC.SEQ2SEQ_STYLE_MODES
    units = {m: NC.units()["%s/%s" % (sc.name, m)] for m in modes}
    model = sc.module().to(dev)
    feats = sc.features.float().to(dev)
    for k in sc.ks:
        for m in modes:              # one <end> per call: mode m's entry is compared at m's own <end>
            end = sc.end(m)
            for what, kw in (("fused", dict(fused_topk=True)), ("unfused", dict(fused_topk=False)), ("loop", {})):
                if what == "loop":
                    monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
                plain = model.sample_beam_styles(feats, START, end, modes=modes, k=k, **kw)
                for p in PENALTIES:
                    got = model.sample_beam_styles(feats, START, end, modes=modes, k=k, nbest=True, length_penalty=p, **kw)
                    assert set(got) == set(modes)
                    _compare(units[m], k, got[m], p, "%s %s" % (what, m))
                    if p == 0.0:
                        for o in modes:
                            assert [hyps[0][0] if hyps else [end] for hyps in got[o]] == plain[o], (what, m, o)
                monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)


# ---- 3. the maps of every hypothesis ---------------------------------------------------------------------------------
def _check_maps(family, feats, i, hyps, maps):
    worst = 0.0
    assert len(maps) == len(hyps)
    for (q, _), m in zip(hyps, maps):
        q = q[0].tolist() if isinstance(q, torch.Tensor) else q
        want = replay(family, i, q)
        assert m.dtype == torch.float32 and m.device.type == "cuda" and tuple(m.shape) == tuple(want.shape) == (len(q) - 1, feats.shape[1])
        worst = max(worst, row_error(m.cpu().double(), want))
    return worst


@pytest.mark.parametrize("u", NC.att_units(), ids=lambda u: NC.ATT_CLASSES[u.name])
def test_maps_of_every_hypothesis(dev, monkeypatch, u):
    family = u.source
    dec = family.make().to(dev).eval()
    assert type(dec).__name__ == NC.ATT_CLASSES[u.name]
    feats, end, kw = family.features().to(dev), family.end, family.kw
    worst = 0.0
    for k in KS:
        assert isinstance(getattr(dec._beam(feats, IMAGES, k, *kw.values(), True)[0], "att", None), decode.AttStack)
        seqs0, maps0 = dec.sample_batch(feats, START, end, k=k, one_call=True, return_alphas=True, **kw)
        for p in PENALTIES:
            got, maps = dec.sample_batch(feats, START, end, k=k, one_call=True, return_alphas=True, nbest=True, length_penalty=p, **kw)
            assert got == dec.sample_batch(feats, START, end, k=k, one_call=True, nbest=True, length_penalty=p, **kw)
            _compare(u, k, got, p, "one_call maps")
            for i in range(IMAGES):
                worst = max(worst, _check_maps(family, feats, i, got[i], maps[i]))
                if p == 0.0 and got[i]:           # the winner's maps are the maps returned without nbest
                    assert got[i][0][0] == seqs0[i] and torch.equal(maps[i][0], maps0[i])
            # the replay routes: the host loop and the device bookkeeping feed every hypothesis back through the composed step
            for route in ({}, dict(on_device=True)):
                got2, maps2 = dec.sample_batch(feats, START, end, k=k, return_alphas=True, nbest=True, length_penalty=p, **route, **kw)
                assert [[q for q, _ in h] for h in got2] == [[q for q, _ in h] for h in got]
                for i in range(IMAGES):
                    worst = max(worst, _check_maps(family, feats, i, got2[i], maps2[i]))
                    for a, b in zip(maps[i], maps2[i]):
                        worst = max(worst, row_error(a.cpu().double(), b.cpu().double()))
        # two chunks give what one gives
        got, maps = dec.sample_batch(feats, START, end, k=k, one_call=True, return_alphas=True, nbest=True, length_penalty=1.0, **kw)
        monkeypatch.setattr(decode, "ALPHA_TRACE_MAX_BYTES", 2 * (MAX_LEN + 1) * k * feats.shape[1] * 4)
        got2, maps2 = dec.sample_batch(feats, START, end, k=k, one_call=True, return_alphas=True, nbest=True, length_penalty=1.0, **kw)
        monkeypatch.setattr(decode, "ALPHA_TRACE_MAX_BYTES", 256 << 20)
        assert got2 == got and all(torch.equal(a, b) for x, y in zip(maps, maps2) for a, b in zip(x, y))
        # sample() on one image
        i = k % IMAGES
        for route in (dict(one_call=True), {}):
            one, m1 = dec.sample(feats[i:i + 1], START, end, k=k, return_alphas=True, nbest=True, length_penalty=1.0, **route, **kw)
            assert [t[0].tolist() for t, _ in one] == [q for q, _ in got[i]]
            worst = max(worst, _check_maps(family, feats, i, one, m1))
    print("%s: worst map error %.2e of max|alpha| (bound %.2e)" % (u.name, worst, BOUND))
    assert worst < BOUND, worst


def test_sample_styles_nbest_with_maps(dev):
    import style_decode_cases
    name = "StackedFactoredLSTMAtt-2"
    family, modes = style_decode_cases.family(name), NC.STYLES[name]
    dec = family.make().to(dev).eval()
    feats, end, k = family.features().to(dev), family.end, 5
    got, maps = dec.sample_styles_nbest(feats, START, end, k=k, modes=modes, length_penalty=1.0, return_alphas=True)
    assert got == dec.sample_styles_nbest(feats, START, end, k=k, modes=modes, length_penalty=1.0)
    plain, maps0 = dec.sample_styles_alphas(feats, START, end, k=k, modes=modes)
    first, first_maps = dec.sample_styles_nbest(feats, START, end, k=k, modes=modes, return_alphas=True)
    for m in modes:
        _compare(NC.units()["%s/%s" % (name, m)], k, got[m], 1.0, "styles maps " + m)
        s1, m1 = dec.sample_batch(feats, START, end, k=k, mode=m, one_call=True, return_alphas=True, nbest=True, length_penalty=1.0)
        assert [[q for q, _ in h] for h in s1] == [[q for q, _ in h] for h in got[m]]
        for i in range(IMAGES):
            assert len(maps[m][i]) == len(got[m][i])
            for (q, _), a, b in zip(got[m][i], maps[m][i], m1[i]):
                assert tuple(a.shape) == (len(q) - 1, feats.shape[1])
                assert row_error(a.cpu().double(), b.cpu().double()) < BOUND, (m, i)
            if first[m][i]:               # penalty 0: the winner and its maps are sample_styles_alphas'
                assert first[m][i][0][0] == plain[m][i] and torch.equal(first_maps[m][i][0], maps0[m][i])
