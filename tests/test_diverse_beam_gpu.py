"""Diverse beam search on the GPU: capnet_beam_advance_diverse and capnet_beam_topk_batched_diverse on stored logits
(tests/diverse_beam_cases.py's tables: a word every group wants, an exact tie only the penalty breaks, a dead group that
counts nothing) -- byte for byte against the plain kernels at strength 0, step by step against the fixed-slot model at 0.5
and 1e4, with and without constraints -- then every route of every image decoder against the fp64 diverse search of every
case (tests/test_diverse_beam_cpu.py asserts that all are admitted: nothing is skipped here).

Tolerances. Tokens, parents, live counts, completion order, trace rows: exact. Scores on stored logits: the siblings',
(len - 1) x seq2seq_cases.need(largest |logit|) against the fp64 model, which carries the unpenalised score. Scores end to
end: constrained_beam_cases.Unit.score_bound's rule, scale the largest |logit| the fp64 search met. Maps:
tests/att_alpha_cases.BOUND. Every test here uses the new keyword or the new entries."""
import pytest
import torch

import diverse_beam_cases as DC
import diverse_beam_ref as R
from att_alpha_cases import BOUND, row_error
from att_alpha_ref import replay
from capnet import ops
from capnet.beam import Diversity
from diverse_beam_cases import IMAGES, PENALTIES, START, TABLE_END, TABLE_N, TABLE_START, TABLE_T
from seq2seq_cases import need

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _clean(dev, monkeypatch):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    yield
    ops.check_device_errors()


def _buffers(dev, rows, count):
    return [torch.empty(rows, dtype=torch.long, device=dev) for _ in range(count)]


# ---- 1. strength 0: the plain kernels, byte for byte -------------------------------------------------------------------
@pytest.mark.parametrize("k,D,V", DC.TABLE_CASES)
def test_strength_zero_leaves_the_state_of_the_plain_searches(dev, k, D, V):
    n, T, kp = TABLE_N, TABLE_T, k // D
    tab = DC.table(k, D, V)
    dv = Diversity(D, 0.0)
    w = _buffers(dev, n * k, 8)
    p = _buffers(dev, n * k, 4)
    diverse, traced = ops.beam_init(n * D, kp, T, TABLE_START, w[0]), ops.beam_init(n * D, kp, T, TABLE_START, w[2])
    plain, plain_t = ops.beam_init(n * D, kp, T, TABLE_START, w[4]), ops.beam_init(n * D, kp, T, TABLE_START, w[6])
    for other in (traced, plain, plain_t):       # (the words no kernel has written yet are whatever the allocator left)
        other.words.copy_(diverse.words)
    trace_d, trace_p = ops.beam_trace(traced), ops.beam_trace(plain_t)
    trace_d.fill_(0x7fffffff)
    trace_p.fill_(0x7fffffff)
    for step in range(1, T + 1):
        x = [tab[step - 1].to(dev) for _ in range(4)]
        s = step & 1
        ops.beam_advance(diverse, x[0], step, TABLE_END, w[s], p[0], diversity=dv)
        ops.beam_advance(traced, x[1], step, TABLE_END, w[2 + s], p[1], diversity=dv, trace=trace_d)
        ops.beam_advance(plain, x[2], step, TABLE_END, w[4 + s], p[2])                  # n D searches of k / D beams
        ops.beam_advance_traced(plain_t, trace_p, x[3], step, TABLE_END, w[6 + s], p[3])
        assert torch.equal(diverse.words, plain.words) and torch.equal(traced.words, plain_t.words), step
        assert torch.equal(diverse.words, traced.words), step
        assert torch.equal(w[s], w[4 + s]) and torch.equal(w[2 + s], w[6 + s]) and torch.equal(w[s], w[2 + s]), step
        assert torch.equal(p[0], p[2]) and torch.equal(p[1], p[3]) and torch.equal(p[0], p[1]), step
        assert torch.equal(trace_d, trace_p), step
        assert torch.equal(x[0], x[2]) and torch.equal(x[1], x[2])                      # logit - 0 * count: not a bit changed
    assert int(diverse.live_total) < n * k                                              # (image 2 completed: the tail ran)


# ---- 2. against the fixed-slot model -------------------------------------------------------------------------------------
def _state(beam):
    """(live [n], n_done [n], scores [n, k], done_score [n, k]) out of the state's words."""
    n, k, w = beam.n, beam.k, beam.words
    f = w[4 + 2 * n:4 + 2 * n + 2 * n * k].view(torch.float32)
    return w[4:4 + n].tolist(), w[4 + n:4 + 2 * n].tolist(), f[:n * k].view(n, k).tolist(), f[n * k:].view(n, k).tolist()


TABLE_RUNS = [(s, c) for s in DC.TABLE_STRENGTHS for c in (None, DC.TABLE_CONSTRAINTS)]


@pytest.mark.parametrize("k,D,V", DC.TABLE_CASES)
def test_advance_equals_the_model_on_stored_logits(dev, k, D, V):
    n, T, kp, L = TABLE_N, TABLE_T, k // D, TABLE_T + 2
    tab = DC.table(k, D, V)
    bound = need(float(tab.abs().max()))
    for strength, con in TABLE_RUNS:
        what = (strength, con)
        model, gap = DC.model(k, D, V, strength, tab, con)
        assert gap > DC.TABLE_GAP
        dv = Diversity(D, strength)
        w, p = _buffers(dev, n * k, 2), _buffers(dev, n * k, 1)[0]
        beam = ops.beam_init(n * D, kp, T, TABLE_START, w[0])
        trace = ops.beam_trace(beam)
        trace.fill_(0x7fffffff)
        for step in range(1, T + 1):
            x = tab[step - 1].to(dev)
            ops.beam_advance(beam, x, step, TABLE_END, w[step & 1], p, constraints=con, diversity=dv, trace=trace)
            want_words, want_rows, _, _ = model.outputs[step]
            assert w[step & 1].tolist() == want_words and p.tolist() == want_rows, (what, step)
            live, n_done, scores, done_score = _state(beam)
            want_live, want_scores, want_done = model.states[step]
            assert live == want_live and n_done == [len(d) for d in want_done], (what, step)
            assert int(beam.live_total) == sum(want_live)
            for q in range(n * D):
                for a, b in zip(scores[q], want_scores[q]):
                    assert abs(a - b) <= step * bound, (what, step, q, a, b)           # unpenalised, at 1e4 too
                for a, (b, tokens) in zip(done_score[q], want_done[q]):
                    assert abs(a - b) <= (len(tokens) - 1) * bound, (what, step, q, a, b)
        for penalty in PENALTIES:
            seqs, lengths, scores, counts, rows = ops.beam_nbest_traced(beam, trace, TABLE_END, penalty)
            want = model.nbest(penalty)
            assert counts.tolist() == [len(h) for h in want]
            for q in range(n * D):
                for r, (tokens, sc) in enumerate(want[q]):
                    ln = int(lengths[q, r])
                    assert seqs[q, r, :ln].tolist() == tokens and seqs[q, r, ln:].tolist() == [0] * (L - ln), (what, penalty, q, r)
                    assert abs(float(scores[q, r]) - sc) <= (ln - 1) * bound, (what, penalty, q, r)
            assert rows.tolist() == model.nbest_rows(T, penalty)
        fin = ops.beam_finish_traced(beam, trace, TABLE_END)
        assert [fin[0][q, :int(fin[1][q])].tolist() for q in range(n * D)] == model.finish()
        assert fin[2].tolist() == model.winner_rows(T)


@pytest.mark.parametrize("k,D,V", DC.TABLE_CASES)
def test_batched_topk_equals_the_model_and_the_groups_share_no_word(dev, k, D, V):
    n, T, kp = TABLE_N, TABLE_T, k // D
    tab = DC.table(k, D, V)
    bound = need(float(tab.abs().max()))
    for strength, con in TABLE_RUNS:
        what = (strength, con)
        model, _ = DC.model(k, D, V, strength, tab, con)
        host = R.DiverseBeam(n, k, D, strength, V, TABLE_START, TABLE_END, con)
        dv = Diversity(D, strength)
        for step in range(1, T + 1):
            x = tab[step - 1].to(dev)
            competing = [(1 if step == 1 else live) if live else 0 for live in host.live]
            bans = None
            if con is not None:
                lists = [[] for _ in range(n * k)]
                for q in range(n * D):
                    for r, b in enumerate(host.bans(step, q, competing[q])):
                        lists[q * kp + r] = b
                cap = max(1, max(len(b) for b in lists))
                bans = torch.tensor([[len(b)] + b + [0] * (cap - len(b)) for b in lists], dtype=torch.int32, device=dev)
            meta = torch.tensor([(q * kp, competing[q], host.live[q]) for q in range(n * D)], dtype=torch.int32, device=dev)
            prev = torch.tensor([v for row in host.scores for v in row], dtype=torch.float32, device=dev)
            scores, flat = ops.beam_topk_batched(x, prev, meta, bans=bans, diversity=dv)
            assert tuple(scores.shape) == (n * D, 16) and tuple(flat.shape) == (n * D, 16)
            scores, flat = scores.tolist(), flat.tolist()
            host.advance(step, lambda q, nrows, kk: (scores[q][:kk], flat[q][:kk]))
            assert host.outputs[step] == model.outputs[step], (what, step)
            for q, (want_scores, want_flat) in model.selected[step].items():
                assert host.selected[step][q][1] == want_flat, (what, step, q)
                for a, b in zip(host.selected[step][q][0], want_scores):
                    assert abs(a - b) <= step * bound, (what, step, q, a, b)
            if strength == 1e4:     # the property, from the device's own selections: live groups of an image share no word
                for i in range(n):
                    assert not R.shared_words(R.group_words(host, step, i)), (what, step, i)
        assert host.finish() == model.finish()
        for i in range(n):
            assert [[t for _, t in d] for d in host.group_done(i)] == [[t for _, t in d] for d in model.group_done(i)]
        if con is None:             # the exact tie of image 1: B_, where the plain tie rule gives A_
            assert host.selected[DC.TIE_STEP][1 * D + 1][1][0] % V == DC.B_


# ---- 3. every route end to end -----------------------------------------------------------------------------------------
ROUTES = (("host", {}), ("on_device", dict(on_device=True)), ("one_call", dict(one_call=True)))


def _check_lists(u, k, D, got, penalty, what, **skw):
    """got: per image [(tokens, score)] against the fp64 diverse search's deduplicated, ranked n-best -> the worst score
    error over its bound."""
    worst = 0.0
    assert len(got) == IMAGES, what
    for i, hyps in enumerate(got):
        want = u.search(k, D, i, **skw).nbest(penalty)
        assert [q for q, _ in hyps] == [q for q, _ in want], (u, what, k, D, i, penalty)
        for (q, sc), (_, ref) in zip(hyps, want):
            bound = u.score_bound(k, D, i, len(q) - 1, **skw)
            assert isinstance(sc, float) and abs(sc - ref) <= bound, (u, what, k, D, i, penalty, sc, ref, bound)
            worst = max(worst, abs(sc - ref) / bound)
    return worst


def _check_groups(u, k, D, got, penalty, what, **skw):
    assert len(got) == IMAGES, what
    for i, entries in enumerate(got):
        want = u.search(k, D, i, **skw).per_group(penalty)
        assert len(entries) == D and [e if e is None else e[0] for e in entries] == [e if e is None else e[0] for e in want], \
            (u, what, k, D, i, penalty)
        for e, ref in zip(entries, want):
            if e is not None:
                assert abs(e[1] - ref[1]) <= u.score_bound(k, D, i, len(e[0]) - 1, **skw), (u, what, k, D, i, e, ref)


@pytest.mark.parametrize("u", DC.units(), ids=lambda u: u.name)
def test_every_route_returns_the_diverse_search(dev, monkeypatch, u):
    family = u.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    worst = 0.0
    for k, D in DC.SHAPES:
        dv, pg = Diversity(D, u.strength(k, D)), Diversity(D, u.strength(k, D), per_group=True)
        assert all(u.admitted(k, D, i) for i in range(IMAGES))
        want = [u.search(k, D, i).winner() for i in range(IMAGES)]
        for what, route in ROUTES:
            assert dec.sample_batch(feats, START, end, k=k, diversity=dv, **route, **kw) == want, (u, k, D, what)
            for p in PENALTIES:
                got = dec.sample_batch(feats, START, end, k=k, diversity=dv, nbest=True, length_penalty=p, **route, **kw)
                worst = max(worst, _check_lists(u, k, D, got, p, what))
                got = dec.sample_batch(feats, START, end, k=k, diversity=pg, nbest=True, length_penalty=p, **route, **kw)
                _check_groups(u, k, D, got, p, what)
            i = k % IMAGES           # sample(): one image
            one = dec.sample(feats[i:i + 1], START, end, k=k, diversity=dv, **route, **kw)
            assert one.dtype == torch.long and one[0].tolist() == want[i], (u, k, D, i, what)
            one = dec.sample(feats[i:i + 1], START, end, k=k, diversity=pg, nbest=True, **route, **kw)
            ref = u.search(k, D, i).per_group(0.0)
            assert [e if e is None else e[0][0].tolist() for e in one] == [e if e is None else e[0] for e in ref], (u, k, D, i, what)
        # the fallback of one_call: the composed step under the device bookkeeping
        monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
        assert dec.sample_batch(feats, START, end, k=k, diversity=dv, one_call=True, **kw) == want, (u, k, D, "composed")
        got = dec.sample_batch(feats, START, end, k=k, diversity=dv, nbest=True, length_penalty=1.0, one_call=True, **kw)
        worst = max(worst, _check_lists(u, k, D, got, 1.0, "composed"))
        monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP")
    print("%s: worst score error %.3f of its bound" % (u.name, worst))


@pytest.mark.parametrize("u", [u for u in DC.units() if DC.is_attention(u)], ids=lambda u: u.name)
def test_maps_of_a_diverse_search(dev, u):
    family = u.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    k, D = DC.SHAPES[2]
    dv, pg = Diversity(D, u.strength(k, D)), Diversity(D, u.strength(k, D), per_group=True)
    worst = 0.0
    for what, route in ROUTES:
        got, maps = dec.sample_batch(feats, START, end, k=k, diversity=dv, return_alphas=True, **route, **kw)
        assert got == [u.search(k, D, i).winner() for i in range(IMAGES)], (u, what)
        for i in range(IMAGES):
            ref = replay(family, i, got[i])
            assert maps[i].dtype == torch.float32 and tuple(maps[i].shape) == tuple(ref.shape), (u, what, i)
            worst = max(worst, row_error(maps[i].cpu().double(), ref))
        hyps, hmaps = dec.sample_batch(feats, START, end, k=k, diversity=dv, return_alphas=True, nbest=True, length_penalty=1.0,
                                       **route, **kw)
        _check_lists(u, k, D, hyps, 1.0, what)
        groups, gmaps = dec.sample_batch(feats, START, end, k=k, diversity=pg, return_alphas=True, nbest=True, **route, **kw)
        _check_groups(u, k, D, groups, 0.0, what)
        for i in range(IMAGES):
            assert len(hmaps[i]) == len(hyps[i]) and len(gmaps[i]) == D
            for (q, _), m in zip(hyps[i], hmaps[i]):
                worst = max(worst, row_error(m.cpu().double(), replay(family, i, q)))
            for e, m in zip(groups[i], gmaps[i]):
                assert (e is None) == (m is None)
                if e is not None:
                    worst = max(worst, row_error(m.cpu().double(), replay(family, i, e[0])))
    one, m1 = dec.sample(feats[1:2], START, end, k=k, diversity=dv, return_alphas=True, one_call=True, **kw)
    assert one[0].tolist() == u.search(k, D, 1).winner()
    worst = max(worst, row_error(m1.cpu().double(), replay(family, 1, one[0].tolist())))
    print("%s: worst map error %.2e of max|alpha| (bound %.2e)" % (u.name, worst, BOUND))
    assert worst < BOUND, worst


@pytest.mark.parametrize("name,k,D", DC.CON_CASES)
def test_with_constraints_and_with_polling(dev, name, k, D):
    u = DC.unit(name)
    family, con = u.family, DC.con_set()
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    dv = Diversity(D, u.strength(k, D))
    want = [u.search(k, D, i, constraints=con).winner() for i in range(IMAGES)]
    assert want != [u.search(k, D, i).winner() for i in range(IMAGES)] or \
        any(u.search(k, D, i, constraints=con).nbest(0.0) != u.search(k, D, i).nbest(0.0) for i in range(IMAGES))
    for what, route in ROUTES:
        assert dec.sample_batch(feats, START, end, k=k, diversity=dv, constraints=con, **route, **kw) == want, (u, what)
        got = dec.sample_batch(feats, START, end, k=k, diversity=dv, constraints=con, nbest=True, length_penalty=1.0, **route, **kw)
        _check_lists(u, k, D, got, 1.0, what, constraints=con)
    # poll_every: the same results, the loop stopped when no beam is live
    want = [u.search(k, D, i).winner() for i in range(IMAGES)]
    for route in (dict(on_device=True, poll_every=2), dict(one_call=True, poll_every=2)):
        assert dec.sample_batch(feats, START, end, k=k, diversity=dv, **route, **kw) == want, (u, route)
        got = dec.sample_batch(feats, START, end, k=k, diversity=dv, nbest=True, **route, **kw)
        _check_lists(u, k, D, got, 0.0, route)


# ---- 4. parity with the plain search, and unchanged defaults -------------------------------------------------------------
@pytest.mark.parametrize("u", DC.units(), ids=lambda u: u.name)
def test_strength_zero_is_the_plain_search_of_each_group_and_one_group_changes_nothing(dev, u):
    family = u.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    for k, D in DC.SHAPES:
        for what, route in ROUTES:
            plain = dec.sample_batch(feats, START, end, k=k // D, **route, **kw)
            got = dec.sample_batch(feats, START, end, k=k, diversity=Diversity(D, 0.0, per_group=True), nbest=True, **route, **kw)
            for i in range(IMAGES):          # tokens only: the row counts differ, so the scores' last bits may
                assert u.admitted(k // D, 1, i)
                assert [None if e is None else e[0] for e in got[i]] == [None if plain[i] == [end] else plain[i]] * D, (u, k, D, what, i)
    k = DC.SHAPES[0][0]
    for what, route in ROUTES:
        free = dec.sample_batch(feats, START, end, k=k, **route, **kw)
        lists = dec.sample_batch(feats, START, end, k=k, nbest=True, **route, **kw)
        for dv in (None, Diversity(1, 0.5), Diversity(1, 0.5, per_group=True)):
            assert dec.sample_batch(feats, START, end, k=k, diversity=dv, **route, **kw) == free, (u, what, dv)
            assert dec.sample_batch(feats, START, end, k=k, diversity=dv, nbest=True, **route, **kw) == lists, (u, what, dv)
        one = dec.sample(feats[:1], START, end, k=k, diversity=Diversity(1, 0.5), **route, **kw)
        assert torch.equal(one, dec.sample(feats[:1], START, end, k=k, **route, **kw))


@pytest.mark.parametrize("name", ["StackedFactoredLSTM-2", "DecoderFactoredLSTMAtt"])
def test_one_call_runs_the_one_call_entries(dev, monkeypatch, name):
    """one_call=True on a supported shape is capnet_beam_decode_diverse / capnet_att_beam_decode_diverse: no Python loop runs."""
    from capnet import decode
    u = DC.unit(name)
    dec = u.family.make().to(dev).eval()
    feats, k, D = u.family.features().to(dev), *DC.SHAPES[0]

    def never(*a, **kw):
        raise AssertionError("a Python loop ran under one_call=True")
    monkeypatch.setattr(decode, "beam_search_device", never)
    monkeypatch.setattr(decode, "beam_search_batched", never)
    got = dec.sample_batch(feats, START, u.end, k=k, diversity=Diversity(D, u.strength(k, D)), one_call=True, **u.family.kw)
    assert got == [u.search(k, D, i).winner() for i in range(IMAGES)]
    calls = []
    lib = ops._lib.lib()
    for entry in ("capnet_beam_decode_diverse", "capnet_att_beam_decode_diverse"):
        real = getattr(lib, entry)
        monkeypatch.setattr(lib, entry, lambda *a, real=real, entry=entry: calls.append(entry) or real(*a))
    dec.sample_batch(feats, START, u.end, k=k, diversity=Diversity(D, u.strength(k, D)), one_call=True, **u.family.kw)
    assert calls == ["capnet_att_beam_decode_diverse" if DC.is_attention(u) else "capnet_beam_decode_diverse"]


def test_refused_on_every_route(dev):
    u = DC.units()[0]
    dec = u.family.make().to(dev).eval()
    feats = u.family.features().to(dev)
    for route in (dict(), dict(on_device=True), dict(one_call=True)):
        with pytest.raises(ops.CapnetError, match="divide"):
            dec.sample_batch(feats, START, u.end, k=5, diversity=Diversity(2, 1.0), **route, **u.family.kw)
        with pytest.raises(ops.CapnetError, match="per_group"):
            dec.sample_batch(feats, START, u.end, k=4, diversity=Diversity(2, 1.0, per_group=True), **route, **u.family.kw)
