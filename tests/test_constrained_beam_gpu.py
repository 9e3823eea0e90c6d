"""Constrained beam search on the GPU: capnet_beam_advance_constrained[_traced] and capnet_beam_topk[_batched]_banned
against the fixed-slot model on stored logits (tests/constrained_beam_cases.py's tables: a word that would repeat forever, a
context seen twice with an exact tie behind it, <end> and a banned word ahead of everything), then every route of every
image decoder against the constrained fp64 search of every case (tests/test_constrained_beam_cpu.py asserts that all are
admitted: nothing is skipped here), the properties of everything returned, and that none of it is vacuous.

Tolerances. Tokens, parents, completion order, trace rows, the -inf written into the logits block: exact. Scores on stored
logits: tests/test_nbest_gpu.py's, (len - 1) x seq2seq_cases.need(largest |logit|) of the fp64 model's -- which takes its
log-sum-exp over the unmodified rows (image 2 of the tables loses about 10 nats a step to a banned word: a log-sum-exp
taken after the removal would be off by that much). Scores end to end and against score_captions: the same rule, scale the
largest |logit| the fp64 search met. Maps: tests/att_alpha_cases.BOUND."""
import pytest
import torch

import constrained_beam_cases as CC
import constrained_beam_ref as R
from att_alpha_cases import BOUND, row_error
from att_alpha_ref import replay
from capnet import ops
from capnet.beam import Constraints
from constrained_beam_cases import IMAGES, KS, MARGIN, PENALTIES, SETS, START, TABLE_END, TABLE_N, TABLE_START, TABLE_T
from seq2seq_cases import need

pytestmark = pytest.mark.gpu
NEG = float("-inf")


@pytest.fixture(autouse=True)
def _clean(dev, monkeypatch):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    yield
    ops.check_device_errors()


# ---- 1. the kernels on stored logits ---------------------------------------------------------------------------------
def _done_scores(beam):
    """done_score [n, k] out of the state's words: [4] | live[n] | n_done[n] | scores[n k] | done_score[n k]."""
    n, k = beam.n, beam.k
    w = beam.words
    return w[4 + n:4 + 2 * n].tolist(), w[4 + 2 * n + n * k:4 + 2 * n + 2 * n * k].view(torch.float32).view(n, k)


@pytest.mark.parametrize("k,V", CC.TABLE_CASES)
def test_advance_equals_the_model_on_stored_logits(dev, k, V):
    n, T, L = TABLE_N, TABLE_T, TABLE_T + 2
    tab = CC.table(k, V)
    scale = float(tab.abs().max())
    for s, c in CC.TABLE_SETS.items():
        model, gap = CC.model(k, V, s, tab)
        assert gap > CC.TABLE_GAP
        words = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(4)]
        parent = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(2)]
        traced, plain = ops.beam_init(n, k, T, TABLE_START, words[0]), ops.beam_init(n, k, T, TABLE_START, words[2])
        trace = ops.beam_trace(traced)
        trace.fill_(0x7fffffff)
        for step in range(1, T + 1):
            x, y = tab[step - 1].to(dev), tab[step - 1].to(dev)
            ops.beam_advance_traced(traced, trace, x, step, TABLE_END, words[step & 1], parent[0], constraints=c)
            ops.beam_advance(plain, y, step, TABLE_END, words[2 + (step & 1)], parent[1], constraints=c)
            want_words, want_rows, competing = model.outputs[step]
            assert words[step & 1].tolist() == words[2 + (step & 1)].tolist() == want_words, (s, step)
            assert parent[0].tolist() == parent[1].tolist() == want_rows, (s, step)
            # the block: -inf over what the rule excludes on the rows that competed, not a bit changed elsewhere
            want = tab[step - 1].clone()
            for i in range(n):
                for r in range(competing[i]):
                    want[i * k + r, model.excluded[step][(i, r)]] = NEG
            assert torch.equal(x.cpu(), want) and torch.equal(y.cpu(), want), (s, step)
        # completion order and scores; the entry without the trace leaves the same state
        n_done, done_score = _done_scores(traced)
        assert _done_scores(plain)[0] == n_done
        assert all(torch.equal(done_score[i, :n_done[i]], _done_scores(plain)[1][i, :n_done[i]]) for i in range(n))
        assert n_done == [len(model.completed(i)) for i in range(n)]
        for i in range(n):
            for j, (sc, q) in enumerate(model.completed(i)):
                assert abs(float(done_score[i, j]) - sc) <= (len(q) - 1) * need(scale), (s, i, j, float(done_score[i, j]), sc)
        # finish and n-best, with the trace rows
        seqs, lengths, rows = ops.beam_finish_traced(traced, trace, TABLE_END)
        assert [seqs[i, :int(lengths[i])].tolist() for i in range(n)] == model.finish()
        assert rows.tolist() == model.winner_rows(T)
        fin = ops.beam_finish(plain, TABLE_END)
        assert torch.equal(fin[0], seqs) and torch.equal(fin[1], lengths)
        for penalty in PENALTIES:
            seqs, lengths, scores, counts, rows = ops.beam_nbest_traced(traced, trace, TABLE_END, penalty)
            want = model.nbest(penalty)
            assert counts.tolist() == [len(w) for w in want]
            for i in range(n):
                for r, (q, sc) in enumerate(want[i]):
                    ln = int(lengths[i, r])
                    assert seqs[i, r, :ln].tolist() == q and seqs[i, r, ln:].tolist() == [0] * (L - ln), (s, penalty, i, r)
                    assert abs(float(scores[i, r]) - sc) <= (ln - 1) * need(scale), (s, penalty, i, r)
            assert rows.tolist() == model.nbest_rows(T, penalty)
        # what the scripts are there for
        every = [q for i in range(n) for q, _ in want[i]]
        assert all(not R.violations(q, TABLE_END, c) for q in every)
        assert int(lengths[2, 0]) == CC.TABLE_MIN_WORDS + 2 and counts[2] == k


@pytest.mark.parametrize("k,V", CC.TABLE_CASES)
def test_banned_topk_equals_the_model_on_stored_logits(dev, k, V):
    n, T = TABLE_N, TABLE_T
    tab = CC.table(k, V)
    scale = float(tab.abs().max())
    for s, c in CC.TABLE_SETS.items():
        model, _ = CC.model(k, V, s, tab)
        host = R.ConstrainedBeam(n, k, V, TABLE_START, TABLE_END, c)
        for step in range(1, T + 1):
            x = tab[step - 1].to(dev)
            competing = [(1 if step == 1 else live) if live else 0 for live in host.live]
            lists = [[] for _ in range(n * k)]
            for i in range(n):
                for r, b in enumerate(host.bans(step, i, competing[i])):
                    lists[i * k + r] = b
            cap = max(1, max(len(b) for b in lists))
            bans = torch.tensor([[len(b)] + b + [0] * (cap - len(b)) for b in lists], dtype=torch.int32, device=dev)
            meta = torch.tensor([(i * k, competing[i], host.live[i]) for i in range(n)], dtype=torch.int32, device=dev)
            prev = torch.tensor([v for row in host.scores for v in row], dtype=torch.float32, device=dev)
            for i in range(n):             # the single-image form, on a copy of the image's rows
                if host.live[i]:
                    one = ops.beam_topk(x[i * k:(i + 1) * k].clone(), prev[i * k:(i + 1) * k], competing[i], host.live[i],
                                        bans=bans[i * k:(i + 1) * k].contiguous())
                    lists[i * k] = (one[0].tolist(), one[1].tolist())
            scores, flat = ops.beam_topk_batched(x, prev, meta, bans=bans)
            scores, flat = scores.tolist(), flat.tolist()
            for i in range(n):
                if host.live[i]:
                    assert lists[i * k] == (scores[i][:host.live[i]], flat[i][:host.live[i]]), (s, step, i)
            host.advance(step, lambda i, nrows, kk: (scores[i][:kk], flat[i][:kk]))
            assert host.outputs[step] == model.outputs[step], (s, step)
        assert host.finish() == model.finish()
        for i in range(n):
            assert [q for _, q in host.completed(i)] == [q for _, q in model.completed(i)]
            for (a, q), (b, _) in zip(host.completed(i), model.completed(i)):
                assert abs(a - b) <= (len(q) - 1) * need(scale), (s, i, a, b)


# ---- 2. every route end to end ---------------------------------------------------------------------------------------
ROUTES = (("host", {}), ("on_device", dict(on_device=True)), ("one_call", dict(one_call=True)))
POLLED = (("on_device poll 3", dict(on_device=True, poll_every=3)), ("one_call poll 3", dict(one_call=True, poll_every=3)))


def _check_nbest(u, s, k, got, penalty, what, images=None):
    """got: per image [(tokens, score)] against the constrained fp64 search -> the worst score error over its bound. The
    order is compared where the ranking gap at this penalty is admitted (nbest_cases' rule), the set everywhere."""
    worst = 0.0
    images = range(IMAGES) if images is None else images
    assert len(got) == len(images), what
    for hyps, i in zip(got, images):
        search = u.search(k, i, s)
        want = search.nbest(penalty)
        if search.gap(penalty) > MARGIN:
            assert [q for q, _ in hyps] == [q for q, _ in want], (u, s, what, k, i, penalty)
        assert sorted(q for q, _ in hyps) == sorted(q for q, _ in want), (u, s, what, k, i, penalty)
        by_tokens = {tuple(q): sc for q, sc in want}
        for q, sc in hyps:
            assert isinstance(sc, float) and not R.violations(q, u.end, SETS[s]), (u, s, what, q)
            bound = u.score_bound(k, i, s, len(q) - 1)
            assert abs(sc - by_tokens[tuple(q)]) <= bound, (u, s, what, k, i, penalty, sc, by_tokens[tuple(q)], bound)
            worst = max(worst, abs(sc - by_tokens[tuple(q)]) / bound)
    return worst


def _check_scores_are_the_models(u, s, k, dec, feats, kw, got):
    """Every n-best score is decoder.score_captions of its tokens, within the score bound."""
    caps = [q for hyps in got for q, _ in hyps]
    if not caps:
        return
    rows = torch.tensor([i for i, hyps in enumerate(got) for _ in hyps], device=feats.device)
    model_scores = dec.score_captions(feats.index_select(0, rows), caps, **kw).tolist()
    at = 0
    for i, hyps in enumerate(got):
        for q, sc in hyps:
            bound = u.score_bound(k, i, s, len(q) - 1)
            assert abs(sc - model_scores[at]) <= bound, (u, s, k, i, q, sc, model_scores[at], bound)
            at += 1


@pytest.mark.parametrize("u", CC.units(), ids=lambda u: u.name)
def test_every_route_returns_the_constrained_search(dev, monkeypatch, u):
    family = u.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    worst = 0.0
    for s, c in SETS.items():
        for k in KS:
            want = [u.winner(k, i, s) for i in range(IMAGES)]
            assert all(u.admitted(k, i, s) for i in range(IMAGES))
            for what, route in ROUTES + POLLED:
                got = dec.sample_batch(feats, START, end, k=k, constraints=c, **route, **kw)
                assert got == want, (u, s, k, what)
            assert all(not R.violations(q, end, c) for q in got if q != [end])          # ([end] alone: nothing completed)
            # sample() per image
            for i in range(IMAGES):
                for what, route in ROUTES:
                    one = dec.sample(feats[i:i + 1], START, end, k=k, constraints=c, **route, **kw)
                    assert one.dtype == torch.long and one[0].tolist() == want[i], (u, s, k, i, what)
            # the n-best lists, their scores, and the model's own log-probability of every hypothesis
            for p in PENALTIES:
                for what, route in ROUTES:
                    got = dec.sample_batch(feats, START, end, k=k, nbest=True, length_penalty=p, constraints=c, **route, **kw)
                    worst = max(worst, _check_nbest(u, s, k, got, p, what))
                    if p == 0.0:
                        assert [hyps[0][0] if hyps else [end] for hyps in got] == want
                    _check_scores_are_the_models(u, s, k, dec, feats, kw, got)
            i = k % IMAGES
            one = dec.sample(feats[i:i + 1], START, end, k=k, nbest=True, length_penalty=1.0, constraints=c, one_call=True, **kw)
            worst = max(worst, _check_nbest(u, s, k, [[(t[0].tolist(), sc) for t, sc in one]], 1.0, "sample nbest", images=[i]))
            # the fallback of one_call: the composed step under the device bookkeeping
            monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
            assert dec.sample_batch(feats, START, end, k=k, constraints=c, one_call=True, **kw) == want, (u, s, k, "composed")
            got = dec.sample_batch(feats, START, end, k=k, nbest=True, length_penalty=1.0, constraints=c, one_call=True, **kw)
            worst = max(worst, _check_nbest(u, s, k, got, 1.0, "composed nbest"))
            monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP")
    print("%s: worst score error %.3f of its bound" % (u.name, worst))


@pytest.mark.parametrize("u", [u for u in CC.units() if CC.is_attention(u)], ids=lambda u: u.name)
def test_maps_under_constraints(dev, u):
    family = u.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    worst = 0.0
    for s, c in SETS.items():
        for k in KS:
            want = [u.winner(k, i, s) for i in range(IMAGES)]
            for what, route in ROUTES:
                got, maps = dec.sample_batch(feats, START, end, k=k, return_alphas=True, constraints=c, **route, **kw)
                assert got == want, (u, s, k, what)          # the tokens are unchanged by the keyword
                for i in range(IMAGES):
                    ref = replay(family, i, got[i])
                    assert maps[i].dtype == torch.float32 and tuple(maps[i].shape) == tuple(ref.shape), (u, s, k, what, i)
                    worst = max(worst, row_error(maps[i].cpu().double(), ref))
            i = k % IMAGES
            one, m1 = dec.sample(feats[i:i + 1], START, end, k=k, return_alphas=True, constraints=c, one_call=True, **kw)
            assert one[0].tolist() == want[i]
            worst = max(worst, row_error(m1.cpu().double(), replay(family, i, want[i])))
            hyps, hmaps = dec.sample_batch(feats, START, end, k=k, return_alphas=True, nbest=True, length_penalty=1.0, constraints=c,
                                           one_call=True, **kw)
            _check_nbest(u, s, k, hyps, 1.0, "nbest maps")
            for i in range(IMAGES):
                for (q, _), m in zip(hyps[i], hmaps[i]):
                    worst = max(worst, row_error(m.cpu().double(), replay(family, i, q)))
    print("%s: worst map error %.2e of max|alpha| (bound %.2e)" % (u.name, worst, BOUND))
    assert worst < BOUND, worst


# ---- 3. not vacuous --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u", CC.units(), ids=lambda u: u.name)
def test_the_constraints_change_the_result_and_none_changes_nothing(dev, u):
    family = u.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    k = KS[1]
    free = {}
    for what, route in ROUTES:
        free[what] = dec.sample_batch(feats, START, end, k=k, **route, **kw)
        assert free[what] == [family.reference(k, i) for i in range(IMAGES)]
        for c in (None, Constraints()):
            assert dec.sample_batch(feats, START, end, k=k, constraints=c, **route, **kw) == free[what], (u, what, c)
            lists = dec.sample_batch(feats, START, end, k=k, nbest=True, constraints=c, **route, **kw)
            assert lists == dec.sample_batch(feats, START, end, k=k, nbest=True, **route, **kw), (u, what, c)
        one = dec.sample(feats[:1], START, end, k=k, constraints=Constraints(), **route, **kw)
        assert torch.equal(one, dec.sample(feats[:1], START, end, k=k, **route, **kw))
    # a case the CPU test lists as changed, under every set: the unconstrained call returns other lists
    for s in SETS:
        if s == "C" and u.name in CC.C_UNCHANGED:
            continue
        kk, i = u.changed(s)[0]
        for what, route in ROUTES:
            with_c = dec.sample_batch(feats, START, end, k=kk, nbest=True, constraints=SETS[s], **route, **kw)
            without = dec.sample_batch(feats, START, end, k=kk, nbest=True, **route, **kw)
            assert [q for q, _ in with_c[i]] != [q for q, _ in without[i]], (u, s, kk, i, what)
            assert sorted(q for q, _ in with_c[i]) == sorted(q for _, q in u.search(kk, i, s).done), (u, s, kk, i, what)
    # ... and the caption itself is another one in the family's first such case
    s, kk, i = CC.other_winner(u)
    for what, route in ROUTES:
        with_c = dec.sample_batch(feats, START, end, k=kk, constraints=SETS[s], **route, **kw)
        without = dec.sample_batch(feats, START, end, k=kk, **route, **kw)
        assert with_c[i] != without[i] and with_c[i] == u.winner(kk, i, s) and without[i] == u.winner(kk, i, None), (u, s, kk, i, what)


def test_refused_on_the_device_routes_too(dev):
    u = CC.units()[0]
    dec = u.family.make().to(dev).eval()
    feats = u.family.features().to(dev)
    for route in (dict(), dict(on_device=True), dict(one_call=True)):
        with pytest.raises(ops.CapnetError, match="end_token"):
            dec.sample_batch(feats, START, u.end, k=3, constraints=Constraints(banned=(u.end,)), **route, **u.family.kw)
        with pytest.raises(ops.CapnetError, match="min_words"):
            dec.sample_batch(feats, START, u.end, k=3, constraints=Constraints(min_words=CC.MAX_LEN), **route, **u.family.kw)
