"""Forced words in beam search on the GPU: capnet_beam_advance_forced (with and without a trace) and
capnet_beam_topk_batched_forced against the fixed-slot model on stored logits (tests/forced_beam_cases.py's tables: a forced
word at -30, a forced word that is also the plain selection's and the row's best, an exact tie inside a bank, <end> far ahead
of words that must come first), then every route of every image decoder against the forced fp64 search of every case
(tests/test_forced_beam_cpu.py asserts that all are admitted: nothing is skipped here), the properties of everything
returned, and that forced=() changes nothing.

Tolerances. Tokens, parents, slot order, completion order, trace rows: exact. Scores on stored logits: tests/test_nbest_gpu.py's,
(len - 1) x seq2seq_cases.need(largest |logit|) of the fp64 model's. Scores end to end and against score_captions: the same
rule, scale the largest |logit| the fp64 search met. Maps: tests/att_alpha_cases.BOUND."""
import pytest
import torch

import forced_beam_cases as FC
import forced_beam_ref as R
from att_alpha_cases import BOUND, row_error
from att_alpha_ref import replay
from capnet import ops
from capnet.beam import Constraints
from capnet.train import evaluate
from forced_beam_cases import IMAGES, KS, MARGIN, PENALTIES, START, TABLE_END, TABLE_N, TABLE_START, TABLE_T
from seq2seq_cases import need

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("k,V", FC.TABLE_CASES)
def test_advance_equals_the_model_on_stored_logits(dev, k, V):
    n, T, L = TABLE_N, TABLE_T, TABLE_T + 2
    tab = FC.table(k, V)
    scale = float(tab.abs().max())
    for s, c in FC.TABLE_SETS.items():
        model, gap = FC.model(k, V, s, tab)
        assert gap > FC.TABLE_GAP
        words = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(4)]
        parent = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(2)]
        traced, plain = ops.beam_init(n, k, T, TABLE_START, words[0]), ops.beam_init(n, k, T, TABLE_START, words[2])
        trace = ops.beam_trace(traced)
        trace.fill_(0x7fffffff)
        for step in range(1, T + 1):
            x, y = tab[step - 1].to(dev), tab[step - 1].to(dev)
            ops.beam_advance_traced(traced, trace, x, step, TABLE_END, words[step & 1], parent[0], constraints=c)
            ops.beam_advance(plain, y, step, TABLE_END, words[2 + (step & 1)], parent[1], constraints=c)
            want_words, want_rows, _ = model.outputs[step]
            assert words[step & 1].tolist() == words[2 + (step & 1)].tolist() == want_words, (s, step)
            assert parent[0].tolist() == parent[1].tolist() == want_rows, (s, step)
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
        for penalty in PENALTIES:
            seqs, lengths, scores, counts, rows = ops.beam_nbest_traced(traced, trace, TABLE_END, penalty)
            want = model.nbest(penalty)
            assert counts.tolist() == [len(w) for w in want]
            for i in range(n):
                for r, (q, sc) in enumerate(want[i]):
                    ln = int(lengths[i, r])
                    assert seqs[i, r, :ln].tolist() == q and seqs[i, r, ln:].tolist() == [0] * (L - ln), (s, penalty, i, r)
                    assert abs(float(scores[i, r]) - sc) <= (ln - 1) * need(scale), (s, penalty, i, r)
                    assert not R.missing(q, c.forced), (s, i, q)
            assert rows.tolist() == model.nbest_rows(T, penalty)
        assert counts[0] >= 1 and counts[3] >= 1            # the scripts that must complete do


@pytest.mark.parametrize("k,V", FC.TABLE_CASES)
def test_forced_topk_equals_the_model_on_stored_logits(dev, k, V):
    n, T = TABLE_N, TABLE_T
    tab = FC.table(k, V)
    scale = float(tab.abs().max())
    for s, c in FC.TABLE_SETS.items():
        model, _ = FC.model(k, V, s, tab)
        host = R.ForcedBeam(n, k, V, TABLE_START, TABLE_END, c)
        for step in range(1, T + 1):
            x = tab[step - 1].to(dev)
            competing = [(1 if step == 1 else live) if live else 0 for live in host.live]
            lists, met = [[] for _ in range(n * k)], [0] * (n * k)
            for i in range(n):
                for r, b in enumerate(host.bans(step, i, competing[i])):
                    lists[i * k + r] = [w for w in b if w != TABLE_END or step <= c.min_words]     # (<end> for a missing word: the kernel's)
                met[i * k:i * k + competing[i]] = host.met(i, competing[i])
            cap = max(1, max(len(b) for b in lists))
            bans = torch.tensor([[len(b)] + b + [0] * (cap - len(b)) for b in lists], dtype=torch.int32, device=dev)
            meta = torch.tensor([(i * k, competing[i], host.live[i]) for i in range(n)], dtype=torch.int32, device=dev)
            prev = torch.tensor([v for row in host.scores for v in row], dtype=torch.float32, device=dev)
            met_d = torch.tensor(met, dtype=torch.int32, device=dev)
            scores, flat = ops.beam_topk_batched(x, prev, meta, bans=bans, forced=(c, met_d, TABLE_END))
            if not c.banned and not c.no_repeat_ngram and not c.min_words:      # no list at all: the same
                s2, f2 = ops.beam_topk_batched(tab[step - 1].to(dev), prev, meta, forced=(c, met_d, TABLE_END))
                for i in range(n):
                    assert torch.equal(f2[i, :host.live[i]], flat[i, :host.live[i]]) and torch.equal(s2[i, :host.live[i]], scores[i, :host.live[i]])
            scores, flat = scores.tolist(), flat.tolist()
            host.advance(step, lambda i, nrows, kk: (scores[i][:kk], flat[i][:kk]))
            assert host.outputs[step] == model.outputs[step], (s, step)
        assert host.finish() == model.finish()
        for i in range(n):
            assert [q for _, q in host.completed(i)] == [q for _, q in model.completed(i)]
            for (a, q), (b, _) in zip(host.completed(i), model.completed(i)):
                assert abs(a - b) <= (len(q) - 1) * need(scale), (s, i, a, b)


# ---- 2. every route end to end ---------------------------------------------------------------------------------------
ROUTES = (("host", {}), ("on_device", dict(on_device=True)), ("one_call", dict(one_call=True)))
POLLED = (("on_device poll 2", dict(on_device=True, poll_every=2)), ("one_call poll 2", dict(one_call=True, poll_every=2)))


def _check_nbest(u, s, k, got, penalty, what, images=None):
    """got: per image [(tokens, score)] against the forced fp64 search -> the worst score error over its bound."""
    worst = 0.0
    images = range(IMAGES) if images is None else images
    assert len(got) == len(images), what
    for hyps, i in zip(got, images):
        search = u.search(k, i, s)
        want = search.nbest(penalty)
        assert search.gap(penalty) > MARGIN
        assert [q for q, _ in hyps] == [q for q, _ in want], (u, s, what, k, i, penalty)
        by_tokens = {tuple(q): sc for q, sc in want}
        for q, sc in hyps:
            assert isinstance(sc, float) and not R.missing(q, u.sets[s].forced) and q[-1] == u.end, (u, s, what, q)
            bound = u.score_bound(k, i, s, len(q) - 1)
            assert abs(sc - by_tokens[tuple(q)]) <= bound, (u, s, what, k, i, penalty, sc, by_tokens[tuple(q)], bound)
            worst = max(worst, abs(sc - by_tokens[tuple(q)]) / bound)
    return worst


def _check_scores_are_the_models(u, s, k, dec, feats, kw, got):
    """Every n-best score is decoder.score_captions of its tokens, within the score bound."""
    caps = [q for hyps in got for q, _ in hyps]
    rows = torch.tensor([i for i, hyps in enumerate(got) for _ in hyps], device=feats.device)
    model_scores = dec.score_captions(feats.index_select(0, rows), caps, **kw).tolist()
    at = 0
    for i, hyps in enumerate(got):
        for q, sc in hyps:
            bound = u.score_bound(k, i, s, len(q) - 1)
            assert abs(sc - model_scores[at]) <= bound, (u, s, k, i, q, sc, model_scores[at], bound)
            at += 1


@pytest.mark.parametrize("u", FC.units(), ids=lambda u: u.name)
def test_every_route_returns_the_forced_search(dev, monkeypatch, u):
    family = u.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    worst = 0.0
    for s, c in u.sets.items():
        for k in KS:
            want = [u.winner(k, i, s) for i in range(IMAGES)]
            assert all(u.admitted(k, i, s) for i in range(IMAGES))
            for what, route in ROUTES + POLLED:
                got = dec.sample_batch(feats, START, end, k=k, constraints=c, **route, **kw)
                assert got == want, (u, s, k, what)
            assert all(not R.missing(q, c.forced) for q in got)
            i = k % IMAGES                  # sample() of one image
            for what, route in ROUTES:
                one = dec.sample(feats[i:i + 1], START, end, k=k, constraints=c, **route, **kw)
                assert one.dtype == torch.long and one[0].tolist() == want[i], (u, s, k, i, what)
            # the n-best lists, their scores, and the model's own log-probability of every hypothesis
            for p in PENALTIES:
                for what, route in ROUTES:
                    got = dec.sample_batch(feats, START, end, k=k, nbest=True, length_penalty=p, constraints=c, **route, **kw)
                    worst = max(worst, _check_nbest(u, s, k, got, p, what))
                _check_scores_are_the_models(u, s, k, dec, feats, kw, got)
            # the fallback of one_call: the composed step under the device bookkeeping
            monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
            assert dec.sample_batch(feats, START, end, k=k, constraints=c, one_call=True, **kw) == want, (u, s, k, "composed")
            got = dec.sample_batch(feats, START, end, k=k, nbest=True, length_penalty=1.0, constraints=c, one_call=True, **kw)
            worst = max(worst, _check_nbest(u, s, k, got, 1.0, "composed nbest"))
            monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP")
    # the case the CPU test names: without the forced words the caption is another one, and lacks one
    s, k, i = u.bites()
    for what, route in ROUTES:
        free = dec.sample_batch(feats, START, end, k=k, **route, **kw)[i]
        assert R.missing(free, u.sets[s].forced) and free == u.winner(k, i, None) != u.winner(k, i, s), (u, what)
    print("%s: worst score error %.3f of its bound" % (u.name, worst))


def test_maps_under_forced_words(dev):
    u = [u for u in FC.units() if FC.is_attention(u)][0]
    family = u.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    worst = 0.0
    for s, c in u.sets.items():
        for k in KS:
            want = [u.winner(k, i, s) for i in range(IMAGES)]
            for what, route in ROUTES:
                got, maps = dec.sample_batch(feats, START, end, k=k, return_alphas=True, constraints=c, **route, **kw)
                assert got == want == dec.sample_batch(feats, START, end, k=k, constraints=c, **route, **kw), (u, s, k, what)
                for i in range(IMAGES):
                    ref = replay(family, i, got[i])
                    assert maps[i].dtype == torch.float32 and tuple(maps[i].shape) == tuple(ref.shape), (u, s, k, what, i)
                    worst = max(worst, row_error(maps[i].cpu().double(), ref))
    print("%s: worst map error %.2e of max|alpha| (bound %.2e)" % (u.name, worst, BOUND))
    assert worst < BOUND, worst


def test_evaluate_takes_forced_words(dev):
    u = [u for u in FC.units() if "mode" in u.family.kw][0]
    family = u.family
    dec = family.make().to(dev).eval()
    start, end, V_ = START, family.end, family.V
    s, k, _ = u.bites()
    c = u.sets[s]

    class Vocab:
        word2idx = {"<start>": start, "<end>": end}
        idx2word = {i: ("<end>" if i == end else "<start>" if i == start else "w%d" % i) for i in range(V_)}

    class Enc(torch.nn.Module):
        def forward(self, images):
            return images
    # the references are the forced captions: the forced evaluation scores them 1, the free one does not
    said = [u.winner(k, i, s) for i in range(IMAGES)]
    caps = [[torch.tensor(q), torch.tensor(q[:-2] + [end])] for q in said]
    batches = [(family.features(), None, None, caps)]
    mode = family.kw["mode"]
    forced = evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k, constraints=c)
    assert forced == evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k, one_call=True, constraints=c)
    assert forced == evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k, on_device=True, constraints=c)
    assert forced[0] > 0.99 and forced != evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k)


# ---- 3. forced=() is no forced word ----------------------------------------------------------------------------------
@pytest.mark.parametrize("u", FC.units()[:2] + [u for u in FC.units() if FC.is_attention(u)][:1], ids=lambda u: u.name)
def test_an_empty_forced_field_changes_nothing(dev, u):
    family = u.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    k = KS[1]
    for fields in (dict(), dict(no_repeat_ngram=1, min_words=3, banned=(0,))):
        with_field, without = Constraints(forced=(), **fields), Constraints(**fields)
        for what, route in ROUTES:
            assert dec.sample_batch(feats, START, end, k=k, constraints=with_field, **route, **kw) == \
                dec.sample_batch(feats, START, end, k=k, constraints=without, **route, **kw), (u, what)
            a = dec.sample_batch(feats, START, end, k=k, nbest=True, constraints=with_field, **route, **kw)
            b = dec.sample_batch(feats, START, end, k=k, nbest=True, constraints=without, **route, **kw)
            assert a == b, (u, what)        # tokens and scores, bit for bit
