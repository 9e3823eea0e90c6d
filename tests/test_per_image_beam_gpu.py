"""Per-image constraints in batched beam search on the GPU: capnet_beam_advance_rules (with and without a trace) and
capnet_beam_topk_batched_rules on stored logits against the fixed-slot models of each image's own entry
(tests/per_image_cases.py), then every route of every image decoder under two mixed assignments against
[the fp64 search of image i alone under entries[i]] (tests/test_per_image_beam_cpu.py asserts that all are admitted and that
the assignments tell a wrong row or a leaking rule: nothing is skipped here), the maps, the collapse of uniform sets onto the
calls that existed, and capnet.train.evaluate over a loader.

Tolerances. Tokens, parents, slot order, completion order, trace rows: exact. Scores on stored logits: (len - 1) x
seq2seq_cases.need(largest |logit|) of the fp64 model's. Scores end to end and against score_captions: the same rule, scale the
largest |logit| the fp64 search of that image met. Maps: tests/att_alpha_cases.BOUND. Uniform sets: bit for bit."""
import pytest
import torch

import forced_beam_ref as R
import per_image_cases as PC
from att_alpha_cases import BOUND, row_error
from att_alpha_ref import replay
from capnet import decode, ops
from capnet.beam import Constraints, PerImage
from capnet.train import evaluate
from per_image_cases import IMAGES, KS, MARGIN, PENALTIES, START, TABLE_END, TABLE_N, TABLE_START, TABLE_T
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


@pytest.mark.parametrize("k,V", PC.TABLE_CASES)
def test_advance_gives_every_image_its_own_model_on_stored_logits(dev, k, V):
    n, T, L = TABLE_N, TABLE_T, TABLE_T + 2
    tab = PC.FC.table(k, V)
    scale = float(tab.abs().max())
    for which, names in PC.TABLE_ASSIGNMENTS.items():
        want = PC.Composed(k, V, which)
        assert want.gap > PC.TABLE_GAP
        p = PC.table_per_image(which)
        words = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(4)]
        parent = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(2)]
        traced, plain = ops.beam_init(n, k, T, TABLE_START, words[0]), ops.beam_init(n, k, T, TABLE_START, words[2])
        trace = ops.beam_trace(traced)
        trace.fill_(0x7fffffff)
        for step in range(1, T + 1):
            x, y = tab[step - 1].to(dev), tab[step - 1].to(dev)
            ops.beam_advance_traced(traced, trace, x, step, TABLE_END, words[step & 1], parent[0], constraints=p)
            ops.beam_advance(plain, y, step, TABLE_END, words[2 + (step & 1)], parent[1], constraints=p)
            want_words, want_rows = want.outputs(step)
            assert words[step & 1].tolist() == words[2 + (step & 1)].tolist() == want_words, (which, step)
            assert parent[0].tolist() == parent[1].tolist() == want_rows, (which, step)
        # completion order and scores; the entry without the trace leaves the same state
        n_done, done_score = _done_scores(traced)
        assert _done_scores(plain)[0] == n_done
        assert all(torch.equal(done_score[i, :n_done[i]], _done_scores(plain)[1][i, :n_done[i]]) for i in range(n))
        assert n_done == [len(want.completed(i)) for i in range(n)]
        for i in range(n):
            for j, (sc, q) in enumerate(want.completed(i)):
                assert abs(float(done_score[i, j]) - sc) <= (len(q) - 1) * need(scale), (which, i, j, float(done_score[i, j]), sc)
        # finish and n-best, with the trace rows
        seqs, lengths, rows = ops.beam_finish_traced(traced, trace, TABLE_END)
        assert [seqs[i, :int(lengths[i])].tolist() for i in range(n)] == want.finish()
        assert rows.tolist() == want.winner_rows(T)
        for penalty in PENALTIES:
            seqs, lengths, scores, counts, rows = ops.beam_nbest_traced(traced, trace, TABLE_END, penalty)
            ranked = want.nbest(penalty)
            assert counts.tolist() == [len(w) for w in ranked]
            for i in range(n):
                c = PC.TABLE_ENTRIES[names[i]] or Constraints()
                for r, (q, sc) in enumerate(ranked[i]):
                    ln = int(lengths[i, r])
                    assert seqs[i, r, :ln].tolist() == q and seqs[i, r, ln:].tolist() == [0] * (L - ln), (which, penalty, i, r)
                    assert abs(float(scores[i, r]) - sc) <= (ln - 1) * need(scale), (which, penalty, i, r)
                    assert not R.missing(q, c.forced), (which, i, q)
            assert rows.tolist() == want.nbest_rows(T, penalty)
        assert counts[0] >= 1 and counts[3] >= 1            # the scripts that must complete do


@pytest.mark.parametrize("k,V", PC.TABLE_CASES)
def test_topk_under_the_host_bookkeeping_gives_every_image_its_own_model(dev, k, V):
    n, T = TABLE_N, TABLE_T
    tab = PC.FC.table(k, V)
    scale = float(tab.abs().max())
    for which in PC.TABLE_ASSIGNMENTS:
        want = PC.Composed(k, V, which)
        p = PC.table_per_image(which)
        host = PC.HostBeam(k, V, which)
        for step in range(1, T + 1):
            x = tab[step - 1].to(dev)
            competing = [(1 if step == 1 else live) if live else 0 for live in host.live]
            lists, met = [[] for _ in range(n * k)], [0] * (n * k)
            for i in range(n):
                c = host.entries[i]
                for r, b in enumerate(host.bans(step, i, competing[i])):
                    lists[i * k + r] = [w for w in b if w != TABLE_END or step <= c.min_words]     # (<end> for a missing word: the kernel's)
                met[i * k:i * k + competing[i]] = host.met(i, competing[i])
            cap = max(1, max(len(b) for b in lists))
            bans = torch.tensor([[len(b)] + b + [0] * (cap - len(b)) for b in lists], dtype=torch.int32, device=dev)
            meta = torch.tensor([(i * k, competing[i], host.live[i]) for i in range(n)], dtype=torch.int32, device=dev)
            prev = torch.tensor([v for row in host.scores for v in row], dtype=torch.float32, device=dev)
            met_d = torch.tensor(met, dtype=torch.int32, device=dev)
            scores, flat = ops.beam_topk_batched(x, prev, meta, bans=bans, forced=(p, met_d, TABLE_END))
            scores, flat = scores.tolist(), flat.tolist()
            host.advance(step, lambda i, nrows, kk: (scores[i][:kk], flat[i][:kk]))
            assert host.outputs[step][:2] == want.outputs(step), (which, step)
        assert host.finish() == want.finish()
        for i in range(n):
            assert [q for _, q in host.completed(i)] == [q for _, q in want.completed(i)]
            for (a, q), (b, _) in zip(host.completed(i), want.completed(i)):
                assert abs(a - b) <= (len(q) - 1) * need(scale), (which, i, a, b)


# ---- 2. every route end to end ---------------------------------------------------------------------------------------
ROUTES = (("host", {}), ("on_device", dict(on_device=True)), ("one_call", dict(one_call=True)))
POLLED = (("on_device poll 2", dict(on_device=True, poll_every=2)), ("one_call poll 2", dict(one_call=True, poll_every=2)))


def _check_nbest(fu, cu, image_keys, k, got, penalty, what):
    """got: per image [(tokens, score)] against the fp64 search of that image under its own entry -> the worst score error over
    its bound."""
    worst = 0.0
    assert len(got) == IMAGES, what
    for i, (hyps, key) in enumerate(zip(got, image_keys)):
        search = PC.search(fu, cu, k, i, key)
        want = search.nbest(penalty)
        assert search.gap(penalty) > MARGIN
        assert [q for q, _ in hyps] == [q for q, _ in want], (fu, what, k, i, key, penalty)
        by_tokens = {tuple(q): sc for q, sc in want}
        c = PC.entry(fu, key) or Constraints()
        for q, sc in hyps:
            assert isinstance(sc, float) and not R.missing(q, c.forced) and q[-1] == fu.end, (fu, what, i, key, q)
            bound = PC.score_bound(fu, cu, k, i, key, len(q) - 1)
            assert abs(sc - by_tokens[tuple(q)]) <= bound, (fu, what, k, i, key, penalty, sc, by_tokens[tuple(q)], bound)
            worst = max(worst, abs(sc - by_tokens[tuple(q)]) / bound)
    return worst


def _check_scores_are_the_models(fu, cu, image_keys, k, dec, feats, kw, got):
    """Every n-best score is decoder.score_captions of its tokens, within the score bound."""
    caps = [q for hyps in got for q, _ in hyps]
    rows = torch.tensor([i for i, hyps in enumerate(got) for _ in hyps], device=feats.device)
    model_scores = dec.score_captions(feats.index_select(0, rows), caps, **kw).tolist()
    at = 0
    for i, hyps in enumerate(got):
        for q, sc in hyps:
            bound = PC.score_bound(fu, cu, k, i, image_keys[i], len(q) - 1)
            assert abs(sc - model_scores[at]) <= bound, (fu, k, i, q, sc, model_scores[at], bound)
            at += 1


@pytest.mark.parametrize("fu,cu", PC.units(), ids=lambda u: u.name)
def test_every_route_returns_every_images_own_search(dev, monkeypatch, fu, cu):
    family = fu.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    worst = 0.0
    for which in PC.ASSIGNMENTS:
        image_keys = PC.keys(fu.name, which)
        p = PC.per_image(fu, which)
        for k in KS:
            want = PC.winners(fu, cu, k, image_keys)
            assert all(PC.admitted(fu, cu, k, i, key, pen) for i, key in enumerate(image_keys) for pen in PENALTIES)
            for what, route in ROUTES + POLLED:
                got = dec.sample_batch(feats, START, end, k=k, constraints=p, **route, **kw)
                assert got == want, (fu, which, k, what)
            for i, key in enumerate(image_keys):
                if key is None:           # an image without a rule returns its unconstrained winner
                    assert got[i] == fu.winner(k, i, None)
                elif key[0] == "forced":
                    assert not R.missing(got[i], fu.sets[key[1]].forced)
            # the n-best lists, their scores, and the model's own log-probability of every hypothesis
            for pen in PENALTIES:
                for what, route in ROUTES:
                    got = dec.sample_batch(feats, START, end, k=k, nbest=True, length_penalty=pen, constraints=p, **route, **kw)
                    worst = max(worst, _check_nbest(fu, cu, image_keys, k, got, pen, what))
                _check_scores_are_the_models(fu, cu, image_keys, k, dec, feats, kw, got)
            # the fallback of one_call: the composed step under the device bookkeeping
            monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
            assert dec.sample_batch(feats, START, end, k=k, constraints=p, one_call=True, **kw) == want, (fu, which, k, "composed")
            got = dec.sample_batch(feats, START, end, k=k, nbest=True, length_penalty=1.0, constraints=p, one_call=True, **kw)
            worst = max(worst, _check_nbest(fu, cu, image_keys, k, got, 1.0, "composed nbest"))
            monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP")
    print("%s: worst score error %.3f of its bound" % (fu.name, worst))


def test_maps_under_a_rule_per_image(dev, monkeypatch):
    fu, cu = [(fu, cu) for fu, cu in PC.units() if PC.FC.is_attention(fu)][0]
    family = fu.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    worst = 0.0

    def check(got, maps, what):
        err = 0.0
        for i in range(IMAGES):
            ref = replay(family, i, got[i])
            assert maps[i].dtype == torch.float32 and tuple(maps[i].shape) == tuple(ref.shape), (fu, what, i)
            err = max(err, row_error(maps[i].cpu().double(), ref))
        return err
    for which in PC.ASSIGNMENTS:
        p = PC.per_image(fu, which)
        for k in KS:
            want = PC.winners(fu, cu, k, PC.keys(fu.name, which))
            for what, route in ROUTES:
                got, maps = dec.sample_batch(feats, START, end, k=k, return_alphas=True, constraints=p, **route, **kw)
                assert got == want == dec.sample_batch(feats, START, end, k=k, constraints=p, **route, **kw), (fu, which, k, what)
                worst = max(worst, check(got, maps, (which, k, what)))
            # the one-call search in chunks of two images and one: every chunk takes its own rows of the rule table
            T, P = dec.max_seq_length + 1, maps[0].shape[1]
            calls = []
            inner = ops.att_beam_decode
            with monkeypatch.context() as m:
                m.setattr(ops, "att_beam_decode", lambda *a, **kws: calls.append(kws["constraints"]) or inner(*a, **kws))
                m.setattr(decode, "ALPHA_TRACE_MAX_BYTES", 2 * T * k * P * 4)
                got, maps = dec.sample_batch(feats, START, end, k=k, return_alphas=True, constraints=p, one_call=True, **kw)
            assert [len(c) for c in calls] == [2, 1] and list(calls[0]) == list(p[0:2]) and list(calls[1]) == list(p[2:3])
            assert got == want, (fu, which, k, "chunks")
            worst = max(worst, check(got, maps, (which, k, "chunks")))
    print("%s: worst map error %.2e of max|alpha| (bound %.2e)" % (fu.name, worst, BOUND))
    assert worst < BOUND, worst


# ---- 3. a set that says one thing is that one thing ------------------------------------------------------------------
@pytest.mark.parametrize("fu,cu", PC.units()[:2] + [u for u in PC.units() if PC.FC.is_attention(u[0])][:1], ids=lambda u: u.name)
def test_uniform_sets_run_the_calls_that_were(dev, monkeypatch, fu, cu):
    family = fu.family
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    k = KS[1]
    lib_calls = []
    inner = ops._lib.lib

    class Spy:
        def __getattr__(self, name):
            if name.endswith("_rules"):
                lib_calls.append(name)
            return getattr(inner(), name)
    monkeypatch.setattr(ops._lib, "lib", lambda: Spy())
    for c in (fu.sets["one"], PC.CC.SETS["D"]):
        same = PerImage([Constraints(c.no_repeat_ngram, c.min_words, c.banned, c.forced) for _ in range(IMAGES)])
        for what, route in ROUTES:
            assert dec.sample_batch(feats, START, end, k=k, constraints=same, **route, **kw) == \
                dec.sample_batch(feats, START, end, k=k, constraints=c, **route, **kw), (fu, what)
            a = dec.sample_batch(feats, START, end, k=k, nbest=True, constraints=same, **route, **kw)
            b = dec.sample_batch(feats, START, end, k=k, nbest=True, constraints=c, **route, **kw)
            assert a == b, (fu, what)        # tokens and scores, bit for bit
    for nothing in (PerImage([None] * IMAGES), PerImage([Constraints()] * IMAGES), PerImage([None, Constraints(), None])):
        for what, route in ROUTES:
            assert dec.sample_batch(feats, START, end, k=k, constraints=nothing, **route, **kw) == \
                dec.sample_batch(feats, START, end, k=k, **route, **kw), (fu, what)
            a = dec.sample_batch(feats, START, end, k=k, nbest=True, constraints=nothing, **route, **kw)
            b = dec.sample_batch(feats, START, end, k=k, nbest=True, **route, **kw)
            assert a == b, (fu, what)
    assert lib_calls == []                   # none of it took a per-image entry
    dec.sample_batch(feats, START, end, k=k, constraints=PC.per_image(fu, "A"), on_device=True, **kw)
    assert lib_calls and set(lib_calls) == {"capnet_beam_advance_rules"}       # ... which a mixed set does


# ---- 4. evaluate -----------------------------------------------------------------------------------------------------
def test_evaluate_takes_a_rule_per_image_over_the_loader(dev):
    fu, cu = [u for u in PC.units() if "mode" in u[0].family.kw][0]
    family = fu.family
    dec = family.make().to(dev).eval()
    start, end, V_ = START, family.end, family.V
    k = PC.telling_k(fu, cu)
    image_keys = PC.keys(fu.name, "A")
    p = PC.per_image(fu, "A")

    class Vocab:
        word2idx = {"<start>": start, "<end>": end}
        idx2word = {i: ("<end>" if i == end else "<start>" if i == start else "w%d" % i) for i in range(V_)}

    class Enc(torch.nn.Module):
        def forward(self, images):
            return images
    # the references are each image's caption under its own entry: the per-image evaluation scores them 1, no other does.
    # Two loader batches, of two images and of one: each takes its slice of the entries
    said = PC.winners(fu, cu, k, image_keys)
    caps = [[torch.tensor(q), torch.tensor(q[:-2] + [end])] for q in said]
    feats = family.features()
    batches = [(feats[0:2], None, None, caps[0:2]), (feats[2:3], None, None, caps[2:3])]
    mode = family.kw["mode"]
    mixed = evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k, constraints=p)
    assert mixed == evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k, one_call=True, constraints=p)
    assert mixed == evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k, on_device=True, constraints=p)
    assert mixed[0] > 0.99 and mixed != evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k)
    for key in image_keys:
        if key is not None:
            assert mixed != evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k, constraints=PC.entry(fu, key))
    with pytest.raises(ops.CapnetError, match="PerImage"):
        evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k, constraints=p[0:2])          # one entry short: at the second batch
    with pytest.raises(ops.CapnetError, match="PerImage"):
        evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=k, constraints=PerImage(list(p) + [None]))   # one too many: at the end
