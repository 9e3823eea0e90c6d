"""sample_random(greedy=True) on the GPU: the greedy caption as one more row of the sampled decode, against the fp64
restatement (tests/greedy_row_ref.py) on all three routes -- the one C call, the composed loop (CAPNET_NO_FUSED_SAMPLE=1) and
the unfolded step (CAPNET_NO_FUSED_DECODE_STEP=1).

Ids are compared exactly and nothing is skipped: tests/test_greedy_row_cpu.py asserts the margin rule for every case of
tests/greedy_row_cases.py. logp: within sample_random_ref.logp_tol per word. The self-checks need no restatement: with one
candidate left (top_k = 1, or a nucleus of top_p = 1e-6) every drawn caption IS the greedy caption and every logp exactly 0
-- which fails if a greedy row gets noise or the layout of the rows is wrong."""
import pytest
import torch

import greedy_row_cases as GC
import sample_random_ref as R
import test_sample_random_gpu as TS
from capnet import CapnetError, decode, ops
from capnet.decode import FUSED_DECODE_OFF, FUSED_SAMPLE_OFF

pytestmark = pytest.mark.gpu

START = GC.START
ROUTES = (("one_call", None), ("no_fused_sample", FUSED_SAMPLE_OFF), ("no_fused_step", FUSED_DECODE_OFF))
LIMITS = ("FUSED_SAMPLE_MAX_ROWS", "FUSED_ATT_SAMPLE_MAX_ROWS", "FUSED_NUCLEUS_MAX_ROWS", "FUSED_NUCLEUS_TOPK_MAX_ROWS",
          "FUSED_ATT_NUCLEUS_MAX_ROWS")


def _routes(monkeypatch, run):
    """{route: run()} with the one call taken at every row count of the cases on the default route; the number of one-call
    decodes of every route rides along as run()'s result [1]."""
    for name in LIMITS:
        monkeypatch.setattr(decode, name, 64)
    calls = TS._count_calls(monkeypatch, "sample_decode", "att_sample_decode")
    out = {}
    for name, env in ROUTES:
        monkeypatch.delenv(FUSED_SAMPLE_OFF, raising=False)
        monkeypatch.delenv(FUSED_DECODE_OFF, raising=False)
        if env:
            monkeypatch.setenv(env, "1")
        before = calls[0]
        out[name] = (run(), calls[0] - before)
    monkeypatch.delenv(FUSED_SAMPLE_OFF, raising=False)
    monkeypatch.delenv(FUSED_DECODE_OFF, raising=False)
    return out


def _setup(case, dev):
    fam = GC.families()[case["family"]]
    return fam, GC.make(fam, dev), fam.features()[:case["n"]].to(dev)


@pytest.mark.parametrize("case", GC.live_cases(), ids=[c["id"] for c in GC.live_cases()])
def test_greedy_row_matches_restatement_on_every_route(dev, monkeypatch, case):
    ids_r, logp_r, tr = GC.reference(case)
    fam, dec, f = _setup(case, dev)
    n, m = case["n"], case["m"]
    tol = R.logp_tol(tr.scale, R.inv_temperature(case["T"]))
    kw = dict(samples=m, temperature=case["T"], top_k=case["top_k"], top_p=case["top_p"], seed=GC.SEEDS[case["id"]], **fam.kw)
    no_end = fam.V                                           # never drawn: all STEPS words
    want = R.cut(ids_r, logp_r, n, m + 1, START, no_end)
    runs = _routes(monkeypatch, lambda: (dec.sample_random(f, START, no_end, greedy=True, **kw), dec.sample_random(f, START, no_end, **kw)))
    for route, ((got, plain), one_calls) in runs.items():
        assert one_calls == (2 if route == "one_call" else 0), (route, one_calls)
        assert len(got) == n and all(len(img) == m + 1 for img in got) and all(len(img) == m for img in plain), route
        assert all(len(q) == GC.STEPS + 1 for img in got for q, _ in img), route
        TS._same_lists(got, want, tol)
        # the first m pairs are those of the call without the keyword, the same route, the same seed
        assert [img[:m] for img in got] == plain, route
    # cut after the first <end> like the others; and the raw rows of the device form are the lists' rows
    end = GC.end_token(case)
    lists, ids, logp = dec.sample_random(f, START, end, greedy=True, device=True, **kw)
    TS._same_lists(lists, R.cut(ids_r, logp_r, n, m + 1, START, end), tol)
    assert lists[0][m][0][-1] == end and len(lists[0][m][0]) <= 5
    assert ids.is_cuda and ids.dtype == torch.int64 and tuple(ids.shape) == (n * (m + 1), GC.STEPS) and tuple(logp.shape) == tuple(ids.shape)
    assert ids.cpu().tolist() == ids_r.tolist()
    ops.check_device_errors()


@pytest.mark.parametrize("case", GC.live_cases(), ids=[c["id"] for c in GC.live_cases()])
def test_greedy_caption_is_the_width_one_beam(dev, case):
    """Wherever the restated greedy caption reaches <end> within STEPS words it is sample_batch(k=1)'s caption."""
    ids_r, _, _ = GC.reference(case)
    fam, dec, f = _setup(case, dev)
    end, m = GC.end_token(case), case["m"]
    got = dec.sample_random(f, START, end, samples=m, greedy=True, temperature=case["T"], top_k=case["top_k"], top_p=case["top_p"],
                            seed=GC.SEEDS[case["id"]], **fam.kw)
    beam = dec.sample_batch(f, START, end, k=1, **fam.kw)
    compared = 0
    for i, row in enumerate(GC.greedy_rows(case)):
        if end in ids_r[row].tolist():
            assert got[i][m][0] == [int(w) for w in beam[i]], i
            compared += 1
    assert compared >= 1                                     # image 0, by the choice of the end token
    ops.check_device_errors()


@pytest.mark.parametrize("family", GC.FAMILIES)
@pytest.mark.parametrize("n,m", GC.SHAPES)
def test_one_candidate_makes_every_row_the_greedy_row(dev, monkeypatch, family, n, m):
    fam = GC.families()[family]
    dec, f = GC.make(fam, dev), fam.features()[:n].to(dev)
    for opts in (dict(top_k=1), dict(top_k=1, top_p=0.9), dict(top_p=1e-6)):
        kw = dict(samples=m, greedy=True, temperature=0.7, seed=5, **opts, **fam.kw)
        runs = _routes(monkeypatch, lambda: dec.sample_random(f, START, fam.V, **kw))
        for route, (got, _) in runs.items():
            for img in got:
                assert len(img) == m + 1
                for q, lp in img:
                    assert q == img[m][0] and lp == 0.0, (route, opts, q, img[m][0], lp)
        # the greedy caption does not depend on the temperature or the truncation
        other = dec.sample_random(f, START, fam.V, samples=m, greedy=True, temperature=1.3, seed=8, **fam.kw)
        assert [img[m][0] for img in other] == [img[m][0] for img in runs["one_call"][0]]
    ops.check_device_errors()


@pytest.mark.parametrize("family", [f for f in GC.FAMILIES if "Att" in f])
def test_sixteen_samples_and_a_greedy_row_raise_on_attention(dev, family):
    fam = GC.families()[family]
    dec, f = GC.make(fam, dev), fam.features()[:1].to(dev)
    with pytest.raises(CapnetError, match="16 rows per image"):
        dec.sample_random(f, START, fam.V, samples=16, greedy=True, seed=0, **fam.kw)
    assert len(dec.sample_random(f, START, fam.V, samples=16, seed=0, **fam.kw)[0]) == 16      # without it: as before
    ops.check_device_errors()


# ---- the stand-alone draws ------------------------------------------------------------------------------------------------------
def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_stride_zero_is_the_call_without_the_argument_and_a_stride_lays_the_rows_out(dev):
    V, rows, g = 257, 7, 3
    z = (torch.randn(rows, V, generator=torch.Generator().manual_seed(3)) * 2.5).to(dev)
    values, index = torch.topk(z, 5, dim=1)
    values, index = values.contiguous(), index.int().contiguous()
    h, W, b, _ = TS._kernel_inputs(64, 37)
    hd, Wd, bd = h[:rows].to(dev), W.to(dev), b.to(dev)
    drawn = [r for r in range(rows) if r % g != g - 1]       # physical rows 0 1 3 4 6 on noise rows 0 .. 4
    greedy = [r for r in range(rows) if r % g == g - 1]
    kw = dict(temperature=0.7, seed=11, step=2)
    calls = (("sample_rows", lambda x, **k: ops.sample_rows(x, **kw, **k), z, lambda r: z[r]),
             ("nucleus_rows", lambda x, **k: ops.nucleus_rows(x, top_p=0.9, **kw, **k), z, lambda r: z[r]),
             ("sample_pick", lambda x, **k: ops.sample_pick(x[0], x[1], V, **kw, **k), (values, index), lambda r: (values[r].contiguous(), index[r].contiguous())),
             ("nucleus_pick", lambda x, **k: ops.nucleus_pick(x[0], x[1], V, top_p=0.9, **kw, **k), (values, index),
              lambda r: (values[r].contiguous(), index[r].contiguous())),
             ("vocab_sample", lambda x, **k: ops.vocab_sample(x, Wd, bd, **kw, **k), hd, lambda r: hd[r].contiguous()))
    for name, call, x, take in calls:
        assert _same(call(x, greedy_stride=0), call(x)), name
        tok, lp = call(x, greedy_stride=g)
        t0, l0 = call(take(drawn))                            # the same rows without greedy rows among them
        assert torch.equal(tok[drawn], t0) and torch.equal(lp[drawn], l0), name
        best = ops.linear(hd, Wd, bd).argmax(1) if name == "vocab_sample" else z.argmax(1)
        assert torch.equal(tok[greedy], best[greedy]), name
        # row0 shifts the physical rows: the last two rows alone, from physical row 5 on
        t5, l5 = call(take([5, 6]), greedy_stride=g, row0=5)
        assert torch.equal(t5, tok[5:]) and torch.equal(l5, lp[5:]), name
    for bad in (-1, 1.5, True):
        with pytest.raises(CapnetError, match="greedy_stride"):
            ops.sample_rows(z, greedy_stride=bad)
    ops.check_device_errors()
