"""Nucleus (top-p) sampling without a GPU: the library's exports, the restatement's nucleus against the textbook
formulation, the margin rule for every case of tests/nucleus_cases.py (the condition under which tests/test_nucleus_gpu.py
compares ids exactly) together with the measurement behind nucleus_ref.SUM_ERR, the argument checks, and top_p = 1.0 as
the unchanged path."""
import numpy as np
import pytest
import torch

import capnet
import nucleus_cases as C
import nucleus_ref as N
import sample_random_ref as R
from capnet import CapnetError, _lib, decode, ops

NEW_SYMBOLS = ("capnet_nucleus_rows", "capnet_nucleus_pick", "capnet_sample_decode_nucleus_ws_bytes",
               "capnet_sample_decode_nucleus", "capnet_att_sample_decode_nucleus_ws_bytes", "capnet_att_sample_decode_nucleus")


def test_library_exports_the_nucleus_symbols():
    lib = capnet.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n


def test_nucleus_equals_sort_cumsum_keep_on_rows_with_ties():
    """{ v : before(v) < p } straight from the definition against "sort descending (stable), cumulative sum, keep while the
    sum before the entry is < p", and against the restatement's own nucleus(), on random rows with tie groups."""
    g = np.random.default_rng(5)
    for trial in range(60):
        V = int(g.integers(1, 120))
        s = np.round(g.normal(size=V) * 2, 1 if trial % 2 else 3)           # one decimal: many equal logits
        idx = np.arange(V)
        for top_p in (N.top_p32(0.5), N.top_p32(0.9), 1e-6, N.top_p32(0.3)):
            want = N.nucleus_by_definition(s, idx, top_p)
            order = np.argsort(-s, kind="stable")                            # ties keep their index order
            p = np.exp(s[order] - s.max())
            p /= p.sum()
            before, kept = 0.0, []
            for j, v in enumerate(order):
                if not before < top_p:
                    break
                kept.append(int(v))
                before += p[j]
            o, n, _ = N.nucleus(s, idx, top_p)
            assert set(kept) == want == set(int(v) for v in idx[o[:n]]), (trial, top_p)
            assert int(np.lexsort((idx, -s))[0]) in want                     # the best entry always stays
    # a shuffled vocabulary: the set depends on (s, index), not on the order in memory
    s = np.array([0.5, 0.5, 0.5, 0.5, 2.0, 0.5])
    perm = np.array([3, 5, 0, 4, 1, 2])
    assert N.nucleus_by_definition(s, np.arange(6), 0.7) == N.nucleus_by_definition(s[perm], perm, 0.7)


def test_draw_with_top_p_on_hand_built_rows():
    z = np.log(np.array([[0.5, 0.2, 0.2, 0.1], [0.1, 0.2, 0.2, 0.5]]))
    seen = [set(), set()]
    for step in range(60):
        d = N.draw(z, 1.0, 3, step, 0, 0, 0.6)
        assert d["size"].tolist() == [2, 2]                                  # 0.5 < 0.6, then 0.7: the tie goes to the lower index
        seen[0].add(int(d["tokens"][0]))
        seen[1].add(int(d["tokens"][1]))
        assert np.allclose(np.exp(d["logp"]), np.where(np.isin(d["tokens"], (0, 3)), 0.5 / 0.7, 0.2 / 0.7))
        assert np.allclose(d["below"], 0.1) and np.allclose(d["above"], 0.1) and np.allclose(d["edge_gap"], 0.0)
    assert seen == [{0, 1}, {3, 1}]
    d = N.draw(z, 1.0, 3, 0, 0, 3, 0.6)                                      # top_k first: renormalised over the three best
    assert d["size"].tolist() == [2, 2] and np.allclose(d["above"], 0.7 / 0.9 - 0.6)
    d = N.draw(np.array([[np.nan, -np.inf]]), 1.0, 3, 0, 0, 0, 0.6)
    assert d["tokens"][0] == 0 and d["logp"][0] == -np.inf and d["size"][0] == 0
    # top_p = 1.0 in the restatement keeps every entry with any mass before it: sample_random_ref's draw
    zz = torch.randn(3, 50, generator=torch.Generator().manual_seed(2), dtype=torch.float64).numpy()
    a, b = N.draw(zz, 0.7, 5, 2, 0, 0, 1.0), R.draw(zz, 0.7, 5, 2, 0, 0)
    assert (a["tokens"] == b["tokens"]).all() and np.allclose(a["logp"], b["logp"])


def test_kernel_sum32_is_the_kernels_order():
    e = np.random.default_rng(1).random(1000).astype(np.float32)
    got = N.kernel_sum32(e)
    assert got.dtype == np.float32 and abs(float(got) - float(e.astype(np.float64).sum())) < 1e-3
    # thread 0's entries are added first to last; a lone entry anywhere is returned exactly
    one = np.zeros(777, dtype=np.float32)
    one[600] = 0.3
    assert N.kernel_sum32(one) == np.float32(0.3)
    # monotone: zeroing entries never raises the sum
    mask = np.random.default_rng(2).random(1000) < 0.5
    assert N.kernel_sum32(np.where(mask, e, 0)) <= got


def _worst_mass_error(case_T, top_k, top_p):
    worst = [0.0]
    inv_T, p32 = R.inv_temperature(case_T), N.top_p32(top_p)

    def on_logits(t, logits):
        for row in logits.double().numpy():
            worst[0] = max(worst[0], N.kernel_mass_error(row, inv_T, p32, top_k))
    return worst, on_logits


def _assert_clears(name, tr, T, top_k, worst):
    inv_T = R.inv_temperature(T)
    print("%s: nucleus %s..%s, key gap %.3g (need %.3g), edge gap %.3g (need %.3g), mass ratio %.3g (need %.3g), below %.3g, "
          "above %.3g, k-th gap %.3g, max|logit| %.3g, fp32 mass error %.3g"
          % (name, tr.min_size, tr.max_size, tr.key_gap, R.need(tr.scale, inv_T), tr.edge_gap, R.need_kth(tr.scale) * inv_T,
             tr.mass_ratio, 4 * R.TOL_STEP * tr.scale * inv_T, tr.below, tr.above, tr.kth_gap, tr.scale, worst))
    assert N.clears(tr, inv_T, top_k) == []
    assert 2 * worst <= N.SUM_ERR                    # the measurement behind SUM_ERR, on this case's own rows


@pytest.mark.parametrize("name", sorted(C.SEQ2SEQ))
def test_seq2seq_case_clears_the_margin_rule(name):
    s = C.SEQ2SEQ[name]
    worst, on_logits = _worst_mass_error(s["T"], s["top_k"], s["top_p"])
    c, p, feats, s, (ids, logp, states, tr, enc) = C.seq2seq_reference(name, on_logits=on_logits)
    assert ids.shape == (c["rows"], c["steps"]) and np.isfinite(logp).all() and (logp <= 0).all()
    _assert_clears(name, tr, s["T"], s["top_k"], worst[0])
    if enc is not None:
        assert enc[0] > C.SC.SC.need(enc[1])


@pytest.mark.parametrize("case", C.IMAGE_CASES, ids=[c["id"] for c in C.IMAGE_CASES])
def test_image_case_clears_the_margin_rule(case):
    worst, on_logits = _worst_mass_error(case["T"], case["top_k"], case["top_p"])
    ids, logp, tr = C.image_reference(case, on_logits=on_logits)
    assert ids.shape == (C.IMAGES * C.SAMPLES, C.MAX_LEN) and np.isfinite(logp).all() and (logp <= 0).all()
    _assert_clears(case["id"], tr, case["T"], case["top_k"], worst[0])
    assert 1 <= tr.min_size <= tr.max_size <= (case["top_k"] or 97)


def test_the_cases_cover_the_values():
    combos = {(c["top_k"], c["top_p"]) for c in C.IMAGE_CASES}
    assert combos == {(0, 0.5), (0, 0.9), (5, 0.5), (5, 0.9)}
    assert {c["T"] for c in C.IMAGE_CASES} == {0.5, 1.0, 2.0}
    assert {c["family"] for c in C.IMAGE_CASES} == {c["family"] for c in C.SC.IMAGE_CASES}


def test_check_sampling_rejects_bad_top_p():
    for bad in (0, 0.0, -0.5, 1.0000001, 2, float("nan"), float("inf"), 1e-60, True, "x", None):
        with pytest.raises(CapnetError):
            ops.check_top_p("t", bad)
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(CapnetError):
            ops.check_sampling("t", 1.0, 0, 0, top_p=bad)
    assert ops.check_sampling("t", 1.0, 5, 7, top_p=0.9) == (1.0, 5, 7, float(np.float32(0.9)))
    assert ops.check_sampling("t", 1.0, 5, 7, top_p=1) == (1.0, 5, 7, 1.0)
    assert ops.check_sampling("t", 1.0, 5, 7) == (1.0, 5, 7)                 # without top_p: the triple it always returned
    assert ops.check_top_p("t", 1.0 - 1e-9) == 1.0                           # rounds to 1.0 in fp32: off
    lib = capnet.lib()
    for bad in (0.0, -0.5, 1.5, float("nan")):
        assert lib.capnet_nucleus_rows(None, 1, 8, 8, 1.0, bad, 0, 0, 0, None, None, None) != 0
        assert b"top_p" in lib.capnet_last_error()
        assert lib.capnet_nucleus_pick(None, None, 1, 5, 8, 1.0, bad, 0, 0, 0, None, None, None) != 0
        assert b"top_p" in lib.capnet_last_error()
    # the loops leave top_p = 1 to the plain entries
    assert lib.capnet_sample_decode_nucleus(1, 1, 1, 64, 64, 37, 4, None, None, None, None, None, None, None, None, 1.0, 0, 1.0, 0,
                                            None, None, 0, None, None, None, None, None) != 0
    assert b"top_p" in lib.capnet_last_error()
    assert lib.capnet_sample_decode_nucleus_ws_bytes(1, 4, 64, 37, 17) == 0 and lib.capnet_sample_decode_nucleus_ws_bytes(0, 4, 64, 37, 0) == 0
    assert lib.capnet_sample_decode_nucleus_ws_bytes(1, 4, 64, 37, 0) >= lib.capnet_sample_decode_ws_bytes(1, 4, 64, 37, 0) - 4096
    assert lib.capnet_sample_decode_nucleus_ws_bytes(1, 4, 64, 37, 5) == lib.capnet_sample_decode_ws_bytes(1, 4, 64, 37, 5)
    assert lib.capnet_att_sample_decode_nucleus_ws_bytes(1, 2, 3, 4, 16, 512, 12, 64, 37, 0) > 0
    assert lib.capnet_att_sample_decode_nucleus_ws_bytes(1, 0, 3, 4, 16, 512, 12, 64, 37, 0) == 0
    with pytest.raises(CapnetError):
        ops.nucleus_rows(torch.zeros(2, 8), top_p=0.5)                       # CPU tensors are refused, as everywhere
    with pytest.raises(CapnetError):
        ops.nucleus_pick(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32), 8, top_p=0.5)


def test_top_p_one_takes_the_unchanged_path(monkeypatch):
    called = []

    def fake(name, result=None):
        def f(*a, **kw):
            called.append((name, kw))
            return result
        monkeypatch.setattr(ops, name, f)
    for name in ("sample_rows", "sample_pick", "nucleus_rows", "nucleus_pick"):
        fake(name, (torch.zeros(2, dtype=torch.int64), torch.zeros(2)))
    logits = torch.randn(2, 9)
    decode.draw_step(logits, 1.0, 0, 3, 0)
    decode.draw_step(logits, 1.0, 0, 3, 0, top_p=1.0)
    decode.draw_step(logits, 1.0, 4, 3, 0, top_p=1.0)
    assert [n for n, _ in called] == ["sample_rows", "sample_rows", "sample_pick"]
    del called[:]
    decode.draw_step(logits, 1.0, 0, 3, 0, top_p=0.9)
    decode.draw_step(logits, 1.0, 4, 3, 0, top_p=0.9)
    assert [n for n, _ in called] == ["nucleus_rows", "nucleus_pick"]
    # the one-call route: ops.sample_decode is called as it was before there was a top_p -- no keyword
    from capnet.seq2seq import Seq2Seq
    m = Seq2Seq(64, 64, 37, 1, dropout=0.0).eval()
    ids = torch.zeros(2, m.encoder.max_seq_length, dtype=torch.int64)
    fake("sample_decode", (ids, ids.float(), torch.zeros(2, 2, 64)))
    feats = torch.zeros(2, 64)
    for kw in ({}, {"top_p": 1.0}, {"top_p": 1}):
        del called[:]
        m.sample_random(feats, 1, seed=0, **kw)
        assert len(called) == 1 and called[0][0] == "sample_decode" and "top_p" not in called[0][1], kw
    del called[:]
    m.sample_random(feats, 1, seed=0, top_k=3, top_p=0.5)
    assert called[0][0] == "sample_decode" and called[0][1]["top_p"] == 0.5
    # the thresholds of the nucleus draw are their own
    monkeypatch.setattr(decode, "FUSED_NUCLEUS_MAX_ROWS", 1)
    monkeypatch.setattr(decode, "FUSED_NUCLEUS_TOPK_MAX_ROWS", 2)
    monkeypatch.setattr(decode, "FUSED_SAMPLE_MAX_ROWS", 12)
    assert decode.fused_sample(2) and not decode.fused_sample(2, False, 0.5) and decode.fused_sample(1, False, 0.5)
    assert decode.fused_sample(2, False, 0.5, 5) and not decode.fused_sample(3, False, 0.5, 5) and decode.fused_sample(3, False, 1.0, 5)
    monkeypatch.setattr(decode, "FUSED_ATT_NUCLEUS_MAX_ROWS", 3)
    assert decode.fused_sample(60, True) and not decode.fused_sample(4, True, 0.5) and decode.fused_sample(3, True, 0.5)
