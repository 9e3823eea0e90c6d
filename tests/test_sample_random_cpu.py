"""Sampled decoding without a GPU: the library's exports, the random stream against its Python-integer restatement, the
stream's quality (chi-square on the restatement alone, fixed seed), the Gumbel error bound TOL_G, the margin rule for every
case of tests/sample_random_cases.py (the condition under which tests/test_sample_random_gpu.py compares ids exactly), and
the argument checks that need no device."""
import numpy as np
import pytest
import torch

import capnet
import sample_random_cases as C
import sample_random_ref as R
from capnet import CapnetError, _lib, ops

NEW_SYMBOLS = ("capnet_sample_uniform", "capnet_vocab_sample_ws_bytes", "capnet_vocab_sample", "capnet_sample_pick",
               "capnet_sample_rows", "capnet_sample_decode_ws_bytes", "capnet_sample_decode",
               "capnet_att_sample_decode_ws_bytes", "capnet_att_sample_decode")

# chi-square quantiles at 99.9 %: 36 and 4 degrees of freedom
CHI2_36, CHI2_4 = 67.985, 18.467


def test_library_exports_the_sampling_symbols():
    lib = capnet.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n


def test_sample_uniform_equals_the_restatement_on_a_grid():
    for seed in (0, 1, 2 ** 63 - 1):
        for step in (0, 1, 65535):
            for row in (0, 1, 2 ** 24 - 1):
                for v in (0, 31, 32, 2 ** 24 - 1):
                    u = ops.sample_uniform(seed, step, row, v)
                    assert u == R.sample_uniform(seed, step, row, v), (seed, step, row, v)
                    assert u == float(R.uniform_np(seed, step, row, v))
                    assert 0.0 < u < 1.0
                    n = u * 2 ** 24
                    assert n == int(n) and int(n) % 2 == 1
                    assert float(np.float32(u)) == u


def test_gumbel_error_bound_over_every_stream_value():
    """TOL_G: numpy's fp32 log against fp64 over ALL 2^23 values the stream can take (the extremes included)."""
    worst, lo, hi = 0.0, np.inf, -np.inf
    for b0 in range(0, 1 << 23, 1 << 20):
        b = np.arange(b0, b0 + (1 << 20), dtype=np.float64)
        u = (2.0 * b + 1.0) / 16777216.0
        g64 = R.gumbel(u)
        u32 = u.astype(np.float32)
        assert (u32.astype(np.float64) == u).all()
        g32 = -np.log(-np.log(u32))
        assert g32.dtype == np.float32
        worst = max(worst, float(np.abs(g32.astype(np.float64) - g64).max()))
        lo, hi = min(lo, float(g64.min())), max(hi, float(g64.max()))
    print("gumbel: fp32 error %.3g, range [%.3f, %.3f]" % (worst, lo, hi))
    assert np.isfinite(lo) and np.isfinite(hi) and hi <= 16.7 and lo >= -2.9
    assert worst <= R.TOL_G


def _chi2(counts, probs):
    exp = probs * counts.sum()
    return float(((counts - exp) ** 2 / exp).sum())


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_stream_quality_chi_square(T):
    """16 rows x 2048 steps of draws at V = 37 against softmax(z / T); top_k = 5 against the renormalised top five."""
    V, rows, steps, seed = 37, 16, 2048, 12345
    z = torch.randn(V, generator=torch.Generator().manual_seed(5), dtype=torch.float64).numpy()
    s = z * R.inv_temperature(T)
    step, row, v = np.meshgrid(np.arange(steps), np.arange(rows), np.arange(V), indexing="ij")
    keys = s[None, None, :] + R.gumbel(R.uniform_np(seed, step, row, v))
    p = np.exp(s - s.max())
    p /= p.sum()
    tokens = keys.argmax(2)
    stat = _chi2(np.bincount(tokens.reshape(-1), minlength=V).astype(np.float64), p)
    top = np.argsort(-z)[:5]
    p5 = p[top] / p[top].sum()
    tok5 = keys[:, :, top].argmax(2)
    stat5 = _chi2(np.bincount(tok5.reshape(-1), minlength=5).astype(np.float64), p5)
    print("T %.1f: chi2 %.1f (36 dof), top-5 %.1f (4 dof), smallest expected count %.1f" % (T, stat, stat5, p.min() * rows * steps))
    assert stat < CHI2_36 and stat5 < CHI2_4
    # different rows and different steps draw differently
    assert (tokens[:, 0] != tokens[:, 1]).any() and (tokens[0] != tokens[1]).any()
    assert len({tuple(tokens[:, r]) for r in range(rows)}) == rows
    # the vectorised draw is draw()'s
    d = R.draw(np.tile(z, (rows, 1)), R.inv_temperature(T), seed, 7, 0, 0)
    assert (d["tokens"] == tokens[7]).all()
    d5 = R.draw(np.tile(z, (rows, 1)), R.inv_temperature(T), seed, 7, 0, 5)
    assert (d5["tokens"] == top[tok5[7]]).all()


def test_draw_never_picks_nan_or_minus_inf():
    z = np.array([[0.5, np.nan, -np.inf, 0.25], [np.nan, -np.inf, -np.inf, np.nan]])
    for seed in range(50):
        d = R.draw(z, 1.0, seed, 0)
        assert d["tokens"][0] in (0, 3) and np.isfinite(d["logp"][0])
        assert d["tokens"][1] == 0 and d["logp"][1] == -np.inf
    p = np.exp([0.5, 0.25])
    assert abs(np.exp(R.draw(z, 1.0, 0, 0)["logp"][0]) - p[[0, 3].index(R.draw(z, 1.0, 0, 0)["tokens"][0])] / p.sum()) < 1e-12


@pytest.mark.parametrize("name", sorted(C.SEQ2SEQ))
def test_seq2seq_case_clears_the_margin_rule(name):
    c, p, feats, s, (ids, logp, states, tr, enc) = C.seq2seq_reference(name)
    inv_T = R.inv_temperature(s["T"])
    print("%s: key gap %.3g (need %.3g), k-th gap %.3g (need %.3g), max|logit| %.3g, encoder %r"
          % (name, tr.key_gap, R.need(tr.scale, inv_T), tr.kth_gap, R.need_kth(tr.scale), tr.scale, enc))
    assert ids.shape == (c["rows"], c["steps"]) and np.isfinite(logp).all() and (logp <= 0).all()
    assert tr.key_gap > R.need(tr.scale, inv_T)
    if s["top_k"]:
        assert tr.kth_gap > R.need_kth(tr.scale)
    if enc is not None:                      # the encoder's greedy pass of an emotion mode: seq2seq_cases' rule
        assert enc[0] > C.SC.need(enc[1])


@pytest.mark.parametrize("case", C.IMAGE_CASES, ids=[c["id"] for c in C.IMAGE_CASES])
def test_image_case_clears_the_margin_rule(case):
    ids, logp, tr = C.image_reference(case)
    inv_T = R.inv_temperature(case["T"])
    print("%s: key gap %.3g (need %.3g), k-th gap %.3g (need %.3g), max|logit| %.3g"
          % (case["id"], tr.key_gap, R.need(tr.scale, inv_T), tr.kth_gap, R.need_kth(tr.scale), tr.scale))
    assert ids.shape == (C.IMAGES * C.SAMPLES, C.MAX_LEN) and np.isfinite(logp).all()
    assert tr.key_gap > R.need(tr.scale, inv_T)
    if case["top_k"]:
        assert tr.kth_gap > R.need_kth(tr.scale)
    # the samples of an image are not all equal, and the early end token of the truncation test cuts row 0
    assert any(len({tuple(ids[i * C.SAMPLES + j]) for j in range(C.SAMPLES)}) > 1 for i in range(C.IMAGES))
    cut = R.cut(ids, logp, C.IMAGES, C.SAMPLES, C.START, C.early_end(ids))
    assert len(cut[0][0][0]) <= 5 and cut[0][0][0][-1] == C.early_end(ids)


def test_argument_checks_need_no_device():
    lib = capnet.lib()
    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.capnet_sample_rows(None, 1, 8, 8, T, 0, 0, 0, None, None, None) != 0
        assert b"temperature" in lib.capnet_last_error()
        with pytest.raises(CapnetError):
            ops.check_sampling("t", T, 0, 0)
    for k in (-1, 17, 1.5, True):
        with pytest.raises(CapnetError):
            ops.check_sampling("t", 1.0, k, 0)
    with pytest.raises(CapnetError):
        ops.check_sampling("t", 1.0, 5, 0, V=4)
    for seed in (-1, 1 << 64, 1.0):
        with pytest.raises(CapnetError):
            ops.check_sampling("t", 1.0, 0, seed)
    assert ops.check_sampling("t", 2, 16, 2 ** 64 - 1) == (2.0, 16, 2 ** 64 - 1)
    # top_k outside 0 .. 16, steps and the stream's fields, before any device work
    assert lib.capnet_sample_decode_ws_bytes(1, 4, 64, 37, 17) == 0 and lib.capnet_sample_decode_ws_bytes(1, 4, 64, 37, -1) == 0
    assert lib.capnet_sample_decode_ws_bytes(1, 4, 64, 37, 0) > 0 and lib.capnet_sample_decode_ws_bytes(1, 4, 64, 37, 5) > 0
    assert lib.capnet_sample_pick(None, None, 1, 17, 37, 1.0, 0, 0, 0, None, None, None) != 0
    assert lib.capnet_vocab_sample(None, None, None, 1, 64, 37, 1.0, 0, 65536, 0, None, None, None, None) != 0
    assert b"step" in lib.capnet_last_error()
    assert lib.capnet_vocab_sample(None, None, None, 1, 100, 37, 1.0, 0, 0, 0, None, None, None, None) != 0
    with pytest.raises(CapnetError):
        ops.sample_uniform(0, 65536, 0, 0)
    with pytest.raises(CapnetError):
        ops.sample_uniform(0, 0, 1 << 24, 0)
    # CPU tensors are refused, as everywhere
    with pytest.raises(CapnetError):
        ops.sample_rows(torch.zeros(2, 8))
    with pytest.raises(CapnetError):
        ops.vocab_sample(torch.zeros(2, 64), torch.zeros(8, 64))
    with pytest.raises(CapnetError):
        ops.sample_pick(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32), 8)


def test_seed_none_draws_from_torchs_generator():
    torch.manual_seed(11)
    a = ops.check_sampling("t", 1.0, 0, None)[2]
    b = ops.check_sampling("t", 1.0, 0, None)[2]
    torch.manual_seed(11)
    assert ops.check_sampling("t", 1.0, 0, None)[2] == a and a != b and 0 <= a < 1 << 63
