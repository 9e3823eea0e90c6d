"""Attention maps from the one-call beam search on the GPU (return_alphas): the step's maps (capnet_att_decode_step_alphas)
against an fp64 restatement written here, across the context kernel's 256-pixel chunk; the row trace
(capnet_beam_advance_traced / capnet_beam_finish_traced) against the Python model with paths on stored logits; the whole
search of every admitted case of tests/att_alpha_cases.py against the fp64 replay of its tokens; the replay routes against
the trace; sample_styles; chunking under decode.ALPHA_TRACE_MAX_BYTES; workspace reuse.

Tolerances. A step's maps: 3e-5 of max|alpha_ref| of the row, tests/test_att_beam_decode_gpu.py's step TOL (the maps are a
softmax of f32 sums over A in front of nothing else). A search's maps: (MAX_LEN + 1) x 3e-5 of max|alpha_ref| of the row
-- the per-step bound accumulated over the steps replayed, the form tests/seq2seq_beam_cases.py uses for logits: the map
of step e comes from a state that went through e - 1 f32 steps. A row sums to 1 within P x 2^-23 x 4."""
import pytest
import torch

import capnet
from att_alpha_cases import (ALPHA_TOL, BOUND, IMAGES, KS, MAX_LEN, START, TABLE_END, TABLE_KV, TABLE_N, TABLE_START, TABLE_T,
                             admitted, alpha_families, class_of, drive_model, row_error, table)
from att_alpha_ref import replay
from capnet import decode, ops

pytestmark = pytest.mark.gpu

E, H, V, A = 12, 64, 23, 16


@pytest.fixture(autouse=True)
def _no_device_error_left(dev):
    yield
    ops.check_device_errors()


# ---- 8. the step's maps against fp64 ---------------------------------------------------------------------------------
def _parents(n, k):
    """Within-image reversals in which every third row repeats its image's first parent: repeats, and rows nobody reads."""
    out = []
    for i in range(n):
        rev = [i * k + k - 1 - r for r in range(k)]
        out += [rev[0] if r % 3 == 1 else p for r, p in enumerate(rev)]
    return out


def _inputs(cell, n, k, P, Cf, seed, feat=None):
    g = torch.Generator().manual_seed(seed)
    nk, kin = n * k, (E + Cf + 15) // 16 * 16

    def u(*shape, a=1.0):
        return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * a)
    d = dict(cell=cell, k=k)
    d["att1"] = u(n, P, A)
    d["feat"] = torch.rand((n, P, Cf), generator=g, dtype=torch.float64) if feat is None else feat
    d["wz"], d["bz"] = u(A + Cf, H, a=(3.0 / H) ** 0.5), u(A + Cf, a=0.1)
    d["w_full"], d["b_full"] = u(1, A, a=(3.0 / A) ** 0.5 * 4), u(1, a=0.1)
    d["emb"] = u(V, E)
    w = u(4 * H, kin + H, a=(3.0 / (E + Cf / 3 + H)) ** 0.5)
    w[:, E + Cf:kin] = 0
    d["wcat"], d["beff"] = [w], [u(4 * H, a=0.1)]
    d["state"] = u(nk, 2, H)
    d["tokens"] = torch.randint(0, V, (nk,), generator=g)
    d["parent"] = torch.tensor(_parents(n, k), dtype=torch.long)
    return d


def _reference_alpha(d, parent):
    """The maps in fp64: h by parent; att2 = decoder_att(h); scores; softmax over the pixels."""
    k, nk = d["k"], d["state"].shape[0]
    src = torch.arange(nk) if parent is None else parent
    z = d["state"].index_select(0, src)[:, 0] @ d["wz"].t() + d["bz"]
    img = torch.arange(nk) // k
    e = torch.relu(d["att1"][img] + z[:, None, :A]) @ d["w_full"][0] + d["b_full"]
    return torch.softmax(e, 1)


def _to(d, dev):
    f = lambda t: t.to(dev, torch.float32 if t.dtype == torch.float64 else t.dtype).contiguous()   # noqa: E731
    return {key: ([f(t) for t in v] if isinstance(v, list) else f(v) if isinstance(v, torch.Tensor) else v) for key, v in d.items()}


def _run(g, parent, alphas=None, groups=1):
    return ops.att_decode_step(g["att1"], g["feat"], g["k"], g["tokens"], g["emb"], g["wz"], g["bz"], g["w_full"], g["b_full"],
                               g["wcat"], g["beff"], g["state"], cell=g["cell"], parent_rows=parent, groups=groups, alphas=alphas)


def _check_maps(got, want, P):
    got = got.cpu().double()
    err = row_error(got, want)
    off = float((got.sum(1) - 1).abs().max())
    print("maps %.2e of max|alpha|, rows sum to 1 within %.2e" % (err, off))
    assert err < ALPHA_TOL, err
    assert off <= P * 2.0 ** -23 * 4, off


@pytest.mark.parametrize("n, k", [(1, 1), (3, 5), (2, 16)])
@pytest.mark.parametrize("P", [1, 6, 255, 256, 257, 260])
@pytest.mark.parametrize("Cf", [512, 2048], ids=["narrow", "wide"])
def test_step_maps_against_fp64(dev, Cf, P, n, k):
    cell = ops.CELL_LSTM if (n + P) % 2 else ops.CELL_FACTORED
    d = _inputs(cell, n, k, P, Cf, seed=1000 * n + 10 * k + P + Cf)
    g = _to(d, dev)
    for parent in (d["parent"], None):
        gp = None if parent is None else g["parent"]
        top0, out0 = _run(g, gp)
        maps = torch.full((n * k, P), float("nan"), device=dev)
        top, out = _run(g, gp, alphas=maps)
        assert torch.equal(top, top0) and torch.equal(out, out0)          # the store changes no arithmetic
        _check_maps(maps, _reference_alpha(d, parent), P)


@pytest.mark.parametrize("P", [6, 260])
def test_step_maps_of_two_weight_groups(dev, P):
    """Two weight groups on the same two images: each group's maps are its own Attention module's, on the shared map."""
    n, k, Cf, G = 2, 5, 512, 2
    ds = [_inputs(ops.CELL_FACTORED, n, k, P, Cf, seed=77 + P)]
    ds.append(_inputs(ops.CELL_FACTORED, n, k, P, Cf, seed=78 + P, feat=ds[0]["feat"]))
    ds[1]["emb"] = ds[0]["emb"]                                    # (the embedding is shared)
    cat = lambda key: torch.cat([x[key] for x in ds], 0)          # noqa: E731
    stack = lambda key: torch.stack([x[key] for x in ds])           # noqa: E731
    both = dict(cell=ds[0]["cell"], k=k, feat=ds[0]["feat"], emb=ds[0]["emb"], att1=cat("att1"), state=cat("state"),
                tokens=cat("tokens"), wz=stack("wz"), bz=stack("bz"), w_full=cat("w_full"), b_full=cat("b_full"),
                wcat=[torch.stack([x["wcat"][0] for x in ds])], beff=[torch.stack([x["beff"][0] for x in ds])])
    parent = torch.cat([ds[0]["parent"], ds[1]["parent"] + n * k])
    g = _to(both, dev)
    gp = parent.to(dev)
    for p, par in ((gp, parent), (None, None)):
        top0, out0 = _run(g, p, groups=G)
        maps = torch.full((G * n * k, P), float("nan"), device=dev)
        top, out = _run(g, p, alphas=maps, groups=G)
        assert torch.equal(top, top0) and torch.equal(out, out0)
        want = torch.cat([_reference_alpha(x, None if par is None else x["parent"]) for x in ds], 0)
        _check_maps(maps, want, P)
        assert row_error(maps[:n * k].cpu().double(), want[n * k:]) > 100 * ALPHA_TOL       # the groups do differ


# ---- 9. the trace against the model ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k, Vt", TABLE_KV)
def test_trace_equals_the_model_on_stored_logits(dev, k, Vt):
    n, T = TABLE_N, TABLE_T
    tab = table(k, Vt)
    model, _ = drive_model(k, Vt, tab)
    words = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(2)]
    parent = torch.empty(n * k, dtype=torch.long, device=dev)
    plain_words = [torch.empty(n * k, dtype=torch.long, device=dev) for _ in range(2)]
    plain_parent = torch.empty(n * k, dtype=torch.long, device=dev)
    beam = ops.beam_init(n, k, T, TABLE_START, words[0])
    plain = ops.beam_init(n, k, T, TABLE_START, plain_words[0])
    trace = ops.beam_trace(beam)
    trace.fill_(0x7fffffff)                                 # whatever it held: nothing of it is read before it is written
    for step in range(1, T + 1):
        logits = tab[step - 1].to(dev)
        ops.beam_advance_traced(beam, trace, logits, step, TABLE_END, words[step & 1], parent)
        ops.beam_advance(plain, logits, step, TABLE_END, plain_words[step & 1], plain_parent)
        assert torch.equal(words[step & 1], plain_words[step & 1]) and torch.equal(parent, plain_parent), step
        assert torch.equal(beam.live, plain.live) and torch.equal(beam.live_total, plain.live_total), step
        for i, live in enumerate(beam.live.tolist()):
            assert torch.equal(beam.scores[i, :live], plain.scores[i, :live]), (step, i)
    seqs, lengths, rows = ops.beam_finish_traced(beam, trace, TABLE_END)
    seqs0, lengths0, _ = ops.beam_finish(plain, TABLE_END)
    assert torch.equal(seqs, seqs0) and torch.equal(lengths, lengths0)
    got = [row[:ln] for row, ln in zip(seqs.tolist(), lengths.tolist())]
    assert got == model.finish()
    assert rows.dtype == torch.int32 and rows.tolist() == model.winner_rows(T)
    for i, ln in enumerate(lengths.tolist()):
        assert rows[i, ln - 1:].tolist() == [-1] * (T - ln + 1)
    assert rows[1].tolist() == [-1] * T                    # the image that completed nothing


# ---- 10. the whole search against fp64 -------------------------------------------------------------------------------
def _check_caption(family, i, tokens, maps, dev):
    want = replay(family, i, tokens)
    assert maps.dtype == torch.float32 and maps.device.type == "cuda" and tuple(maps.shape) == tuple(want.shape), (maps.shape, want.shape)
    return row_error(maps.cpu().double(), want)


@pytest.mark.parametrize("family", alpha_families(), ids=lambda f: f.name)
def test_search_maps_against_the_fp64_replay(dev, monkeypatch, family):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    ok, worst = admitted(family), 0.0
    for k in KS:
        att = getattr(dec._beam(feats, IMAGES, k, *kw.values(), True)[0], "att", None)
        assert isinstance(att, decode.AttStack)                      # the one call does run: the maps are the trace's
        plain = dec.sample_batch(feats, START, end, k=k, one_call=True, **kw)
        seqs, maps = dec.sample_batch(feats, START, end, k=k, one_call=True, return_alphas=True, **kw)
        assert seqs == plain and len(maps) == IMAGES
        for i in range(IMAGES):
            assert maps[i].shape[0] == len(seqs[i]) - 1
            if (k, i) not in ok:
                continue
            assert seqs[i] == family.reference(k, i), (k, i)
            worst = max(worst, _check_caption(family, i, seqs[i], maps[i], dev))
            if seqs[i] == [end]:
                assert tuple(maps[i].shape) == (0, feats.shape[1])
        i = [i for i in range(IMAGES) if (k, i) in ok][0]
        one0 = dec.sample(feats[i:i + 1], START, end, k=k, one_call=True, **kw)
        one, m1 = dec.sample(feats[i:i + 1], START, end, k=k, one_call=True, return_alphas=True, **kw)
        assert torch.equal(one, one0) and one.cpu().tolist() == [family.reference(k, i)]
        assert m1.shape[0] == one.shape[1] - 1
        worst = max(worst, _check_caption(family, i, one[0].tolist(), m1, dev))
    print("%s: worst map error %.2e of max|alpha| (bound %.2e)" % (family.name, worst, BOUND))
    assert worst < BOUND, worst


# ---- 11. the routes agree --------------------------------------------------------------------------------------------
ROUTE_FAMILIES = ("DecoderFactoredLSTMAtt-P260@34", "StackedFactoredLSTMAtt-2@22", "DecoderRNNAtt@10", "StackedDecoderRNNAtt-2@3")


def _by_name(name):
    return [f for f in alpha_families() if f.name == name][0]


@pytest.mark.parametrize("name", ROUTE_FAMILIES)
def test_the_replay_routes_agree_with_the_trace(dev, monkeypatch, name):
    """One case per class: the host path, on_device=True and CAPNET_NO_FUSED_DECODE_STEP=1 replay the tokens through the
    composed step; the one-call search records. Same tokens, maps within the bound of each other's fp64 reference -- both
    sides are within BOUND of the same replay, so they are compared with it. poll_every changes nothing."""
    family = _by_name(name)
    assert class_of(family) in name
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    dec = family.make().to(dev).eval()
    feats, end, kw, k = family.features().to(dev), family.end, family.kw, 5
    ok = admitted(family)
    seqs, maps = dec.sample_batch(feats, START, end, k=k, one_call=True, return_alphas=True, **kw)
    seqs2, maps2 = dec.sample_batch(feats, START, end, k=k, one_call=True, return_alphas=True, poll_every=2, **kw)
    assert seqs2 == seqs and all(torch.equal(a, b) for a, b in zip(maps, maps2))

    def check(route, got_seqs, got_maps):
        worst = 0.0
        for i in range(IMAGES):
            if (k, i) not in ok:
                continue
            assert got_seqs[i] == seqs[i], (route, i)
            assert got_maps[i].shape == maps[i].shape and got_maps[i].device.type == "cuda"
            worst = max(worst, _check_caption(family, i, got_seqs[i], got_maps[i], dev))
            if maps[i].shape[0]:
                worst = max(worst, row_error(got_maps[i].cpu().double(), maps[i].cpu().double()))
        print("%s %s: %.2e" % (name, route, worst))
        assert worst < BOUND, (route, worst)
    check("host", *dec.sample_batch(feats, START, end, k=k, return_alphas=True, **kw))
    check("on_device", *dec.sample_batch(feats, START, end, k=k, on_device=True, return_alphas=True, **kw))
    i = [i for i in range(IMAGES) if (k, i) in ok][0]
    one, m1 = dec.sample(feats[i:i + 1], START, end, k=k, return_alphas=True, **kw)            # sample(): the host path
    assert one.cpu().tolist() == [seqs[i]] and m1.shape == maps[i].shape
    assert _check_caption(family, i, seqs[i], m1, dev) < BOUND
    monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
    assert getattr(dec._beam(feats, IMAGES, k, *kw.values(), True)[0], "att", None) is None    # no one call: replay
    check("composed", *dec.sample_batch(feats, START, end, k=k, one_call=True, return_alphas=True, **kw))


def test_an_embedding_width_off_four_replays(dev, monkeypatch):
    import nic_stacked_ref
    from capnet.nic_model_att import DecoderRNNAtt
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    dec = DecoderRNNAtt(16, 10, 64, 37, 1, feature_size=512)
    dec.load_state_dict({key: v.float() for key, v in nic_stacked_ref.decode_params(dec, seed=3).items()})
    dec.max_seq_length = MAX_LEN
    dec = dec.to(dev).eval()
    family = _by_name("DecoderRNNAtt@10")
    feats = family.features().to(dev)
    assert getattr(dec._beam(feats, IMAGES, 5, True)[0], "att", None) is None
    seqs, maps = dec.sample_batch(feats, START, family.end, k=5, one_call=True, return_alphas=True)
    assert seqs == dec.sample_batch(feats, START, family.end, k=5, one_call=True)
    host_seqs, host_maps = dec.sample_batch(feats, START, family.end, k=5, return_alphas=True)
    for i in range(IMAGES):
        assert tuple(maps[i].shape) == (len(seqs[i]) - 1, feats.shape[1])
        if maps[i].shape[0]:
            assert float((maps[i].sum(1) - 1).abs().max()) < 1e-5
            if host_seqs[i] == seqs[i]:
                assert row_error(maps[i].cpu().double(), host_maps[i].cpu().double()) < BOUND


# ---- 12. styles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, end", [("DecoderFactoredLSTMAtt-P260@34", 34), ("StackedFactoredLSTMAtt-2@22", 55)])
def test_sample_styles_returns_every_modes_own_maps(dev, monkeypatch, name, end):
    """(The stacked family decodes towards 55 here: at 22 only its factual mode completes anything, and two modes can be
    compared only on an image both have a caption for; at 55, in fp64, each of the three modes completes on two images.)"""
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family = _by_name(name)
    dec = family.make().to(dev).eval()
    feats, k = family.features().to(dev), 3
    modes = ("factual", "happy", "sad")
    plain = dec.sample_styles(feats, START, end, k=k, modes=modes)
    seqs, maps = dec.sample_styles_alphas(feats, START, end, k=k, modes=modes)
    assert seqs == plain and set(maps) == set(modes)
    for m in modes:
        s1, m1 = dec.sample_batch(feats, START, end, k=k, mode=m, one_call=True, return_alphas=True)
        assert seqs[m] == s1
        for i in range(IMAGES):
            assert maps[m][i].shape == m1[i].shape and maps[m][i].shape[0] == len(s1[i]) - 1
            if m1[i].shape[0]:
                assert row_error(maps[m][i].cpu().double(), m1[i].cpu().double()) < BOUND, (m, i)
    # the modes look at different places: the first maps (same initial state, each mode's own Attention module) and on
    far = 0.0
    for a in range(len(modes)):
        for b in range(a + 1, len(modes)):
            for i in range(IMAGES):
                ma, mb = maps[modes[a]][i].cpu().double(), maps[modes[b]][i].cpu().double()
                rows = min(ma.shape[0], mb.shape[0])
                if rows:
                    far = max(far, row_error(ma[:rows], mb[:rows]))
    print("%s: modes differ by %.2e of max|alpha|" % (name, far))
    assert far > 10 * BOUND, far


# ---- 13. chunking ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["DecoderFactoredLSTMAtt-P260@34", "StackedDecoderRNNAtt-2@3"])
def test_a_lower_cap_decodes_in_two_chunks_with_equal_results(dev, monkeypatch, name):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family = _by_name(name)
    dec = family.make().to(dev).eval()
    feats, end, kw, k = family.features().to(dev), family.end, family.kw, 5
    seqs, maps = dec.sample_batch(feats, START, end, k=k, one_call=True, return_alphas=True, **kw)
    calls = []
    real = ops.att_beam_decode
    monkeypatch.setattr(ops, "att_beam_decode", lambda *a, **b: calls.append(a[1].shape[0]) or real(*a, **b))
    monkeypatch.setattr(decode, "ALPHA_TRACE_MAX_BYTES", 2 * (MAX_LEN + 1) * k * feats.shape[1] * 4)
    seqs2, maps2 = dec.sample_batch(feats, START, end, k=k, one_call=True, return_alphas=True, **kw)
    assert calls == [2, 1]
    assert seqs2 == seqs and all(torch.equal(a, b) for a, b in zip(maps, maps2))
    if "Factored" in name:
        calls.clear()
        modes = ("happy", "angry")
        monkeypatch.setattr(decode, "ALPHA_TRACE_MAX_BYTES", 2 * 2 * (MAX_LEN + 1) * k * feats.shape[1] * 4)
        s3, m3 = dec.sample_styles_alphas(feats, START, end, k=k, modes=modes)
        assert calls == [4, 2]
        monkeypatch.setattr(decode, "ALPHA_TRACE_MAX_BYTES", 256 << 20)
        s4, m4 = dec.sample_styles_alphas(feats, START, end, k=k, modes=modes)
        assert s3 == s4 and all(torch.equal(a, b) for m in modes for a, b in zip(m3[m], m4[m]))


# ---- 14. workspace reuse ---------------------------------------------------------------------------------------------
def test_two_calls_on_one_workspace_give_equal_results(dev, monkeypatch):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family = _by_name("StackedFactoredLSTMAtt-2-wide@55")
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    a = dec.sample_batch(feats, START, end, k=5, one_call=True, return_alphas=True, **kw)
    other = dec.sample_batch(feats.flip(0).contiguous(), START, end, k=5, one_call=True, return_alphas=True, **kw)   # same shape: same workspace

    def alpha_workspaces():         # the unified cache's entries of this size function
        return [key for key in ops._search_ws if key[0] == "capnet_att_beam_decode_alphas_ws_bytes"]
    assert len(alpha_workspaces()) >= 1
    n_ws = len(alpha_workspaces())
    b = dec.sample_batch(feats, START, end, k=5, one_call=True, return_alphas=True, **kw)
    assert len(alpha_workspaces()) == n_ws
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert other[0] == a[0][::-1]
    assert capnet.lib().capnet_att_beam_decode_alphas_ws_bytes(2, 1, IMAGES, 5, 5, 20, 2048, 12, 64, 97, MAX_LEN + 1) > 0
