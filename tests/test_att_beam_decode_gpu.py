"""The one-call beam search of the attention decoders on the GPU: one step (capnet_att_decode_step: z from the ungathered h,
the beam-aware attention kernels on one map per image, layer 0 on the narrow or the wide decode step, the upper layers)
against an fp64 restatement written here; that it leaves z alone, mends a bad parent and reads no per-row map; the whole
search (capnet_att_beam_decode) against the host path and the fp64 beam search of every family of att_beam_cases;
poll_every; the fallbacks; evaluate.

Tolerance of a step: tests/test_stacked_decode_gpu.py's TOL for forward_step, 3e-5 of max|ref| of the new state and of the
top h. The attention adds f32 sums over A and P (1e-7-grade, relative) in front of the same cell."""
import pytest
import torch

import capnet
from att_beam_cases import IMAGES, KS, MAX_LEN, START, WIDE, families
from capnet import decode, ops

pytestmark = pytest.mark.gpu

TOL = 3e-5
E, H, V = 12, 64, 23


# ---- 1. one step against fp64 --------------------------------------------------------------------------------------
def _parents(n, k):
    """Within-image reversals in which every third row repeats its image's first parent: repeats, and rows nobody reads."""
    out = []
    for i in range(n):
        rev = [i * k + k - 1 - r for r in range(k)]
        out += [rev[0] if r % 3 == 1 else p for r, p in enumerate(rev)]
    return out


def _inputs(dev, cell, L, n, k, P, A, Cf, seed, E=E, H=H, V=V):
    g = torch.Generator().manual_seed(seed)
    nk, kin = n * k, (E + Cf + 15) // 16 * 16

    def u(*shape, a=1.0):
        return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * a)
    d = dict(cell=cell, k=k)
    d["att1"], d["feat"] = u(n, P, A), torch.rand((n, P, Cf), generator=g, dtype=torch.float64)
    d["wz"], d["bz"] = u(A + Cf, H, a=(3.0 / H) ** 0.5), u(A + Cf, a=0.1)
    d["w_full"], d["b_full"] = u(1, A, a=(3.0 / A) ** 0.5 * 4), u(1, a=0.1)
    d["emb"] = u(V, E)
    wcat, beff = [], []
    for l in range(L):
        K = (kin if l == 0 else H) + H
        w = u(4 * H, K, a=(3.0 / (E + Cf / 3 + H if l == 0 else 2 * H)) ** 0.5)
        if l == 0:
            w[:, E + Cf:kin] = 0
        wcat.append(w)
        beff.append(u(4 * H, a=0.1))
    d["wcat"], d["beff"] = wcat, beff
    d["state"] = u(nk, 2 * L, H)
    d["tokens"] = torch.randint(0, V, (nk,), generator=g)
    d["parent"] = torch.tensor(_parents(n, k), dtype=torch.long)
    return d


def _reference(d, parent):
    """The step in fp64: gather h, c by parent; z; scores, softmax, context, gate; [emb | ctx]; the cell; the upper layers."""
    n, P, A = d["att1"].shape
    k, nk, L, H = d["k"], d["state"].shape[0], len(d["wcat"]), d["state"].shape[2]
    src = torch.arange(nk) if parent is None else parent
    st = d["state"].index_select(0, src)
    z = st[:, 0] @ d["wz"].t() + d["bz"]
    img = torch.arange(nk) // k
    e = torch.relu(d["att1"][img] + z[:, None, :A]) @ d["w_full"][0] + d["b_full"]
    alpha = torch.softmax(e, 1)
    ctx = (alpha[:, :, None] * d["feat"][img]).sum(1)
    x = torch.cat([d["emb"][d["tokens"]], torch.sigmoid(z[:, A:]) * ctx], 1)
    new = torch.empty_like(st)
    for l in range(L):
        w = d["wcat"][l]
        kin = w.shape[1] - H
        xin = torch.cat([x, x.new_zeros(nk, kin - x.shape[1]), st[:, 2 * l]], 1)
        i, f, o, gt = (xin @ w.t() + d["beff"][l]).chunk(4, 1)
        c = torch.sigmoid(f) * st[:, 2 * l + 1] + torch.sigmoid(i) * torch.tanh(gt)
        h = torch.sigmoid(o) * (torch.tanh(c) if d["cell"] == ops.CELL_LSTM else c)
        new[:, 2 * l], new[:, 2 * l + 1] = h, c
        x = h
    return x, new


def _to(d, dev):
    f = lambda t: t.to(dev, torch.float32 if t.dtype == torch.float64 else t.dtype).contiguous()   # noqa: E731
    return {key: ([f(t) for t in v] if isinstance(v, list) else f(v) if isinstance(v, torch.Tensor) else v) for key, v in d.items()}


def _run(g, parent, workspace=None, **over):
    a = dict(g, **over)
    return ops.att_decode_step(a["att1"], a["feat"], a["k"], a["tokens"], a["emb"], a["wz"], a["bz"], a["w_full"], a["b_full"],
                               a["wcat"], a["beff"], a["state"], cell=a["cell"], parent_rows=parent, workspace=workspace)


def _check_step(dev, d):
    g = _to(d, dev)
    for parent in (d["parent"], None):
        want_top, want = _reference(d, parent)
        top, out = _run(g, None if parent is None else g["parent"])
        err_s = float((out.cpu().double() - want).abs().max() / want.abs().max())
        err_t = float((top.cpu().double() - want_top).abs().max() / want_top.abs().max())
        print("state %.2e top %.2e" % (err_s, err_t))
        assert err_s < TOL and err_t < TOL, (err_s, err_t, parent is None)
    ops.check_device_errors()


@pytest.mark.parametrize("n, k", [(1, 1), (1, 5), (3, 5), (2, 16), (7, 5)])
@pytest.mark.parametrize("P", [1, 6, 50])
@pytest.mark.parametrize("A", [16, 260])
@pytest.mark.parametrize("Cf", [512, 2048], ids=["narrow", "wide"])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("cell", [ops.CELL_FACTORED, ops.CELL_LSTM], ids=["factored", "lstm"])
def test_step_against_fp64(dev, cell, L, Cf, A, P, n, k):
    _check_step(dev, _inputs(dev, cell, L, n, k, P, A, Cf, seed=1000 * L + 100 * n + 10 * k + P + A + Cf))


def test_step_at_the_reference_shape(dev):
    _check_step(dev, _inputs(dev, ops.CELL_FACTORED, 2, 2, 5, 49, 512, 2048, seed=5, E=300, H=512, V=101))


def test_z_is_read_not_written(dev):
    """Parents repeat: a sigmoid written back into z would be applied twice. z after the step is the product itself."""
    d = _inputs(dev, ops.CELL_FACTORED, 1, 3, 5, 6, 16, 512, seed=11)
    g = _to(d, dev)
    n, k, A, Cf = 3, 5, 16, 512
    ws = ops.att_decode_step_workspace(n, k, 6, A, Cf, E, dev)
    top, out = _run(g, g["parent"], ws)
    z = ws[:n * k * (A + Cf)].view(n * k, A + Cf)
    before = z.clone()
    assert torch.equal(before, ops.linear(g["state"][:, 0].contiguous(), g["wz"], g["bz"]))
    top2, out2 = _run(g, g["parent"], ws)                 # the same buffer again
    assert torch.equal(z, before) and torch.equal(out2, out) and torch.equal(top2, top)
    ops.check_device_errors()


@pytest.mark.parametrize("bad", ["rows", -1])
@pytest.mark.parametrize("Cf", [512, 2048], ids=["narrow", "wide"])
def test_a_parent_out_of_range_sets_the_flag_and_reads_the_row_itself(dev, Cf, bad):
    ops.check_device_errors()
    d = _inputs(dev, ops.CELL_LSTM, 2, 3, 5, 6, 16, Cf, seed=12)
    g = _to(d, dev)
    r = 7
    mended = g["parent"].clone()
    mended[r] = r
    want_top, want = _run(g, mended)
    ops.check_device_errors()
    parent = g["parent"].clone()
    parent[r] = 15 if bad == "rows" else bad
    top, out = _run(g, parent)
    assert torch.equal(out, want) and torch.equal(top, want_top)
    with pytest.raises(capnet.CapnetError):
        ops.check_device_errors()
    ops.check_device_errors()                       # (the check cleared the flag)


def test_the_maps_are_per_image(dev):
    """att1 / feat hold exactly n maps; another map for one image changes that image's k rows and no other."""
    n, k = 3, 5
    d = _inputs(dev, ops.CELL_FACTORED, 2, n, k, 6, 16, 512, seed=13)
    g = _to(d, dev)
    assert g["att1"].shape[0] == n and g["feat"].shape[0] == n
    top, out = _run(g, g["parent"])
    feat, att1 = g["feat"].clone(), g["att1"].clone()
    feat[1] = feat[1].flip(0) * 0.5
    att1[1] = att1[1].flip(0) + 0.25
    top2, out2 = _run(g, g["parent"], feat=feat, att1=att1)
    mine = slice(k, 2 * k)
    for a, b in ((top, top2), (out, out2)):
        assert torch.equal(a[:k], b[:k]) and torch.equal(a[2 * k:], b[2 * k:])
        assert all(not torch.equal(a[r], b[r]) for r in range(k, 2 * k)), mine
    ops.check_device_errors()


# ---- 2. the search -------------------------------------------------------------------------------------------------
def _family(name):
    return [f for f in families() if f.name == name][0]


def _att(dec, feats, n, k, kw):
    return getattr(dec._beam(feats, n, k, *kw.values(), True)[0], "att", None)


@pytest.mark.parametrize("family", families(), ids=lambda f: f.name)
def test_one_call_equals_the_host_path_and_fp64(dev, monkeypatch, family):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    for k in KS:
        att = _att(dec, feats, IMAGES, k, kw)
        assert isinstance(att, decode.AttStack)                         # the one call does run
        assert att.feat.shape[0] == IMAGES and att.att1.shape[0] == IMAGES and att.state.shape[0] == IMAGES * k
        assert (att.wcat[0].shape[1] > 2048) == (family.name in WIDE)
        want = [family.reference(k, i) for i in range(IMAGES)]
        assert dec.sample_batch(feats, START, end, k=k, **kw) == want, k
        assert dec.sample_batch(feats, START, end, k=k, one_call=True, **kw) == want, k
        for i in range(IMAGES):
            assert isinstance(_att(dec, feats[i:i + 1], None, k, kw), decode.AttStack)
            one = dec.sample(feats[i:i + 1], START, end, k=k, one_call=True, **kw)
            assert one.dtype == torch.int64 and one.dim() == 2 and one.device.type == "cuda"
            assert one.cpu().tolist() == [want[i]], (k, i)
    ops.check_device_errors()


def _biased(dev, end_bias):
    family = _family("StackedDecoderRNNAtt-2")
    dec = family.make().to(dev).eval()
    with torch.no_grad():
        dec.linear.bias[family.end] += end_bias
    return family, dec


def _one_call(dec, feats, k, end, poll):
    a = _att(dec, feats, feats.shape[0], k, {})
    return ops.att_beam_decode(a.cell, a.att1, a.feat, a.emb, a.wz, a.bz, a.full_att.weight, a.full_att.bias, a.wcat, a.beff, a.Cw,
                               a.Cb, a.state, k, dec.max_seq_length + 1, START, end, poll_every=poll, return_steps=True)


@pytest.mark.parametrize("k", KS)
def test_poll_every_stops_early_with_the_same_result(dev, monkeypatch, k):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family, dec = _biased(dev, 60.0)                 # <end> wins on every row from the first step on
    feats, end = family.features().to(dev), family.end
    want, steps = _one_call(dec, feats, k, end, 0)
    assert steps == MAX_LEN + 1
    assert all(2 <= len(s) <= 3 and s[0] == START and s[-1] == end for s in want), want
    assert want == dec.sample_batch(feats, START, end, k=k, on_device=True)
    for m in (1, 3):
        got, steps = _one_call(dec, feats, k, end, m)
        assert got == want and steps <= 2 + m, (m, steps)
        assert dec.sample_batch(feats, START, end, k=k, one_call=True, poll_every=m) == want, m
    ops.check_device_errors()


def test_nothing_completed_returns_end(dev, monkeypatch):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family, dec = _biased(dev, -60.0)
    feats = family.features().to(dev)
    for m in (1, 3):
        got, steps = _one_call(dec, feats, 3, family.end, m)
        assert got == [[family.end]] * IMAGES and steps == MAX_LEN + 1, m
    assert dec.sample_batch(feats, START, family.end, k=3, one_call=True) == [[family.end]] * IMAGES
    ops.check_device_errors()


# ---- 3. fallbacks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", families(), ids=lambda f: f.name)
def test_the_composed_step_switch_takes_the_device_loop(dev, monkeypatch, family):
    monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features().to(dev), family.end, family.kw
    assert _att(dec, feats, IMAGES, 5, kw) is None
    for poll in (0, 3):
        assert dec.sample_batch(feats, START, end, k=5, one_call=True, poll_every=poll, **kw) == \
            dec.sample_batch(feats, START, end, k=5, on_device=True, poll_every=poll, **kw)
    ops.check_device_errors()


def test_an_embedding_width_off_four_takes_the_device_loop(dev, monkeypatch):
    import nic_stacked_ref
    from capnet.nic_model_att import DecoderRNNAtt
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    dec = DecoderRNNAtt(16, 10, 64, 37, 1, feature_size=512)
    dec.load_state_dict({key: v.float() for key, v in nic_stacked_ref.decode_params(dec, seed=3).items()})
    dec.max_seq_length = MAX_LEN
    dec = dec.to(dev).eval()
    family = _family("DecoderRNNAtt")
    feats = family.features().to(dev)
    assert _att(dec, feats, IMAGES, 5, {}) is None
    assert dec.sample_batch(feats, START, family.end, k=5, one_call=True) == \
        dec.sample_batch(feats, START, family.end, k=5, on_device=True)
    assert dec.sample(feats[:1], START, family.end, k=3, one_call=True).cpu().tolist() == \
        dec.sample(feats[:1], START, family.end, k=3, on_device=True).cpu().tolist()
    ops.check_device_errors()


def test_a_start_token_out_of_range_raises_after_the_call(dev, monkeypatch):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family = _family("DecoderFactoredLSTMAtt")
    dec = family.make().to(dev).eval()
    feats = family.features().to(dev)
    ops.check_device_errors()
    with pytest.raises(capnet.CapnetError, match="token id out of range"):
        dec.sample_batch(feats, family.V + 3, family.end, k=3, one_call=True, **family.kw)
    ops.check_device_errors()                       # (raised and cleared)
    assert dec.sample_batch(feats, START, family.end, k=3, one_call=True, **family.kw) == \
        [family.reference(3, i) for i in range(IMAGES)]


# ---- 4. evaluate -----------------------------------------------------------------------------------------------------
def test_evaluate_one_call(dev, monkeypatch):
    from capnet.train import evaluate
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    family = _family("DecoderFactoredLSTMAtt")
    dec = family.make().to(dev).eval()
    start, end, V_ = START, family.end, family.V

    class Vocab:
        word2idx = {"<start>": start, "<end>": end}
        idx2word = {i: ("<end>" if i == end else "<start>" if i == start else "w%d" % i) for i in range(V_)}

    class Enc(torch.nn.Module):
        def forward(self, images):
            return images
    # the references are what the decoder says, one of them cut short: BLEU is not degenerate, and a changed caption shows
    said = dec.sample_batch(family.features().to(dev), start, end, k=5, **family.kw)
    caps = [[torch.tensor(s), torch.tensor(s[:-2] + [end])] for s in said]
    batches = [(family.features(), None, None, caps)]
    mode = family.kw["mode"]
    one = evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=5, one_call=True)
    assert one == evaluate(Enc(), dec, Vocab(), batches, mode=mode, k=5, on_device=True)
    assert one[0] > 0.99
