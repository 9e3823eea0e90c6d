"""capnet.seq2seq on the GPU: the reference fixture (tests/golden/seq2seq_tiny.npz), the fp64 restatement
(tests/seq2seq_ref.py, pinned to the fixture by tests/test_seq2seq_cpu.py) at full sizes and with dropout on, the
vocab_argmax kernel, the one-call greedy decode against the composed loop and the restatement, and two train steps.

Tolerances. Fixture: those tests/test_decoder_gpu.py applies to the NIC reference fixture (logits 2e-5 and gradients 5e-5
of max|ref|, loss 1e-6 relative). Restatement: tests/test_nic_stacked_gpu.py's TOL_LOGITS, TOL_LOSS, TOL_GRAD = 2e-5,
1e-5, 2e-4 with its _grad_ok form; a decode state TOL_STEP = 3e-5. Greedy ids are compared exactly: the CPU test asserts
the margins of every case (tests/seq2seq_cases.py)."""
import random

import pytest
import torch
import torch.nn.functional as Fn

import seq2seq_cases as SC
import seq2seq_ref as SR
import vocab_edge_cases as VC
from capnet import CapnetError, ops
from capnet.nic_model import DecoderRNN as NicDecoderRNN
from capnet.optim import Adam
from capnet.seq2seq import FUSED_GREEDY_OFF, Seq2Seq
from capnet.train import CrossEntropyLoss
from helpers import load_golden, pin_dropout_seed, rel_err, t
from oracle import dropout_ref as R

pytestmark = pytest.mark.gpu

TOL_LOGITS, TOL_LOSS, TOL_GRAD, TOL_STEP = 2e-5, 1e-5, 2e-4, 3e-5


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _grad_ok(a, b, rtol=TOL_GRAD):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return (a - b).abs().max().item() <= rtol * b.abs().max().item() + 1e-6


def _model(p, E, H, V, L, dev, dropout=0.0, train=True):
    m = Seq2Seq(E, H, V, L, dropout=dropout)
    m.load_state_dict({k: v.float() for k, v in p.items()}, strict=True)
    m.to(dev)
    return m.train() if train else m.eval()


def _fixture(L):
    z = load_golden("seq2seq_tiny.npz")
    pre = "L%d.param." % L
    return z, {k[len(pre):]: t(z[k]) for k in z.files if k.startswith(pre)}


def _force_draws(monkeypatch, tf):
    """random.random() yields 0.0 (< any ratio: teacher forced) or 0.99 (free running), step by step."""
    it = iter([0.0 if x else 0.99 for x in tf])
    monkeypatch.setattr(random, "random", lambda: next(it))


# ---- 5. the reference fixture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("mode", ["factual", "happy"])
@pytest.mark.parametrize("tag", ["tf10", "tf00", "tf05"])
def test_matches_reference_fixture(dev, L, mode, tag):
    z, p = _fixture(L)
    E, H, V = z["dims"].tolist()[:3]
    m = _model(p, E, H, V, L, dev)
    c = "L%d.case.%s_%s." % (L, mode, tag)
    feats = t(z["features"]).to(dev)
    src, sl = t(z["src"]).to(dev), z["src_lengths"].tolist()
    dst, dl = t(z["dst_in"]).to(dev), z["dst_lengths"].tolist()
    random.seed(int(z[c + "seed"]))
    out = m(feats, (src, sl), (dst, dl), teacher_forcing_ratio=float(z[c + "ratio"]), mode=mode)
    targets = ops.packed_targets(src, sl) if mode == "factual" else ops.packed_targets(t(z["dst_tgt"]).to(dev), dl)
    loss = ops.cross_entropy(out, targets)
    loss.backward()
    ops.check_device_errors()
    print("%s logits %.2e loss %.2e" % (c, rel_err(out, z[c + "logits"]),
                                        abs(loss.item() - float(z[c + "loss"])) / float(z[c + "loss"])))
    assert rel_err(out, z[c + "logits"]) < 2e-5
    assert abs(loss.item() - float(z[c + "loss"])) / float(z[c + "loss"]) < 1e-6
    n = 0
    for k, v in m.named_parameters():
        if c + "grad." + k in z.files:
            assert v.grad is not None, k
            assert rel_err(v.grad, z[c + "grad." + k]) < 5e-5, (k, rel_err(v.grad, z[c + "grad." + k]))
            n += 1
        else:
            assert v.grad is None, k
    assert n == 3 + 4 * L
    if mode == "factual":
        random.seed(int(z[c + "seed"]))
        _, (h, cc) = m.encoder(feats, src, sl, float(z[c + "ratio"]))
        assert tuple(h.shape) == (L, 1, H) and not h.requires_grad and not cc.requires_grad
        assert rel_err(h, z["L%d.states_%s.h" % (L, tag)]) < 2e-5 and rel_err(cc, z["L%d.states_%s.c" % (L, tag)]) < 2e-5


# ---- 6. / 7. full sizes against the restatement, dropout off and on ----------------------------------------------------
def _module_run(m, c, feats, tokens, lengths, targets, tf, dev, monkeypatch, seed_k=None):
    m.zero_grad()
    _force_draws(monkeypatch, tf)
    if seed_k is not None:
        pin_dropout_seed(seed_k)
    if c["mode"] == "factual":
        out, states = m.encoder(feats.float().to(dev), tokens.to(dev), lengths, 0.5)
    else:
        out, states = getattr(m, "decoder_" + c["mode"])((None, None), tokens.to(dev), lengths, 0.5), None
    loss = ops.cross_entropy(out, ops.packed_targets(targets.to(dev), lengths))
    loss.backward()
    ops.check_device_errors()
    return out.detach().cpu(), float(loss.detach()), {k: v.grad.detach().cpu() for k, v in m.named_parameters() if v.grad is not None}, states


def _ref_run(c, p, feats, tokens, lengths, targets, tf, drop_mask=None, layer_masks=None):
    prefix = "encoder" if c["mode"] == "factual" else "decoder_" + c["mode"]
    q = {k: (v.clone().requires_grad_(True) if k.startswith(prefix + ".") else v) for k, v in p.items()}
    margins = []
    out, states = SR.rnn_forward(q, prefix, c["layers"], feats if c["mode"] == "factual" else None, tokens, lengths, tf,
                                 drop_mask=drop_mask, layer_masks=layer_masks, margins=margins)
    tg = torch.cat([targets[:b, i] for i, b in enumerate(SR.batch_sizes(lengths))], 0)
    loss = Fn.cross_entropy(out, tg)
    loss.backward()
    grads = {k: v.grad for k, v in q.items() if v.requires_grad}
    return out.detach(), float(loss), grads, states, min(margins)


def _check(name, got, want):
    out, loss, grads, _ = got
    out_r, loss_r, grads_r, _, margin = want
    need = 2 * TOL_LOGITS * float(out_r.abs().max())
    print("%s: fed-back margin %.2e (needed %.2e), logits %.2e, loss %.2e" %
          (name, margin, need, _rel(out, out_r), abs(loss - loss_r) / abs(loss_r)))
    assert margin > need, (margin, need)                  # fed-back rows are well posed before anything is compared
    assert _rel(out, out_r) < TOL_LOGITS, _rel(out, out_r)
    assert abs(loss - loss_r) <= TOL_LOSS * abs(loss_r), (loss, loss_r)
    assert set(grads) == set(grads_r)
    for k in grads_r:
        assert _grad_ok(grads[k], grads_r[k]), (k, _rel(grads[k], grads_r[k]))


@pytest.mark.parametrize("name", [n for n in sorted(SC.TRAIN) if SC.TRAIN[n]["p"] == 0.0])
def test_full_size_matches_restatement(dev, monkeypatch, name):
    c, p, feats, (tokens, lengths), targets, tf = SC.train_case(name)
    m = _model(p, c["E"], c["H"], c["V"], c["layers"], dev)
    got = _module_run(m, c, feats, tokens, lengths, targets, tf, dev, monkeypatch)
    want = _ref_run(c, p, feats, tokens, lengths, targets, tf)
    _check(name, got, want)
    if c["mode"] == "factual":
        (h, cc), (h_r, c_r) = got[3], want[3]
        assert tuple(h.shape) == tuple(h_r.shape) and _rel(h, h_r) < TOL_LOGITS and _rel(cc, c_r) < TOL_LOGITS


@pytest.mark.parametrize("name", [n for n in sorted(SC.TRAIN) if SC.TRAIN[n]["p"] > 0.0])
def test_dropout_on_embeddings_only(dev, monkeypatch, name):
    """The kernels' embedding mask restated by oracle.dropout_ref, and NO mask between the layers. Negative controls: a
    column-shifted mask, no mask at all, and the between-layer masks the other stacked decoders draw must each land at
    least 100x farther from the GPU than the right mask."""
    c, p, feats, (tokens, lengths), targets, tf = SC.train_case(name)
    pd, B, T, E, H, L = c["p"], c["B"], c["T"], c["E"], c["H"], c["layers"]
    assert L == 3
    m = _model(p, E, H, c["V"], L, dev, dropout=pd)
    seed = pin_dropout_seed(77)
    got = _module_run(m, c, feats, tokens, lengths, targets, tf, dev, monkeypatch, seed_k=77)
    mask = torch.from_numpy(R.embedding_mask(seed, B, T, E, pd)).double()
    want = _ref_run(c, p, feats, tokens, lengths, targets, tf, drop_mask=mask)
    _check(name, got, want)
    right = _rel(got[0], want[0])
    N = sum(lengths)
    lm = {l: torch.from_numpy(R.layer_mask(seed, N, H, pd, l)).double() for l in range(1, L)}
    for label, kw in (("shifted", dict(drop_mask=mask.roll(1, 1))), ("none", dict(drop_mask=None)),
                      ("between layers", dict(drop_mask=mask, layer_masks=lm))):
        bad = _rel(got[0], _ref_run(c, p, feats, tokens, lengths, targets, tf, **kw)[0])
        print("%s: %s mask %.2e vs right %.2e" % (name, label, bad, right))
        assert bad > 100 * right, (label, bad, right)
    # backward regenerates the same mask: a second run under the same seed gives the same gradients, bit for bit
    again = _module_run(m, c, feats, tokens, lengths, targets, tf, dev, monkeypatch, seed_k=77)
    for k in got[2]:
        assert torch.equal(got[2][k], again[2][k]), k


# ---- 8. one layer, teacher forcing only: the NIC decoder's sequence call ------------------------------------------------
def test_one_layer_decoder_is_the_nic_decoder(dev):
    """Bit for bit: both are ops.SeqFn with the LSTM cell, one layer and no feature column on the same tensors; the
    `input_dropout_only` bit only changes what happens BETWEEN layers."""
    E, H, V, B, T = 24, 64, 61, 6, 8
    p = SR.make_params(SC.shapes(E, H, V, 1), seed=5)
    m = _model(p, E, H, V, 1, dev)
    nic = NicDecoderRNN(E, H, V, 1, dropout=0.0)
    d = m.decoder_sad
    nic.load_state_dict({"embed.weight": d.embed.weight, "lstm.weight_ih": d.lstm.weight_ih_l0,
                         "lstm.weight_hh": d.lstm.weight_hh_l0, "lstm.bias_ih": d.lstm.bias_ih_l0,
                         "lstm.bias_hh": d.lstm.bias_hh_l0, "linear.weight": d.linear.weight, "linear.bias": d.linear.bias})
    nic.to(dev).train()
    g = torch.Generator().manual_seed(6)
    tokens = torch.randint(3, V, (B, T), generator=g).to(dev)
    lengths = [8, 7, 5, 5, 3, 2]
    a = d((None, None), tokens, lengths, 1.0)
    b = nic(tokens, lengths, None, tf_mask=[True] * T)
    assert torch.equal(a, b)
    ops.cross_entropy(a, ops.packed_targets(tokens, lengths)).backward()
    ops.cross_entropy(b, ops.packed_targets(tokens, lengths)).backward()
    assert torch.equal(d.lstm.weight_hh_l0.grad, nic.lstm.weight_hh.grad)
    assert torch.equal(d.embed.weight.grad, nic.embed.weight.grad)


# ---- 9. the vocab_argmax kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("V", [37, 7411, 8192])
def test_vocab_argmax_matches_composed_and_fp64(dev, H, V):
    g = torch.Generator().manual_seed(V + H)
    W = torch.randn(V, H, generator=g) / H ** 0.5
    b = torch.randn(V, generator=g) * 0.1
    Wd, bd = W.to(dev), b.to(dev)
    for rows in (1, 5, 16, 17, 64, 96):
        h = torch.rand(rows, H, generator=g) * 2 - 1
        logits = h.double() @ W.double().t() + b.double()
        top2 = logits.topk(2, 1)[0]
        clear = (top2[:, 0] - top2[:, 1]) > 2 * TOL_STEP * logits.abs().max()     # rows whose argmax fp32 must agree on
        got = ops.vocab_argmax(h.to(dev), Wd, bd)
        assert got.dtype == torch.int64 and tuple(got.shape) == (rows,)
        composed = ops.argmax_rows(ops.linear(h.to(dev), Wd, bd)).long()
        want = logits.argmax(1)
        assert clear.sum() >= rows - 1
        assert torch.equal(got.cpu()[clear], want[clear]) and torch.equal(composed.cpu()[clear], want[clear]), rows
    nb = (h.double() @ W.double().t())                    # and without a bias (the last `rows`)
    t2 = nb.topk(2, 1)[0]
    ok = (t2[:, 0] - t2[:, 1]) > 2 * TOL_STEP * nb.abs().max()
    assert torch.equal(ops.vocab_argmax(h.to(dev), Wd).cpu()[ok], nb.argmax(1)[ok])


def test_vocab_argmax_ties_and_counter_rearm(dev):
    H, V, rows = 64, 200, 19
    W = torch.zeros(V, H)
    h = torch.zeros(rows, H)
    h[:, 0] = 1.0
    b = torch.zeros(V)
    W[5, 0] = W[9, 0] = 2.0            # an exact tie inside one workgroup's 32 entries
    assert ops.vocab_argmax(h.to(dev), W.to(dev), b.to(dev)).cpu().tolist() == [5] * rows
    W[150, 0] = 2.0                    # ... and across workgroups: the lowest index wins
    W[2, 0] = 2.0
    assert ops.vocab_argmax(h.to(dev), W.to(dev), b.to(dev)).cpu().tolist() == [2] * rows
    W2 = torch.zeros(V, H)
    W2[180, 0] = 2.0
    W2[40, 0] = 2.0
    assert ops.vocab_argmax(h.to(dev), W2.to(dev)).cpu().tolist() == [40] * rows
    # a row of equal logits -> 0; -inf / NaN are never picked; nothing to pick -> 0 (as ops.argmax_rows)
    assert ops.vocab_argmax(h.to(dev), torch.zeros(V, H).to(dev), torch.full((V,), 0.25).to(dev)).cpu().tolist() == [0] * rows
    bn = torch.full((V,), float("-inf"))
    bn[77] = -3.0
    bn[3] = float("nan")
    assert ops.vocab_argmax(h.to(dev), torch.zeros(V, H).to(dev), bn.to(dev)).cpu().tolist() == [77] * rows
    assert ops.vocab_argmax(h.to(dev), torch.zeros(V, H).to(dev), torch.full((V,), float("-inf")).to(dev)).cpu().tolist() == [0] * rows
    # back-to-back launches on one stream sharing one workspace: the counter re-arms
    g = torch.Generator().manual_seed(1)
    Wr = torch.randn(7411, 512, generator=g).to(dev)
    ws = ops.vocab_argmax_workspace(64, 7411, dev)
    hs = [torch.randn(64, 512, generator=g).to(dev) for _ in range(6)]
    outs = [ops.vocab_argmax(x, Wr, workspace=ws) for x in hs]
    torch.cuda.synchronize()
    assert int(ws[0].item()) & 0xffffffff == 0
    for x, o in zip(hs, outs):
        assert torch.equal(o, ops.vocab_argmax(x, Wr))
        assert torch.equal(o.cpu(), (x.double().cpu() @ Wr.double().cpu().t()).argmax(1))


@pytest.mark.parametrize("case", VC.ARGMAX, ids=VC.case_id)
def test_vocab_argmax_edges_of_the_shared_front(dev, case):
    """258 workgroups (the second pass of the last arriver's loop), one workgroup (the only arriver is the last), and the
    one-row-tile instantiation of H = 1024 with one group and two: tests/vocab_edge_cases.py, the rule above."""
    name, H, V, rows, groups = case
    h, Ws, bs, logits = VC.argmax_inputs(*case)
    hd, Wd, bd = h.to(dev), [W.to(dev) for W in Ws], [b.to(dev) for b in bs]
    alone = [ops.vocab_argmax(hd[i * rows:(i + 1) * rows], Wd[i], bd[i]) for i in range(groups)]
    for i, z in enumerate(logits):
        clear = VC.argmax_clear(z)
        assert clear.sum() >= rows - 1
        assert alone[i].dtype == torch.int64 and tuple(alone[i].shape) == (rows,)
        assert torch.equal(alone[i].cpu()[clear], z.argmax(1)[clear]), i
    if groups > 1:
        assert torch.equal(ops.vocab_argmax_groups(hd, Wd, bd), torch.cat(alone))


# ---- 10. sample -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 3])
def test_sample_matches_reference_fixture(dev, L):
    z, p = _fixture(L)
    E, H, V = z["dims"].tolist()[:3]
    m = _model(p, E, H, V, L, dev, train=False)
    feats = t(z["features"]).to(dev)
    ids, (h, c) = m.encoder.sample(feats)
    assert ids.dtype == torch.int64 and torch.equal(ids.cpu(), t(z["L%d.sample.factual.ids" % L]))
    assert tuple(h.shape) == (L, 4, H)
    assert rel_err(h, z["L%d.sample.factual.h" % L]) < TOL_STEP and rel_err(c, z["L%d.sample.factual.c" % L]) < TOL_STEP
    assert torch.equal(m.sample(feats, int(z["start_token"])), ids)
    happy = m.sample(feats[:1], int(z["start_token"]), mode="happy")
    assert torch.equal(happy.cpu(), t(z["L%d.sample.happy.ids" % L]))


@pytest.mark.parametrize("name", sorted(SC.GREEDY))
def test_greedy_decode_full_size(dev, monkeypatch, name):
    c, p, feats = SC.greedy_case(name)
    want, margin, scale, states_r = SC.greedy_reference(name)
    assert margin > SC.need(scale)
    m = _model(p, c["E"], c["H"], c["V"], c["layers"], dev, train=False)
    f = feats.float().to(dev)
    runs = {}
    for path in ("fused", "composed"):
        if path == "fused":
            monkeypatch.delenv(FUSED_GREEDY_OFF, raising=False)
        else:
            monkeypatch.setenv(FUSED_GREEDY_OFF, "1")
        runs[path] = m.sample(f, 1, mode=c["mode"])
        _, (h, cc) = m.encoder.sample(f)
        assert _rel(h, states_r[0]) < TOL_STEP and _rel(cc, states_r[1]) < TOL_STEP, path
    # the one C call itself at every row count (sample() routes more than 16 rows to the composed loop)
    from capnet.nic_stacked import _pack_cell
    enc = m.encoder
    packed = [_pack_cell(cell, (c["E"] + 15) // 16 * 16 if l == 0 else c["H"]) for l, cell in enumerate(enc._layers())]
    ids, st = ops.lstm_greedy_decode(40, [w for w, _ in packed], [b for _, b in packed], enc.embed.weight, enc.linear.weight,
                                     enc.linear.bias, features=f)
    want_enc = want if c["mode"] == "factual" else SR.greedy(p, "encoder", c["layers"], 40, features=feats)[0]
    assert torch.equal(ids.cpu(), want_enc), name
    assert _rel(st[:, 0::2].transpose(0, 1), states_r[0]) < TOL_STEP and _rel(st[:, 1::2].transpose(0, 1), states_r[1]) < TOL_STEP
    assert tuple(runs["fused"].shape) == (c["rows"], 40)
    assert torch.equal(runs["fused"].cpu(), want), name
    assert torch.equal(runs["fused"], runs["composed"]), name
    if c["mode"] != "factual" and c["rows"] > 1:          # B rows at once = B calls of one row
        monkeypatch.delenv(FUSED_GREEDY_OFF, raising=False)
        for i in range(c["rows"]):
            assert torch.equal(m.sample(f[i:i + 1], 1, mode=c["mode"])[0], runs["fused"][i]), i


def test_out_of_range_start_token_raises_and_process_stays_usable(dev):
    c, p, feats = SC.greedy_case("sad_r1_l2_v7411")
    m = _model(p, c["E"], c["H"], c["V"], c["layers"], dev, train=False)
    f = feats.float().to(dev)
    with pytest.raises(CapnetError):
        m.sample(f, c["V"] + 5, mode="sad")
    assert torch.equal(m.sample(f, 1, mode="sad").cpu(), SC.greedy_reference("sad_r1_l2_v7411")[0])


# ---- 11. two train steps ----------------------------------------------------------------------------------------------
def test_two_train_steps_match_torch_adam(dev, monkeypatch):
    """seq2seq/train.py:147-150: Adam(lr 2e-4) over everything for a factual step, then a decoder's own Adam for an
    emotion step. Losses within TOL_LOSS; parameters after the steps within 2e-5 of max|ref|, the bound
    tests/test_decoder_gpu.py holds its clamp + Adam steps to; the emotion step leaves the encoder alone."""
    E, H, V, L, B, T = 12, 64, 37, 2, 6, 7
    p = SR.make_params(SC.shapes(E, H, V, L), seed=21, out_scale=4.0)
    m = _model(p, E, H, V, L, dev)
    g = torch.Generator().manual_seed(22)
    feats = torch.randn(B, E, generator=g, dtype=torch.float64) * 0.5
    seq = torch.randint(3, V, (B, T + 1), generator=g)
    lengths = [7, 6, 6, 4, 3, 2]
    tf = [True, True, False, True, True, False, True]
    crit = CrossEntropyLoss()
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    opt = Adam(list(m.parameters()), lr=2e-4)
    opt_h = Adam(list(m.decoder_happy.parameters()), lr=2e-4)
    ropt = torch.optim.Adam(list(q.values()), lr=2e-4)
    ropt_h = torch.optim.Adam([v for k, v in q.items() if k.startswith("decoder_happy.")], lr=2e-4)

    def targets_of(x):
        return torch.cat([x[:b, i] for i, b in enumerate(SR.batch_sizes(lengths))], 0)

    # factual
    _force_draws(monkeypatch, tf)
    opt.zero_grad()
    out = m(feats.float().to(dev), (seq[:, :T].to(dev), lengths), teacher_forcing_ratio=0.5)
    loss = crit(out, ops.packed_targets(seq[:, :T].to(dev), lengths))
    loss.backward()
    opt.step()
    margins = []
    out_r = SR.seq2seq_forward(q, L, feats, (seq[:, :T], lengths), (None, None), tf, "factual", margins=margins)
    scale = float(out_r.detach().abs().max())
    loss_r = Fn.cross_entropy(out_r, targets_of(seq[:, :T]))
    ropt.zero_grad()
    loss_r.backward()
    ropt.step()
    assert abs(loss.item() - float(loss_r)) <= TOL_LOSS * float(loss_r)
    # an emotion step: the encoder's draws first, then the decoder's
    _force_draws(monkeypatch, tf + tf)
    m.zero_grad()
    out = m(feats.float().to(dev), (seq[:, :T].to(dev), lengths), (seq[:, :T].to(dev), lengths), teacher_forcing_ratio=0.5,
            mode="happy")
    loss = crit(out, ops.packed_targets(seq[:, 1:].contiguous().to(dev), lengths))
    loss.backward()
    for k, v in m.encoder.named_parameters():
        assert v.grad is None, k
    enc_before = {k: v.detach().clone() for k, v in m.encoder.named_parameters()}
    opt_h.step()
    out_r = SR.seq2seq_forward(q, L, feats, (seq[:, :T], lengths), (seq[:, :T], lengths), tf + tf, "happy", margins=margins)
    scale = max(scale, float(out_r.detach().abs().max()))
    loss_r = Fn.cross_entropy(out_r, targets_of(seq[:, 1:]))
    for v in q.values():
        v.grad = None
    loss_r.backward()
    ropt_h.step()
    ops.check_device_errors()
    assert min(margins) > 2 * TOL_LOGITS * scale, (min(margins), scale)      # fed-back rows are clear of ties
    assert abs(loss.item() - float(loss_r)) <= TOL_LOSS * float(loss_r)
    for k, v in m.encoder.named_parameters():
        assert torch.equal(v.detach(), enc_before[k]), k
    worst = max((_rel(v.detach(), q[k].detach()), k) for k, v in m.named_parameters())
    print("parameters after the two steps: worst %.2e (%s)" % worst)
    for k, v in m.named_parameters():
        assert _rel(v.detach(), q[k].detach()) < 2e-5, (k, _rel(v.detach(), q[k].detach()))
