"""GPU parity of the decoders (through the Python mirror classes and the C ABI) against
(a) fixtures produced by the reference's own classes and (b) the CPU oracle on larger seeded
cases. fp32 tolerance: 1e-4 relative on the loss is the north-star bar; these tests hold
2e-5 on logits/grads at tiny sizes and 1e-4 at full size."""
import random

import pytest
import torch

import capnet
from capnet import _lib, ops, synthetic
from capnet.model import DecoderFactoredLSTM
from capnet.model_att import DecoderFactoredLSTMAtt
from capnet.nic_model import DecoderRNN
from capnet.nic_model_att import DecoderRNNAtt
from capnet.optim import Adam
from capnet.utils import clip_gradient
from helpers import golden_case, golden_params, load_golden, rel_err, t
from oracle import decoders_ref as D
from oracle import step_ref as S

pytestmark = pytest.mark.gpu


def _packed_targets(captions, lengths):
    return D.packed_targets(captions, lengths)


def _run_product(dec, captions, lengths, feats, seed, ratio, dev, **kw):
    dec.zero_grad()
    f = None
    if feats is not None:
        f = feats.to(dev).requires_grad_(True)
    random.seed(seed)
    if isinstance(dec, DecoderRNN):
        out = dec(captions.to(dev), lengths, f, teacher_forcing_ratio=ratio)
    else:
        out = dec(captions.to(dev), lengths, f, teacher_forcing_ratio=ratio, **kw)
    loss = ops.cross_entropy(out, _packed_targets(captions, lengths).to(dev))
    loss.backward()
    ops.check_device_errors()
    return out, loss, f


def _compare_with_case(dec, out, loss, f, c, tol=2e-5):
    assert rel_err(out, c["logits"]) < tol
    assert abs(loss.item() - float(c["loss"])) / float(c["loss"]) < 1e-6
    n = 0
    for k, p in dec.named_parameters():
        key = "grad." + k
        if key in c:
            assert p.grad is not None, k
            assert rel_err(p.grad, c[key]) < 5e-5, k
            n += 1
        else:
            assert p.grad is None, k      # other modes' S matrices get no gradient (SURVEY A-11)
    assert n > 0
    if f is not None:
        if float(abs(c["dfeatures"]).max()) == 0.0:
            assert f.grad is None or float(f.grad.abs().max()) == 0.0
        else:
            assert rel_err(f.grad, c["dfeatures"]) < 5e-5


@pytest.mark.parametrize("cname,seed,ratio", [("tf1_factual", 100, 1.0), ("tf0_factual", 101, 0.0),
                                              ("tfmix_factual", 3, 0.6), ("tfmix_happy", 5, 0.6),
                                              ("tfmix_angry_nofeat", 8, 0.6)])
def test_factored_matches_reference_fixture(dev, cname, seed, ratio):
    z = load_golden("decoder_factored_tiny.npz")
    E, H, F, V = z["dims"].tolist()
    dec = DecoderFactoredLSTM(E, H, F, V, 1, dropout=0.0)
    dec.load_state_dict(golden_params(z))
    dec.to(dev).train()
    c = golden_case(z, cname)
    feats = t(z["features"]) if int(c["with_features"]) else None
    out, loss, f = _run_product(dec, t(z["captions"]), z["lengths"].tolist(), feats, seed, ratio, dev,
                                mode=str(c["mode"]))
    _compare_with_case(dec, out, loss, f, c)


@pytest.mark.parametrize("cname,seed,ratio", [("tf1", 100, 1.0), ("tf0", 101, 0.0), ("tfmix", 3, 0.6)])
def test_nic_matches_reference_fixture(dev, cname, seed, ratio):
    z = load_golden("decoder_nic_tiny.npz")
    E, H, _, V = z["dims"].tolist()
    dec = DecoderRNN(E, H, V, 1, dropout=0.0)
    dec.load_state_dict(golden_params(z))
    dec.to(dev).train()
    c = golden_case(z, cname)
    out, loss, f = _run_product(dec, t(z["captions"]), z["lengths"].tolist(), t(z["features"]), seed,
                                ratio, dev)
    _compare_with_case(dec, out, loss, f, c)


def test_forward_step_matches_reference_fixture(dev):
    z = load_golden("decoder_factored_tiny.npz")
    E, H, F, V = z["dims"].tolist()
    dec = DecoderFactoredLSTM(E, H, F, V, 1, dropout=0.0)
    dec.load_state_dict(golden_params(z))
    dec.to(dev).eval()
    x, h0, c0 = [t(z[k]).to(dev) for k in ("step.x", "step.h0", "step.c0")]
    with torch.no_grad():
        for mode in ("factual", "happy", "sad", "angry"):
            h, (h2, c) = dec.forward_step(x, (h0, c0), mode)
            assert rel_err(h, z["step.%s.h" % mode]) < 2e-5
            assert rel_err(c, z["step.%s.c" % mode]) < 2e-5
    with pytest.raises(ValueError):
        dec.forward_step(x, (h0, c0), "joyful")


def test_clamp_adam_sequence_matches_reference_fixture(dev):
    z = load_golden("decoder_factored_tiny.npz")
    a = load_golden("decoder_factored_tiny_adam.npz")
    E, H, F, V = z["dims"].tolist()
    dec = DecoderFactoredLSTM(E, H, F, V, 1, dropout=0.0)
    dec.load_state_dict(golden_params(z))
    dec.to(dev).train()
    captions, lengths, feats = t(z["captions"]), z["lengths"].tolist(), t(z["features"])
    opt = Adam(dec.parameters(), lr=float(a["lr"]))
    targets = _packed_targets(captions, lengths).to(dev)
    for it, mode in enumerate([str(m) for m in a["modes"]]):
        random.seed(int(a["seeds"][it]))
        out = dec(captions.to(dev), lengths, feats.to(dev), teacher_forcing_ratio=float(a["ratio"]), mode=mode)
        loss = ops.cross_entropy(out, targets)
        dec.zero_grad()
        loss.backward()
        clip_gradient(opt, float(a["clip"]))
        opt.step()
        assert abs(loss.item() - float(a["losses"][it])) / float(a["losses"][it]) < 1e-5
    for k, v in dec.state_dict().items():
        assert rel_err(v, a["final." + k]) < 2e-5, k


def _oracle_case(dec, p, forward, B, V, seed, ratio, dev, ragged_len=None, **kw):
    _, captions, lengths = synthetic.make_batch(B, V, seed=seed, images=False, min_len=3,
                                                max_len=ragged_len or 12)
    g = torch.Generator().manual_seed(seed + 1)
    feats = torch.randn(B, dec.embed_size, generator=g)
    random.seed(seed)
    tf = [random.random() < ratio for _ in range(max(lengths))]
    loss_r, grads_r, dfeat_r, logits_r = S.decoder_loss_and_grads(forward, p, captions, lengths, feats,
                                                                 tf, **kw)
    out, loss, f = _run_product(dec, captions, lengths, feats, seed, ratio, dev, **kw)
    assert rel_err(out, logits_r) < 5e-5
    assert abs(loss.item() - loss_r.item()) / loss_r.item() < 1e-5
    for k, prm in dec.named_parameters():
        gr = grads_r[k]
        if gr is None:
            assert prm.grad is None, k
        else:
            assert rel_err(prm.grad, gr) < 2e-4, k
    if dfeat_r is not None:
        assert rel_err(f.grad, dfeat_r) < 2e-4


@pytest.mark.parametrize("B,V,E,F,H,mode,ratio", [
    (9, 203, 20, 24, 28, "sad", 0.7),        # ragged everything (non multiples of 4)
    (33, 1000, 300, 64, 96, "factual", 0.8),
    (64, 7411, 300, 512, 512, "factual", 0.8),   # full-size cell, ragged vocabulary
    (12, 8192, 300, 1024, 512, "happy", 0.8),    # BASELINE configs[4] cell (factored 1024) at 96/8 per GPU
    (96, 1000, 300, 1024, 512, "factual", 0.8),  # the same cell at the undivided batch 96 (> 64 rows per step)
])
def test_factored_matches_oracle_seeded(dev, B, V, E, F, H, mode, ratio):
    dec = DecoderFactoredLSTM(E, H, F, V, 1, dropout=0.0)
    p = synthetic.decoder_state(dec.state_dict(), seed=B, bias_range=0.05)
    dec.load_state_dict(p)
    dec.to(dev).train()
    _oracle_case(dec, p, D.factored_lstm_forward, B, V, 17 + B, ratio, dev, mode=mode)


def test_nic_matches_oracle_seeded(dev):
    B, V, E, H = 8, 8192, 300, 512           # BASELINE config 1 decoder
    dec = DecoderRNN(E, H, V, 1, dropout=0.0)
    p = synthetic.decoder_state(dec.state_dict(), seed=3, bias_range=0.05)
    dec.load_state_dict(p)
    dec.to(dev).train()
    _oracle_case(dec, p, D.lstm_forward, B, V, 5, 0.8, dev, ragged_len=24)


def test_factored_full_size_losses_match_reference_scalars(dev):
    """BASELINE config 2 decoder: 4 clamp+Adam steps against the reference's own run -- per step the loss, the logits
    checksums and EVERY parameter's gradient norm (a 1e-4 bound on a loss near ln V alone cannot tell inputs apart).
    The inputs are re-drawn from capnet.synthetic; tests/test_fixture_inputs_cpu.py holds their digests and the oracle
    to the same fixture on CPU, so a stale fixture fails in the GPU-less container first."""
    z = load_golden("decoder_factored_full_scalars.npz")
    E, H, F, V, B = z["dims"].tolist()
    dec = DecoderFactoredLSTM(E, H, F, V, 1, dropout=0.0)
    dec.load_state_dict(synthetic.decoder_state(dec.state_dict(), seed=1234))
    dec.to(dev).train()
    _, captions, lengths = synthetic.make_batch(B, V, seed=0, images=False)
    g = torch.Generator().manual_seed(77)
    feats = torch.randn(B, E, generator=g).to(dev)
    opt = Adam(dec.parameters(), lr=2e-4)
    targets = _packed_targets(captions, lengths).to(dev)
    cap_d = captions.to(dev)
    random.seed(0)
    names = [str(s) for s in z["grad_names"]]
    for it in range(4):
        out = dec(cap_d, lengths, feats, teacher_forcing_ratio=0.8, mode="factual")
        loss = ops.cross_entropy(out, targets)
        dec.zero_grad()
        loss.backward()
        assert abs(loss.item() - float(z["losses"][it])) / float(z["losses"][it]) < 1e-4, it
        labs = float(z["logits_abs_sum"][it])
        assert abs(out.double().abs().sum().item() - labs) < 1e-4 * labs, it
        assert abs(out.double().sum().item() - float(z["logits_sum"][it])) < 1e-5 * labs, it
        grads = dict(dec.named_parameters())
        tol = 1e-4 if it == 0 else 1e-3      # later steps see parameters that went through Adam's g / (|g| + eps)
        for k, want in zip(names, z["grad_norms"][it].tolist()):
            gk = grads[k].grad
            got = gk.double().norm().item() if gk is not None else 0.0
            assert abs(got - want) <= tol * want + 1e-12, (it, k, got, want)
        clip_gradient(opt, 0.5)
        opt.step()
    ops.check_device_errors()


def _same_bits_as_the_single_layer_entries(fn, cfg, captions, feats, emb, Cw, Cb, weights, cdims, single):
    """Runs fn (ops.SeqFn / ops.AttSeqFn) forward and backward on leaf copies of the inputs, then single(...) -- the same
    forward and backward through the single-layer C entries -- and asserts bitwise-equal outputs and gradients."""
    leaves = [w.detach().clone().requires_grad_(True) for w in (emb,) + tuple(weights)]
    f = feats.detach().clone().requires_grad_(fn is ops.SeqFn) if feats is not None else None
    outs = fn.apply(cfg, captions, f, leaves[0], Cw, Cb, *leaves[1:])
    outs = outs if isinstance(outs, tuple) else (outs,)
    d_outs = [torch.randn(o.shape, generator=torch.Generator().manual_seed(7)).to(o.device) for o in outs]
    torch.autograd.backward(outs, d_outs)
    want_outs, want_grads = single(cfg, captions, f, emb.detach(), Cw, Cb, [w.detach() for w in weights], cdims, d_outs)
    for got, want in zip(outs, want_outs):
        assert torch.equal(got, want)
    got_grads = [leaves[0].grad] + [w.grad for w in leaves[1:]] + ([f.grad] if fn is ops.SeqFn and f is not None else [])
    assert len(got_grads) == len(want_grads)
    for k, (got, want) in enumerate(zip(got_grads, want_grads)):
        assert torch.equal(got, want), k


def _single_seq(cfg, captions, feats, emb, Cw, Cb, ws, dims, d_outs):
    """capnet_seq_forward / capnet_seq_backward -> ((hiddens,), [d emb, per-weight gradients, d features])."""
    L, dev, cell = capnet.lib(), emb.device, dims[-1]
    B, T, steps, N, E, F, H, V = dims[:8]
    cd = _lib.int_array(dims)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    saved, saved_i = new(L.capnet_seq_saved_floats(cd)), torch.empty(L.capnet_seq_saved_ints(cd), dtype=torch.int32, device=dev)
    hid = new(N, H)
    table = _lib.ptr_array(ws if cell == ops.CELL_FACTORED else ops._lstm_slots(ws))
    args = (float(cfg["dropout"]), int(cfg["seed"]), int(cfg["training"]))
    _lib.check(L.capnet_seq_forward(cd, _lib.int_array(cfg["batch_sizes"]), ops._tf_bytes(cfg["tf_mask"]), _lib.ptr(captions),
                                    _lib.ptr(feats), _lib.ptr(emb), table, _lib.ptr(Cw), _lib.ptr(Cb), *args, _lib.ptr(saved),
                                    _lib.ptr(saved_i), _lib.ptr(new(L.capnet_seq_fwd_scratch_floats(cd))), _lib.ptr(hid),
                                    _lib.ptr(ops.err_flag(dev)), _lib.current_stream()), "capnet_seq_forward")
    if cell == ops.CELL_FACTORED:
        g = [new(4 * F, E), new(4 * F), new(4, F, F), new(4 * F), new(4, H, F), new(4 * H), new(4 * H, H)]
    else:
        g = [new(4 * H, E), None, None, None, None, new(4 * H), new(4 * H, H)]
    dEmb, dFeat = new(V, E), new(B, E) if feats is not None else None
    _lib.check(L.capnet_seq_backward(cd, _lib.int_array(cfg["batch_sizes"]), _lib.ptr(d_outs[0]), _lib.ptr(hid),
                                     _lib.ptr(saved), _lib.ptr(saved_i), _lib.ptr(new(L.capnet_seq_bwd_scratch_floats(cd))),
                                     _lib.ptr_array(g + [dEmb, dFeat]), *args, _lib.current_stream()), "capnet_seq_backward")
    return (hid,), [dEmb] + ops._gate_grads(cell, F, H, *g) + ([dFeat] if feats is not None else [])


def _single_att(cfg, captions, feats, emb, Cw, Cb, ws, dims, d_outs):
    """capnet_att_seq_forward / capnet_att_seq_backward -> ((hiddens, alphas), [d emb, per-weight gradients])."""
    L, dev, cell = capnet.lib(), emb.device, dims[-1]
    B, T, steps, N, E, F, H, V, A, P, Cf = dims[:11]
    cd = _lib.int_array(dims)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    saved, saved_i = new(L.capnet_att_saved_floats(cd)), torch.empty(L.capnet_att_saved_ints(cd), dtype=torch.int32, device=dev)
    hid, alphas = new(N, H), new(B, steps, P)
    table = _lib.ptr_array(ws if cell == ops.CELL_FACTORED else ops._lstm_slots(ws[:4]) + ws[4:])
    args = (float(cfg["dropout"]), int(cfg["seed"]), int(cfg["training"]))
    _lib.check(L.capnet_att_seq_forward(cd, _lib.int_array(cfg["batch_sizes"]), ops._tf_bytes(cfg["tf_mask"]),
                                        _lib.ptr(captions), _lib.ptr(feats), _lib.ptr(emb), table, _lib.ptr(Cw), _lib.ptr(Cb),
                                        *args, _lib.ptr(saved), _lib.ptr(saved_i),
                                        _lib.ptr(new(L.capnet_att_fwd_scratch_floats(cd))), _lib.ptr(hid), _lib.ptr(alphas),
                                        _lib.ptr(ops.err_flag(dev)), _lib.current_stream()), "capnet_att_seq_forward")
    if cell == ops.CELL_FACTORED:
        g = [new(4 * F, E + Cf), new(4 * F), new(4, F, F), new(4 * F), new(4, H, F)]
    else:
        g = [new(4 * H, E + Cf), None, None, None, None]
    dWz, dbz = new(4 * H + A + Cf, H), new(4 * H + A + Cf)
    rest = [new(A, Cf), new(A), new(1, A), new(1), new(H, Cf), new(H), new(H, Cf), new(H)]
    dWe, dbe, dwf, dbf, dWih, dbih, dWic, dbic = rest
    dEmb = new(V, E)
    _lib.check(L.capnet_att_seq_backward(cd, _lib.int_array(cfg["batch_sizes"]), _lib.ptr(d_outs[0]), _lib.ptr(d_outs[1]),
                                         _lib.ptr(hid), _lib.ptr(feats), table, _lib.ptr(saved), _lib.ptr(saved_i),
                                         _lib.ptr(new(L.capnet_att_bwd_scratch_floats(cd))),
                                         _lib.ptr_array(g + [dWz, dbz] + rest + [dEmb]), *args, _lib.current_stream()),
               "capnet_att_seq_backward")
    return (hid, alphas), ([dEmb] + ops._gate_grads(cell, F, H, *g, dbz, dWz) +
                           [dWih, dbih, dWic, dbic, dWe, dbe, dWz[4 * H:4 * H + A], dbz[4 * H:4 * H + A], dwf, dbf,
                            dWz[4 * H + A:], dbz[4 * H + A:]])


def test_dropout_is_deterministic_and_scaled(dev):
    E, H, F, V, B = 32, 32, 32, 101, 6
    dec = DecoderFactoredLSTM(E, H, F, V, 1, dropout=0.5).to(dev).train()
    _, captions, lengths = synthetic.make_batch(B, V, seed=1, images=False, min_len=3, max_len=9)
    feats = torch.randn(B, E).to(dev)
    torch.manual_seed(5); random.seed(1)
    a = dec(captions.to(dev), lengths, feats, teacher_forcing_ratio=1.0)
    torch.manual_seed(5); random.seed(1)
    b = dec(captions.to(dev), lengths, feats, teacher_forcing_ratio=1.0)
    torch.manual_seed(6); random.seed(1)
    c = dec(captions.to(dev), lengths, feats, teacher_forcing_ratio=1.0)
    assert torch.equal(a, b) and not torch.equal(a, c)
    dec.eval()
    random.seed(1)
    d1 = dec(captions.to(dev), lengths, feats, teacher_forcing_ratio=1.0)
    dec.dropout.p = 0.0
    dec.train(); random.seed(1)
    d2 = dec(captions.to(dev), lengths, feats, teacher_forcing_ratio=1.0)
    assert torch.equal(d1, d2)
    # the single-layer C entries (the stacked entries at one layer; no Python path calls them) give the same bits as
    # ops.SeqFn / ops.AttSeqFn, dropout on, scheduled sampling mixed, on a small case of each cell
    random.seed(2)
    bs, cap = ops.batch_sizes_from_lengths(lengths), captions.to(dev)
    cfg = {"batch_sizes": bs, "tf_mask": [random.random() < 0.6 for _ in bs], "hidden_size": H, "dropout": 0.5,
           "seed": 12345, "training": True}
    N, P, A, Cf = sum(bs), 9, 16, 512
    rnn = DecoderRNN(E, H, V, 1).to(dev)
    lstm_w = [rnn.lstm.weight_ih, rnn.lstm.bias_ih, rnn.lstm.weight_hh, rnn.lstm.bias_hh]
    for cell, ws in ((ops.CELL_FACTORED, dec._weights("happy")), (ops.CELL_LSTM, lstm_w)):
        cf = dict(cfg, cell=cell, factored_size=F) if cell == ops.CELL_FACTORED else dict(cfg, cell=cell)
        _same_bits_as_the_single_layer_entries(ops.SeqFn, cf, cap, feats, dec.B.weight, dec.C.weight,
                                               dec.C.bias, ws, [B, cap.shape[1], len(bs), N, E, F if cell == 0 else 0, H, V,
                                                                1, cell], _single_seq)
    fmap = torch.randn(B, P, Cf, generator=torch.Generator().manual_seed(3)).to(dev)
    att = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=Cf).to(dev)
    natt = DecoderRNNAtt(A, E, H, V, 1, feature_size=Cf).to(dev)
    for cell, ws in ((ops.CELL_FACTORED, att._weights("sad")), (ops.CELL_LSTM, natt._weights())):
        _same_bits_as_the_single_layer_entries(ops.AttSeqFn, dict(cfg, cell=cell, factored_size=F, attention_size=A), cap, fmap,
                                               dec.B.weight, dec.C.weight, dec.C.bias, ws,
                                               [B, cap.shape[1], len(bs), N, E, F if cell == 0 else 4, H, V, A, P, Cf, cell],
                                               _single_att)
    ops.check_device_errors()


@pytest.mark.parametrize("E,V,ratio,p", [(300, 7, 1.0, 0.0), (600, 7, 0.6, 0.0), (64, 23, 1.0, 0.5)])
def test_gradients_are_bit_reproducible_when_tokens_repeat(dev, E, V, ratio, p):
    """The embedding gradient sums the rows of a token in row order (scatter_input_grad_kernel: one writer per table row):
    twelve backward passes over captions of a handful of words give the same bits (E = 600: two column sweeps). Values
    are the oracle tests' business."""
    B, H = 48, 64
    dec = DecoderFactoredLSTM(E, H, H, V, 1, dropout=p).to(dev).train()
    dec.load_state_dict(synthetic.decoder_state(dec.state_dict(), seed=3))
    _, captions, lengths = synthetic.make_batch(B, V, seed=4, images=False, min_len=4, max_len=22)
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(1))
    grads = []
    for _ in range(12):
        junk = torch.randn(1 << 18, device=dev)          # (moves the allocations of the pass around)
        torch.manual_seed(5)
        _, loss, f = _run_product(dec, captions, lengths, feats, 9, ratio, dev, mode="factual")
        grads.append({k: q.grad.clone() for k, q in dec.named_parameters() if q.grad is not None})
        grads[-1]["features"] = f.grad.clone()
        del junk
    for g in grads[1:]:
        for k, v in g.items():
            assert torch.equal(v, grads[0][k]), k
    emb = grads[0]["B.weight"]
    used = torch.unique(captions)
    assert float(emb[used].abs().max()) > 0
    unused = torch.ones(V, dtype=torch.bool)
    unused[used] = False
    if ratio == 1.0 and unused.any():                    # (free-running steps feed whatever word they predicted)
        assert float(emb[unused.to(dev)].abs().max()) == 0.0


def test_bad_inputs_raise(dev):
    dec = DecoderFactoredLSTM(8, 8, 8, 11, 1, dropout=0.0).to(dev)
    cap = torch.ones(2, 4, dtype=torch.long, device=dev)
    with pytest.raises(capnet.CapnetError):
        dec(cap, [2, 4], torch.zeros(2, 8, device=dev))          # not sorted decreasing
    cap[0, 1] = 99                                                # token id >= vocab
    dec(cap, [4, 2], torch.zeros(2, 8, device=dev), teacher_forcing_ratio=1.0)
    with pytest.raises(capnet.CapnetError):
        ops.check_device_errors()
