"""The attention kernels (csrc/att_kernels.hip, att_loss_* of csrc/loss_optim.hip) at other attention-map sizes than the
two the rest of the suite runs (P = 9 and 196). Their pixel loops have tails: the forward context splits P into four
quarters swept 14 pixels at a time with a clamped, zero-weighted rest; the backward kernels and att_datt1 sweep all of P
14 at a time; the scores kernel takes 4 pixels per wave over score_chunks(rows, P) workgroups per row.
tests/long_cases.py lists the map sizes and says which path each takes (asserted in tests/test_long_inputs_cpu.py).

1. capnet_att_step_fwd against an fp64 restatement of oracle.decoders_ref.attention_step plus the sigmoid gate.
2. The backward kernels through DecoderFactoredLSTMAtt / DecoderRNNAtt on short batches against the oracle's autograd,
   every P also with TAIL-ONLY features (zero but at the pixels the tail code handles), so that one mishandled pixel is
   an O(1) error instead of 1 / P of a sum over the map.
3. capnet_att_loss_fwd / bwd (ops.attention_loss) against fp64, below and above the grid caps.
4. EncoderCNN's pooling to encoded_image_size 7 and 28, and the refusal of a non-multiple."""
import ctypes as C
import types

import pytest
import torch
import torch.nn.functional as Fn

import capnet
from capnet import ops, synthetic
from capnet._lib import current_stream, lib, ptr
from capnet.model_att import DecoderFactoredLSTMAtt, EncoderCNN
from capnet.nic_model_att import DecoderRNNAtt
from helpers import rel_err
import long_cases as LC
from oracle import decoders_ref as D

pytestmark = pytest.mark.gpu

NAN = float("nan")

# (P, rows, A, C): every P of LC.P_LIST, every row count of {1, 12, 16, 17, 64, 128}, every A of {4, 24, 132, 512}, both
# C; P < 16 meets rows = 128 (4 pixel chunks per row, most of them empty) and rows = 1 (as many chunks as pixels allow)
STEP_SHAPES = []
for _k, _P in enumerate([1, 2, 3, 4, 5, 13, 14, 15]):
    STEP_SHAPES.append((_P, 128, (4, 24, 132, 512)[_k % 4], 512))
    STEP_SHAPES.append((_P, 1, (512, 132, 24, 4)[_k % 4], 2048 if _k % 2 else 512))
STEP_SHAPES += [(16, 17, 132, 2048), (49, 12, 512, 512), (55, 16, 24, 512), (56, 64, 4, 512), (57, 17, 132, 512),
                (64, 128, 24, 512), (196, 12, 512, 2048), (197, 16, 132, 512), (256, 17, 24, 512), (441, 1, 512, 2048),
                (441, 64, 4, 512), (784, 1, 132, 512), (784, 12, 512, 512)]


def test_step_shapes_cover_the_lists():
    assert sorted({s[0] for s in STEP_SHAPES}) == LC.P_LIST
    assert {s[1] for s in STEP_SHAPES} == {1, 12, 16, 17, 64, 128}
    assert {s[2] for s in STEP_SHAPES} == {4, 24, 132, 512} and {s[3] for s in STEP_SHAPES} == {512, 2048}
    for P in (1, 2, 3, 4, 5, 13, 14, 15):
        assert (P, 128) in {s[:2] for s in STEP_SHAPES} and (P, 1) in {s[:2] for s in STEP_SHAPES}


def _step_reference(att1, feat, att2, gpre, wf, bf):
    """fp64: Attention.forward (oracle.decoders_ref.attention_step with att1 hoisted) and the f_beta gate."""
    att1, feat, att2, gpre, wf, bf = [x.double() for x in (att1, feat, att2, gpre, wf, bf)]
    e = torch.relu(att1 + att2.unsqueeze(1)) @ wf + bf
    alpha = torch.softmax(e, dim=1)
    awe = (feat * alpha.unsqueeze(2)).sum(dim=1)
    gate = torch.sigmoid(gpre)
    return alpha, awe, gate, gate * awe


def _step_call(att1, feat, z, A, Cf, wf, bf, rows, P, alpha, alphas_bt, steps, t, awe, xa, xa_col, escore):
    return lib().capnet_att_step_fwd(ptr(att1), ptr(feat), ptr(z), C.c_void_p(z.data_ptr() + 4 * A), z.shape[1], ptr(wf),
                                     ptr(bf), rows, P, A, Cf, ptr(alpha), ptr(alphas_bt), steps, t, ptr(awe),
                                     C.c_void_p(xa.data_ptr() + 4 * xa_col), xa.shape[1], ptr(escore), current_stream())


@pytest.mark.parametrize("P,rows,A,Cf", STEP_SHAPES)
@pytest.mark.parametrize("tail_only", [False, True], ids=["dense", "tail-only"])
def test_att_step_fwd_matches_float64(dev, P, rows, A, Cf, tail_only):
    """Bound 2e-5 of the largest reference value: fp32's eps is 6e-8, a score sums A <= 512 products and the context
    P <= 784 (typical error sqrt(K) eps = 1.7e-6, worst case K eps = 4.7e-5), expf and the division add a few ulp; one
    pixel dropped or counted twice is 1 / P >= 1.3e-3 of the context with dense features and O(1) with tail-only ones."""
    g = torch.Generator().manual_seed(1000 * P + rows)
    att1 = torch.randn(rows, P, A, generator=g)
    feat = torch.randn(rows, P, Cf, generator=g).abs() * 0.5
    if tail_only:
        feat = LC.tail_only_features(feat)
    att2 = torch.randn(rows, A, generator=g)
    gpre = torch.randn(rows, Cf, generator=g)
    wf, bf = torch.randn(A, generator=g) * 0.5, torch.randn(1, generator=g)
    ldz, ldx, xa_col, steps, t = A + Cf + 8, Cf + 12, 4, 3, 1
    z = torch.full((rows + 1, ldz), NAN)
    z[:rows, :A], z[:rows, A:A + Cf] = att2, gpre
    z = z.to(dev)
    new = lambda *shape: torch.full(shape, NAN, device=dev)
    alpha, alphas_bt, awe, xa, escore = new(rows + 1, P), new(rows + 1, steps, P), new(rows + 1, Cf), new(rows + 1, ldx), \
        new(rows + 1, P)
    st = _step_call(att1.to(dev), feat.to(dev), z, A, Cf, wf.to(dev), bf.to(dev), rows, P, alpha, alphas_bt, steps, t, awe,
                    xa, xa_col, escore)
    assert st == 0, lib().capnet_last_error()
    torch.cuda.synchronize()
    r_alpha, r_awe, r_gate, r_xa = _step_reference(att1, feat, att2, gpre, wf, bf)
    tol = 2e-5
    e = {"alpha": rel_err(alpha[:rows], r_alpha), "alphas_bt": rel_err(alphas_bt[:rows, t], r_alpha),
         "awe": rel_err(awe[:rows], r_awe), "gate": rel_err(z[:rows, A:A + Cf], r_gate),
         "xa": rel_err(xa[:rows, xa_col:xa_col + Cf], r_xa)}
    print("P %d rows %d A %d C %d %s: %s" % (P, rows, A, Cf, "tail-only" if tail_only else "dense",
                                              " ".join("%s %.1e" % kv for kv in e.items())))
    for k, v in e.items():
        assert v < tol, (k, v)
    assert torch.equal(alpha[:rows], alphas_bt[:rows, t])
    assert float((alpha[:rows].double().sum(1) - 1).abs().max()) < 1e-5
    # what must not be written: the other steps' rows of alphas_bt, the guard row of every buffer, the columns around
    # the gate and around xa; att2 is read only
    nan = lambda x: bool(torch.isnan(x).all())
    assert nan(alphas_bt[:, 0]) and nan(alphas_bt[:, 2]) and nan(alphas_bt[rows])
    assert nan(alpha[rows]) and nan(awe[rows]) and nan(xa[rows]) and nan(z[rows]) and nan(escore[rows])
    assert nan(z[:, A + Cf:]) and nan(xa[:, :xa_col]) and nan(xa[:, xa_col + Cf:])
    assert torch.equal(z[:rows, :A].cpu(), att2)


def test_att_step_fwd_refuses_bad_shapes(dev):
    """P = 0, P = 4097, A not a multiple of 4, C not a multiple of 512, rows not 16-byte aligned, t outside the steps:
    an error status and no launch (the NaN-filled outputs stay NaN)."""
    rows, P, A, Cf = 2, 8, 8, 512
    z = torch.zeros(rows, A + Cf + 4, device=dev)
    att1, feat = torch.zeros(rows, 4100, A + 4, device=dev), torch.zeros(rows, 4100, Cf, device=dev)
    wf, bf = torch.zeros(A + 4, device=dev), torch.zeros(1, device=dev)
    new = lambda *shape: torch.full(shape, NAN, device=dev)
    alpha, alphas_bt, awe, xa, escore = new(rows, 4100), new(rows, 1, 4100), new(rows, Cf + 512), new(rows, Cf + 516), \
        new(rows, 4100)
    call = lambda P_=P, A_=A, C_=Cf, col=0, t=0, zz=z: _step_call(att1, feat, zz, A_, C_, wf, bf, rows, P_, alpha, alphas_bt,
                                                                  1, t, awe, xa, col, escore)
    assert call() == 0
    torch.cuda.synchronize()
    for buf in (alpha, alphas_bt, awe, xa, escore):
        buf.fill_(NAN)
    assert call(P_=0) != 0 and call(P_=4097) != 0
    assert call(A_=6) != 0 and call(C_=256) != 0 and call(C_=768) != 0
    assert call(col=1) != 0                              # xa rows off 16-byte alignment
    assert call(zz=z[:, 1:]) != 0                        # att2 / gate rows off 16-byte alignment (and an odd ld)
    assert call(t=1) != 0 and call(t=-1) != 0
    assert b"att_step_fwd" in lib().capnet_last_error()
    torch.cuda.synchronize()
    for buf in (alpha, alphas_bt, awe, xa, escore):
        assert bool(torch.isnan(buf).all())
    assert call(P_=4096) == 0                            # the largest map accepted
    torch.cuda.synchronize()
    assert not torch.isnan(alpha.view(-1)[:rows * 4096]).any()         # rows of 4096 in the 4100-wide buffer
    ops.check_device_errors()


# ---- 2. backward through the decoders ------------------------------------------------------------------------------
def grad_close(a, b, rtol):
    """max|a-b| <= rtol*max|b| + 1e-6 (tests/test_decoder_att_gpu.py)."""
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return (a - b).abs().max().item() <= rtol * b.abs().max().item() + 1e-6


BWD_DIMS = dict(A=24, E=20, H=28, F=24, V=203, Cf=512)
BWD_LENGTHS = {1: [4], 5: [6, 5, 4, 3, 3], 20: [5, 5, 5, 4, 4, 4, 4, 4, 4, 4, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3]}


@pytest.mark.parametrize("P", LC.P_LIST)
@pytest.mark.parametrize("family", ["factored_att", "nic_att"])
@pytest.mark.parametrize("tail_only", [False, True], ids=["dense", "tail-only"])
def test_attention_backward_at_map_sizes(dev, P, family, tail_only):
    """att_context_bwd, att_scores_bwd and att_datt1 have no entry of their own: every parameter gradient of a short
    training step against the fp64 oracle's autograd, bounds of tests/test_decoder_att_gpu.py (1e-4 / 1e-5 / 5e-4)."""
    d = BWD_DIMS
    B = (1, 5, 20)[(LC.P_LIST.index(P) + (family == "nic_att")) % 3]
    lengths = BWD_LENGTHS[B]
    if family == "factored_att":
        dec = DecoderFactoredLSTMAtt(d["A"], d["E"], d["H"], d["F"], d["V"], 1, feature_size=d["Cf"], dropout=0.0)
        forward, kw = D.factored_att_forward, {"mode": "sad"}
    else:
        dec = DecoderRNNAtt(d["A"], d["E"], d["H"], d["V"], 1, feature_size=d["Cf"], dropout=0.0)
        forward, kw = D.lstm_att_forward, {}
    p = synthetic.decoder_state(dec.state_dict(), seed=P, bias_range=0.05)
    dec.load_state_dict(p)
    dec.to(dev).train()
    captions = LC._captions(lengths, d["V"], P)
    feats = torch.randn(B, P, d["Cf"], generator=torch.Generator().manual_seed(P + B)).abs() * 0.5
    if tail_only:
        feats = LC.tail_only_features(feats)
        assert int((feats.abs().sum(2) > 0).sum()) == B * len(LC.tail_pixels(P))
    tf = [True] * max(lengths)
    leaves = {k: v.double().requires_grad_(True) for k, v in p.items()}
    logits_r, alphas_r = forward(leaves, captions, lengths, feats.double(), tf, **kw)
    loss_r = D.att_loss(logits_r, alphas_r, D.packed_targets(captions, lengths))
    loss_r.backward()
    out, alphas = dec(captions.to(dev), lengths, feats.to(dev), tf_mask=tf, **kw)
    loss = ops.attention_loss(ops.cross_entropy(out, D.packed_targets(captions, lengths).to(dev)), alphas, 1.0)
    loss.backward()
    ops.check_device_errors()
    assert rel_err(out, logits_r) < 1e-4
    assert rel_err(alphas, alphas_r) < 1e-4
    assert abs(loss.item() - loss_r.item()) / loss_r.item() < 1e-5
    n, worst = 0, (0.0, None)
    for k, prm in dec.named_parameters():
        gr = leaves[k].grad
        if gr is None:
            assert prm.grad is None, k
            continue
        e = rel_err(prm.grad, gr)
        if float(gr.abs().max()) > 1e-4 and e > worst[0]:
            worst = (e, k)
        assert grad_close(prm.grad, gr, 5e-4), (k, e)
        n += 1
    assert n >= 19
    print("%s P %d B %d %s: worst gradient %.1e (%s)" % (family, P, B, "tail-only" if tail_only else "dense", worst[0], worst[1]))


# ---- 3. the attention loss -----------------------------------------------------------------------------------------
LOSS_SHAPES = [(P, 3, (1, 30, 128)[k % 3]) for k, P in enumerate(LC.P_LIST)] + \
              [(784, 170, 30), (441, 300, 1), (196, 700, 128), (5, 27000, 1), (13, 40, 128)]


@pytest.mark.parametrize("P,B,steps", LOSS_SHAPES)
def test_attention_loss_at_map_sizes(dev, P, B, steps):
    """nll + ((1 - sum_t alpha)^2).mean() and its gradient. The column sums add `steps` fp32 terms in order (error at most
    steps x eps of the sum, 7.6e-6 at 128 steps) and the gradient is proportional to (sum - 1), here about 0.25 of the
    sum: bound 3e-5 of the largest gradient, 1e-5 on the loss (the mean averages the errors)."""
    g = torch.Generator().manual_seed(P * 131 + B)
    alphas = torch.rand(B, steps, P, generator=g) * (1.5 / steps)
    nll = torch.tensor(2.5)
    a_d = alphas.to(dev).requires_grad_(True)
    n_d = nll.to(dev).requires_grad_(True)
    loss = ops.attention_loss(n_d, a_d, 0.7)
    loss.backward()
    a_r = alphas.double().requires_grad_(True)
    loss_r = nll.double() + 0.7 * ((1.0 - a_r.sum(dim=1)) ** 2).mean()
    loss_r.backward()
    e_loss = abs(loss.item() - loss_r.item()) / loss_r.item()
    e_grad = rel_err(a_d.grad, a_r.grad)
    print("P %d B %d steps %d (B P = %d, B steps P = %d): loss %.1e gradient %.1e" % (P, B, steps, B * P, B * steps * P,
                                                                                 e_loss, e_grad))
    assert e_loss < 1e-5 and e_grad < 3e-5
    assert float(n_d.grad) == 1.0


def test_attention_loss_shapes_straddle_the_grid_caps():
    bp = [B * P for P, B, _ in LOSS_SHAPES]
    assert min(bp) < 256 * 512 < max(bp)                                  # att_loss_colsum: at most 512 workgroups
    tot = [B * P * s for P, B, s in LOSS_SHAPES]
    assert min(tot) < 256 * 1024 < max(tot)                               # att_loss_bwd: at most 1024 workgroups
    assert {P for P, _, _ in LOSS_SHAPES} == set(LC.P_LIST) and {s for _, _, s in LOSS_SHAPES} == {1, 30, 128}


# ---- 4. the encoder's pooling --------------------------------------------------------------------------------------
def test_encoder_pooling_sizes(dev):
    fmap = torch.randn(3, 7, 7, 2048, generator=torch.Generator().manual_seed(5))
    for side in (7, 14, 28):
        enc = types.SimpleNamespace(encoded_image_size=side)
        out = EncoderCNN._pool(enc, fmap.to(dev))
        ref = Fn.adaptive_avg_pool2d(fmap.double().permute(0, 3, 1, 2), side).permute(0, 2, 3, 1)
        assert out.shape == (3, side, side, 2048)
        assert rel_err(out, ref) < 1e-6
    for side in (10, 20, 6):
        with pytest.raises(capnet.CapnetError):
            EncoderCNN._pool(types.SimpleNamespace(encoded_image_size=side), fmap.to(dev))
    ops.check_device_errors()
