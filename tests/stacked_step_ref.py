"""The step-by-step engine of capnet.stacked.StackedFactoredLSTM, the reference of tests/test_stacked_gpu.py for the one C
call each way the module makes: per layer and step the gate chains U_g(S_g(V_g x)) as ops.linear products, the W product
and the fused cell kernel (ops.lstm_cell), with torch autograd composing the backward. torch is glue here (embedding
gather, bias adds, concatenations). Same definition as the module: the feature prepended as step 0, one teacher-forcing
decision per step, batches shrinking over time, the top layer's argmax fed back on free-running steps. No dropout."""
import torch
import torch.nn.functional as Fn

from capnet import ops


def _chain(dec, l, mode, x):
    V, S, U, _ = dec._mods(l, mode)
    return torch.cat([ops.linear(ops.linear(ops.linear(x, V[k].weight, V[k].bias), S[k].weight, S[k].bias),
                                 U[k].weight, U[k].bias) for k in range(4)], 1)


def _wcat(dec, l, mode):
    _, _, _, W = dec._mods(l, mode)
    return torch.cat([w.weight for w in W], 0), torch.cat([w.bias for w in W], 0)


def stacked_step_forward(dec, captions, lengths, features, tf_mask, mode="factual"):
    """-> packed logits [sum(lengths), V] of `dec` (a StackedFactoredLSTM on the GPU, dropout off)."""
    assert not (dec.training and dec.dropout_p > 0), "the step-by-step engine runs without dropout"
    L, H = dec.num_layers, dec.hidden_size
    bs = ops.batch_sizes_from_lengths(lengths)
    steps = len(bs)
    tf_mask = [bool(v) for v in tf_mask[:steps]]
    Bn = captions.size(0)
    emb = Fn.embedding(captions, dec.B.weight)                        # B(captions)
    if features is not None:
        emb = torch.cat((features.unsqueeze(1), emb), 1)
    wcat = [_wcat(dec, l, mode) for l in range(L)]
    h = [torch.zeros(Bn, H, device=captions.device) for _ in range(L)]
    c = [torch.zeros(Bn, H, device=captions.device) for _ in range(L)]
    top = []                                                          # top-layer hiddens, step by step
    predicted = None
    t = 0
    while t < steps:
        # a run: consecutive teacher-forced steps, or ONE free-running step (its input needs the previous step's top)
        t1 = t + 1
        if tf_mask[t]:
            while t1 < steps and tf_mask[t1]:
                t1 += 1
            x = torch.cat([emb[:bs[u], u, :] for u in range(t, t1)], 0)
        else:
            if predicted is None:                                     # step 0 free-running: B(<start>)
                predicted = captions[:, 0]
            x = Fn.embedding(predicted[:bs[t]], dec.B.weight)         # no dropout on the feedback
        for l in range(L):
            pre = _chain(dec, l, mode, x)
            Wc, bc = wcat[l]
            outs, off = [], 0
            for u in range(t, t1):
                b = bs[u]
                g = pre[off:off + b] + ops.linear(h[l][:b], Wc, bc)
                h[l], c[l] = ops.lstm_cell(g, c[l][:b], 0)
                outs.append(h[l])
                off += b
            x = torch.cat(outs, 0) if len(outs) > 1 else outs[0]
        top.append(x)
        if t1 < steps and not tf_mask[t1]:
            with torch.no_grad():
                predicted = ops.argmax_rows(ops.linear(h[L - 1].detach(), dec.C.weight.detach(), dec.C.bias.detach())).long()
        t = t1
    hiddens = torch.cat(top, 0)
    return ops.linear(hiddens, dec.C.weight, dec.C.bias)
