"""CPU restatement of capnet.nic_stacked (StackedDecoderRNN, StackedDecoderRNNAtt). TEST INFRASTRUCTURE. PARITY
UNPINNED with more than one layer: the reference ignores num_layers (nic/model.py:35, nic/model_att.py:79).

  * layer 0 is oracle.decoders_ref.lstmcell_step with the reference's parameters; layer l > 0 is lstmcell_step on
    h^{l-1}_t (times layer_masks[l] at its packed rows, if given) with the parameters lstm{l}.*;
  * the plain stack starts every layer at zero and runs oracle.decoders_ref._run's loop; the attention stack runs
    _att_run's loop with layer 0's attention and f_beta gate on h^0_{t-1} and init_h{l} / init_c{l}(mean) per layer;
  * only the top layer feeds `linear`; the beam searches are oracle.beam_ref._beam with DecoderRNN.sample's /
    DecoderRNNAtt.sample's semantics over the stack (no dropout).
"""
import re

import torch
import torch.nn.functional as Fn

from oracle import beam_ref, decoders_ref as D


def layer_params(p, l):
    """Layer l's cell parameters under layer 0's names (lstm{l}.weight_ih -> lstm.weight_ih, ...)."""
    if l == 0:
        return p
    pat = re.compile(r"^lstm%d\.(.*)$" % l)
    return {"lstm." + m.group(1): v for k, v in p.items() for m in [pat.match(k)] if m}


def _lin(p, name, x):
    return Fn.linear(x, p[name + ".weight"], p[name + ".bias"])


def stacked_step(p, x, hs, cs, num_layers):
    """One inference step of the stack -> (top h, [h per layer], [c per layer])."""
    hs2, cs2 = [], []
    for l in range(num_layers):
        h, c = D.lstmcell_step(layer_params(p, l), x, hs[l], cs[l])
        hs2.append(h)
        cs2.append(c)
        x = h
    return x, hs2, cs2


def stacked_lstm_forward(p, captions, lengths, features, tf_mask, num_layers, drop_mask=None, layer_masks=None):
    """StackedDecoderRNN.forward -> packed logits [N, V]. drop_mask: [B, T, E] mask of the embeddings; layer_masks:
    {l: [N, H]} masks of layer l > 0's input by packed row."""
    H = p["lstm.weight_hh"].shape[1]
    B = captions.size(0)
    emb_w = p["embed.weight"]
    embeddings = emb_w[captions]
    if drop_mask is not None:
        embeddings = embeddings * drop_mask
    if features is not None:
        embeddings = torch.cat((features.unsqueeze(1), embeddings), 1)
    layer_masks = layer_masks or {}
    hs = [torch.zeros(B, H, dtype=emb_w.dtype) for _ in range(num_layers)]
    cs = [torch.zeros(B, H, dtype=emb_w.dtype) for _ in range(num_layers)]
    hiddens, predicted, r0 = [], captions[:, 0:1], 0
    for i, b in enumerate(D.batch_sizes(lengths)):
        x = embeddings[:b, i, :] if tf_mask[i] else emb_w[predicted][:b, 0, :]
        for l in range(num_layers):
            if l in layer_masks:
                x = x * layer_masks[l][r0:r0 + b]
            hs[l], cs[l] = D.lstmcell_step(layer_params(p, l), x, hs[l][:b], cs[l][:b])
            x = hs[l]
        hiddens.append(x)
        predicted = _lin(p, "linear", x).max(1)[1].unsqueeze(1)
        r0 += b
    return _lin(p, "linear", torch.cat(hiddens, 0))


def stacked_lstm_att_forward(p, captions, lengths, features, tf_mask, num_layers, drop_mask=None, layer_masks=None):
    """StackedDecoderRNNAtt.forward -> (packed logits [N, V], alphas [B, max(lengths), P])."""
    B = captions.size(0)
    feat = features.reshape(B, -1, features.size(-1))
    P = feat.size(1)
    emb_w = p["embed.weight"]
    embeddings = emb_w[captions]
    if drop_mask is not None:
        embeddings = embeddings * drop_mask
    layer_masks = layer_masks or {}
    mean = feat.mean(dim=1)
    tags = [""] + [str(l) for l in range(1, num_layers)]
    hs = [_lin(p, "init_h" + t, mean) for t in tags]
    cs = [_lin(p, "init_c" + t, mean) for t in tags]
    hiddens, alpha_list, predicted, r0 = [], [], captions[:, 0:1], 0
    for i, b in enumerate(D.batch_sizes(lengths)):
        h0 = hs[0][:b]
        awe, alpha = D.attention_step(p, "attention", feat[:b], h0)
        awe = torch.sigmoid(_lin(p, "f_beta", h0)) * awe
        x = embeddings[:b, i, :] if tf_mask[i] else emb_w[predicted][:b, 0, :]
        x = torch.cat([x, awe], dim=1)
        for l in range(num_layers):
            if l in layer_masks:
                x = x * layer_masks[l][r0:r0 + b]
            hs[l], cs[l] = D.lstmcell_step(layer_params(p, l), x, hs[l][:b], cs[l][:b])
            x = hs[l]
        hiddens.append(x)
        alpha_list.append((b, alpha))
        predicted = _lin(p, "linear", x).max(1)[1].unsqueeze(1)
        r0 += b
    alphas = torch.cat([torch.cat([a, torch.zeros(B - b, P, dtype=a.dtype)], 0).unsqueeze(1) for b, a in alpha_list], 1)
    return _lin(p, "linear", torch.cat(hiddens, 0)), alphas


# ---- beam search ------------------------------------------------------------------------------------------------
def _plain_step_fn(p, num_layers):
    def step_fn(prev_words, state):
        L = num_layers
        x = p["embed.weight"][prev_words].squeeze(1)
        top, hs, cs = stacked_step(p, x, list(state[:L]), list(state[L:2 * L]), L)
        return _lin(p, "linear", top), tuple(hs + cs) + tuple(state[2 * L:])
    return step_fn


def _att_step_fn(p, num_layers):
    def step_fn(prev_words, state):
        L = num_layers
        hs, cs, f = list(state[:L]), list(state[L:2 * L]), state[2 * L]
        awe, _ = D.attention_step(p, "attention", f, hs[0])
        awe = torch.sigmoid(_lin(p, "f_beta", hs[0])) * awe
        x = torch.cat([p["embed.weight"][prev_words].squeeze(1), awe], dim=1)
        top, hs, cs = stacked_step(p, x, hs, cs, L)
        return _lin(p, "linear", top), tuple(hs + cs) + (f,)
    return step_fn


def _initial(p, num_layers, k, features=None):
    """(step_fn, initial state) of the plain stack (features None) or of the attention stack on ONE image."""
    if features is None:
        H = p["lstm.weight_hh"].shape[1]
        z = tuple(torch.zeros(k, H, dtype=p["lstm.weight_hh"].dtype) for _ in range(2 * num_layers))
        return _plain_step_fn(p, num_layers), z
    feat = features.reshape(1, -1, features.size(-1))
    feat = feat.expand(k, feat.size(1), feat.size(2))
    mean = feat.mean(dim=1)
    tags = [""] + [str(l) for l in range(1, num_layers)]
    hs = tuple(_lin(p, "init_h" + t, mean) for t in tags)
    cs = tuple(_lin(p, "init_c" + t, mean) for t in tags)
    return _att_step_fn(p, num_layers), hs + cs + (feat,)


def sample_stacked(p, num_layers, start_token, end_token, k=5, features=None, max_seq_length=40):
    """StackedDecoderRNN.sample (features None) / StackedDecoderRNNAtt.sample restated: LongTensor [1, L]."""
    step_fn, state = _initial(p, num_layers, k, features)
    return beam_ref._beam(step_fn, state, p["linear.weight"].shape[0], start_token, end_token, k, max_seq_length)


def greedy_path(p, num_layers, start_token, steps, features=None):
    """The first `steps` tokens of the restatement's greedy decode (no end token): tests take their end token from it."""
    step_fn, state = _initial(p, num_layers, 1, features)
    words, out = torch.LongTensor([[start_token]]), []
    for _ in range(steps):
        logits, state = step_fn(words, state)
        words = logits.argmax(1, keepdim=True)
        out.append(int(words))
    return out


def beam_margin(p, num_layers, start_token, end_token, k=5, features=None, max_seq_length=40):
    """The smallest gap, over the steps of sample_stacked's beam search, between the k-th and the (k+1)-th best
    candidate score, and between the best and the second-best completed sequence (as tests/stacked_decode_ref.py)."""
    V = p["linear.weight"].shape[0]
    step_fn, state = _initial(p, num_layers, k, features)
    words = torch.LongTensor([[start_token]] * k)
    top = torch.zeros(k, 1, dtype=p["linear.weight"].dtype)
    margin, done, step = float("inf"), [], 1
    while True:
        out, state = step_fn(words, state)
        scores = top.expand_as(out) + Fn.log_softmax(out, dim=1)
        flat = scores[0] if step == 1 else scores.view(-1)
        best, idx = flat.topk(min(k + 1, flat.numel()), 0, True, True)
        if best.numel() > k:
            margin = min(margin, float(best[k - 1] - best[k]))
        best, idx = best[:k], idx[:k]
        prev, nxt = idx // V, idx % V
        keep = [i for i, w in enumerate(nxt.tolist()) if w != end_token]
        done += [float(best[i]) for i in range(k) if i not in keep]
        k = len(keep)
        if k == 0 or step > max_seq_length:
            break
        state = tuple(s[prev[keep]] for s in state)
        top = best[keep].unsqueeze(1)
        words = nxt[keep].unsqueeze(1)
        step += 1
    done.sort(reverse=True)
    if len(done) > 1:
        margin = min(margin, done[0] - done[1])
    return margin


def decode_params(module, seed, emb_scale=1.0, out_scale=8.0):
    """fp64 parameters for `module`'s state_dict: matrices U(-a, a) with a = sqrt(3 / fan_in), biases U(-0.05, 0.05),
    embed U(-emb_scale, emb_scale), linear scaled by out_scale (well-separated beam candidates)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in module.state_dict().items():
        if v.dim() > 1:
            a = 3.0 ** 0.5 / v.shape[1] ** 0.5
            if k == "embed.weight":
                a = emb_scale
            elif k == "linear.weight":
                a *= out_scale
        else:
            a = 0.05
        out[k] = (torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1) * a
    return out
