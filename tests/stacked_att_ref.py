"""CPU restatement of capnet.stacked_att.StackedFactoredLSTMAtt's definition (PARITY UNPINNED: the reference ignores
num_layers, stylenet/model_att.py:81). It composes oracle.decoders_ref.attention_step / factored_step the way
oracle.decoders_ref.stacked_factored_lstm_forward composes the non-attention cell:

  * layer 0 is factored_att_forward's cell: attention and the f_beta gate read layer 0's own h^0_{t-1}, the input is
    [x_t | gate * awe], the initial state init_h / init_c(mean over pixels);
  * layer l > 0 is factored_step on h^{l-1}_t (times layer_masks[l] at its packed rows, if given) with the parameters
    V{l}_g, S{l}_{mode}g, U{l}_g, W{l}_g and the initial state init_h{l} / init_c{l}(mean over pixels);
  * the top layer feeds C (packed logits, argmax on free-running steps); alphas are layer 0's.
"""
import re

import torch
import torch.nn.functional as Fn

from oracle import decoders_ref as D


def layer_params(p, l):
    """Layer l's cell parameters under layer 0's names (V{l}_i -> V_i, S{l}_happy_i -> S_happy_i, ...)."""
    pat = re.compile(r"^([VSUW])%d_(.*)$" % l)
    out = {}
    for k, v in p.items():
        m = pat.match(k)
        if m:
            out["%s_%s" % (m.group(1), m.group(2))] = v
    return out


def _lin(p, name, x):
    return Fn.linear(x, p[name + ".weight"], p[name + ".bias"])


def stacked_factored_att_forward(p, captions, lengths, features, tf_mask, mode="factual", num_layers=2, drop_mask=None,
                                 layer_masks=None):
    """-> (packed logits [N, V], alphas [B, max(lengths), P]). drop_mask: optional [B, T, E] mask of the embeddings
    (oracle.decoders_ref._att_run's); layer_masks: optional {l: [N, H]} masks of layer l > 0's input by packed row."""
    B = captions.size(0)
    feat = features.reshape(B, -1, features.size(-1))
    P = feat.size(1)
    emb_w = p["B.weight"]
    embeddings = emb_w[captions]
    if drop_mask is not None:
        embeddings = embeddings * drop_mask
    layer_masks = layer_masks or {}
    bs = D.batch_sizes(lengths)
    mean = feat.mean(dim=1)
    tags = [""] + [str(l) for l in range(1, num_layers)]
    hs = [_lin(p, "init_h" + tag, mean) for tag in tags]
    cs = [_lin(p, "init_c" + tag, mean) for tag in tags]
    lp = [p] + [layer_params(p, l) for l in range(1, num_layers)]
    hiddens, alpha_list = [], []
    predicted = captions[:, 0:1]
    r0 = 0
    for i, b in enumerate(bs):
        h0 = hs[0][:b]
        awe, alpha = D.attention_step(p, D.MODE_ATT[mode], feat[:b], h0)
        awe = torch.sigmoid(_lin(p, "f_beta", h0)) * awe
        x = embeddings[:b, i, :] if tf_mask[i] else emb_w[predicted][:b, 0, :]
        x = torch.cat([x, awe], dim=1)
        for l in range(num_layers):
            if l in layer_masks:
                x = x * layer_masks[l][r0:r0 + b]
            hs[l], cs[l] = D.factored_step(lp[l], x, hs[l][:b], cs[l][:b], mode)
            x = hs[l]
        hiddens.append(x)
        alpha_list.append((b, alpha))
        predicted = _lin(p, "C", x).max(1)[1].unsqueeze(1)
        r0 += b
    alphas = torch.cat([torch.cat([a, torch.zeros(B - b, P, dtype=a.dtype)], 0).unsqueeze(1) for b, a in alpha_list], 1)
    return _lin(p, "C", torch.cat(hiddens, 0)), alphas


def greedy_decode(p, features, start_token, end_token, max_len, mode="factual", num_layers=2):
    """k = 1 decode of ONE image by the definition: feed back the argmax until <end> or max_len tokens
    (the sequence starts with start_token, as capnet.beam returns it). -> (tokens, smallest gap between the best and
    the second-best logit over the steps)."""
    feat = features.reshape(1, -1, features.size(-1))
    mean = feat.mean(dim=1)
    tags = [""] + [str(l) for l in range(1, num_layers)]
    hs = [_lin(p, "init_h" + tag, mean) for tag in tags]
    cs = [_lin(p, "init_c" + tag, mean) for tag in tags]
    lp = [p] + [layer_params(p, l) for l in range(1, num_layers)]
    seq = [int(start_token)]
    margin = float("inf")
    while len(seq) < max_len:
        awe, _ = D.attention_step(p, D.MODE_ATT[mode], feat, hs[0])
        awe = torch.sigmoid(_lin(p, "f_beta", hs[0])) * awe
        x = torch.cat([p["B.weight"][seq[-1]].unsqueeze(0), awe], dim=1)
        for l in range(num_layers):
            hs[l], cs[l] = D.factored_step(lp[l], x, hs[l], cs[l], mode)
            x = hs[l]
        logits = _lin(p, "C", x)[0]
        top2 = logits.topk(2).values
        margin = min(margin, float(top2[0] - top2[1]))
        seq.append(int(logits.argmax()))
        if seq[-1] == end_token:
            break
    return seq, margin
