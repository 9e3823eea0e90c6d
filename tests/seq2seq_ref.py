"""CPU restatement of capnet.seq2seq (EncoderRNN, DecoderRNN, Seq2Seq) in plain torch, any dtype (the tests use fp64).
TEST INFRASTRUCTURE. Pinned to the reference by tests/test_seq2seq_cpu.py against tests/golden/seq2seq_tiny.npz (written by
tools/gen_golden_seq2seq.py from the reference's own classes); used where that fp32 fixture cannot reach: full sizes,
dropout on, argmax margins.

Parameters are one dict under Seq2Seq's state_dict names ("encoder.lstm.weight_ih_l0", ...); `prefix` picks the module
("encoder", "decoder_happy", ...). tf_mask is the list of per-step `random.random() < teacher_forcing_ratio` outcomes.
drop_mask: [B, T, E] multiplied into embed(tokens) (the layout of oracle.decoders_ref / oracle.dropout_ref.embedding_mask).
Nothing is dropped between the layers (nn.LSTM without dropout=); layer_masks ({l: [N, H]} by packed row) exists only for
the negative control that drops there.
"""
import torch
import torch.nn.functional as Fn

EMOTIONS = ("happy", "sad", "angry")


def batch_sizes(lengths):
    return [sum(1 for l in lengths if l > t) for t in range(lengths[0])]


def _cell(p, prefix, l, x, h, c):
    g = (Fn.linear(x, p["%s.lstm.weight_ih_l%d" % (prefix, l)], p["%s.lstm.bias_ih_l%d" % (prefix, l)]) +
         Fn.linear(h, p["%s.lstm.weight_hh_l%d" % (prefix, l)], p["%s.lstm.bias_hh_l%d" % (prefix, l)]))
    i, f, gg, o = g.chunk(4, 1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def _logits(p, prefix, h):
    return Fn.linear(h, p[prefix + ".linear.weight"], p[prefix + ".linear.bias"])


def step(p, prefix, num_layers, x, hs, cs, masks=None):
    """One step of the stack on x [b, E]: (top h, [h per layer], [c per layer])."""
    hs2, cs2 = [], []
    for l in range(num_layers):
        if masks is not None and l in masks:
            x = x * masks[l]
        h, c = _cell(p, prefix, l, x, hs[l], cs[l])
        hs2.append(h)
        cs2.append(c)
        x = h
    return x, hs2, cs2


def rnn_forward(p, prefix, num_layers, features, tokens, lengths, tf_mask, drop_mask=None, layer_masks=None,
                margins=None):
    """EncoderRNN.forward (features [B, E]) / DecoderRNN.forward (features None) -> (packed logits [N, V], (h, c)
    [num_layers, b_last, H]). margins: a list that receives the top-1 / top-2 logit gap of every fed-back row."""
    emb_w = p[prefix + ".embed.weight"]
    H = p[prefix + ".lstm.weight_hh_l0"].shape[1]
    B = tokens.size(0)
    embeddings = emb_w[tokens]
    if drop_mask is not None:
        embeddings = embeddings * drop_mask
    if features is not None:
        embeddings = torch.cat((features.unsqueeze(1), embeddings), 1)
    hs = [torch.zeros(B, H, dtype=emb_w.dtype) for _ in range(num_layers)]
    cs = [torch.zeros(B, H, dtype=emb_w.dtype) for _ in range(num_layers)]
    hiddens, predicted, r0 = [], tokens[:, 0], 0
    bs = batch_sizes(lengths)
    for i, b in enumerate(bs):
        x = embeddings[:b, i, :] if tf_mask[i] else emb_w[predicted[:b]]
        masks = None if not layer_masks else {l: m[r0:r0 + b] for l, m in layer_masks.items()}
        top, hs, cs = step(p, prefix, num_layers, x, [h[:b] for h in hs], [c[:b] for c in cs], masks)
        hiddens.append(top)
        out = _logits(p, prefix, top)
        predicted = out.max(1)[1]
        if margins is not None and i + 1 < len(bs) and not tf_mask[i + 1]:
            top2 = out[:bs[i + 1]].detach().topk(2, 1)[0]
            margins.append(float((top2[:, 0] - top2[:, 1]).min()))
        r0 += b
    return _logits(p, prefix, torch.cat(hiddens, 0)), (torch.stack(hs), torch.stack(cs))


def seq2seq_forward(p, num_layers, features, src, dst, tf_mask, mode, drop_mask=None, layer_masks=None, margins=None):
    """Seq2Seq.forward -> packed logits. tf_mask: the draws of the encoder's steps followed, in an emotion mode, by the
    decoder's (the encoder always runs first and consumes its draws; its outputs are discarded in an emotion mode).
    drop_mask / layer_masks belong to the module whose logits are returned."""
    n_src = src[1][0]
    if mode == "factual":
        return rnn_forward(p, "encoder", num_layers, features, src[0], src[1], tf_mask[:n_src], drop_mask, layer_masks,
                           margins)[0]
    assert mode in EMOTIONS
    return rnn_forward(p, "decoder_" + mode, num_layers, None, dst[0], dst[1], tf_mask[n_src:], drop_mask, layer_masks,
                       margins)[0]


def greedy(p, prefix, num_layers, steps, features=None, start_token=None, states=None, rows=None):
    """EncoderRNN.sample (features) / DecoderRNN.sample (start_token broadcast to the states' rows) ->
    (ids [rows, steps], (h, c) [num_layers, rows, H], the smallest top-1 / top-2 logit gap over every row and step, the
    largest |logit| met)."""
    emb_w = p[prefix + ".embed.weight"]
    H = p[prefix + ".lstm.weight_hh_l0"].shape[1]
    if features is not None:
        rows = features.size(0)
    elif states is not None and states[0] is not None:
        rows = states[0].size(1)
    rows = rows or 1
    zeros = torch.zeros(num_layers, rows, H, dtype=emb_w.dtype)
    h, c = (zeros, zeros) if states is None else (zeros if s is None else s.to(emb_w.dtype) for s in states)
    hs, cs = list(h), list(c)
    x = features if features is not None else emb_w[torch.full((rows,), int(start_token), dtype=torch.long)]
    ids, margin, scale = [], float("inf"), 0.0
    for _ in range(steps):
        top, hs, cs = step(p, prefix, num_layers, x, hs, cs)
        out = _logits(p, prefix, top)
        scale = max(scale, float(out.abs().max()))
        if out.size(1) > 1:
            top2 = out.topk(2, 1)[0]
            margin = min(margin, float((top2[:, 0] - top2[:, 1]).min()))
        predicted = out.max(1)[1]
        ids.append(predicted)
        x = emb_w[predicted]
    return torch.stack(ids, 1), (torch.stack(hs), torch.stack(cs)), margin, scale


def seq2seq_sample(p, num_layers, steps, features, start_token, mode):
    """Seq2Seq.sample -> (ids, the smallest logit gap met on the way (the encoder's pass included), the largest |logit|,
    the encoder's final (h, c))."""
    ids, states, margin, scale = greedy(p, "encoder", num_layers, steps, features=features)
    if mode == "factual":
        return ids, margin, scale, states
    ids, _, m2, s2 = greedy(p, "decoder_" + mode, num_layers, steps, start_token=start_token, states=states)
    return ids, min(margin, m2), max(scale, s2), states


def make_params(module_or_shapes, seed, out_scale=1.0, lstm_scale=1.0):
    """fp64 parameters with torch's constructor distributions for a Seq2Seq state_dict (or {name: shape}): embed N(0, 1),
    everything else U(-1/sqrt(H), 1/sqrt(H)); linear.weight times out_scale, the LSTM weight matrices times lstm_scale
    (wider top-1 / top-2 gaps for the greedy tests)."""
    shapes = (module_or_shapes if isinstance(module_or_shapes, dict)
              else {k: tuple(v.shape) for k, v in module_or_shapes.state_dict().items()})
    g = torch.Generator().manual_seed(seed)
    out = {}
    H = [s for k, s in shapes.items() if k.endswith("lstm.weight_hh_l0")][0][1]
    for k, s in shapes.items():
        if k.endswith("embed.weight"):
            out[k] = torch.randn(s, generator=g, dtype=torch.float64)
            continue
        v = (torch.rand(s, generator=g, dtype=torch.float64) * 2 - 1) / H ** 0.5
        if k.endswith("linear.weight"):
            v = v * out_scale
        elif ".lstm.weight" in k:
            v = v * lstm_scale
        out[k] = v
    return out
