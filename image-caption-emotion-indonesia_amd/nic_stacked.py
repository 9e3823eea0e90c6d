"""Stacked NIC decoders: DecoderRNN / DecoderRNNAtt whose num_layers is honoured.

PERF-ONLY for the attention stack, PARITY UNPINNED for both: the reference's NIC decoders accept `num_layers` and ignore
it (nic/model.py:35, nic/model_att.py:79), while its README reports a grid over `lstm_layers: 1, 2, 3`. The semantics
built here are SURVEY App. A-1's, as in capnet.stacked / capnet.stacked_att:

  * layer 0 is the reference's cell with the reference's parameter names (`embed`, `lstm`, `linear`; the attention stack
    adds `init_h`, `init_c`, `attention`, `f_beta`);
  * layer l > 0 is `lstm{l}` = LSTMCell(H, H) on dropout_l(h^{l-1}_t) at the same step (the mask capnet_rows_dropout
    draws for layer index l, in training only); in the attention stack it has its own initial state init_h{l} /
    init_c{l}, each Linear(C -> H) of the mean feature, and the attention and the f_beta gate query layer 0's own
    h^0_{t-1} (alphas are layer 0's); in the plain stack every layer starts at zero;
  * only the top layer feeds `linear` (the packed logits and the argmax fed back on free-running steps);
  * everything else is the reference loop: one teacher-forcing draw per step, shrinking batches, no dropout on the
    feedback embedding.
A stack of LSTMCells each reading the layer below at the same step is torch.nn.LSTM(num_layers=L): under teacher forcing
the plain stack is pinned to torch's own LSTM (tests/test_nic_stacked_gpu.py). Upper-layer parameters are registered
after all of the reference's, so num_layers = 1 has DecoderRNN's / DecoderRNNAtt's state_dict keys in their order, and
their outputs.

Training: DecoderRNN.forward / DecoderRNNAtt.forward with this class's upper layers (_upper_layers) -> ops.SeqFn /
ops.AttSeqFn -> capnet_seq_forward_stacked / capnet_att_seq_forward_stacked with cell = 1, one C call each way. A lone
upper-layer step of <= 16 rows in the attention stack is one launch of csrc/lstm_upper_step.hip's LSTM-cell instance
(CAPNET_NO_FUSED_UPPER_STEP=1: the composed step).

Decoding: the sample semantics of DecoderRNN / DecoderRNNAtt over the stack, no dropout. A beam step of the plain stack is
ONE capnet_stacked_decode_step_cell call (one launch per layer of csrc/lstm_decode_step.hip's LSTM-cell instance, layer 0
gathering its embedding rows by token id), then `linear` and capnet_beam_topk; the beam state is one [rows, 2L, H] tensor.
In the attention stack, layer 0's input is E + 2048 wide, beyond the kernel's K: its step stays composed (attention step,
then the LSTMCell products); the upper layers are one capnet_stacked_decode_step_cell call on h^0 with a [rows, 2(L-1), H]
state. CAPNET_NO_FUSED_DECODE_STEP=1 (read at every call) takes the composed step per layer, which also serves the shapes
the kernel does not take.
"""
import os

import torch

from . import ops
from ._lib import CapnetError
from .model import Linear
from .nic_model import DecoderRNN, LSTMCell
from .nic_model_att import DecoderRNNAtt
from .stacked import FUSED_DECODE_OFF

_GATE_BLOCKS = (0, 1, 3, 2)     # the kernel's gate blocks i, f, o, c~ from torch's i, f, g, o


def _pack_cell(cell, kin):
    """(wcat [4H, kin + H] = [weight_ih, zero columns up to kin | weight_hh], beff [4H] = bias_ih + bias_hh), gate
    blocks reordered for capnet_stacked_decode_step_cell."""
    H, n_in = cell.hidden_size, cell.input_size
    dev = cell.weight_ih.device
    wcat = torch.zeros((4 * H, kin + H), dtype=torch.float32, device=dev)
    beff = torch.empty(4 * H, dtype=torch.float32, device=dev)
    with torch.no_grad():
        for dst, src in enumerate(_GATE_BLOCKS):
            rows, srows = slice(dst * H, (dst + 1) * H), slice(src * H, (src + 1) * H)
            wcat[rows, :n_in].copy_(cell.weight_ih[srows])
            wcat[rows, kin:].copy_(cell.weight_hh[srows])
            torch.add(cell.bias_ih[srows], cell.bias_hh[srows], out=beff[rows])
    return wcat, beff


def _fused_decode(num_layers, E, H):
    return (os.environ.get(FUSED_DECODE_OFF, "")[:1] != "1" and num_layers <= 8 and ops.stacked_decode_supported(E, H))


def _stepper(cells, E, H):
    """step(x, tokens, state [rows, 2L, H]) -> (top h [rows, H], state') over `cells` (L LSTMCells, the first reading E
    columns): x is the embedding table when `tokens` is given, else the first cell's inputs. The fused step (weights
    packed here, once) unless CAPNET_NO_FUSED_DECODE_STEP=1 or the shape is one the kernel does not take."""
    if _fused_decode(len(cells), E, H):
        packed = [_pack_cell(c, (E + 15) // 16 * 16 if l == 0 else H) for l, c in enumerate(cells)]
        wcat, beff = [w for w, _ in packed], [b for _, b in packed]

        def step(x, tokens, state):
            return ops.stacked_decode_step(state, wcat, beff, x, tokens, cell=ops.CELL_LSTM)
    else:
        def step(x, tokens, state):
            if tokens is not None:
                x = ops.embedding(tokens, x)
            new = torch.empty_like(state)
            for l, c in enumerate(cells):
                h, cc = c(x, (state[:, 2 * l].contiguous(), state[:, 2 * l + 1].contiguous()))
                new[:, 2 * l], new[:, 2 * l + 1] = h, cc
                x = h
            return x, new
    return step


def _as_state(states):
    """A [rows, 2L, H] state from a tensor of that shape or a sequence of L (h, c) pairs."""
    if isinstance(states, torch.Tensor):
        return states
    return torch.stack([t for hc in states for t in hc], 1)


class StackedDecoderRNN(DecoderRNN):
    """DecoderRNN(embed_size, hidden_size, vocab_size, num_layers, ...) whose num_layers is honoured. Layer 0 is
    `lstm`, layer l > 0 `lstm{l}` = LSTMCell(H, H) (`lstm1.weight_ih` [4H, H], ...)."""

    _built = False

    def __init__(self, embed_size, hidden_size, vocab_size, num_layers, feature_size=2048, dropout=0.22,
                 max_seq_length=40):
        if num_layers < 1:
            raise CapnetError("num_layers must be >= 1")
        super(StackedDecoderRNN, self).__init__(embed_size, hidden_size, vocab_size, num_layers, feature_size, dropout,
                                                max_seq_length)
        self.num_layers = num_layers
        for l in range(1, num_layers):
            setattr(self, "lstm%d" % l, LSTMCell(hidden_size, hidden_size, bias=True))
        self._built = True
        self.reset_parameters()
        self.init_weights()

    def reset_parameters(self):
        if self._built:          # (once, over every layer's parameters)
            super(StackedDecoderRNN, self).reset_parameters()

    def init_weights(self):
        if self._built:
            super(StackedDecoderRNN, self).init_weights()

    def _cells(self):
        return [self.lstm] + [getattr(self, "lstm%d" % l) for l in range(1, self.num_layers)]

    def _upper_layers(self):
        weights = []
        for c in self._cells()[1:]:
            weights += [c.weight_ih, c.bias_ih, c.weight_hh, c.bias_hh]
        return self.num_layers, weights

    # ---- decoding -----------------------------------------------------------------------------
    def forward_step(self, embedded, states):
        """One decode step of the stack at inference (no dropout) on layer 0's input `embedded` [rows, E]. states: every
        layer's (h, c), as one tensor [rows, 2L, H] (slot 2l = h of layer l, 2l+1 = its c) or a sequence of L (h, c)
        pairs. Returns (the top layer's h [rows, H], the new states [rows, 2L, H]). Packs the weights on every call:
        sample() / sample_batch() pack once per decode."""
        with torch.no_grad():
            step = _stepper(self._cells(), self.embed_size, self.hidden_size)
            return step(embedded.detach().contiguous(), None, _as_state(states).detach().contiguous())

    def _beam_step(self):
        step, emb = _stepper(self._cells(), self.embed_size, self.hidden_size), self.embed.weight.detach()

        def step_fn(prev_words, state):
            top, st = step(emb, prev_words, state[0])
            return self.linear(top), (st,)
        return step_fn

    def sample(self, features, start_token, end_token, k=5):
        """Beam search, nic/model.py:117-207, over the stack: the image is NOT an input (`features` only fixes the
        device), every layer starts at zero, the first input is embed(<start>). Returns LongTensor [1, L]."""
        from .beam import beam_search
        dev = self.embed.weight.device
        with torch.no_grad():
            zeros = torch.zeros((k, 2 * self.num_layers, self.hidden_size), dtype=torch.float32, device=dev)
            return beam_search(self._beam_step(), (zeros,), self.vocab_size, start_token, end_token, k,
                               self.max_seq_length, dev)

    def sample_batch(self, features, start_token, end_token, k=5):
        """sample() for every row of `features` at once (capnet.beam.beam_search_batched). Returns a list of token lists,
        each equal to sample(features[i:i+1], ...)[0].tolist()."""
        from .beam import beam_search_batched
        dev = self.embed.weight.device
        n = features.size(0)
        with torch.no_grad():
            zeros = torch.zeros((n * k, 2 * self.num_layers, self.hidden_size), dtype=torch.float32, device=dev)
            return beam_search_batched(self._beam_step(), (zeros,), n, self.vocab_size, start_token, end_token, k,
                                       self.max_seq_length, dev)


class StackedDecoderRNNAtt(DecoderRNNAtt):
    """DecoderRNNAtt(attention_size, embed_size, hidden_size, vocab_size, num_layers, ...) whose num_layers is honoured.
    Layer 0 carries the reference's parameters; layer l > 0 has `init_h{l}`, `init_c{l}` (Linear(C -> H)) and `lstm{l}`
    = LSTMCell(H, H)."""

    _built = False

    def __init__(self, attention_size, embed_size, hidden_size, vocab_size, num_layers, feature_size=2048, dropout=0.22,
                 max_seq_length=40):
        if num_layers < 1:
            raise CapnetError("num_layers must be >= 1")
        super(StackedDecoderRNNAtt, self).__init__(attention_size, embed_size, hidden_size, vocab_size, num_layers,
                                                   feature_size, dropout, max_seq_length)
        self.num_layers = num_layers
        for l in range(1, num_layers):
            setattr(self, "init_h%d" % l, Linear(feature_size, hidden_size))
            setattr(self, "init_c%d" % l, Linear(feature_size, hidden_size))
            setattr(self, "lstm%d" % l, LSTMCell(hidden_size, hidden_size, bias=True))
        self._built = True
        self.reset_parameters()
        self.init_weights()

    def reset_parameters(self):
        if self._built:
            super(StackedDecoderRNNAtt, self).reset_parameters()

    def init_weights(self):
        if self._built:
            super(StackedDecoderRNNAtt, self).init_weights()

    def _upper_cells(self):
        return [getattr(self, "lstm%d" % l) for l in range(1, self.num_layers)]

    def _upper_layers(self):
        weights = []
        for l in range(1, self.num_layers):
            c = getattr(self, "lstm%d" % l)
            weights += [c.weight_ih, c.bias_ih, c.weight_hh, c.bias_hh]
            for m in (getattr(self, "init_h%d" % l), getattr(self, "init_c%d" % l)):
                weights += [m.weight, m.bias]
        return self.num_layers, weights

    def _upper_state(self, mean_features, rows=None):
        """[rows, 2(L-1), H]: init_h{l} / init_c{l}(mean feature) of every upper layer (rows: an index_select of the
        images' rows)."""
        hc = []
        for l in range(1, self.num_layers):
            hc += [getattr(self, "init_h%d" % l)(mean_features), getattr(self, "init_c%d" % l)(mean_features)]
        if not hc:
            return torch.zeros((mean_features.shape[0] if rows is None else rows.numel(), 0, self.hidden_size),
                               dtype=torch.float32, device=mean_features.device)
        st = torch.stack(hc, 1)
        return (st if rows is None else st.index_select(0, rows)).contiguous()

    def _upper_stepper(self):
        """step(h0 [rows, H], upper [rows, 2(L-1), H]) -> (top h, upper')."""
        if self.num_layers == 1:
            return lambda h0, upper: (h0, upper)
        step = _stepper(self._upper_cells(), self.hidden_size, self.hidden_size)
        return lambda h0, upper: step(h0.contiguous(), None, upper)

    def forward_step(self, embedded, states):
        """One decode step of the stack at inference (no dropout) on layer 0's input `embedded` [rows, E + C] (embedding
        | gated context). states: every layer's (h, c), as a sequence of L (h, c) pairs or as (h0, c0, upper) with upper
        [rows, 2(L-1), H] (slot 2(l-1) = h of layer l, 2l-1 = its c). Returns (the top layer's h [rows, H],
        (h0, c0, upper'))."""
        with torch.no_grad():
            if len(states) == 3 and isinstance(states[2], torch.Tensor) and states[2].dim() == 3:
                h0, c0, upper = states
            else:
                (h0, c0), rest = states[0], states[1:]
                upper = (_as_state(rest) if rest else
                         torch.zeros((h0.shape[0], 0, self.hidden_size), dtype=torch.float32, device=h0.device))
            h0, c0 = self.lstm(embedded.detach(), (h0.detach(), c0.detach()))
            top, upper = self._upper_stepper()(h0, upper.detach().contiguous())
            return top, (h0, c0, upper)

    def _att_beam_step(self, att1_of, feat_of, n_att):
        """step_fn over (h0, c0, upper, *extra): attention step (composed), layer 0's LSTMCell, the upper layers."""
        attention = self.attention
        E, dev = self.embed_size, self.embed.weight.device
        wz = torch.cat([attention.decoder_att.weight, self.f_beta.weight], 0).contiguous()
        bz = torch.cat([attention.decoder_att.bias, self.f_beta.bias], 0).contiguous()
        upper_step = self._upper_stepper()

        def step_fn(prev_words, state):
            h, c, upper = state[0], state[1], state[2]
            s_rows = h.shape[0]
            z = ops.linear(h, wz, bz).contiguous()
            xa = torch.empty((s_rows, E + n_att), dtype=torch.float32, device=dev)
            xa[:, :E] = self.embed(prev_words)
            ops.attention_step(att1_of(state, s_rows), feat_of(state, s_rows), z, self.attention_size,
                               attention.full_att.weight, attention.full_att.bias, xa=xa, xa_col=E)
            h, c = self.lstm(xa, (h, c))
            top, upper = upper_step(h, upper)
            return self.linear(top), (h, c, upper) + tuple(state[3:])
        return step_fn

    def sample(self, features, start_token, end_token, k=5):
        """Beam search with attention, nic/model_att.py:204-297, over the stack: the beam state is layer 0's (h, c) and
        the upper layers' [k, 2(L-1), H]. `features`: the encoder map of ONE image. Returns LongTensor [1, L]."""
        from .beam import beam_search
        dev = self.embed.weight.device
        A, Cdim = self.attention_size, features.size(-1)
        with torch.no_grad():
            feat1 = features.reshape(1, -1, Cdim).to(dev).contiguous()
            P = feat1.size(1)
            feat_k = feat1.expand(k, P, Cdim).contiguous()
            att1_k = self.attention.encoder_att(feat1[0]).reshape(1, P, A).expand(k, P, A).contiguous()
            h0, c0 = self.init_hidden_state(feat_k)
            upper = self._upper_state(feat_k.mean(dim=1))
            step_fn = self._att_beam_step(lambda st, r: att1_k[:r], lambda st, r: feat_k[:r], Cdim)
            return beam_search(step_fn, (h0, c0, upper), self.vocab_size, start_token, end_token, k,
                               self.max_seq_length, dev)

    def sample_batch(self, features, start_token, end_token, k=5):
        """sample() for every image of `features` at once (capnet.beam.beam_search_batched). Returns a list of token
        lists, each equal to sample(features[i:i+1], ...)[0].tolist()."""
        from .beam import beam_search_batched
        dev = self.embed.weight.device
        A, Cdim = self.attention_size, features.size(-1)
        n = features.size(0)
        with torch.no_grad():
            feat = features.reshape(n, -1, Cdim).to(dev).contiguous()
            P = feat.size(1)
            att1 = self.attention.encoder_att(feat.reshape(n * P, Cdim)).reshape(n, P, A).contiguous()
            h0, c0 = self.init_hidden_state(feat)
            img = torch.arange(n, device=dev).repeat_interleave(k)
            h0, c0 = h0.index_select(0, img).contiguous(), c0.index_select(0, img).contiguous()
            upper = self._upper_state(feat.mean(dim=1), rows=img)
            step_fn = self._att_beam_step(lambda st, r: att1.index_select(0, st[3]),
                                          lambda st, r: feat.index_select(0, st[3]), Cdim)
            return beam_search_batched(step_fn, (h0, c0, upper, img), n, self.vocab_size, start_token, end_token, k,
                                       self.max_seq_length, dev)
