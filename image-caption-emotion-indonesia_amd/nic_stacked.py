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
the kernel does not take. The stepper, the packing and the attention beam step are capnet.decode's (cell_stepper,
pack_cell, att_beam_step); sample / sample_batch are the base classes' over this module's _beam / _upper_beam.
"""
import torch

from . import ops
from ._lib import CapnetError
from .decode import as_state, cell_stepper, plain_stack
from .decode import pack_cell as _pack_cell  # noqa: F401  (the packing's name while it lived here; the tests pack by it)
from .model import Linear
from .nic_model import DecoderRNN, LSTMCell
from .nic_model_att import DecoderRNNAtt


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
            step = cell_stepper(self._cells(), self.embed_size, self.hidden_size)
            return step(embedded.detach().contiguous(), None, as_state(states).detach().contiguous())

    @torch.no_grad()
    def _beam(self, rows, plain=False):
        """(step_fn, the zero state (one tensor [rows, 2L, H],)) of a beam search: the weights are packed here, once (and
        serve one_call=True as they are: `plain` asks for nothing more)."""
        emb = self.embed.weight.detach()
        zeros = torch.zeros((rows, 2 * self.num_layers, self.hidden_size), dtype=torch.float32, device=emb.device)
        step = cell_stepper(self._cells(), self.embed_size, self.hidden_size)

        def step_fn(prev_words, state):
            top, st = step(emb, prev_words, state[0])
            return self.linear(top), (st,)
        return plain_stack(step_fn, step.packed, ops.CELL_LSTM, emb, self.linear), (zeros,)

    # sample / sample_batch: DecoderRNN's, over this _beam (the image is NOT an input, every layer starts at zero)


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

    def _cells(self):
        return [self.lstm] + self._upper_cells()

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
        step = cell_stepper(self._upper_cells(), self.hidden_size, self.hidden_size)
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
                upper = (as_state(rest) if rest else
                         torch.zeros((h0.shape[0], 0, self.hidden_size), dtype=torch.float32, device=h0.device))
            h0, c0 = self.lstm(embedded.detach(), (h0.detach(), c0.detach()))
            top, upper = self._upper_stepper()(h0, upper.detach().contiguous())
            return top, (h0, c0, upper)

    def _beam_upper(self):
        """capnet.decode.att_beam_step's `upper`: the upper layers' step on the entries after layer 0's (h, c)."""
        step = self._upper_stepper()

        def upper(h, rest):
            top, up = step(h, rest[0])
            return top, (up,)
        return upper

    def _upper_beam(self, feat, img):
        """The beam state is layer 0's (h, c) and the upper layers' one tensor [rows, 2(L-1), H]."""
        return (self._upper_state(feat.mean(dim=1), rows=img),), self._beam_upper

    # sample / sample_batch: DecoderRNNAtt's, over _beam with this _upper_beam
