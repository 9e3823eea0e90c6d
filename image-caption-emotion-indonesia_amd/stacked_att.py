"""Stacked attention decoder for BASELINE configs[3] (the attention path with a 2-layer LSTM-512).

PERF-ONLY, PARITY UNPINNED. The reference's DecoderFactoredLSTMAtt accepts `num_layers` and ignores it
(stylenet/model_att.py:81): there is no stacking code to be equal to. The definition built here follows SURVEY App. A-1
and capnet.stacked:

  * layer 0 is DecoderFactoredLSTMAtt unchanged: same parameters and names; attention and the f_beta gate are queried
    with layer 0's own h^0_{t-1}; its input is [x_t | gate * awe]; its initial state is init_h / init_c(mean over pixels);
  * layer l > 0 is the factored cell on dropout(h^{l-1}_t) at the same step, with its own parameters V{l}_g: Linear(H -> F),
    S{l}_f{g}, S{l}_{happy,sad,angry}_{g}, U{l}_g, W{l}_g and its own initial state init_h{l} / init_c{l}, each
    Linear(C -> H) of the same mean feature. The dropout mask between layers is the one capnet_rows_dropout draws for
    layer index l, in training only;
  * only the top layer feeds C: the packed logits and the argmax fed back on free-running steps;
  * everything else is stylenet/model_att.py:238-305: one teacher-forcing draw per step, batches shrinking over time,
    no dropout on the feedback embedding, and alphas [B, max(lengths), P] are layer 0's (ops.attention_loss and
    train_step_att apply unchanged).

Layer 0's parameters are registered exactly as DecoderFactoredLSTMAtt's and layer l's follow, so num_layers = 1 has
DecoderFactoredLSTMAtt's state_dict keys in their order.

Why the attention query is layer 0's state and not the top layer's: the attention then stays inside layer 0, and a run of
teacher-forced steps goes up the stack run by run (layer 0 steps through the run, then each upper layer takes the run's
rows in one persistent launch). A query from the top layer would serialise every layer at every step.

Engine: the whole recurrence is ONE C call each way: DecoderFactoredLSTMAtt.forward with this class's upper layers
(_upper_layers) -> ops.AttSeqFn -> capnet_att_seq_forward_stacked / capnet_att_seq_backward_stacked
(csrc/decoder_att_seq.cpp). A lone step of an upper layer with <= 16 rows (every free-running step, at 12 rows per GPU)
is one launch of csrc/lstm_upper_step.hip; CAPNET_NO_FUSED_UPPER_STEP=1 takes the composed path (rows_dropout, three
chain products, the fused recurrent step) instead. capnet.parallel is parameter-generic: data-parallel training needs
nothing more.

Decoding: DecoderFactoredLSTMAtt's sample / sample_batch (capnet.decode's attention beam step) with this class's upper
layers (_upper_beam): the beam state is every layer's (h, c), and each upper layer takes the composed step
(capnet.decode.factored_step). one_call=True: the whole search in one C call on every layer's folded chain (_fold).
"""
from ._lib import CapnetError
from .decode import factored_step, fold_factored
from .model import Linear, _MODES, _layer_mods
from .model_att import DecoderFactoredLSTMAtt


class StackedFactoredLSTMAtt(DecoderFactoredLSTMAtt):
    """DecoderFactoredLSTMAtt(attention_size, embed_size, hidden_size, factored_size, vocab_size, num_layers, ...) whose
    num_layers is honoured (the module docstring has the definition). Layer 0 carries the reference's parameter names,
    layer l > 0 the same names with the layer number in front of the gate (`U1_i`, `S1_fi`, `S1_happy_i`, `V1_i`, `W1_i`)
    and its own `init_h1` / `init_c1`."""

    _built = False

    def __init__(self, attention_size, embed_size, hidden_size, factored_size, vocab_size, num_layers, feature_size=2048,
                 bias=True, dropout=0.22, max_seq_length=40):
        if num_layers < 1:
            raise CapnetError("num_layers must be >= 1")
        super(StackedFactoredLSTMAtt, self).__init__(attention_size, embed_size, hidden_size, factored_size, vocab_size,
                                                     num_layers, feature_size, bias, dropout, max_seq_length)
        self.num_layers = num_layers
        for l in range(1, num_layers):
            setattr(self, "init_h%d" % l, Linear(feature_size, hidden_size))
            setattr(self, "init_c%d" % l, Linear(feature_size, hidden_size))
            for g in "ifoc":
                setattr(self, "U%d_%s" % (l, g), Linear(factored_size, hidden_size))
                setattr(self, "S%d_f%s" % (l, g), Linear(factored_size, factored_size))
                setattr(self, "V%d_%s" % (l, g), Linear(hidden_size, factored_size))
                setattr(self, "W%d_%s" % (l, g), Linear(hidden_size, hidden_size))
            for emo in ("happy", "sad", "angry"):
                for g in "ifoc":
                    setattr(self, "S%d_%s_%s" % (l, emo, g), Linear(factored_size, factored_size))
        self._built = True
        self.reset_parameters()
        self.init_weights()

    def reset_parameters(self):
        if self._built:          # (once, over every layer's parameters)
            super(StackedFactoredLSTMAtt, self).reset_parameters()

    def init_weights(self):
        if self._built:
            super(StackedFactoredLSTMAtt, self).init_weights()

    # ---- upper layers ---------------------------------------------------------------------------
    def _upper_mods(self, l, mode):
        if mode not in _MODES:
            self._mode_modules(mode)          # the reference's message and error
        return _layer_mods(self, str(l), mode)

    def _upper_weights(self, l, mode):
        out = []
        for grp in self._upper_mods(l, mode):
            out += [m.weight for m in grp]
            out += [m.bias for m in grp]
        for m in (getattr(self, "init_h%d" % l), getattr(self, "init_c%d" % l)):
            out += [m.weight, m.bias]
        return out

    def _upper_layers(self, mode):
        weights = []
        for l in range(1, self.num_layers):
            weights += self._upper_weights(l, mode)
        return self.num_layers, weights

    def _upper_init(self, l, mean_features):
        return getattr(self, "init_h%d" % l)(mean_features), getattr(self, "init_c%d" % l)(mean_features)

    def _upper_step(self, l, x, h, c, mode):
        """One step of layer l > 0 on its input x (no dropout: inference) -> (h, c)."""
        return factored_step(*self._upper_mods(l, mode), x, h, c)

    # ---- decoding ---------------------------------------------------------------------------------
    def _fold(self, mode):
        """DecoderFactoredLSTMAtt._fold with the upper layers' chains folded as well (H -> H cells)."""
        return super(StackedFactoredLSTMAtt, self)._fold(mode) + [fold_factored(*self._upper_mods(l, mode))
                                                                  for l in range(1, self.num_layers)]

    def _style_layers(self):
        return self.num_layers

    def _upper_beam(self, feat, img, mode):
        """The beam state is every layer's (h, c): the upper layers' init_h{l} / init_c{l}(mean feature), tiled by image
        index, and their step on the entries after layer 0's."""
        mean_features, state = feat.mean(dim=1), ()
        for l in range(1, self.num_layers):
            h, c = self._upper_init(l, mean_features)
            if img is not None:
                h, c = h.index_select(0, img).contiguous(), c.index_select(0, img).contiguous()
            state += (h, c)

        def step(hidden, rest):
            new, x = [], hidden
            for l in range(1, self.num_layers):
                h, c = self._upper_step(l, x, rest[2 * l - 2], rest[2 * l - 1], mode)
                new += [h, c]
                x = h
            return x, new
        return state, lambda: step
