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
"""
import torch

from . import ops
from ._lib import CapnetError
from .model import Linear, _MODES
from .model_att import DecoderFactoredLSTMAtt

_S_PREFIX = {"factual": "f", "happy": "happy_", "sad": "sad_", "angry": "angry_"}


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
        s = _S_PREFIX[mode]
        return ([getattr(self, "V%d_%s" % (l, g)) for g in "ifoc"],
                [getattr(self, "S%d_%s%s" % (l, s, g)) for g in "ifoc"],
                [getattr(self, "U%d_%s" % (l, g)) for g in "ifoc"],
                [getattr(self, "W%d_%s" % (l, g)) for g in "ifoc"])

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
        V, S, U, W = self._upper_mods(l, mode)
        pre = torch.cat([U[k](S[k](V[k](x))) + W[k](h) for k in range(4)], 1)
        return ops.lstm_pointwise(pre, c, ops.CELL_FACTORED)

    def _stack_state(self, mean_features, h0, c0, rows=None):
        state = [h0, c0]
        for l in range(1, self.num_layers):
            h, c = self._upper_init(l, mean_features)
            if rows is not None:
                h, c = h.index_select(0, rows).contiguous(), c.index_select(0, rows).contiguous()
            state += [h, c]
        return state

    def _step_upper_layers(self, hidden, state, mode):
        new = []
        x = hidden
        for l in range(1, self.num_layers):
            h, c = self._upper_step(l, x, state[2 * l], state[2 * l + 1], mode)
            new += [h, c]
            x = h
        return x, new

    # ---- decoding ---------------------------------------------------------------------------------
    def sample(self, features, start_token, end_token, k=5, factual_limit=-1, mode='factual'):
        """Beam search with attention (stylenet/model_att.py:307-426) over the stack: the beam state is every layer's
        (h, c). `features`: the encoder map of ONE image. Returns LongTensor [1, L]."""
        from .beam import beam_search
        dev = self.B.weight.device
        attention, _ = self._mode_modules(mode)
        E, A, Cdim = self.embed_size, self.attention_size, features.size(-1)
        with torch.no_grad():
            feat1 = features.reshape(1, -1, Cdim).to(dev).contiguous()
            P = feat1.size(1)
            feat_k = feat1.expand(k, P, Cdim).contiguous()
            att1_k = attention.encoder_att(feat1[0]).reshape(1, P, A).expand(k, P, A).contiguous()
            h0, c0 = self.init_hidden_state(feat_k)
            state0 = self._stack_state(feat_k.mean(dim=1), h0, c0)
            wz = torch.cat([attention.decoder_att.weight, self.f_beta.weight], 0).contiguous()
            bz = torch.cat([attention.decoder_att.bias, self.f_beta.bias], 0).contiguous()

            def step_fn(prev_words, state):
                h, c = state[0], state[1]
                s_rows = h.shape[0]
                z = ops.linear(h, wz, bz).contiguous()
                xa = torch.empty((s_rows, E + Cdim), dtype=torch.float32, device=dev)
                xa[:, :E] = self.B(prev_words)
                ops.attention_step(att1_k[:s_rows], feat_k[:s_rows], z, A, attention.full_att.weight,
                                   attention.full_att.bias, xa=xa, xa_col=E)
                hidden, (h, c) = self.forward_step(xa, (h, c), mode=mode)
                top, upper = self._step_upper_layers(hidden, state, mode)
                return self.C(top), tuple([h, c] + upper)

            return beam_search(step_fn, tuple(state0), self.vocab_size, start_token, end_token, k,
                               self.max_seq_length, dev)

    def sample_batch(self, features, start_token, end_token, k=5, factual_limit=-1, mode='factual'):
        """sample() for every image of `features` at once (capnet.beam.beam_search_batched), as
        DecoderFactoredLSTMAtt.sample_batch. Returns a list of token lists."""
        from .beam import beam_search_batched
        dev = self.B.weight.device
        attention, _ = self._mode_modules(mode)
        E, A, Cdim = self.embed_size, self.attention_size, features.size(-1)
        n = features.size(0)
        with torch.no_grad():
            feat = features.reshape(n, -1, Cdim).to(dev).contiguous()
            P = feat.size(1)
            att1 = attention.encoder_att(feat.reshape(n * P, Cdim)).reshape(n, P, A).contiguous()
            h0, c0 = self.init_hidden_state(feat)
            img = torch.arange(n, device=dev).repeat_interleave(k)
            h0, c0 = h0.index_select(0, img).contiguous(), c0.index_select(0, img).contiguous()
            state0 = self._stack_state(feat.mean(dim=1), h0, c0, rows=img)
            wz = torch.cat([attention.decoder_att.weight, self.f_beta.weight], 0).contiguous()
            bz = torch.cat([attention.decoder_att.bias, self.f_beta.bias], 0).contiguous()

            def step_fn(prev_words, state):
                h, c, im = state[0], state[1], state[-1]
                s_rows = h.shape[0]
                z = ops.linear(h, wz, bz).contiguous()
                xa = torch.empty((s_rows, E + Cdim), dtype=torch.float32, device=dev)
                xa[:, :E] = self.B(prev_words)
                ops.attention_step(att1.index_select(0, im), feat.index_select(0, im), z, A, attention.full_att.weight,
                                   attention.full_att.bias, xa=xa, xa_col=E)
                hidden, (h, c) = self.forward_step(xa, (h, c), mode=mode)
                top, upper = self._step_upper_layers(hidden, state, mode)
                return self.C(top), tuple([h, c] + upper + [im])

            return beam_search_batched(step_fn, tuple(state0 + [img]), n, self.vocab_size, start_token, end_token, k,
                                       self.max_seq_length, dev)
