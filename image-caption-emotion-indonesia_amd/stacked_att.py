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

Engine: the whole recurrence is ONE C call each way (StackedAttSeqFn -> capnet_att_seq_forward_stacked /
capnet_att_seq_backward_stacked, csrc/decoder_att_seq.cpp). A lone step of an upper layer with <= 16 rows (every
free-running step, at 12 rows per GPU) is one launch of csrc/lstm_upper_step.hip; CAPNET_NO_FUSED_UPPER_STEP=1 takes
the composed path (rows_dropout, three chain products, the fused recurrent step) instead. capnet.parallel is
parameter-generic: data-parallel training needs nothing more.
"""
import torch
import torch.nn as nn

from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import CapnetError, check, current_stream, int_array, ptr
from .model import Linear, _MODES, _dropout_seed, _resolve_tf_mask
from .model_att import DecoderFactoredLSTMAtt

_S_PREFIX = {"factual": "f", "happy": "happy_", "sad": "sad_", "angry": "angry_"}


class StackedAttSeqFn(torch.autograd.Function):
    """(top-layer hiddens [N, H], alphas [B, steps, P]) of the stacked attention recurrence.
    weights: layer 0's 44 tensors (DecoderAttSeqFn's order), then 36 per upper layer: V w x4, V b x4, S w x4, S b x4,
    U w x4, U b x4, W w x4, W b x4, init_h{l} w, b, init_c{l} w, b. `features` gets no gradient (frozen trunk)."""

    @staticmethod
    def forward(ctx, cfg, captions, features, emb, Cw, Cb, *weights):
        ops._need_cuda(captions, features, emb, Cw, Cb, *weights)
        nl = cfg["num_layers"]
        if len(weights) != 44 + 36 * (nl - 1):
            raise CapnetError("stacked attention decoder takes 44 + 36 (num_layers - 1) weight tensors")
        captions = captions.contiguous()
        if captions.dtype != torch.int64:
            raise CapnetError("captions must be int64")
        dev = emb.device
        bs, tf = cfg["batch_sizes"], cfg["tf_mask"]
        B, T = captions.shape
        V, E = emb.shape
        H, A, F = cfg["hidden_size"], cfg["attention_size"], cfg["factored_size"]
        features = features.contiguous()
        if features.dim() != 3 or features.shape[0] != B:
            raise CapnetError("features must be [batch, pixels, feature_size]")
        P, Cf = features.shape[1], features.shape[2]
        N = sum(bs)
        if len(tf) != len(bs) or bs[0] != B:
            raise CapnetError("attention decoder: batch_sizes / tf_mask do not match the batch")
        dims = [B, T, len(bs), N, E, F, H, V, A, P, Cf, ops.CELL_FACTORED]
        ws = [w.contiguous() for w in weights]
        emb_c, Cw_c, Cb_c = emb.contiguous(), Cw.contiguous(), Cb.contiguous()
        cdims = int_array(dims)
        L = _lib.lib()
        saved = [torch.empty(L.capnet_att_stacked_saved_floats(cdims, l), dtype=torch.float32, device=dev) for l in range(nl)]
        saved_i = [torch.empty(L.capnet_att_stacked_saved_ints(cdims, l), dtype=torch.int32, device=dev) for l in range(nl)]
        scratch = torch.empty(L.capnet_att_stacked_fwd_scratch_floats(cdims, nl), dtype=torch.float32, device=dev)
        # upper layers: B leading rows hold the initial state
        hid = [torch.empty((N if l == 0 else B + N, H), dtype=torch.float32, device=dev) for l in range(nl)]
        alphas = torch.empty((B, len(bs), P), dtype=torch.float32, device=dev)
        tfm = (_lib.C.c_ubyte * len(tf))(*[1 if x else 0 for x in tf])
        check(L.capnet_att_seq_forward_stacked(cdims, nl, int_array(bs), tfm, ptr(captions), ptr(features), ptr(emb_c),
                                               _lib.ptr_array(ws), ptr(Cw_c), ptr(Cb_c), float(cfg["dropout"]),
                                               int(cfg["seed"]), int(cfg["training"]), _lib.ptr_array(saved),
                                               _lib.ptr_array(saved_i), ptr(scratch), _lib.ptr_array(hid), ptr(alphas),
                                               ptr(ops.err_flag(dev)), current_stream()),
              "capnet_att_seq_forward_stacked")
        ctx.cfg, ctx.dims = cfg, dims
        ctx.save_for_backward(*(saved + saved_i + hid), features, *ws)
        return (hid[0] if nl == 1 else hid[-1][B:]), alphas

    @staticmethod
    @once_differentiable
    def backward(ctx, d_hiddens, d_alphas):
        cfg, dims = ctx.cfg, ctx.dims
        nl = cfg["num_layers"]
        t = ctx.saved_tensors
        saved, saved_i, hid = list(t[:nl]), list(t[nl:2 * nl]), list(t[2 * nl:3 * nl])
        features, ws = t[3 * nl], list(t[3 * nl + 1:])
        B, T, steps, N, E, F, H, V, A, P, Cf, _ = dims
        dev = features.device
        L = _lib.lib()
        cdims = int_array(dims)
        scratch = torch.empty(L.capnet_att_stacked_bwd_scratch_floats(cdims, nl), dtype=torch.float32, device=dev)

        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)

        d_hiddens = d_hiddens.contiguous() if d_hiddens is not None else torch.zeros((N, H), dtype=torch.float32, device=dev)
        d_alphas = d_alphas.contiguous() if d_alphas is not None else None
        ZW, XW = 4 * H + A + Cf, E + Cf
        dV, dbV, dS, dbS, dU = new(4 * F, XW), new(4 * F), new(4, F, F), new(4 * F), new(4, H, F)
        dWz, dbz = new(ZW, H), new(ZW)
        dWe, dbe, dwf, dbf = new(A, Cf), new(A), new(1, A), new(1)
        dWih, dbih, dWic, dbic = new(H, Cf), new(H), new(H, Cf), new(H)
        dEmb = new(V, E)
        grads = [dV, dbV, dS, dbS, dU, dWz, dbz, dWe, dbe, dwf, dbf, dWih, dbih, dWic, dbic, dEmb]
        upper = []
        for _ in range(1, nl):
            g = [new(4 * F, H), new(4 * F), new(4, F, F), new(4 * F), new(4, H, F), new(4 * H), new(4 * H, H),
                 new(H, Cf), new(H), new(H, Cf), new(H)]
            grads += g
            upper.append(g)
        dh_work = [new(N, H) for _ in range(nl - 1)]
        check(L.capnet_att_seq_backward_stacked(cdims, nl, int_array(cfg["batch_sizes"]), ptr(d_hiddens), ptr(d_alphas),
                                                _lib.ptr_array(hid), ptr(features), _lib.ptr_array(ws),
                                                _lib.ptr_array(saved), _lib.ptr_array(saved_i), ptr(scratch),
                                                _lib.ptr_array(dh_work) if dh_work else None, _lib.ptr_array(grads),
                                                float(cfg["dropout"]), int(cfg["seed"]), int(cfg["training"]),
                                                current_stream()), "capnet_att_seq_backward_stacked")
        wg = ([dV[g * F:(g + 1) * F] for g in range(4)] + [dbV[g * F:(g + 1) * F] for g in range(4)] +
              [dS[g] for g in range(4)] + [dbS[g * F:(g + 1) * F] for g in range(4)] + [dU[g] for g in range(4)] +
              [dbz[g * H:(g + 1) * H] for g in range(4)] + [dWz[g * H:(g + 1) * H] for g in range(4)] +
              [dbz[g * H:(g + 1) * H].clone() for g in range(4)] +
              [dWih, dbih, dWic, dbic, dWe, dbe, dWz[4 * H:4 * H + A], dbz[4 * H:4 * H + A], dwf, dbf,
               dWz[4 * H + A:], dbz[4 * H + A:]])
        for uV, ubV, uS, ubS, uU, ubUW, uW, uih, ubih, uic, ubic in upper:
            wg += ([uV[g * F:(g + 1) * F] for g in range(4)] + [ubV[g * F:(g + 1) * F] for g in range(4)] +
                   [uS[g] for g in range(4)] + [ubS[g * F:(g + 1) * F] for g in range(4)] + [uU[g] for g in range(4)] +
                   [ubUW[g * H:(g + 1) * H] for g in range(4)] + [uW[g * H:(g + 1) * H] for g in range(4)] +
                   [ubUW[g * H:(g + 1) * H].clone() for g in range(4)] + [uih, ubih, uic, ubic])
        # cfg, captions, features, emb, Cw, Cb, *weights
        return (None, None, None, dEmb, None, None) + tuple(wg)


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

    # ---- training -----------------------------------------------------------------------------------
    def forward(self, captions, lengths, features, teacher_forcing_ratio=0.8, mode='factual', tf_mask=None):
        """Returns (outputs [N, V], alphas [B, max(lengths), P]) -- layer 0's alphas."""
        batch_size = captions.size(0)
        features = features.reshape(batch_size, -1, features.size(-1))
        batch_sizes = ops.batch_sizes_from_lengths(lengths)
        weights = self._weights(mode)
        for l in range(1, self.num_layers):
            weights += self._upper_weights(l, mode)
        cfg = {
            "batch_sizes": batch_sizes,
            "tf_mask": _resolve_tf_mask(tf_mask, len(batch_sizes), teacher_forcing_ratio),
            "hidden_size": self.hidden_size,
            "factored_size": self.factored_size,
            "attention_size": self.attention_size,
            "num_layers": self.num_layers,
            "dropout": self.dropout.p if self.training else 0.0,
            "seed": _dropout_seed(self.training, self.dropout.p),
            "training": self.training,
        }
        hiddens, alphas = StackedAttSeqFn.apply(cfg, captions, features.detach(), self.B.weight, self.C.weight,
                                                self.C.bias, *weights)
        return self.C(hiddens), alphas
