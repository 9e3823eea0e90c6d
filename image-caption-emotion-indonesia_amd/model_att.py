"""Attention path on the MI355X kernels: EncoderCNN, Attention, DecoderFactoredLSTMAtt
(stylenet/model_att.py).

EncoderCNN(encoded_image_size=14): ResNet-152 children[:-2] under no_grad, AdaptiveAvgPool2d
to 14x14 (an exact 2x replication of the 7x7 map), permuted to NHWC. The trunk already produces
NHWC, so the permute costs nothing here.
"""
import sys

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import CapnetError, check, current_stream, ptr
from . import decode
from .decode import att_beam_start, att_beam_step, attend, beam_decode, factored_step, fold_factored
from .model import Dropout, Embedding, Linear, _Marker, _MODES, _TrunkRunner, _layer_mods, _resnet152_children, _seq_cfg


class EncoderCNN(nn.Module):

    def __init__(self, encoded_image_size=14):
        super(EncoderCNN, self).__init__()
        self.resnet = _resnet152_children(with_avgpool=False)
        self.adaptive_pool = _Marker()   # parameter-less, as nn.AdaptiveAvgPool2d
        self.encoded_image_size = encoded_image_size
        self._runner = [None]

    def _trunk(self):
        if self._runner[0] is None:
            self._runner[0] = _TrunkRunner(self.resnet)
        return self._runner[0]

    def forward(self, images, slot=0, defer_stats=False, balance_tails=True, graph=False):
        """slot / defer_stats: see _TrunkRunner.forward (capnet.train.TrunkPipeline); with
        defer_stats the result is (features, apply_running_stats or None)."""
        with torch.no_grad():
            res = self._trunk().forward(images, self.training, False, True, slot=slot,
                                        defer_stats=defer_stats and self.training,
                                        balance_tails=balance_tails, graph=graph)
            fmap = res[1]
            apply_fn = res[2] if len(res) > 2 else None
            out = self._pool(fmap)
        return (out, apply_fn) if defer_stats else out

    def zero_grad(self, set_to_none=True):
        """No trainable parameter and no gradient anywhere (the trunk runs under no_grad)."""
        return None

    def _pool(self, fmap):
        """AdaptiveAvgPool2d(encoded_image_size) of the 7x7 map: an exact replication."""
        b, side = fmap.shape[0], fmap.shape[1]
        out_side = self.encoded_image_size
        if out_side == side:
            return fmap
        if out_side % side != 0:
            raise CapnetError("encoded_image_size %d must be a multiple of the trunk's %d"
                              % (out_side, side))
        out = torch.empty((b, out_side, out_side, 2048), dtype=torch.float32, device=fmap.device)
        check(_lib.lib().capnet_adaptive_pool_replicate(ptr(fmap), ptr(out), b, side, out_side,
                                                        2048, current_stream()),
              "capnet_adaptive_pool_replicate")
        return out


class Attention(nn.Module):
    """stylenet/model_att.py:32-70 (parameter container + single-step forward)."""

    def __init__(self, encoder_dim, decoder_dim, attention_dim):
        super(Attention, self).__init__()
        self.encoder_att = Linear(encoder_dim, attention_dim)
        self.decoder_att = Linear(decoder_dim, attention_dim)
        self.full_att = Linear(attention_dim, 1)
        self.relu = _Marker()
        self.softmax = _Marker()

    def forward(self, encoder_out, decoder_hidden):
        """(attention-weighted encoding [s, C], alpha [s, P]) -- stylenet/model_att.py:51-70.
        Inference-only entry (no autograd); training goes through the fused sequence kernels."""
        return attend(self, encoder_out, decoder_hidden)


class DecoderFactoredLSTMAtt(nn.Module):
    """stylenet/model_att.py:73-426. `num_layers` is accepted and ignored, as in the reference.
    The image features carry no gradient (the attention encoder has no trainable parameter)."""

    def __init__(self,
                 attention_size,
                 embed_size,
                 hidden_size,
                 factored_size,
                 vocab_size,
                 num_layers,
                 feature_size=2048,
                 bias=True,
                 dropout=0.22,
                 max_seq_length=40):
        super(DecoderFactoredLSTMAtt, self).__init__()
        if not bias:
            raise CapnetError("DecoderFactoredLSTMAtt: bias=False is not supported by the HIP path")
        self.attention_size = attention_size
        self.feature_size = feature_size
        self.hidden_size = hidden_size
        self.factored_size = factored_size
        self.embed_size = embed_size
        self.vocab_size = vocab_size
        self.max_seq_length = max_seq_length
        # registration order follows stylenet/model_att.py:92-164 (state_dict order)
        self.init_h = Linear(feature_size, hidden_size)
        self.init_c = Linear(feature_size, hidden_size)
        self.dropout = Dropout(dropout)
        self.attention = Attention(feature_size, hidden_size, attention_size)
        self.B = Embedding(vocab_size, embed_size)
        self.f_beta = Linear(hidden_size, feature_size)
        self.sigmoid = _Marker()
        for g in "ifoc":
            setattr(self, "U_" + g, Linear(factored_size, hidden_size, bias=bias))
            setattr(self, "S_f" + g, Linear(factored_size, factored_size, bias=bias))
            setattr(self, "V_" + g, Linear(embed_size + feature_size, factored_size, bias=bias))
            setattr(self, "W_" + g, Linear(hidden_size, hidden_size, bias=bias))
        for emo in ("happy", "sad", "angry"):
            setattr(self, "attention_" + emo, Attention(feature_size, hidden_size, attention_size))
            for g in "ifoc":
                setattr(self, "S_%s_%s" % (emo, g), Linear(factored_size, factored_size, bias=bias))
        self.C = Linear(hidden_size, vocab_size, bias=bias)
        self.reset_parameters()
        self.init_weights()

    def reset_parameters(self):
        for p in self.parameters():
            if p.data.ndimension() >= 2:
                nn.init.xavier_uniform_(p.data)
            else:
                nn.init.zeros_(p.data)

    def init_weights(self):
        self.B.weight.data.uniform_(-0.1, 0.1)
        self.C.bias.data.fill_(0)
        self.C.weight.data.uniform_(-0.1, 0.1)

    def _mode_modules(self, mode):
        if mode == "factual":
            return self.attention, [getattr(self, "S_f" + g) for g in "ifoc"]
        if mode in _MODES:
            return (getattr(self, "attention_" + mode),
                    [getattr(self, "S_%s_%s" % (mode, g)) for g in "ifoc"])
        sys.stderr.write("mode name wrong!")      # the reference then fails with UnboundLocalError
        raise ValueError("unknown mode %r (expected one of %s)" % (mode, ", ".join(_MODES)))

    def _weights(self, mode):
        att, S = self._mode_modules(mode)
        V = [getattr(self, "V_" + g) for g in "ifoc"]
        U = [getattr(self, "U_" + g) for g in "ifoc"]
        W = [getattr(self, "W_" + g) for g in "ifoc"]
        out = []
        for grp in (V, S, U, W):
            out += [m.weight for m in grp]
            out += [m.bias for m in grp]
        for m in (self.init_h, self.init_c, att.encoder_att, att.decoder_att, att.full_att, self.f_beta):
            out += [m.weight, m.bias]
        return out

    def _upper_layers(self, mode):
        """(num_layers, the weights of the layers above layer 0) for the sequence call. One layer here: num_layers is
        ignored, as in the reference (capnet.stacked_att stacks)."""
        return 1, []

    def init_hidden_state(self, features):
        """h0, c0 = init_h / init_c (mean over pixels) -- stylenet/model_att.py:185-194."""
        mean_features = features.mean(dim=1)
        return self.init_h(mean_features), self.init_c(mean_features)

    def forward_step(self, embedded, states, mode):
        """One factored-LSTM step on [embedding | gated context] -- model_att.py:196-236."""
        h_t, c_t = states
        _, S = self._mode_modules(mode)
        V = [getattr(self, "V_" + g) for g in "ifoc"]
        U = [getattr(self, "U_" + g) for g in "ifoc"]
        W = [getattr(self, "W_" + g) for g in "ifoc"]
        h_t, c_t = factored_step(V, S, U, W, embedded, h_t, c_t)
        return h_t, (h_t, c_t)

    def _upper_beam(self, feat, img, mode):
        """(the beam state's entries after layer 0's (h0, c0), att_beam_step's `upper`). One layer here."""
        return (), None

    def _fold(self, mode):
        """[(wcat, beff)] of every layer for capnet_att_decode_step: the factored chains folded (capnet.decode.fold_factored;
        layer 0's reads E + C columns). One layer here."""
        self._mode_modules(mode)          # the reference's message and error for an unknown mode
        return [fold_factored(*_layer_mods(self, "", mode))]

    @torch.no_grad()
    def _beam(self, features, n, k, mode, one_call=False):
        """(step_fn, initial state) of a beam search over one image (n None) or n images: the state is layer 0's (h, c),
        then what _upper_beam adds, then (n images) every beam's image index. one_call: the AttStack of the search as one C
        call rides on step_fn where the shape is supported (capnet.decode.att_stack: only then is anything folded); the
        steps of step_fn itself stay the composed chain."""
        attention, _ = self._mode_modules(mode)
        feat, att1_of, feat_of, h0, c0, img, maps = att_beam_start(self, attention, features, n, k)
        state, upper = self._upper_beam(feat, img, mode)
        step_fn = att_beam_step(attention, self.f_beta, self.B, lambda xa, hc: self.forward_step(xa, hc, mode=mode)[1],
                                self.C, att1_of, feat_of, features.size(-1), upper)
        if one_call:
            decode.att_stack(step_fn, self, ops.CELL_FACTORED, lambda: self._fold(mode), attention, self.B, self.C,
                             maps, k, (h0, c0) + state)
        return step_fn, (h0, c0) + state + (() if img is None else (img,))

    def sample(self, features, start_token, end_token, k=5, factual_limit=-1, mode='factual', on_device=False, poll_every=0,
               one_call=False, return_alphas=False, constraints=None, diversity=None, nbest=False, length_penalty=0.0):
        """Beam search with attention, stylenet/model_att.py:307-426. `features`: the encoder map
        of ONE image ([1, S, S, C] or [1, P, C]). Returns LongTensor [1, L].
        on_device / poll_every: capnet.decode.beam_decode's (the bookkeeping on the device, same sequences).
        one_call: the whole search in one C call (capnet_att_beam_decode: the k beams of an image on one read of its maps,
        the chain folded); on_device=True for a shape that call does not take. Same sequences.
        return_alphas: -> (ids [1, L], alphas float32 [L - 1, P]), row e - 1 the map of the mode's Attention module that
        preceded word e (capnet.decode.beam_decode: recorded by the one-call search, replayed on every other route).
        constraints: a capnet.beam.Constraints -- no n-gram twice, no <end> before min_words words, no banned word --
        kept inside the search on whichever route runs (capnet.decode.beam_decode); the scores stay the model's own.
        diversity: a capnet.beam.Diversity -- the k beams as groups that pay for the words earlier groups chose at the same
        step, for several different captions of one image (capnet.decode.beam_decode); the scores stay the model's own.
        nbest / length_penalty: capnet.decode.beam_decode's -- every completed hypothesis as a (tokens, score) pair, best
        first, in place of the one caption. With return_alphas, every hypothesis's own maps beside the list."""
        return beam_decode(self, *self._beam(features, None, k, mode, one_call), None, k, start_token, end_token, on_device, poll_every,
                           one_call, return_alphas, nbest, length_penalty, constraints, diversity)

    def sample_random(self, features, start_token, end_token, samples=1, temperature=1.0, top_k=0, seed=None, mode='factual',
                      top_p=1.0, device=False, greedy=False, exclude=None):
        """`samples` captions per image of `features` ([n, S, S, C] or [n, P, C]), DRAWN from the decoder's distribution
        softmax(logits / temperature) (top_k > 0: renormalised over the top_k best words of every step;
        top_p < 1: over the nucleus) instead of searched
        for: a list of n lists of `samples` (tokens, logprob) pairs, tokens = [start, w_1 .. w_j] cut after the first
        end_token (none: all max_seq_length words), logprob the float sum of the kept words' log-probabilities under the
        distribution sampled from. seed: an integer makes the call a pure function of its arguments; None draws a 63-bit
        seed from torch's CPU generator (torch.manual_seed). One C call (capnet_att_sample_decode: an image's maps read once
        per step for all its samples) or the composed loop, the same lists: capnet.decode.sample_random.
        greedy=True: every image's pairs are followed by one more, its greedy caption (the argmax of every step), decoded as
        one more row of the same call; the first `samples` pairs are those of the call without it.
        device=True: (the lists, ids, logp), the decode's raw rows [n samples, max_seq_length] left on the device
        (capnet.decode.sample_random_device).
        exclude (a capnet.beam.Constraints without forced words): what no caption may draw -- a repeated n-gram, <end> within
        min_words, banned words -- excluded words being not pickable and logprob that of the distribution renormalised over
        the allowed words (capnet.decode.sample_random_device); None: the call as it was."""
        n = features.size(0)
        return decode.sample_random(self, *self._beam(features, n, int(samples) + bool(greedy), mode, True), n, samples, start_token, end_token,
                                    temperature, top_k, seed, top_p, device, greedy, exclude)

    def score_captions(self, features, captions, mode='factual'):
        """float32 [len(captions)] on the device: the model's log-probability of every caption [start, w_1 .. w_j] given its
        image, summed over w_1 .. w_j (<end> too where present), in the caller's order. captions: a flat list of token lists,
        caption r on row r of `features` ([n, S, S, C] or [n, P, C]), or the nested list sample_random returns, list i on image
        i (the logprob of a (tokens, logprob) pair is ignored). Under no_grad, dropout following self.training:
        capnet.decode.score_captions."""
        return decode.score_captions(self, features, captions, mode)

    def sample_batch(self, features, start_token, end_token, k=5, factual_limit=-1, mode='factual', on_device=False,
                     poll_every=0, one_call=False, return_alphas=False, constraints=None, diversity=None, nbest=False, length_penalty=0.0):
        """sample() for every image of `features` ([n, S, S, C] or [n, P, C]) at once: the reference's evaluator
        (stylenet/evaluator.py:63-120) decodes its test images one sample() call at a time; here all live beams of all
        images take their decoder step together (capnet.beam.beam_search_batched). Returns a list of token lists; with
        return_alphas, (the n token lists, n float32 [len - 1, P] tensors) as sample()."""
        n = features.size(0)
        return beam_decode(self, *self._beam(features, n, k, mode, one_call), n, k, start_token, end_token, on_device, poll_every, one_call,
                           return_alphas, nbest, length_penalty, constraints, diversity)

    def _style_layers(self):
        """The layers sample_styles folds: one here (capnet.stacked_att: num_layers)."""
        return 1

    def sample_styles(self, features, start_token, end_token, k=5, modes=_MODES, poll_every=0):
        """sample_batch(one_call=True) in every style of `modes` at once -> {mode: [n token lists]}, each list equal to
        sample_batch(features, ..., mode=mode, one_call=True): ONE search over len(modes) x n x k rows
        (capnet_att_beam_decode_groups). A mode brings its folded chains and its Attention module (encoder_att(feat) per
        mode, [decoder_att; f_beta], full_att); the maps, the embedding, f_beta, the projection and the initial state are
        shared, the maps read in place by every mode. modes: a non-empty sequence of distinct mode names (an unknown one
        as in sample()). A shape capnet_att_beam_decode does not take, an embedding width that is no multiple of 4 or
        CAPNET_NO_FUSED_DECODE_STEP=1: the modes are decoded one sample_batch(one_call=True) after the other.
        poll_every: capnet.decode.beam_decode's. (With the attention maps: sample_styles_alphas.)"""
        return self._styles(features, start_token, end_token, k, modes, poll_every, False)

    def sample_styles_alphas(self, features, start_token, end_token, k=5, modes=_MODES, poll_every=0):
        """sample_styles with return_alphas=True -> ({mode: [n token lists]}, {mode: [n float32 [len - 1, P] tensors]}): the
        lists are sample_styles', and each mode's maps are those of sample_batch(mode=mode, one_call=True,
        return_alphas=True), from the mode's own Attention module, recorded by the one grouped search -- where the happy
        caption looked next to where the angry one did. (A method of its own: sample_styles' parameters are pinned.)"""
        return self._styles(features, start_token, end_token, k, modes, poll_every, True)

    def sample_styles_nbest(self, features, start_token, end_token, k=5, modes=_MODES, poll_every=0, length_penalty=0.0,
                            return_alphas=False):
        """sample_styles with nbest=True -> {mode: [n lists of (tokens, score)]}, each equal to sample_batch(mode=mode,
        one_call=True, nbest=True, length_penalty=length_penalty); with return_alphas, followed by {mode: [n lists of float32
        [len - 1, P] tensors]}, every hypothesis's own maps. The one grouped search, its completed lists read by
        capnet_beam_nbest. (A method of its own: sample_styles' parameters are pinned.)"""
        return self._styles(features, start_token, end_token, k, modes, poll_every, return_alphas, True, length_penalty)

    def _styles(self, features, start_token, end_token, k, modes, poll_every, return_alphas, nbest=False, length_penalty=0.0):
        modes = decode.check_styles(modes, self._mode_modules)
        return decode.att_styles(self, lambda l, m: _layer_mods(self, "" if l == 0 else str(l), m), self._style_layers(),
                                 features, k, start_token, end_token, modes, poll_every,
                                 lambda m: self.sample_batch(features, start_token, end_token, k=k, mode=m, one_call=True,
                                                             poll_every=poll_every, return_alphas=return_alphas, nbest=nbest,
                                                             length_penalty=length_penalty),
                                 return_alphas, nbest, length_penalty)

    def forward(self,
                captions,
                lengths,
                features,
                teacher_forcing_ratio=0.8,
                mode='factual',
                tf_mask=None):
        """Returns (outputs [N, V], alphas [B, max(lengths), P])."""
        batch_size = captions.size(0)
        features = features.reshape(batch_size, -1, features.size(-1))
        batch_sizes = ops.batch_sizes_from_lengths(lengths)
        weights = self._weights(mode)
        num_layers, upper = self._upper_layers(mode)
        cfg = _seq_cfg(self, batch_sizes, self.dropout.p, tf_mask, teacher_forcing_ratio, num_layers=num_layers,
                       factored_size=self.factored_size, attention_size=self.attention_size)
        hiddens, alphas = ops.AttSeqFn.apply(cfg, captions, features.detach(), self.B.weight, self.C.weight, self.C.bias,
                                             *weights, *upper)
        return self.C(hiddens), alphas
