"""Stacked FactoredLSTM decoder for BASELINE configs[3] / [4] ("2-layer", "3-layer").

PERF-ONLY, PARITY UNPINNED. The reference advertises `lstm_layers: 1, 2, 3` (README.md:24, BLEU rows :63,:66) but its
decoders accept `num_layers` and ignore it (stylenet/model.py:37, model_att.py:81): there is no stacking code in the
tree to be equal to. The semantics built here are SURVEY.md App. A-1's, modelled on the only stacking the tree has
(seq2seq/model.py:45-49, nn.LSTM(num_layers) = each layer reads the layer below at the same time step):

  * layer 0 is the reference's cell with the reference's parameter names (B, U_g, S_{mode}g, V_g: Linear(E -> F), W_g);
  * layer l > 0 is the same factored cell on the hidden state of the layer below at the same step, with its own
    V{l}_g: Linear(H -> F), S{l}_{mode}g, U{l}_g, W{l}_g, and dropout between the layers;
  * only the top layer feeds C (the packed logits and, on free-running steps, the argmax that is fed back);
  * everything else -- feature prepended as step 0, one teacher-forcing draw per step, shrinking batches, the feedback
    embedding without dropout -- is stylenet/model.py:157-196.

With num_layers = 1 it is DecoderFactoredLSTM's function (tests/test_stacked_gpu.py); the numbers for more layers are
checked against the same definition restated on the CPU (oracle/decoders_ref.py: stacked_factored_lstm_forward).

Training: the whole stacked recurrence is ONE C call each way (ops.SeqFn -> capnet_seq_forward_stacked /
capnet_seq_backward_stacked, csrc/decoder_seq.cpp: the single-layer driver with a layer loop inside; embedding gather,
dropout masks, chains, persistent runs, BPTT are all kernels of the library).

Decoding (forward_step / sample / sample_batch) runs the same stack at inference: no dropout anywhere, so each gate's
chain folds into one matrix, Weff_g = U_g S_g V_g (H x in), and beff_g = U_g (S_g bV_g + bS_g) + bU_g + bW_g. The fold is
done once per sample / sample_batch call, per layer, for the requested mode, with the library's GEMMs. A beam step is then
one launch per layer (capnet_stacked_decode_step, csrc/lstm_decode_step.hip: [x | h] . [Weff | W]^T + beff and the gates;
layer 0 gathers its embedding rows by token id itself), plus C and capnet_beam_topk. The beam state is ONE tensor
[rows, 2L, H] (slot 2l = h of layer l, 2l+1 = its c), so re-ordering the beams is one index_select per step.
CAPNET_NO_FUSED_DECODE_STEP=1 (read at every call) takes the composed step instead -- per layer the V, S, U and W
products and the pointwise cell, unfolded -- which is also the path for shapes the kernel does not take. That choice and
the beam-search front end are capnet.decode's (stack_stepper, beam_decode); this class adds its fold and its composed step."""
import sys

import torch
import torch.nn as nn

from . import ops
from ._lib import CapnetError
from .decode import (as_state, beam_decode, check_styles, factored_step, fold_factored, plain_stack, plain_styles, sample_random, score_captions,
                     stack_stepper)
from .model import Embedding as _Embedding, Linear as _Linear, _layer_mods, _seq_cfg

MODES = ("factual", "happy", "sad", "angry")


def _check_mode(mode):
    if mode not in MODES:
        sys.stderr.write("mode name wrong!")
        raise ValueError("unknown mode %r" % (mode,))


class StackedFactoredLSTM(nn.Module):
    """DecoderFactoredLSTM(embed_size, hidden_size, factored_size, vocab_size, num_layers, ...) whose num_layers is
    honoured. Layer 0 carries the reference's parameter names, layer l > 0 the same names with the layer number in
    front of the gate (`U1_i`, `S1_fi`, `S1_happy_i`, `V1_i`, `W1_i`, ...)."""

    def __init__(self, embed_size, hidden_size, factored_size, vocab_size, num_layers, feature_size=2048, bias=True,
                 dropout=0.22, max_seq_length=40):
        super().__init__()
        if not bias:
            raise CapnetError("bias=False is not supported")
        if num_layers < 1:
            raise CapnetError("num_layers must be >= 1")
        self.embed_size, self.hidden_size, self.factored_size = embed_size, hidden_size, factored_size
        self.vocab_size, self.num_layers = vocab_size, num_layers
        self.feature_size, self.max_seq_length = feature_size, max_seq_length
        self.dropout_p = dropout
        self.B = _Embedding(vocab_size, embed_size)
        for l in range(num_layers):
            tag = "" if l == 0 else str(l)
            for g in "ifoc":
                setattr(self, "U%s_%s" % (tag, g), _Linear(factored_size, hidden_size))
                setattr(self, "S%s_f%s" % (tag, g), _Linear(factored_size, factored_size))
                setattr(self, "V%s_%s" % (tag, g), _Linear(embed_size if l == 0 else hidden_size, factored_size))
                setattr(self, "W%s_%s" % (tag, g), _Linear(hidden_size, hidden_size))
        for l in range(num_layers):
            tag = "" if l == 0 else str(l)
            for emo in ("happy", "sad", "angry"):
                for g in "ifoc":
                    setattr(self, "S%s_%s_%s" % (tag, emo, g), _Linear(factored_size, factored_size))
        self.C = _Linear(hidden_size, vocab_size)
        self.reset_parameters()

    def reset_parameters(self):
        """stylenet/model.py:99-113: xavier on matrices, zeros on vectors, then B and C.weight U(-0.1, 0.1)."""
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
            else:
                nn.init.zeros_(p)
        self.B.weight.data.uniform_(-0.1, 0.1)
        self.C.weight.data.uniform_(-0.1, 0.1)

    # ---- one layer's pieces -------------------------------------------------------------------
    def _mods(self, l, mode):
        return _layer_mods(self, "" if l == 0 else str(l), mode)

    # ---- decoding -----------------------------------------------------------------------------
    def _fold(self, mode):
        """[(wcat, beff)] per layer for capnet_stacked_decode_step: wcat [4H, kin + H] = [U_g S_g V_g, zero columns up
        to kin | W_g] in gate blocks i, f, o, c~ (kin: the layer's input width rounded up to 16), beff [4H] =
        U_g (S_g bV_g + bS_g) + bU_g + bW_g (capnet.decode.fold_factored, layer by layer)."""
        return [fold_factored(*self._mods(l, mode)) for l in range(self.num_layers)]

    def _composed_step(self, x, state, mode):
        """One inference step of the stack, unfolded: per layer the V, S, U and W products and the pointwise cell."""
        new = torch.empty_like(state)
        for l in range(self.num_layers):
            h, c = factored_step(*self._mods(l, mode), x, state[:, 2 * l].contiguous(), state[:, 2 * l + 1])
            new[:, 2 * l], new[:, 2 * l + 1] = h, c
            x = h
        return x, new

    def _decode_stepper(self, mode):
        """step(x, tokens, state [rows, 2L, H]) -> (top h [rows, H], state'): x is the embedding table when `tokens` is
        given, else layer 0's inputs. The fused step (weights folded here, once) unless CAPNET_NO_FUSED_DECODE_STEP=1
        or the shape is one the kernel does not take."""
        return stack_stepper(self.num_layers, self.embed_size, self.hidden_size, ops.CELL_FACTORED,
                             lambda: self._fold(mode), lambda x, state: self._composed_step(x, state, mode))

    def forward_step(self, embedded, states, mode):
        """One decode step of the stack at inference (no dropout) on layer 0's input `embedded` [rows, E]. states: every
        layer's (h, c), as one tensor [rows, 2L, H] (slot 2l = h of layer l, 2l+1 = its c) or a sequence of L (h, c)
        pairs. Returns (the top layer's h [rows, H], the new states [rows, 2L, H]). Folds the weights on every call:
        sample() / sample_batch() fold once per decode."""
        _check_mode(mode)
        with torch.no_grad():
            return self._decode_stepper(mode)(embedded.detach(), None, as_state(states).detach())

    @torch.no_grad()
    def _beam(self, rows, mode, plain=False):
        """(step_fn, the zero state (one tensor [rows, 2L, H],)) of a beam search: the weights are folded here, once (and
        serve one_call=True as they are: `plain` asks for nothing more)."""
        _check_mode(mode)
        step, emb = self._decode_stepper(mode), self.B.weight.detach()

        def step_fn(prev_words, state):
            top, st = step(emb, prev_words, state[0])
            return self.C(top), (st,)
        zeros = torch.zeros((rows, 2 * self.num_layers, self.hidden_size), dtype=torch.float32, device=emb.device)
        return plain_stack(step_fn, step.packed, ops.CELL_FACTORED, emb, self.C), (zeros,)

    def sample(self, features, start_token, end_token, k=5, factual_limit=-1, mode='factual', on_device=False, poll_every=0,
               one_call=False, constraints=None, diversity=None, nbest=False, length_penalty=0.0):
        """Beam search, stylenet/model.py:198-294, over the stack: as DecoderFactoredLSTM.sample, the image is NOT an
        input (`features` only fixes the device), every layer's state starts at zero, the first input is B(<start>) and
        factual_limit is ignored. Returns LongTensor [1, L].
        on_device / poll_every / one_call: capnet.decode.beam_decode's (the bookkeeping on the device; the whole search
        in one C call; same sequences).
        constraints: a capnet.beam.Constraints -- no n-gram twice, no <end> before min_words words, no banned word --
        kept inside the search on whichever route runs (capnet.decode.beam_decode); the scores stay the model's own.
        diversity: a capnet.beam.Diversity -- the k beams as groups that pay for the words earlier groups chose at the same
        step, for several different captions of one image (capnet.decode.beam_decode); the scores stay the model's own.
        nbest / length_penalty: capnet.decode.beam_decode's -- every completed hypothesis as a (tokens, score) pair, best
        first, in place of the one caption."""
        return beam_decode(self, *self._beam(k, mode), None, k, start_token, end_token, on_device, poll_every, one_call,
                           nbest=nbest, length_penalty=length_penalty, constraints=constraints, diversity=diversity)

    def sample_random(self, features, start_token, end_token, samples=1, temperature=1.0, top_k=0, seed=None, mode='factual',
                      top_p=1.0, device=False, greedy=False, exclude=None):
        """`samples` captions per row of `features`, DRAWN from the decoder's distribution softmax(logits / temperature)
        (top_k > 0: renormalised over the top_k best words of every step;
        top_p < 1: over the nucleus) instead of searched for: a list of n lists of
        `samples` (tokens, logprob) pairs, tokens = [start, w_1 .. w_j] cut after the first end_token (none: all
        max_seq_length words), logprob the float sum of the kept words' log-probabilities under the distribution sampled
        from. As in sample(), the image is not an input of the decode steps. seed: an integer makes the call a pure function
        of its arguments; None draws a 63-bit seed from torch's CPU generator (torch.manual_seed). One C call
        (capnet_sample_decode) or the composed loop, the same lists: capnet.decode.sample_random.
        greedy=True: every image's pairs are followed by one more, its greedy caption (the argmax of every step), decoded as
        one more row of the same call; the first `samples` pairs are those of the call without it.
        device=True: (the lists, ids, logp), the decode's raw rows [n samples, max_seq_length] left on the device
        (capnet.decode.sample_random_device).
        exclude (a capnet.beam.Constraints without forced words): what no caption may draw -- a repeated n-gram, <end> within
        min_words, banned words -- excluded words being not pickable and logprob that of the distribution renormalised over
        the allowed words (capnet.decode.sample_random_device); None: the call as it was."""
        n = features.size(0)
        return sample_random(self, *self._beam(n * (int(samples) + bool(greedy)), mode, True), n, samples, start_token, end_token, temperature,
                             top_k, seed, top_p, device, greedy, exclude)

    def score_captions(self, features, captions, mode='factual'):
        """float32 [len(captions)] on the device: the model's log-probability of every caption [start, w_1 .. w_j], summed over
        w_1 .. w_j (<end> too where present), in the caller's order. captions: a flat list of token lists, or the nested
        list sample_random returns (the logprob of a (tokens, logprob) pair is ignored). As in sample(), the image is not an
        input: `features` is not read. Under no_grad, dropout following self.training: capnet.decode.score_captions."""
        return score_captions(self, features, captions, mode)

    def sample_batch(self, features, start_token, end_token, k=5, factual_limit=-1, mode='factual', on_device=False,
                     poll_every=0, one_call=False, constraints=None, diversity=None, nbest=False, length_penalty=0.0):
        """sample() for every row of `features` at once (capnet.beam.beam_search_batched). Returns a list of token lists,
        each equal to sample(features[i:i+1], ...)[0].tolist()."""
        n = features.size(0)
        return beam_decode(self, *self._beam(n * k, mode), n, k, start_token, end_token, on_device, poll_every, one_call,
                           nbest=nbest, length_penalty=length_penalty, constraints=constraints, diversity=diversity)

    def sample_styles(self, features, start_token, end_token, k=5, modes=MODES, poll_every=0):
        """sample_batch(one_call=True) in every style of `modes` at once -> {mode: [n token lists]}, each list equal to
        sample_batch(features, ..., mode=mode, one_call=True). The modes differ only in the folded chains, so the search
        runs ONCE over len(modes) x n x k rows on the grouped decode step (capnet_beam_decode_groups), every mode's chain
        folded into its slice of one buffer per layer. As in sample(), the image is not an input: the styles of a plain
        factored decoder differ, the images' captions do not. modes: a non-empty sequence of distinct names of MODES (an
        unknown one as in sample()). Where the fused step does not serve (the shape, CAPNET_NO_FUSED_DECODE_STEP=1) the
        modes are decoded one sample_batch(one_call=True) after the other. poll_every: capnet.decode.beam_decode's."""
        modes = check_styles(modes, _check_mode)
        return plain_styles(self, self._mods, self.num_layers, self.B.weight, self.C, features.size(0), k, start_token, end_token,
                            modes, poll_every,
                            lambda m: self.sample_batch(features, start_token, end_token, k=k, mode=m, one_call=True,
                                                        poll_every=poll_every))

    def sample_styles_nbest(self, features, start_token, end_token, k=5, modes=MODES, poll_every=0, length_penalty=0.0):
        """sample_styles with nbest=True -> {mode: [n lists of (tokens, score)]}, each equal to sample_batch(mode=mode,
        one_call=True, nbest=True, length_penalty=length_penalty): the one grouped search, its completed lists read by
        capnet_beam_nbest. (A method of its own: sample_styles' parameters are pinned.)"""
        modes = check_styles(modes, _check_mode)
        return plain_styles(self, self._mods, self.num_layers, self.B.weight, self.C, features.size(0), k, start_token, end_token,
                            modes, poll_every,
                            lambda m: self.sample_batch(features, start_token, end_token, k=k, mode=m, one_call=True,
                                                        poll_every=poll_every, nbest=True, length_penalty=length_penalty),
                            nbest=True, length_penalty=length_penalty)

    # ---- forward ------------------------------------------------------------------------------
    def forward(self, captions, lengths, features=None, teacher_forcing_ratio=0.8, mode="factual", tf_mask=None):
        """-> packed logits [sum(lengths), V] in pack_padded_sequence order (stylenet/model.py:157-196 with stacked
        cells). tf_mask: the per-step teacher-forcing decisions (else one random.random() draw per step)."""
        _check_mode(mode)
        if not captions.is_cuda:
            raise CapnetError("StackedFactoredLSTM runs on the GPU only")
        bs = ops.batch_sizes_from_lengths(lengths)
        cfg = _seq_cfg(self, bs, self.dropout_p, tf_mask, teacher_forcing_ratio, factored_size=self.factored_size,
                       num_layers=self.num_layers)
        weights = []
        for l in range(self.num_layers):
            for grp in self._mods(l, mode):
                weights += [m.weight for m in grp] + [m.bias for m in grp]
        hiddens = ops.SeqFn.apply(cfg, captions, features, self.B.weight, self.C.weight, self.C.bias, *weights)
        return ops.linear(hiddens, self.C.weight, self.C.bias)
