"""Seq2Seq caption-to-styled-caption model on the MI355X kernels: EncoderRNN, DecoderRNN, Seq2Seq.

Mirrors seq2seq/model.py of the reference (factual caption in, happy / sad / angry caption out): constructor and method
signatures, attribute names and state_dict keys in the reference's order. This is the one package of the reference whose
`num_layers` is honoured (nn.LSTM(embed, hidden, num_layers, batch_first=True), seq2seq/model.py:46-49, 140-143), so the
stacked LSTM sequence path (capnet_seq_forward_stacked / _backward_stacked with the LSTM cell) is REFERENCE-PINNED here
(tests/golden/seq2seq_tiny.npz), unlike capnet.stacked / capnet.nic_stacked.

  * `lstm` is a parameter container with nn.LSTM's names and shapes (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0,
    ..._l1, ...); torch's LSTM kernel is never called. Initial values follow torch's constructor defaults (Embedding
    N(0, 1); LSTM and Linear U(+-1/sqrt(fan))), drawn in the reference's order; the reference has no reset_parameters /
    init_weights in this package.
  * Training: forward -> ops.SeqFn (LSTM cell, num_layers layers; `features` for the encoder, None for the decoders), one C
    call each way. Dropout acts on the token embeddings ONLY: nn.LSTM is built without dropout=, so nothing is dropped
    between the layers (cfg["input_dropout_only"]).
  * Decoding: sample() is greedy over a whole batch for exactly max_seq_length steps, no end token, no dropout
    (seq2seq/model.py:100-122, 193-217). One capnet_lstm_greedy_decode call: per step one launch per layer of
    csrc/lstm_decode_step.hip's LSTM-cell instance and one launch of csrc/vocab_argmax.hip, tokens and logits never
    leaving the device. CAPNET_NO_FUSED_GREEDY=1 (read at every sample call) takes the composed loop
    (ops.stacked_decode_step -> linear -> ops.argmax_rows -> next tokens), which also serves the shapes the decode kernel
    does not take (ops.stacked_decode_supported) and batches of more than FUSED_GREEDY_MAX_ROWS = 16 rows: measured
    (profiles/README.md), the one call is 1.3x to 2.3x faster at 1 and 12 rows and no faster at 64 (slower at 2 and 3
    layers), so a batch beyond one 16-row tile goes to the composed loop; 17 to 63 rows were not measured.
  * Every emotion at once: Seq2Seq.sample_styles runs the encoder's greedy loop ONCE and then the emotion decoders as ONE
    capnet_lstm_greedy_decode_groups call from the encoder's final state repeated per decoder: per step one launch per
    layer on a (H / 4, decoders) grid and one vocab_argmax launch on a (V / 32, decoders) grid, workgroup (., g) on
    decoder g's own embedding, LSTM weights and projection. The embeddings and projections are used where they lie (one
    pointer per decoder); only the packed LSTM weights are stacked. Every entry equals sample(mode=...) exactly.
  * Beam search: sample_beam on all three classes (the reference has none here; the loop is the image decoders',
    oracle.beam_ref._beam) -- B sentences x k beams as ONE capnet_lstm_beam_decode call from the given state, the
    encoder's first step on `features`. Per step one gathered decode-step launch per layer, then either the FUSED
    selection (csrc/vocab_topk.hip: projection, per-row top-k and log-sum-exp in one launch, no logits in memory, and
    capnet_beam_advance_topk on the candidates) or capnet_beam_decode's (sgemm_splitk's logits block, capnet_beam_advance).
    fused_topk=None routes by FUSED_TOPK_MAX_ROWS, set from profiles/time_seq2seq_beam.jsonl; CAPNET_NO_FUSED_TOPK=1 (read
    at every call) forces the unfused step. A shape the decode kernel does not take, or CAPNET_NO_FUSED_DECODE_STEP=1:
    capnet.beam.beam_search_device on cell_stepper. Same lists on every route (under the margin rule: the fused logits
    differ from the slab's in the last bits).
  * Beam search in every emotion at once: Seq2Seq.sample_beam_styles runs the encoder's greedy loop ONCE and then the
    emotion decoders' searches as ONE capnet_lstm_beam_decode_groups call over decoders x B sentences, from the encoder's
    final state repeated per decoder: per step one gathered decode-step launch per layer on a (H / 4, decoders) grid and
    either one capnet_vocab_topk_groups launch on a (V / 32, decoders) grid (workgroup (., g) on decoder g's projection,
    its own partials and its own arrival counter) with one capnet_beam_advance_topk, or one sgemm_splitk per decoder and one
    capnet_beam_advance. fused_topk=None routes on the rows per decoder (B k) by FUSED_TOPK_GROUPS_MAX_ROWS, set from
    profiles/time_seq2seq_beam_styles.jsonl. `factual` is the encoder's own sample_beam, not a group. Every entry equals
    sample_beam(mode=...). One emotion, unequal decoder shapes, a shape the decode kernel does not take or
    CAPNET_NO_FUSED_DECODE_STEP=1: one DecoderRNN.sample_beam after the other on the one encoder run.
  * Sampled decoding: sample_random on all three classes -- sample() with every word a draw from softmax(logits /
    temperature) (top_k: renormalised over the step's k best), returning (ids, logp); Gumbel-max on a counter-based stream
    (csrc/sample_rng.h), so an integer seed makes a call a pure function. One capnet_sample_decode call (per step one launch
    per layer and csrc/vocab_sample.hip, or capnet_vocab_topk + capnet_sample_pick) up to capnet.decode.FUSED_SAMPLE_MAX_ROWS
    rows; CAPNET_NO_FUSED_SAMPLE=1 (read at every call), CAPNET_NO_FUSED_DECODE_STEP=1, more rows or a shape the decode
    kernel does not take: the composed loop on the same stream, the same tokens.
  * Constraints: EncoderRNN.sample_beam and DecoderRNN.sample_beam take constraints= (a capnet.beam.Constraints:
    no repeated n-gram, a minimum length, banned words, forced words), the image decoders' rule on every route here; on
    Seq2Seq the constrained searches are sample_beam_constrained and sample_beam_styles_constrained (its sample_beam and
    sample_beam_styles keep their signatures). The fused step stays
    the default for a handful of sentences: one more small launch per step writes what each beam row may not select
    (capnet_beam_exclusion_mask, from the hypotheses in the beam state) and csrc/vocab_topk.hip's select-only instance keeps
    those words out of its k candidates but IN the log-sum-exp, so a caption's score is still the model's own summed
    log-probability; capnet_beam_advance_topk is unchanged. The unfused step selects with capnet_beam_advance_constrained.
    Forced words always take the unfused in-call step (capnet_beam_advance_forced). sample_random takes exclude= / end_token=
    (capnet.decode.sample_random's meaning: an excluded word is not pickable); EncoderRNN's goes through the composed loop,
    since the one call's hypotheses begin with start tokens and the encoder's first input is the feature column.
"""
import os
import random

import torch
import torch.nn as nn

from . import ops
from ._lib import CapnetError
from .beam import Constraints, beam_search_device
from .decode import cell_stepper, check_styles, fused_decode_step, fused_sample, pack_cells, sample_steps
from .model import Dropout, Embedding, Linear, _dropout_seed, _seq_cfg
from .nic_model import LSTMCell

device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')  # seq2seq/model.py:8

FUSED_GREEDY_OFF = "CAPNET_NO_FUSED_GREEDY"
FUSED_GREEDY_MAX_ROWS = 16
FUSED_TOPK_OFF = "CAPNET_NO_FUSED_TOPK"
# the largest n k at which the fused step's median beat the unfused step's by more than the spread at 1, 2 and 3 layers
# (profiles/time_seq2seq_beam.jsonl); above it fused_topk=None takes the unfused step in the same C call. Under
# constraints the crossover is where it was (profiles/time_seq2seq_constrained.jsonl)
FUSED_TOPK_MAX_ROWS = 15
# the same for the grouped search of sample_beam_styles, in rows PER DECODER (B k): the largest measured row count at which
# the grouped fused step's median beat the grouped unfused step's by more than the spread at 1 and 3 layers
# (profiles/time_seq2seq_beam_styles.jsonl); above it fused_topk=None takes the unfused step in the same C call
FUSED_TOPK_GROUPS_MAX_ROWS = 15
_EMOTIONS = ("happy", "sad", "angry")


def _fused_topk(fused_topk, rows, max_rows):
    """Whether a beam search of `rows` rows takes the fused top-k step now: never under CAPNET_NO_FUSED_TOPK=1 (read here, at
    every call); else as fused_topk says, None meaning up to `max_rows` rows."""
    if os.environ.get(FUSED_TOPK_OFF, "")[:1] == "1":
        return False
    return rows <= max_rows if fused_topk is None else bool(fused_topk)


def _check_constraints(constraints, V, end_token, k, T):
    """sample_beam's `constraints` checked (Constraints.check(V, end_token, k, T), T = max_seq_length + 1) -> the Constraints,
    or None for None and for one that excludes nothing (the calls then run as they did before there was the keyword)."""
    if constraints is None:
        return None
    if not isinstance(constraints, Constraints):
        raise CapnetError("constraints must be a capnet.beam.Constraints, not %r" % (constraints,))
    if not constraints.active:
        return None
    constraints.check(V, end_token, k, T)
    return constraints


def _require_constraints(who, constraints):
    if not isinstance(constraints, Constraints):
        raise CapnetError("%s: constraints must be a capnet.beam.Constraints, not %r" % (who, constraints))


def _check_exclude(exclude, end_token, V, top_k, steps):
    """sample_random's `exclude` / `end_token` checked (Constraints.check_exclude) -> (the Constraints or None for one that
    excludes nothing, end_token as an int). end_token is required where min_words > 0; without it no id is <end>."""
    if exclude is None:
        return None, None
    if not isinstance(exclude, Constraints):
        raise CapnetError("exclude must be a capnet.beam.Constraints, not %r" % (exclude,))
    if end_token is None:
        if exclude.min_words > 0:
            raise CapnetError("sample_random: exclude with min_words=%d needs end_token" % exclude.min_words)
        end_token = -1                          # no word id: nothing is <end>
    exclude.check_exclude(V, end_token, top_k, steps)
    return (exclude if exclude.active else None), int(end_token)


class LSTM(nn.Module):
    """nn.LSTM(input_size, hidden_size, num_layers) parameter container: weight_ih_l{k} [4H, in], weight_hh_l{k} [4H, H],
    bias_ih_l{k}, bias_hh_l{k} [4H] per layer, gate order i, f, g, o, every tensor U(-1/sqrt(H), 1/sqrt(H))."""

    def __init__(self, input_size, hidden_size, num_layers):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        k = 1.0 / hidden_size ** 0.5
        for l in range(num_layers):
            n_in = input_size if l == 0 else hidden_size
            for name, shape in (("weight_ih", (4 * hidden_size, n_in)), ("weight_hh", (4 * hidden_size, hidden_size)),
                                ("bias_ih", (4 * hidden_size,)), ("bias_hh", (4 * hidden_size,))):
                setattr(self, "%s_l%d" % (name, l), nn.Parameter(torch.empty(shape).uniform_(-k, k)))

    def layer(self, l):
        return _Layer(self, l)


class _Layer:
    """Layer l of an LSTM container under nn.LSTMCell's names (what capnet.decode's step and packing read)."""

    def __init__(self, lstm, l):
        self.input_size = lstm.input_size if l == 0 else lstm.hidden_size
        self.hidden_size = lstm.hidden_size
        for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            setattr(self, name, getattr(lstm, "%s_l%d" % (name, l)))

    def __call__(self, x, states):
        return LSTMCell.forward(self, x, states)


def _to_rows(h, c):
    """(h, c) [L, rows, H] -> the decode kernels' [rows, 2L, H] (slot 2l = h of layer l, 2l + 1 = c)."""
    L, rows, H = h.shape
    return torch.stack([h, c], 1).permute(2, 0, 1, 3).reshape(rows, 2 * L, H).contiguous()


def _from_rows(state):
    rows, L2, H = state.shape
    hc = state.view(rows, L2 // 2, 2, H).permute(2, 1, 0, 3)
    return hc[0].contiguous(), hc[1].contiguous()


class _RNN(nn.Module):
    """What EncoderRNN and DecoderRNN share: the modules in the reference's order, one step, the sequence call, greedy."""

    def __init__(self, embed_size, hidden_size, vocab_size, num_layers, dropout=0.22, max_seq_length=40):
        super().__init__()
        if not 1 <= num_layers <= 8:
            raise CapnetError("num_layers must be 1 to 8 (the sequence call's limit)")
        self.max_seq_length = max_seq_length
        self.num_layers = num_layers
        self.hidden_size = hidden_size
        self.embed_size = embed_size
        self.vocab_size = vocab_size
        self.dropout = Dropout(dropout)
        self.embed = Embedding(vocab_size, embed_size)
        self.lstm = LSTM(embed_size, hidden_size, num_layers)
        self.linear = Linear(hidden_size, vocab_size)

    def _layers(self):
        return [self.lstm.layer(l) for l in range(self.num_layers)]

    def _zeros(self, rows):
        return torch.zeros((rows, 2 * self.num_layers, self.hidden_size), dtype=torch.float32,
                           device=self.embed.weight.device)

    def forward_step(self, embedded, states):
        """One step at inference (no dropout) on `embedded` [b, E] or [b, 1, E]; states (h, c), each [num_layers, b, H]
        or None for zeros. Returns (the top layer's hiddens [b, H], (h, c))."""
        with torch.no_grad():
            if embedded.dim() == 3:
                embedded = embedded.squeeze(1)
            h, c = states
            b = embedded.size(0)
            zeros = torch.zeros((self.num_layers, b, self.hidden_size), dtype=torch.float32, device=embedded.device)
            state = _to_rows(zeros if h is None else h.detach(), zeros if c is None else c.detach())
            step = cell_stepper(self._layers(), self.embed_size, self.hidden_size)
            top, state = step(embedded.detach().contiguous(), None, state)
            return top, _from_rows(state)

    def _sequence(self, features, tokens, lengths, teacher_forcing_ratio):
        """(packed logits [N, V], (h, c)): one random.random() draw per step, then ops.SeqFn."""
        batch_sizes = ops.batch_sizes_from_lengths(lengths)
        cfg = _seq_cfg(self, batch_sizes, self.dropout.p, None, teacher_forcing_ratio, cell=ops.CELL_LSTM,
                       num_layers=self.num_layers, input_dropout_only=True, want_final_state=True)
        weights = []
        for c in self._layers():
            weights += [c.weight_ih, c.bias_ih, c.weight_hh, c.bias_hh]
        hiddens = ops.SeqFn.apply(cfg, tokens, features, self.embed.weight, self.linear.weight, self.linear.bias, *weights)
        return self.linear(hiddens), cfg["final_state"]

    def _advance_streams(self, lengths):
        """Consume what _sequence consumes of `random` and of torch's generator, without its arithmetic."""
        for _ in ops.batch_sizes_from_lengths(lengths):
            random.random()
        _dropout_seed(self.training, self.dropout.p)

    def _greedy(self, features, start_tokens, state):
        """max_seq_length greedy steps from `features` [rows, E] or emb[start_tokens]; state [rows, 2L, H].
        Returns (ids [rows, max_seq_length] int64, state')."""
        E, H, steps = self.embed_size, self.hidden_size, self.max_seq_length
        emb, Cw, Cb = self.embed.weight.detach(), self.linear.weight.detach(), self.linear.bias.detach()
        layers = self._layers()
        with torch.no_grad():
            if (os.environ.get(FUSED_GREEDY_OFF, "")[:1] != "1" and ops.stacked_decode_supported(E, H)
                    and state.shape[0] <= FUSED_GREEDY_MAX_ROWS):
                packed = pack_cells(layers, E)
                return ops.lstm_greedy_decode(steps, [w for w, _ in packed], [b for _, b in packed], emb, Cw, Cb,
                                              features=features, start_tokens=start_tokens, state=state)
            step = cell_stepper(layers, E, H)
            ids, tokens = [], start_tokens
            for t in range(steps):
                if t == 0 and features is not None:
                    top, state = step(features.detach().contiguous(), None, state)
                else:
                    top, state = step(emb, tokens, state)
                tokens = ops.argmax_rows(ops.linear(top, Cw, Cb)).long()
                ids.append(tokens)
            return torch.stack(ids, 1), state


    def _sampled(self, features, start_tokens, state, temperature, top_k, seed, top_p=1.0, exclude=None, end_token=None):
        """max_seq_length SAMPLED steps from `features` [rows, E] or emb[start_tokens]; state [rows, 2L, H]: every word a draw
        from softmax(logits / temperature) (top_k > 0: renormalised over the step's top_k best), row r on stream row r, step
        t on stream step t; top_p < 1: over the nucleus (capnet.decode.sample_random). Returns (ids [rows, max_seq_length] int64, logp [rows, max_seq_length] float32, state').
        One capnet_sample_decode call where the decode kernel takes the shape, the rows are at most
        capnet.decode.FUSED_SAMPLE_MAX_ROWS and neither CAPNET_NO_FUSED_SAMPLE=1 nor CAPNET_NO_FUSED_DECODE_STEP=1 is set;
        else the composed loop (capnet.decode.sample_steps on step -> ops.linear) on the same stream: the same tokens.
        exclude (a capnet.beam.Constraints without forced words; end_token required where min_words > 0): what no row may draw,
        capnet.decode.sample_random_device's keyword -- a row is the hypothesis [its start token, its words so far] (from
        `features`: the words alone). The one call is capnet_sample_decode_excl where there are start tokens; from `features`
        the composed loop. None or a Constraints() that excludes nothing: the calls as they were."""
        E, H, V, steps = self.embed_size, self.hidden_size, self.vocab_size, self.max_seq_length
        temperature, top_k, seed, top_p = ops.check_sampling("sample_random", temperature, top_k, seed, V, top_p)
        kw = {} if top_p == 1.0 else {"top_p": top_p}      # top_p == 1.0: the calls as they were before there was a top_p
        exclude, end_token = _check_exclude(exclude, end_token, V, top_k, steps)
        ex = {} if exclude is None else {"exclude": exclude, "end_token": end_token}
        emb, Cw, Cb = self.embed.weight.detach(), self.linear.weight.detach(), self.linear.bias.detach()
        layers = self._layers()
        with torch.no_grad():
            if (fused_sample(state.shape[0], False, top_p, top_k) and fused_decode_step(self.num_layers, E, H)
                    and ops.sample_decode_supported(E, H, V, top_k) and (exclude is None or start_tokens is not None)):
                packed = pack_cells(layers, E)
                return ops.sample_decode(ops.CELL_LSTM, steps, [w for w, _ in packed], [b for _, b in packed], emb, Cw, Cb,
                                         temperature, top_k, seed, first_inputs=features, start_tokens=start_tokens, state=state,
                                         **kw, **ex)
            cells = cell_stepper(layers, E, H)

            def step(t, tokens, state):
                if t == 0 and features is not None:
                    top, state = cells(features.detach().float().contiguous(), None, state)
                else:
                    top, state = cells(emb, tokens, state)
                return ops.linear(top, Cw, Cb), state
            if exclude is None:
                return sample_steps(step, steps, start_tokens, state, temperature, top_k, seed, kw)
            return sample_steps(step, steps, start_tokens, state, temperature, top_k, seed, kw, exclude, V, end_token)

    def _beam_search(self, features, start_token, end_token, state, k, poll_every, fused_topk, nbest=False, length_penalty=0.0,
                     constraints=None):
        """Beam search of B = state.shape[0] sentences x k beams from `state` [B, 2L, H]; the first input is `features`
        [B, E] or, None, embed(start_token). max_seq_length + 1 steps at most. Returns B token lists, each starting with
        start_token ([end_token] where nothing completed). Routing: the module's docstring. nbest: per sentence the list of
        (tokens, score) of its completed hypotheses, best first (capnet.decode.beam_decode's keyword), on every route.
        constraints (a capnet.beam.Constraints, checked here): every route selects under them -- the fused step through the
        selection mask (not with forced words: those take the unfused in-call step at every row count), the unfused step and
        beam_search_device through capnet_beam_advance_constrained / _forced. None or a Constraints() that excludes nothing:
        exactly the calls without the keyword."""
        E, H, V, L = self.embed_size, self.hidden_size, self.vocab_size, self.num_layers
        length_penalty = ops.check_length_penalty("sample_beam", nbest, length_penalty)
        k, constraints = self._check_beam_args(k, end_token, constraints)
        con = {} if constraints is None else {"constraints": constraints}
        emb, Cw, Cb = self.embed.weight.detach(), self.linear.weight.detach(), self.linear.bias.detach()
        layers = self._layers()
        B = state.shape[0]
        with torch.no_grad():
            state = state.detach().repeat_interleave(k, 0).contiguous()
            first = None if features is None else features.detach().float().repeat_interleave(k, 0).contiguous()
            if fused_decode_step(L, E, H) and ops.lstm_beam_decode_supported(E, H, k, V, L):
                fused = _fused_topk(fused_topk, B * k, FUSED_TOPK_MAX_ROWS) and not ops.has_forced(constraints)
                packed = pack_cells(layers, E)
                return ops.lstm_beam_decode(ops.CELL_LSTM, [w for w, _ in packed], [b for _, b in packed], emb, Cw, Cb, B, k,
                                            self.max_seq_length + 1, start_token, end_token, first_inputs=first, state=state,
                                            fused_topk=fused, poll_every=poll_every, nbest=nbest, length_penalty=length_penalty,
                                            **con)
            step = cell_stepper(layers, E, H)
            calls = [0]

            def step_fn(prev_words, st):
                calls[0] += 1
                if calls[0] == 1 and first is not None:
                    top, new = step(first, None, st[0])
                else:
                    top, new = step(emb, prev_words, st[0])
                return ops.linear(top, Cw, Cb), (new,)
            return beam_search_device(step_fn, (state,), B, V, start_token, end_token, k, self.max_seq_length,
                                      emb.device, poll_every, nbest=nbest, length_penalty=length_penalty, **con)

    def _check_beam_args(self, k, end_token, constraints):
        """(k, the constraints or None for none that exclude anything) of a beam search on this stack, checked."""
        k, V = int(k), self.vocab_size
        if not 1 <= k <= 16 or k > V:
            raise CapnetError("sample_beam: k=%d (1 <= k <= 16, k <= vocab_size = %d)" % (k, V))
        return k, _check_constraints(constraints, V, end_token, k, self.max_seq_length + 1)

    def _rows_state(self, states, rows, dev):
        h, c = states
        zeros = torch.zeros((self.num_layers, rows, self.hidden_size), dtype=torch.float32, device=dev)
        return _to_rows(zeros if h is None else h, zeros if c is None else c)


class EncoderRNN(_RNN):
    """seq2seq/model.py:30-122."""

    def forward(self, features, src_tokens, lengths, teacher_forcing_ratio=0.5):
        """Inputs [features, dropout(embed(w_0)), ...] packed by `lengths`; every layer starts at zero; a free-running
        step feeds embed(argmax(linear(h_top))) without dropout, a free-running step 0 embed(src_tokens[:, 0]).
        Returns (outputs [N, V], (h, c)) with h, c [num_layers, b_last, H]: the state after the last step of the rows
        still alive there. The returned states are copies with NO gradient path (requires_grad=False): the reference
        never differentiates through them."""
        return self._sequence(features, src_tokens, lengths, teacher_forcing_ratio)

    def sample(self, features, states=(None, None)):
        """Greedy: (ids [B, max_seq_length] int64, (h, c) [num_layers, B, H]); the first input is `features`."""
        h, c = states
        rows = features.size(0)
        if h is None and c is None:
            state = None
        else:
            zeros = torch.zeros((self.num_layers, rows, self.hidden_size), dtype=torch.float32, device=features.device)
            state = _to_rows(zeros if h is None else h, zeros if c is None else c)
        ids, state = self._greedy(features, None, self._zeros(rows) if state is None else state)
        return ids, _from_rows(state)

    def sample_random(self, features, states=(None, None), temperature=1.0, top_k=0, seed=None, top_p=1.0, exclude=None,
                      end_token=None):
        """sample() with every word DRAWN from softmax(logits / temperature) (top_k > 0: renormalised over the step's top_k
        best words) instead of the argmax: (ids [B, max_seq_length] int64, logp [B, max_seq_length] float32 -- each word's
        log-probability under the distribution sampled from --, (h, c) [num_layers, B, H]); the first input is `features`.
        seed: an integer makes the call a pure function; None draws one from torch's CPU generator (torch.manual_seed).
        exclude / end_token: what no row may draw (_RNN._sampled); the hypotheses are the drawn words alone.
        Routing: _RNN._sampled."""
        state = self._rows_state(states, features.size(0), features.device)
        ids, logp, state = self._sampled(features, None, state, temperature, top_k, seed, top_p, exclude, end_token)
        return ids, logp, _from_rows(state)

    def sample_beam(self, features, start_token, end_token, states=(None, None), k=5, poll_every=0, fused_topk=None,
                    constraints=None, nbest=False, length_penalty=0.0):
        """Beam search (k beams per sentence, max_seq_length + 1 steps at most, a beam completes at end_token) whose first
        input is `features` [B, E]: a list of B token lists. start_token only seeds the bookkeeping (no step reads its
        embedding), so it is dropped from every list that has more than one element; [end_token] where nothing completed.
        poll_every as capnet.beam.beam_search_device; fused_topk: None routes by FUSED_TOPK_MAX_ROWS, True / False force
        the fused / unfused step (CAPNET_NO_FUSED_TOPK=1 forces False). nbest / length_penalty: per sentence the list of
        (tokens, score) of every completed hypothesis, best first, start_token dropped from each (the key still counts the
        generated words: len(tokens) here); empty where nothing completed. constraints: a capnet.beam.Constraints
        (_RNN._beam_search); the hypotheses begin with start_token, which counts as a token of the rule."""
        state = self._rows_state(states, features.size(0), features.device)
        lists = self._beam_search(features, start_token, end_token, state, k, poll_every, fused_topk, nbest, length_penalty,
                                  constraints)
        if nbest:
            return [[(q[1:], sc) for q, sc in hyps] for hyps in lists]
        return [s[1:] if len(s) > 1 else s for s in lists]


class DecoderRNN(_RNN):
    """seq2seq/model.py:125-217."""

    def _start(self, start_token, states):
        """(start_token once per row -- None for None --, the state [rows, 2L, H]) of `states` (h, c) [num_layers, rows, H]:
        either may be None for zeros, both for one row of them."""
        h, c = states
        given = h if h is not None else c
        rows = 1 if given is None else given.size(1)
        dev = self.embed.weight.device
        state = self._rows_state(states, rows, dev)
        return None if start_token is None else torch.full((rows,), int(start_token), dtype=torch.int64, device=dev), state

    def forward(self, states, dst_tokens, lengths, teacher_forcing_ratio=0.5):
        """Packed logits [N, V] of dst_tokens (no feature column). `states` is IGNORED and every layer starts at zero,
        as in the reference (seq2seq/model.py:169-172): the encoder's state reaches the decoders in sample() only."""
        return self._sequence(None, dst_tokens, lengths, teacher_forcing_ratio)[0]

    def sample(self, start_token, states):
        """Greedy from embed(start_token) and `states` (h, c) [num_layers, B, H] -> ids [B, max_seq_length] int64. The
        start token is broadcast to the states' batch (the reference's own sample only works for B = 1, where the two
        agree). An out-of-range start_token raises CapnetError through the device error word."""
        tokens, state = self._start(start_token, states)
        ids, _ = self._greedy(None, tokens, state)
        ops.check_device_errors()
        return ids

    def sample_random(self, start_token, states, temperature=1.0, top_k=0, seed=None, top_p=1.0, exclude=None, end_token=None):
        """sample() with every word drawn (EncoderRNN.sample_random): from embed(start_token) and `states` (h, c)
        [num_layers, B, H] -> (ids [B, max_seq_length] int64, logp [B, max_seq_length] float32). An out-of-range
        start_token raises CapnetError through the device error word. exclude / end_token: what no row may draw
        (_RNN._sampled); a row's hypothesis is [start_token, its words so far]."""
        tokens, state = self._start(start_token, states)
        ids, logp, _ = self._sampled(None, tokens, state, temperature, top_k, seed, top_p, exclude, end_token)
        ops.check_device_errors()
        return ids, logp

    def sample_beam(self, start_token, end_token, states, k=5, poll_every=0, fused_topk=None, constraints=None, nbest=False,
                    length_penalty=0.0):
        """Beam search from embed(start_token) and `states` (h, c) [num_layers, B, H]: a list of B token lists, one per
        column of `states`, each what oracle.beam_ref._beam returns for that sentence -- it begins with start_token, and is
        [end_token] where nothing completed. max_seq_length + 1 steps at most. poll_every / fused_topk: as
        EncoderRNN.sample_beam. An out-of-range start_token raises CapnetError through the device error word.
        nbest / length_penalty: per sentence the list of (tokens, score) of every completed hypothesis, best first by score /
        (len(tokens) - 1)^length_penalty; empty where nothing completed. constraints: a capnet.beam.Constraints
        (_RNN._beam_search)."""
        _, state = self._start(None, states)
        return self._beam_search(None, start_token, end_token, state, k, poll_every, fused_topk, nbest, length_penalty, constraints)


def _groupable(decoders):
    """Whether `decoders` can share a grouped call: 2 to ops.MAX_GROUPS of them, of equal shapes."""
    shapes = {(x.embed_size, x.hidden_size, x.vocab_size, x.num_layers, x.max_seq_length) for x in decoders}
    return 2 <= len(decoders) <= ops.MAX_GROUPS and len(shapes) == 1


def _grouped_weights(decoders):
    """(wcat, beff, embs, Cws, Cbs) of equal-shaped decoders as the grouped calls take them: per layer pack_cell of every
    decoder stacked ([groups, 4H, kin_l + H], [groups, 4H]); per decoder its embedding, projection and bias where they lie."""
    d = decoders[0]
    packed = [pack_cells(x._layers(), d.embed_size) for x in decoders]
    return ([torch.stack([p[l][0] for p in packed]) for l in range(d.num_layers)],
            [torch.stack([p[l][1] for p in packed]) for l in range(d.num_layers)],
            [x.embed.weight.detach() for x in decoders], [x.linear.weight.detach() for x in decoders],
            [x.linear.bias.detach() for x in decoders])


class Seq2Seq(nn.Module):
    """seq2seq/model.py:220-301: one encoder (the factual captioner) and one decoder per emotion."""

    def __init__(self, embed_size, hidden_size, vocab_size, num_layers, dropout=0.22, max_seq_length=40):
        super(Seq2Seq, self).__init__()
        self.hidden_size = hidden_size
        self.max_seq_length = max_seq_length
        self.encoder = EncoderRNN(embed_size, hidden_size, vocab_size, num_layers, dropout=dropout)
        self.decoder_happy = DecoderRNN(embed_size, hidden_size, vocab_size, num_layers, dropout=dropout)
        self.decoder_sad = DecoderRNN(embed_size, hidden_size, vocab_size, num_layers, dropout=dropout)
        self.decoder_angry = DecoderRNN(embed_size, hidden_size, vocab_size, num_layers, dropout=dropout)

    def _decoder(self, mode):
        if mode not in _EMOTIONS:
            raise CapnetError("mode name wrong: %r (factual, happy, sad, angry)" % (mode,))
        return getattr(self, "decoder_" + mode)

    def forward(self, features, src, dst=(None, None), teacher_forcing_ratio=0.8, mode='factual'):
        """factual: the encoder's packed logits of `src` = (tokens, lengths). An emotion mode: that decoder's packed
        logits of `dst` from zero state; the reference runs the encoder first and discards its outputs, so here only its
        draws are consumed (`random`, one per encoder step, and the dropout seed), exactly as if it had run."""
        src_tokens, src_lengths = src
        dst_tokens, dst_lengths = dst
        if mode == 'factual':
            return self.encoder(features, src_tokens, src_lengths, teacher_forcing_ratio)[0]
        decoder = self._decoder(mode)
        self.encoder._advance_streams(src_lengths)
        return decoder((None, None), dst_tokens, dst_lengths, teacher_forcing_ratio)

    def sample(self, features, start_token, states=(None, None), mode='factual'):
        """factual: the encoder's greedy ids [B, max_seq_length]. An emotion mode: that decoder's greedy ids from
        embed(start_token) and the encoder's final state."""
        decoder = None if mode == 'factual' else self._decoder(mode)
        sampled_ids, states = self.encoder.sample(features, states)
        if decoder is None:
            return sampled_ids
        return decoder.sample(start_token, states)

    def sample_random(self, features, start_token, states=(None, None), mode='factual', temperature=1.0, top_k=0, seed=None,
                      top_p=1.0, exclude=None, end_token=None):
        """factual: the encoder's sampled (ids, logp) [B, max_seq_length] (EncoderRNN.sample_random). An emotion mode: the
        encoder's GREEDY sample for the state, exactly as sample(mode=...) does, then that decoder's sampled (ids, logp)
        from embed(start_token) and it: only the emotion decoder samples. exclude / end_token: what the sampling stack may
        not draw (the two sample_random)."""
        decoder = None if mode == 'factual' else self._decoder(mode)
        if decoder is None:
            ids, logp, _ = self.encoder.sample_random(features, states, temperature, top_k, seed, top_p, exclude, end_token)
            return ids, logp
        if exclude is not None:          # refused before the encoder's pass runs (the decoder checks again)
            _check_exclude(exclude, end_token, decoder.vocab_size, ops.check_sampling("sample_random", temperature, top_k, 0)[1],
                           decoder.max_seq_length)
        _, states = self.encoder.sample(features, states)
        return decoder.sample_random(start_token, states, temperature, top_k, seed, top_p, exclude, end_token)

    def sample_beam(self, features, start_token, end_token, states=(None, None), mode='factual', k=5, poll_every=0,
                    fused_topk=None, nbest=False, length_penalty=0.0):
        """factual: the encoder's beam search (EncoderRNN.sample_beam). An emotion mode: the encoder's GREEDY sample for
        the state, as sample() does, then that decoder's beam search from it (DecoderRNN.sample_beam). A list of B token
        lists; nbest / length_penalty: of B n-best lists, as the two sample_beam. Under constraints:
        sample_beam_constrained."""
        return self._sample_beam(features, start_token, end_token, states, mode, k, poll_every, fused_topk, None, nbest,
                                 length_penalty)

    def sample_beam_constrained(self, features, start_token, end_token, constraints, states=(None, None), mode='factual', k=5,
                                poll_every=0, fused_topk=None, nbest=False, length_penalty=0.0):
        """sample_beam under `constraints` (a capnet.beam.Constraints, required) on the stack that searches -- the encoder's
        or the decoder's sample_beam(constraints=...); the encoder's greedy pass for an emotion's state is not constrained.
        A Constraints() that excludes nothing is sample_beam. (A method of its own: this class's sample_beam and
        sample_beam_styles keep the signatures they had.)"""
        _require_constraints("sample_beam_constrained", constraints)
        return self._sample_beam(features, start_token, end_token, states, mode, k, poll_every, fused_topk, constraints, nbest,
                                 length_penalty)

    def _sample_beam(self, features, start_token, end_token, states, mode, k, poll_every, fused_topk, constraints, nbest,
                     length_penalty):
        decoder = None if mode == 'factual' else self._decoder(mode)
        if decoder is None:
            return self.encoder.sample_beam(features, start_token, end_token, states, k, poll_every, fused_topk, constraints, nbest,
                                            length_penalty)
        decoder._check_beam_args(k, end_token, constraints)      # refused before the encoder's pass runs
        _, states = self.encoder.sample(features, states)
        return decoder.sample_beam(start_token, end_token, states, k, poll_every, fused_topk, constraints, nbest, length_penalty)

    def _check_mode(self, mode):
        if mode != 'factual':
            self._decoder(mode)

    def _grouped_greedy_ok(self, decoders, rows):
        """Whether `decoders` decode `rows` rows each in one grouped call now (CAPNET_NO_FUSED_GREEDY is read here)."""
        d = decoders[0]
        return (_groupable(decoders) and os.environ.get(FUSED_GREEDY_OFF, "")[:1] != "1"
                and ops.stacked_decode_supported(d.embed_size, d.hidden_size) and rows <= FUSED_GREEDY_MAX_ROWS)

    def sample_styles(self, features, start_token, states=(None, None), modes=('factual', 'happy', 'sad', 'angry')):
        """{mode: ids [B, max_seq_length] int64} for every mode of `modes` (a non-empty sequence of distinct names), each
        entry equal to sample(features, start_token, states, mode=mode). The encoder's greedy loop runs once, whatever is
        asked for; its ids are the `factual` entry. Two or more emotions then decode as ONE grouped call
        (ops.lstm_greedy_decode_groups) from the encoder's final state, copied once per decoder. One emotion, more than
        FUSED_GREEDY_MAX_ROWS rows, a shape the decode kernel does not take or CAPNET_NO_FUSED_GREEDY=1: one
        DecoderRNN.sample after the other on that one encoder run."""
        modes = check_styles(modes, self._check_mode)
        emotions = [m for m in modes if m != 'factual']
        decoders = [self._decoder(m) for m in emotions]
        factual, (h, c) = self.encoder.sample(features, states)
        out = {'factual': factual}
        rows = h.size(1)
        if decoders and self._grouped_greedy_ok(decoders, rows):
            d, G = decoders[0], len(decoders)
            with torch.no_grad():
                weights = _grouped_weights(decoders)
                state = _to_rows(h, c).repeat(G, 1, 1)
                tokens = torch.full((G * rows,), int(start_token), dtype=torch.int64, device=h.device)
                ids, _ = ops.lstm_greedy_decode_groups(d.max_seq_length, *weights, tokens, state)
            ops.check_device_errors()
            for g, m in enumerate(emotions):
                out[m] = ids[g * rows:(g + 1) * rows]
        else:
            for m, x in zip(emotions, decoders):
                out[m] = x.sample(start_token, (h, c))
        return {m: out[m] for m in modes}

    def _grouped_beam_ok(self, decoders, k):
        """Whether `decoders` search in one grouped call now (CAPNET_NO_FUSED_DECODE_STEP is read here)."""
        d = decoders[0]
        return (_groupable(decoders) and fused_decode_step(d.num_layers, d.embed_size, d.hidden_size)
                and ops.lstm_beam_decode_supported(d.embed_size, d.hidden_size, k, d.vocab_size, d.num_layers))

    def sample_beam_styles(self, features, start_token, end_token, states=(None, None),
                           modes=('factual', 'happy', 'sad', 'angry'), k=5, poll_every=0, fused_topk=None, nbest=False,
                           length_penalty=0.0):
        """{mode: [B token lists]} for every mode of `modes` (a non-empty sequence of distinct names), each entry equal to
        sample_beam(features, start_token, end_token, states, mode=mode, k=k). `factual` is the encoder's own sample_beam
        (its first input is `features`, it starts from `states`). The encoder's greedy sample runs once, and only if an
        emotion is asked for. Two or more emotions with equal shapes then search as ONE grouped call
        (ops.lstm_beam_decode_groups) from the encoder's final state, repeated per decoder; fused_topk=None routes that call
        on the rows per decoder (B k) by FUSED_TOPK_GROUPS_MAX_ROWS, True / False force the fused / unfused step
        (CAPNET_NO_FUSED_TOPK=1 forces False). One emotion, unequal decoder shapes, a shape the decode kernel does not take
        or CAPNET_NO_FUSED_DECODE_STEP=1: one DecoderRNN.sample_beam after the other on that one encoder run. An
        out-of-range start_token raises CapnetError through the device error word. nbest / length_penalty: {mode: [B n-best
        lists]}, as sample_beam's, on the grouped call and on the loop. Under constraints: sample_beam_styles_constrained."""
        return self._sample_beam_styles(features, start_token, end_token, states, modes, k, poll_every, fused_topk, None, nbest,
                                        length_penalty)

    def sample_beam_styles_constrained(self, features, start_token, end_token, constraints, states=(None, None),
                                       modes=('factual', 'happy', 'sad', 'angry'), k=5, poll_every=0, fused_topk=None, nbest=False,
                                       length_penalty=0.0):
        """sample_beam_styles under `constraints` (a capnet.beam.Constraints, required), the same on every route -- the
        encoder's own search, the grouped call (fused: capnet_vocab_topk_groups_masked under the selection mask; forced words:
        its unfused step) and the loop: every entry equals sample_beam_constrained(..., mode=mode). A Constraints() that
        excludes nothing is sample_beam_styles."""
        _require_constraints("sample_beam_styles_constrained", constraints)
        return self._sample_beam_styles(features, start_token, end_token, states, modes, k, poll_every, fused_topk, constraints,
                                        nbest, length_penalty)

    def _sample_beam_styles(self, features, start_token, end_token, states, modes, k, poll_every, fused_topk, constraints, nbest,
                            length_penalty):
        length_penalty = ops.check_length_penalty("sample_beam_styles", nbest, length_penalty)
        try:
            modes = check_styles(modes, self._check_mode)
        except ValueError as e:                    # an empty or repeated list: refused as every other bad argument here
            raise CapnetError("sample_beam_styles: %s" % e)
        emotions = [m for m in modes if m != 'factual']
        decoders = [self._decoder(m) for m in emotions]
        for x in [self.encoder] * ('factual' in modes) + decoders:      # refused before anything runs
            x._check_beam_args(k, end_token, constraints)
        out = {}
        if 'factual' in modes:
            out['factual'] = self.encoder.sample_beam(features, start_token, end_token, states, k, poll_every, fused_topk, constraints,
                                                      nbest, length_penalty)
        if decoders:
            _, (h, c) = self.encoder.sample(features, states)
            B, k = h.size(1), int(k)
            d, G = decoders[0], len(decoders)
            con = d._check_beam_args(k, end_token, constraints)[1]
            if self._grouped_beam_ok(decoders, k):
                fused = _fused_topk(fused_topk, B * k, FUSED_TOPK_GROUPS_MAX_ROWS) and not ops.has_forced(con)
                with torch.no_grad():
                    weights = _grouped_weights(decoders)
                    state = _to_rows(h, c).repeat(G, 1, 1).repeat_interleave(k, 0).contiguous()
                    lists = ops.lstm_beam_decode_groups(
                        ops.CELL_LSTM, *weights, B, k, d.max_seq_length + 1, start_token, end_token, state=state,
                        fused_topk=fused, poll_every=poll_every, nbest=nbest, length_penalty=length_penalty,
                        **({} if con is None else {"constraints": con}))
                ops.check_device_errors()
                for g, m in enumerate(emotions):
                    out[m] = lists[g * B:(g + 1) * B]
            else:
                for m, x in zip(emotions, decoders):
                    out[m] = x.sample_beam(start_token, end_token, (h, c), k, poll_every, fused_topk, constraints, nbest, length_penalty)
                ops.check_device_errors()
        return {m: out[m] for m in modes}
