"""NIC models on the MI355X kernels: EncoderCNN (shared) and DecoderRNN.

Mirrors nic/model.py of the reference: DecoderRNN = Embedding + nn.LSTMCell(embed, hidden) +
Linear(hidden, vocab), same scheduled-sampling loop as the StyleNet decoder. The recurrence
runs in libcapnet_hip.so (cell 1 of capnet_seq_forward/backward).
"""
import torch
import torch.nn as nn

from . import ops
from .decode import beam_decode, fused_decode_step, input_width, pack_cell, plain_stack, sample_random, score_captions, zero_state
from .model import Dropout, Embedding, EncoderCNN, Linear, _seq_cfg  # noqa: F401


class LSTMCell(nn.Module):
    """nn.LSTMCell parameter container (weight_ih [4H,E], weight_hh [4H,H], two biases;
    gate order i, f, g, o)."""

    def __init__(self, input_size, hidden_size, bias=True):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        k = 1.0 / hidden_size ** 0.5
        self.weight_ih = nn.Parameter(torch.empty(4 * hidden_size, input_size).uniform_(-k, k))
        self.weight_hh = nn.Parameter(torch.empty(4 * hidden_size, hidden_size).uniform_(-k, k))
        self.bias_ih = nn.Parameter(torch.empty(4 * hidden_size).uniform_(-k, k))
        self.bias_hh = nn.Parameter(torch.empty(4 * hidden_size).uniform_(-k, k))

    def forward(self, x, states):
        h, c = states
        pre = ops.linear(x, self.weight_ih, self.bias_ih) + ops.linear(h, self.weight_hh, self.bias_hh)
        return ops.lstm_pointwise(pre, c, ops.CELL_LSTM)


class DecoderRNN(nn.Module):
    """nic/model.py:29-207. `num_layers` is accepted and ignored, as in the reference."""

    def __init__(self,
                 embed_size,
                 hidden_size,
                 vocab_size,
                 num_layers,
                 feature_size=2048,
                 dropout=0.22,
                 max_seq_length=40):
        super(DecoderRNN, self).__init__()
        self.feature_size = feature_size
        self.hidden_size = hidden_size
        self.embed_size = embed_size
        self.vocab_size = vocab_size
        self.max_seq_length = max_seq_length
        self.dropout = Dropout(dropout)
        self.embed = Embedding(vocab_size, embed_size)
        self.lstm = LSTMCell(embed_size, hidden_size, bias=True)
        self.linear = Linear(hidden_size, vocab_size)
        self.reset_parameters()
        self.init_weights()

    def reset_parameters(self):
        for p in self.parameters():
            if p.data.ndimension() >= 2:
                nn.init.xavier_uniform_(p.data)
            else:
                nn.init.zeros_(p.data)

    def init_weights(self):
        self.embed.weight.data.uniform_(-0.1, 0.1)
        self.linear.bias.data.fill_(0)
        self.linear.weight.data.uniform_(-0.1, 0.1)

    def forward_step(self, embedded, states):
        h_t, c_t = self.lstm(embedded, states)
        return h_t, (h_t, c_t)

    def _upper_layers(self):
        """(num_layers, the weights of the layers above layer 0) for the sequence call. One layer here: num_layers is
        ignored, as in the reference (capnet.nic_stacked stacks)."""
        return 1, []

    def forward(self, captions, lengths, features, teacher_forcing_ratio=0.8, tf_mask=None):
        batch_sizes = ops.batch_sizes_from_lengths(lengths)
        num_layers, upper = self._upper_layers()
        cfg = _seq_cfg(self, batch_sizes, self.dropout.p, tf_mask, teacher_forcing_ratio, cell=ops.CELL_LSTM,
                       num_layers=num_layers)
        weights = [self.lstm.weight_ih, self.lstm.bias_ih, self.lstm.weight_hh, self.lstm.bias_hh]
        hiddens = ops.SeqFn.apply(cfg, captions, features, self.embed.weight, self.linear.weight, self.linear.bias,
                                  *weights, *upper)
        return self.linear(hiddens)

    def _beam(self, rows, plain=False):
        """(step_fn, the zero state of `rows` beams) of a beam search. plain (one_call=True): the cell packed for the fused
        decode step rides on step_fn where that step takes the shape (capnet.decode.plain_stack)."""
        def step_fn(prev_words, state):
            hidden, (h, c) = self.forward_step(self.embed(prev_words), state)
            return self.linear(hidden), (h, c)
        if plain and fused_decode_step(1, self.embed_size, self.hidden_size):
            plain_stack(step_fn, [pack_cell(self.lstm, input_width(self.embed_size))], ops.CELL_LSTM, self.embed.weight, self.linear)
        return step_fn, zero_state(rows, self.hidden_size, self.embed.weight.device)

    def sample(self, features, start_token, end_token, k=5, on_device=False, poll_every=0, one_call=False, constraints=None, diversity=None, nbest=False,
               length_penalty=0.0):
        """Beam search, nic/model.py:117-207 (the image features are not an input of the decode
        steps there either). Returns LongTensor [1, L].
        on_device / poll_every / one_call: capnet.decode.beam_decode's (the bookkeeping on the device; the whole search
        in one C call; same sequences).
        constraints: a capnet.beam.Constraints -- no n-gram twice, no <end> before min_words words, no banned word --
        kept inside the search on whichever route runs (capnet.decode.beam_decode); the scores stay the model's own.
        diversity: a capnet.beam.Diversity -- the k beams as groups that pay for the words earlier groups chose at the same
        step, for several different captions of one image (capnet.decode.beam_decode); the scores stay the model's own.
        nbest / length_penalty: capnet.decode.beam_decode's -- every completed hypothesis as a (tokens, score) pair, best
        first, in place of the one caption."""
        return beam_decode(self, *self._beam(k, one_call), None, k, start_token, end_token, on_device, poll_every, one_call,
                           nbest=nbest, length_penalty=length_penalty, constraints=constraints, diversity=diversity)

    def sample_random(self, features, start_token, end_token, samples=1, temperature=1.0, top_k=0, seed=None, top_p=1.0, device=False, greedy=False, exclude=None):
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
        return sample_random(self, *self._beam(n * (int(samples) + bool(greedy)), True), n, samples, start_token, end_token, temperature, top_k,
                             seed, top_p, device, greedy, exclude)

    def score_captions(self, features, captions):
        """float32 [len(captions)] on the device: the model's log-probability of every caption [start, w_1 .. w_j], summed over
        w_1 .. w_j (<end> too where present), in the caller's order. captions: a flat list of token lists, or the nested
        list sample_random returns (the logprob of a (tokens, logprob) pair is ignored). As in sample(), the image is not an
        input: `features` is not read. Under no_grad, dropout following self.training: capnet.decode.score_captions."""
        return score_captions(self, features, captions)

    def sample_batch(self, features, start_token, end_token, k=5, on_device=False, poll_every=0, one_call=False, constraints=None, diversity=None, nbest=False,
                     length_penalty=0.0):
        """sample() for every row of `features` at once (capnet.beam.beam_search_batched)."""
        n = features.size(0)
        return beam_decode(self, *self._beam(n * k, one_call), n, k, start_token, end_token, on_device, poll_every, one_call,
                           nbest=nbest, length_penalty=length_penalty, constraints=constraints, diversity=diversity)
