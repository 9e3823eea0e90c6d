"""NIC attention path on the MI355X kernels: EncoderCNN, Attention, DecoderRNNAtt
(nic/model_att.py of the reference).

DecoderRNNAtt is the attention loop of stylenet/model_att.py around an nn.LSTMCell(E + C, H)
instead of the factored cell: no modes, gate order i,f,g,o, h = o*tanh(c). The sequence runs in
libcapnet_hip.so (capnet_att_seq_forward/backward with cell = 1).
"""
import torch
import torch.nn as nn

from . import decode, ops
from .decode import att_beam_start, att_beam_step, beam_decode, pack_cells
from .model import Dropout, Embedding, Linear, _Marker, _seq_cfg
from .model_att import Attention, EncoderCNN  # noqa: F401  (same classes as the StyleNet path)
from .nic_model import LSTMCell


class DecoderRNNAtt(nn.Module):
    """nic/model_att.py:72-297. `num_layers` is accepted and ignored, as in the reference."""

    def __init__(self,
                 attention_size,
                 embed_size,
                 hidden_size,
                 vocab_size,
                 num_layers,
                 feature_size=2048,
                 dropout=0.22,
                 max_seq_length=40):
        super(DecoderRNNAtt, self).__init__()
        self.attention_size = attention_size
        self.feature_size = feature_size
        self.hidden_size = hidden_size
        self.embed_size = embed_size
        self.vocab_size = vocab_size
        self.max_seq_length = max_seq_length
        # registration order follows nic/model_att.py:89-113 (state_dict order)
        self.init_h = Linear(feature_size, hidden_size)
        self.init_c = Linear(feature_size, hidden_size)
        self.dropout = Dropout(dropout)
        self.attention = Attention(feature_size, hidden_size, attention_size)
        self.embed = Embedding(vocab_size, embed_size)
        self.f_beta = Linear(hidden_size, feature_size)
        self.sigmoid = _Marker()
        self.lstm = LSTMCell(embed_size + feature_size, hidden_size, bias=True)
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

    def init_hidden_state(self, feature):
        mean_feature = feature.mean(dim=1)
        return self.init_h(mean_feature), self.init_c(mean_feature)

    def forward_step(self, embedded, states):
        h_t, c_t = self.lstm(embedded, states)
        return h_t, (h_t, c_t)

    def _weights(self):
        att = self.attention
        out = [self.lstm.weight_ih, self.lstm.bias_ih, self.lstm.weight_hh, self.lstm.bias_hh]
        for m in (self.init_h, self.init_c, att.encoder_att, att.decoder_att, att.full_att, self.f_beta):
            out += [m.weight, m.bias]
        return out

    def _upper_layers(self):
        """(num_layers, the weights of the layers above layer 0) for the sequence call. One layer here: num_layers is
        ignored, as in the reference (capnet.nic_stacked stacks)."""
        return 1, []

    def forward(self, captions, lengths, features, teacher_forcing_ratio=0.8, tf_mask=None):
        """Returns (outputs [N, V], alphas [B, max(lengths), P]) -- nic/model_att.py:152-202."""
        batch_size = captions.size(0)
        features = features.reshape(batch_size, -1, features.size(-1))
        batch_sizes = ops.batch_sizes_from_lengths(lengths)
        num_layers, upper = self._upper_layers()
        cfg = _seq_cfg(self, batch_sizes, self.dropout.p, tf_mask, teacher_forcing_ratio, cell=ops.CELL_LSTM,
                       num_layers=num_layers, attention_size=self.attention_size)
        hiddens, alphas = ops.AttSeqFn.apply(cfg, captions, features.detach(), self.embed.weight, self.linear.weight,
                                             self.linear.bias, *self._weights(), *upper)
        return self.linear(hiddens), alphas

    def _upper_beam(self, feat, img):
        """(the beam state's entries after layer 0's (h0, c0), att_beam_step's `upper`). One layer here."""
        return (), None

    def _cells(self):
        """The LSTMCells of every layer, bottom up. One layer here."""
        return [self.lstm]

    @torch.no_grad()
    def _beam(self, features, n, k, one_call=False):
        """(step_fn, initial state) of a beam search over one image (n None) or n images: the state is layer 0's (h, c),
        then what _upper_beam adds, then (n images) every beam's image index. one_call: the AttStack of the search as one C
        call rides on step_fn where the shape is supported (capnet.decode.att_stack: only then are the cells packed)."""
        feat, att1_of, feat_of, h0, c0, img, maps = att_beam_start(self, self.attention, features, n, k)
        state, upper = self._upper_beam(feat, img)
        step_fn = att_beam_step(self.attention, self.f_beta, self.embed, self.lstm, self.linear, att1_of, feat_of,
                                features.size(-1), upper)
        if one_call:
            decode.att_stack(step_fn, self, ops.CELL_LSTM, lambda: pack_cells(self._cells(), self.lstm.input_size),
                             self.attention, self.embed, self.linear, maps, k, (h0, c0) + state)
        return step_fn, (h0, c0) + state + (() if img is None else (img,))

    def sample(self, features, start_token, end_token, k=5, on_device=False, poll_every=0, one_call=False, return_alphas=False,
               constraints=None, diversity=None, nbest=False, length_penalty=0.0):
        """Beam search with attention, nic/model_att.py:204-297. Returns LongTensor [1, L].
        on_device / poll_every: capnet.decode.beam_decode's (the bookkeeping on the device, same sequences).
        one_call: the whole search in one C call (capnet_att_beam_decode: the k beams of an image on one read of its maps);
        on_device=True for a shape that call does not take. Same sequences.
        return_alphas: -> (ids [1, L], alphas float32 [L - 1, P]), row e - 1 the attention map that preceded word e
        (capnet.decode.beam_decode: recorded by the one-call search, replayed on every other route).
        constraints: a capnet.beam.Constraints -- no n-gram twice, no <end> before min_words words, no banned word --
        kept inside the search on whichever route runs (capnet.decode.beam_decode); the scores stay the model's own.
        diversity: a capnet.beam.Diversity -- the k beams as groups that pay for the words earlier groups chose at the same
        step, for several different captions of one image (capnet.decode.beam_decode); the scores stay the model's own.
        nbest / length_penalty: capnet.decode.beam_decode's -- every completed hypothesis as a (tokens, score) pair, best
        first, in place of the one caption. With return_alphas, every hypothesis's own maps beside the list."""
        return beam_decode(self, *self._beam(features, None, k, one_call), None, k, start_token, end_token, on_device, poll_every, one_call,
                           return_alphas, nbest, length_penalty, constraints, diversity)

    def sample_random(self, features, start_token, end_token, samples=1, temperature=1.0, top_k=0, seed=None, top_p=1.0, device=False, greedy=False, exclude=None):
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
        return decode.sample_random(self, *self._beam(features, n, int(samples) + bool(greedy), True), n, samples, start_token, end_token,
                                    temperature, top_k, seed, top_p, device, greedy, exclude)

    def score_captions(self, features, captions):
        """float32 [len(captions)] on the device: the model's log-probability of every caption [start, w_1 .. w_j] given its
        image, summed over w_1 .. w_j (<end> too where present), in the caller's order. captions: a flat list of token lists,
        caption r on row r of `features` ([n, S, S, C] or [n, P, C]), or the nested list sample_random returns, list i on image
        i (the logprob of a (tokens, logprob) pair is ignored). Under no_grad, dropout following self.training:
        capnet.decode.score_captions."""
        return decode.score_captions(self, features, captions)

    def sample_batch(self, features, start_token, end_token, k=5, on_device=False, poll_every=0, one_call=False,
                     return_alphas=False, constraints=None, diversity=None, nbest=False, length_penalty=0.0):
        """sample() for every image of `features` ([n, S, S, C] or [n, P, C]) at once (capnet.beam.beam_search_batched).
        Returns a list of token lists, each equal to sample(features[i:i+1], ...)[0].tolist(); with return_alphas, (the n
        token lists, n float32 [len - 1, P] tensors) as sample()."""
        n = features.size(0)
        return beam_decode(self, *self._beam(features, n, k, one_call), n, k, start_token, end_token, on_device, poll_every, one_call,
                           return_alphas, nbest, length_penalty, constraints, diversity)
