"""Inputs shared by tests/test_seq2seq_beam_cpu.py (the rule) and tests/test_seq2seq_beam_gpu.py (the runs): capnet.seq2seq's
sample_beam against its fp64 restatement. TEST INFRASTRUCTURE.

The restatement is oracle.beam_ref._beam on a step_fn made of seq2seq_ref.step and seq2seq_ref._logits; the state is the
tuple of the per-layer h and c. `factual` (EncoderRNN.sample_beam): zeros, and the first call is on the sentence's
`features` row; an emotion (Seq2Seq.sample_beam): sentence r's column of the encoder's greedy final state, every call on
the previous words. <end> is the fifth token of sentence 0's greedy decode (device_beam_cases.Family.end's choice).

THE RULE. The device computes in fp32, and the fused selection's logits differ from the unfused path's in the last bits, so
a case is compared only if device_beam_ref.beam_margin of every (k, sentence) exceeds
    max(device_beam_cases.MARGIN, (MAX_LEN + 1) x seq2seq_cases.need(scale)),    scale = the largest |logit| met:
a candidate's score is a sum of at most MAX_LEN + 1 log-probabilities, each carrying a logit's error twice over. An emotion
case starts from the encoder's GREEDY state, so there the encoder's smallest top-1 / top-2 gap must clear need(scale) too
(seq2seq_cases' rule). tests/test_seq2seq_beam_cpu.py asserts both for every case below; nothing is skipped on the GPU.
Seeds are the first from 0 upwards that clear the rule at the case's shape and scales (search(): about one (seed, mode)
pair in five does)."""
import torch

import seq2seq_cases as SC
import seq2seq_ref as SR
from device_beam_cases import MARGIN, MAX_LEN, START
from device_beam_ref import beam_margin
from oracle import beam_ref

KS = (3, 5)


class Case:
    def __init__(self, name, E, H, V, L, rows, seed, mode, out_scale, lstm_scale, ks=KS):
        self.name, self.E, self.H, self.V, self.L, self.rows, self.seed, self.mode = name, E, H, V, L, rows, seed, mode
        self.out_scale, self.lstm_scale, self.ks = out_scale, lstm_scale, tuple(ks)
        self.prefix = "encoder" if mode == "factual" else "decoder_" + mode
        self._made = self._end = None
        self.scale = 0.0                       # the largest |logit| any step_fn of this case has met
        self._ref = {}

    def __repr__(self):
        return self.name

    # ---- inputs ----
    def _make(self):
        if self._made is None:
            p = SR.make_params(SC.shapes(self.E, self.H, self.V, self.L), seed=1000 + self.seed, out_scale=self.out_scale,
                               lstm_scale=self.lstm_scale)
            g = torch.Generator().manual_seed(2000 + self.seed)
            feats = torch.randn(self.rows, self.E, generator=g, dtype=torch.float64) * 0.5
            states, gap = None, float("inf")
            if self.mode != "factual":
                _, states, gap, scale = SR.greedy(p, "encoder", self.L, MAX_LEN, features=feats)
                self.scale = max(self.scale, scale)
            self._made = (p, feats, states, gap)
        return self._made

    @property
    def params(self):
        return self._make()[0]

    @property
    def features(self):
        """[rows, E] fp64."""
        return self._make()[1]

    @property
    def encoder_gap(self):
        """The smallest top-1 / top-2 logit gap of the encoder's greedy pass (inf for `factual`: it is not run)."""
        return self._make()[3]

    def module(self):
        """capnet.seq2seq.Seq2Seq on the CPU with the case's parameters, max_seq_length MAX_LEN everywhere."""
        from capnet.seq2seq import Seq2Seq
        m = Seq2Seq(self.E, self.H, self.V, self.L, dropout=0.0, max_seq_length=MAX_LEN)
        m.load_state_dict({k: v.float() for k, v in self.params.items()})
        for x in (m.encoder, m.decoder_happy, m.decoder_sad, m.decoder_angry):
            x.max_seq_length = MAX_LEN
        return m.eval()

    # ---- the restatement ----
    def initial(self, k, r):
        """(step_fn, state) of sentence r with k beams."""
        p, feats, states, _ = self._make()
        L, prefix = self.L, self.prefix
        if states is None:
            z = torch.zeros(k, self.H, dtype=torch.float64)
            state = tuple(z.clone() for _ in range(2 * L))
            first = feats[r:r + 1]
        else:
            h, c = states
            state = tuple(h[l, r:r + 1].expand(k, -1).clone() for l in range(L)) + \
                tuple(c[l, r:r + 1].expand(k, -1).clone() for l in range(L))
            first = None
        calls = [0]

        def step_fn(prev_words, state):
            calls[0] += 1
            rows = state[0].shape[0]
            if calls[0] == 1 and first is not None:
                x = first.expand(rows, -1)
            else:
                x = p[prefix + ".embed.weight"][prev_words.reshape(-1)]
            top, hs, cs = SR.step(p, prefix, L, x, list(state[:L]), list(state[L:]))
            out = SR._logits(p, prefix, top)
            self.scale = max(self.scale, float(out.abs().max()))
            return out, tuple(hs + cs)
        return step_fn, state

    @property
    def end(self):
        if self._end is None:
            step_fn, state = self.initial(1, 0)
            words = torch.LongTensor([[START]])
            for _ in range(5):
                logits, state = step_fn(words, state)
                words = logits.argmax(1, keepdim=True)
            self._end = int(words)
        return self._end

    def margin(self, k, r):
        step_fn, state = self.initial(k, r)
        return beam_margin(step_fn, state, self.V, START, self.end, k, MAX_LEN)

    def beam(self, k, r, end=None):
        """oracle.beam_ref._beam's list of sentence r, START included."""
        step_fn, state = self.initial(k, r)
        return beam_ref._beam(step_fn, state, self.V, START, self.end if end is None else end, k, MAX_LEN)[0].tolist()

    def reference(self, k, r):
        """What the case's sample_beam returns for sentence r: _beam's list; `factual` without the seeding START."""
        if (k, r) not in self._ref:
            s = self.beam(k, r)
            self._ref[(k, r)] = s[1:] if self.mode == "factual" and len(s) > 1 else s
        return self._ref[(k, r)]

    def check(self):
        """(smallest beam margin over every (k, sentence), the bound it must exceed, the encoder's greedy gap and its
        bound). The margins are computed first: the bound uses the largest |logit| they met."""
        m = min(self.margin(k, r) for k in self.ks for r in range(self.rows))
        return m, max(MARGIN, (MAX_LEN + 1) * SC.need(self.scale)), self.encoder_gap, SC.need(self.scale)

    def clears(self):
        m, bound, gap, gbound = self.check()
        return m > bound and gap > gbound


def search(E, H, V, L, rows, mode, out_scale, lstm_scale, ks=KS, seeds=range(40)):
    """The first seed whose case clears the rule, or None."""
    for seed in seeds:
        if Case("probe", E, H, V, L, rows, seed, mode, out_scale, lstm_scale, ks).clears():
            return seed
    return None


SMALL = dict(E=12, H=64, V=37, L=2, rows=3, out_scale=24.0, lstm_scale=3.0)
FULL = dict(E=300, H=512, V=8192, L=2, rows=2, out_scale=64.0, lstm_scale=2.0, ks=(5,))

CASES = [
    Case("small-happy-s5", seed=5, mode="happy", **SMALL),          # two workgroups, the last ragged; lists of 5 to 10 tokens
    Case("small-happy-s7", seed=7, mode="happy", **SMALL),
    Case("small-factual-s7", seed=7, mode="factual", **SMALL),
    Case("full-factual-s2", seed=2, mode="factual", **FULL),
    Case("full-angry-s3", seed=3, mode="angry", **FULL),
    # an embedding width off 4 (layer 0's inputs by scalar loads), one layer; three layers
    Case("e10-l1-happy-s0", 10, 64, 37, 1, 3, 0, "happy", 24.0, 3.0),
    Case("e10-l1-factual-s10", 10, 64, 37, 1, 3, 10, "factual", 24.0, 3.0),      # seeds 0..9 do not clear the rule
    Case("l3-happy-s3", 12, 64, 37, 3, 3, 3, "happy", 24.0, 3.0),                # seeds 0..2 do not
    Case("l3-factual-s6", 12, 64, 37, 3, 3, 6, "factual", 24.0, 3.0),            # seeds 0..5 do not
    # seven workgroups, the last ragged, H = 128 (`happy`: no seed below 30 clears at out_scale 32)
    Case("mid-factual-s15", 30, 128, 211, 1, 3, 15, "factual", 32.0, 3.0),        # seeds 0..14 do not
]

# a hidden size the decode step does not take (16): capnet.beam.beam_search_device on the composed step
COMPOSED = [
    Case("h16-happy-s15", 12, 16, 37, 1, 3, 15, "happy", 24.0, 3.0),             # seeds 0..14 do not clear the rule
    Case("h16-factual-s0", 12, 16, 37, 1, 3, 0, "factual", 24.0, 3.0),
]


def case(name):
    return [c for c in CASES + COMPOSED if c.name == name][0]
