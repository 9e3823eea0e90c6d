"""The cases of the n-best tests (tests/test_nbest_cpu.py, tests/test_nbest_gpu.py). TEST INFRASTRUCTURE.

End to end, a case is (unit, k, image, penalty): a unit is one decoder under one mode -- a family of device_beam_cases /
att_beam_cases, a (family, mode) of style_decode_cases, a Case of seq2seq_beam_cases or one mode of a StyleCase of
seq2seq_beam_style_cases -- with its fp64 restatement initial(k, image) -> (step_fn, state). THE RULE: the case is
admitted only where the fp64 search's beam_margin exceeds the unit's bound (the search selects the same hypotheses) AND the
smallest gap between neighbours of its ranked completed list, in the ranking key at that penalty, exceeds it too (the
ranking is the same). The bound is device_beam_cases.MARGIN; for the seq2seq units seq2seq_beam_cases' max(MARGIN,
(MAX_LEN + 1) x need(scale)). tests/test_nbest_cpu.py asserts that EVERY case of every unit below is admitted, so nothing
is skipped on the GPU, and that every family (a unit's decoder: the modes of one style family count together) has a case with
three or more completed hypotheses and one that penalty 1 reorders. StackedDecoderRNNAtt-2 of att_beam_cases (seed 1) has
no case that penalty 1 reorders, so that class runs on a family of its own here, seed 5 -- the first seed from 2 upwards
at which every case is admitted and one is reordered. small-happy-s5 and the `angry` mode of small-all each have a case
whose penalty-1 gap is under the seq2seq bound: small-happy-s7 and the other three modes are used.

A score is a sum of len - 1 log-probabilities, each carrying a logit's error twice over: score_bound(search, tokens) =
(len - 1) x seq2seq_cases.need(scale), scale the largest |logit| the fp64 search met.

The stored-logits tables drive capnet_beam_advance_traced and then capnet_beam_nbest[_traced] against the Python model
(nbest_ref.NBestBeam) without a decoder: n = 3 images, V = 37, 6 steps, one script per image --
  0  step 1: words 3 and 4 far ahead, <end> third and far behind (the FIRST completion has the worst score: completion
     order differs from score order); step 2: <end> certain on slot 0 (the best raw score, two words); word 5 certain
     everywhere else until step 6 completes the rest: the line of word 4 ends with six words and a raw score below the
     two-word caption's, but above it per word -- the penalty changes rank 0; all k complete
  1  step 1: words 3 and 4 EXACTLY equal; step 2: slots 0 and 1 carry the same row with <end> certain -- two completions in
     one step with scores equal in fp32 (and in fp64), resolved to the earlier; step 3: <end> certain everywhere: all k
     complete, the image is dead from step 4 on
  2  nothing: <end> is never among the k best.
With k = 1 an image completes at most one hypothesis, so the situations are asserted for k >= 3 only."""
import torch
import torch.nn.functional as Fn

import att_beam_cases
import device_beam_cases
import nbest_ref
import seq2seq_beam_cases
import seq2seq_beam_style_cases
import seq2seq_cases
import style_decode_cases
from device_beam_cases import IMAGES, KS, MARGIN, MAX_LEN, START   # noqa: F401

PENALTIES = (0.0, 1.0)


class Unit:
    """name; kind: "image" (sample_batch of an image decoder), "style" (one mode of sample_styles), "seq2seq" (sample_beam)
    or "seq2seq-style" (one mode of sample_beam_styles); source: the family / case it wraps; mode: the mode keyword or
    None; images: its images / sentences."""

    def __init__(self, name, kind, source, V, initial, mode=None, images=IMAGES, ks=KS):
        self.name, self.kind, self.source, self.V, self.initial, self.mode = name, kind, source, V, initial, mode
        self.family = source.name
        self.images, self.ks = images, tuple(ks)
        self._search = {}

    def __repr__(self):
        return self.name

    @property
    def end(self):
        return self.source.end(self.mode) if self.kind == "seq2seq-style" else self.source.end

    def search(self, k, image):
        """nbest_ref.nbest_search of (k, image), computed once."""
        if (k, image) not in self._search:
            step_fn, state = self.initial(k, image)
            self._search[(k, image)] = nbest_ref.nbest_search(step_fn, state, self.V, START, self.end, k, MAX_LEN)
        return self._search[(k, image)]

    def bound(self):
        """What margin and gap must exceed: MARGIN; seq2seq: max(MARGIN, (MAX_LEN + 1) x need(scale)) at the largest |logit|
        any of the unit's searches met."""
        if not self.kind.startswith("seq2seq"):
            return MARGIN
        scale = max(self.search(k, i).scale for k in self.ks for i in range(self.images))
        return max(MARGIN, (MAX_LEN + 1) * seq2seq_cases.need(scale))

    def cases(self):
        return [(k, i) for k in self.ks for i in range(self.images)]

    def admitted(self, k, image, penalty):
        s = self.search(k, image)
        return s.margin > self.bound() and s.gap(penalty) > self.bound()

    def nbest(self, k, image, penalty):
        """[(tokens, score)] in fp64, best first. (seq2seq `factual`: sample_beam drops the seeding START.)"""
        out = self.search(k, image).nbest(penalty)
        if self.kind.startswith("seq2seq") and self.mode == "factual":
            out = [(q[1:], s) for q, s in out]
        return out

    def score_bound(self, k, image, words):
        """The bound on |score - fp64 score| of a hypothesis of `words` generated words."""
        return words * seq2seq_cases.need(self.search(k, image).scale)


def _family_unit(f):
    return Unit(f.name, "image", f, f.V, f.initial, f.kw.get("mode"))


def _style_unit(f, mode):
    return Unit("%s/%s" % (f.name, mode), "style", f, f.V, lambda k, i: f.initial(mode, k, i), mode)


def _seq2seq_unit(c):
    return Unit(c.name, "seq2seq", c, c.V, c.initial, c.mode, images=c.rows, ks=c.ks)


def _seq2seq_style_units(sc):
    return [Unit("%s/%s" % (sc.name, m), "seq2seq-style", sc, sc.V, sc.cases[m].initial, m, images=sc.rows, ks=sc.ks)
            for m in sc.modes]


STYLES = {"StackedFactoredLSTM-2": ("happy", "sad", "angry"), "StackedFactoredLSTMAtt-2": ("factual", "happy", "sad")}
SEQ2SEQ_CASES = ("small-happy-s7", "small-factual-s7")
SEQ2SEQ_STYLE_CASE, SEQ2SEQ_STYLE_MODES = "small-all", ("factual", "happy", "sad")
STACKED_RNN_ATT = "StackedDecoderRNNAtt-2-s5"
ATT_CLASSES = {"DecoderRNNAtt": "DecoderRNNAtt", "StackedFactoredLSTMAtt-2": "StackedFactoredLSTMAtt",
               "DecoderFactoredLSTMAtt": "DecoderFactoredLSTMAtt", STACKED_RNN_ATT: "StackedDecoderRNNAtt"}


def _stacked_rnn_att():
    from capnet.nic_stacked import StackedDecoderRNNAtt
    return att_beam_cases._rnn_att(STACKED_RNN_ATT, StackedDecoderRNNAtt, 2, 5, A=16, E=12, H=64, V=37, Cf=512, P=6)


_units = None


def units():
    """Every unit, by name."""
    global _units
    if _units is None:
        us = [_family_unit(f) for f in device_beam_cases.families()]
        us += [_family_unit(f) for f in att_beam_cases.new_families() + [_stacked_rnn_att()] if f.name in ATT_CLASSES]
        us += [_style_unit(style_decode_cases.family(n), m) for n, modes in STYLES.items() for m in modes]
        us += [_seq2seq_unit(seq2seq_beam_cases.case(n)) for n in SEQ2SEQ_CASES]
        us += [u for u in _seq2seq_style_units(seq2seq_beam_style_cases.case(SEQ2SEQ_STYLE_CASE)) if u.mode in SEQ2SEQ_STYLE_MODES]
        _units = {u.name: u for u in us}
    return _units


def of_kind(kind):
    return [u for u in units().values() if u.kind == kind]


def families():
    """{family name: its units}: the units of one decoder."""
    out = {}
    for u in units().values():
        out.setdefault((u.kind, u.family), []).append(u)
    return out


def device_units():
    """The four families of tests/device_beam_cases.py: 24 cases."""
    names = [f.name for f in device_beam_cases.families()]
    return [units()[n] for n in names]


def att_units():
    """One unit per attention class."""
    return [units()[n] for n in ATT_CLASSES]


# ---- stored logits ---------------------------------------------------------------------------------------------------
TABLE_N, TABLE_T, TABLE_V, TABLE_END, TABLE_START = 3, 6, 37, 2, 1
TABLE_KS = (1, 3, 5, 16)
TABLE_GAP = 1e-3          # every gap the model's selections and rankings rest on, exact ties apart, is above this
SITUATIONS = {"completion order differs from score order", "two equal scores", "nothing completed", "all k completed",
              "several completions in one step", "the penalty changes rank 0"}


def table(k):
    """Logits [T][n k][V]: normal noise of scale 6 with <end> held far down, then the scripts of the module's docstring."""
    n, T, V, E_ = TABLE_N, TABLE_T, TABLE_V, TABLE_END
    x = torch.randn(T, n * k, V, generator=torch.Generator().manual_seed(11 + k)) * 6.0
    x[:, :, E_] = -60.0
    a, b = slice(0, k), slice(k, 2 * k)
    # image 0
    x[0, 0, 3], x[0, 0, 4], x[0, 0, E_] = 42.0, 41.5, 36.0
    x[1, 0, E_] = 60.0
    x[1, 1:k, 5] = 60.0
    x[2:5, a, 5] = 60.0
    x[5, a, E_] = 60.0
    # image 1
    x[0, k, 3] = x[0, k, 4] = 42.0
    x[1, k, E_] = 60.0
    if k > 1:
        x[1, k + 1] = x[1, k]
    x[2, b, E_] = 60.0
    return x


def drive_model(k, tab=None):
    """nbest_ref.NBestBeam over table(k), its top-k in fp64 with ties to the lower flat index (the kernel's rule) ->
    (the beam, the smallest non-zero gap between neighbours among the candidates taken and the first one left out)."""
    n, T, V = TABLE_N, TABLE_T, TABLE_V
    tab = table(k) if tab is None else tab
    beam = nbest_ref.NBestBeam(n, k, V, TABLE_START, TABLE_END)
    gap = [float("inf")]
    for step in range(1, T + 1):
        logp = Fn.log_softmax(tab[step - 1].double(), dim=1)

        def topk(i, nrows, kk, logp=logp):
            prev = torch.tensor(beam.scores[i], dtype=torch.float64)
            flat = (prev[:nrows, None] + logp[i * k:i * k + nrows]).reshape(-1).tolist()
            best = sorted(range(len(flat)), key=lambda j: (-flat[j], j))[:kk + 1]
            for p, q in zip(best, best[1:]):
                if flat[p] != flat[q]:
                    gap[0] = min(gap[0], flat[p] - flat[q])
            return [flat[j] for j in best[:kk]], best[:kk]
        beam.advance(step, topk)
    return beam, gap[0]


def table_rank_gap(beam, penalty):
    """The smallest non-zero gap in the key between neighbours of any image's ranked list."""
    gap = float("inf")
    for i in range(beam.n):
        keys = sorted((nbest_ref.key(s, q, penalty) for s, q in beam.completed(i)), reverse=True)
        gap = min([gap] + [a - b for a, b in zip(keys, keys[1:]) if a != b])
    return gap
