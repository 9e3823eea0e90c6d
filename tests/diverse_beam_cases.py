"""The cases of the diverse-beam-search tests (tests/test_diverse_beam_cpu.py, tests/test_diverse_beam_gpu.py).
TEST INFRASTRUCTURE.

End to end, a case is (family, (k, D, strength), image): the families of device_beam_cases, att_beam_cases and
beam_decode_cases (each name once) with their IMAGES, MAX_LEN and MARGIN, at (k, D) = (4, 2), (6, 2), (6, 3) and strength
1.0. THE RULE: a case is admitted only where the fp64 diverse search's margin (diverse_beam_ref.diverse_search: the gap
between the live-th key and the next one, in any group at any step) and the smallest gap between the ranking keys of its
completed hypotheses with distinct token lists, at length_penalty 0 and 1, all exceed MARGIN.
tests/test_diverse_beam_cpu.py asserts that every listed case is admitted, so nothing is skipped on the GPU.
Rejected at strength 1.0: StackedFactoredLSTMAtt-2-wide, (k, D) = (6, 3), image 2, whose margin is 4.3e-5; that family
runs (6, 3) at STRENGTH_OTHER instead (all its images: sample_batch takes one Diversity), chosen on the CPU by the rule.

The stored-logits tables drive capnet_beam_advance_diverse and capnet_beam_topk_batched_diverse against the fixed-slot
model (diverse_beam_ref.DiverseBeam) without a decoder: n = 3 images, 7 steps, normal noise of scale 6, one script per image
  0  word FAR is 60 ahead on every row at every step: every group wants it; <end> is held far down
  1  at step TIE_STEP word A_ is far ahead on group 0's rows, and on group 1's rows A_ and B_ > A_ are EXACTLY equal and far
     ahead: without the penalty the tie goes to A_, with any strength > 0 B_ must win
  2  <end> is far ahead on every row from step 3 (and far down before): group 0 dies at step 3; at a strength beyond every
     lead (1e4) group 1 cannot end at step 3 and must end at step 4, when the dead group counts nothing
at (k, D) of TABLE_CASES, V = 37 (fewer entries than the workgroup's 1024 threads) and one at V = 1500 (the strided loop).
V - 1 >= k in every table, so at 1e4 the groups of an image never share a word."""
import torch

import att_beam_cases
import beam_decode_cases
import device_beam_cases
import diverse_beam_ref as R
from capnet.beam import Constraints
from device_beam_cases import IMAGES, MARGIN, MAX_LEN, START   # noqa: F401

SHAPES = ((4, 2), (6, 2), (6, 3))
STRENGTH = 1.0
STRENGTH_OTHER = {("StackedFactoredLSTMAtt-2-wide", 6, 3): 0.75}
PENALTIES = (0.0, 1.0)
# with constraints (constrained_beam_cases' set D: no word twice, six words at least, two banned), a plain and an attention
# family, all images admitted by the same rule
CON_SET, CON_CASES = "D", (("DecoderFactoredLSTM", 4, 2), ("DecoderRNNAtt-wide", 4, 2))


class Unit:
    """One family: the fp64 searches of its cases, computed once."""

    def __init__(self, family):
        self.family, self.name, self.V = family, family.name, family.V
        self._search = {}

    def __repr__(self):
        return self.name

    @property
    def end(self):
        return self.family.end

    def strength(self, k, D):
        return STRENGTH_OTHER.get((self.name, k, D), STRENGTH)

    def search(self, k, D, image, strength=None, constraints=None):
        """The diverse fp64 search; D = 1: the plain k-beam search in the same form."""
        strength = self.strength(k, D) if strength is None else strength
        key = (k, D, image, strength, repr(constraints))
        if key not in self._search:
            self._search[key] = R.diverse_search(lambda rows: self.family.initial(rows, image), self.V, START, self.end, k, D,
                                                 strength, MAX_LEN, constraints)
        return self._search[key]

    def cases(self):
        return [(k, D, i) for k, D in SHAPES for i in range(IMAGES)]

    def smallest(self, k, D, image, **kw):
        q = self.search(k, D, image, **kw)
        return min([q.margin] + [q.gap(p) for p in PENALTIES])

    def admitted(self, k, D, image, **kw):
        return self.smallest(k, D, image, **kw) > MARGIN

    def score_bound(self, k, D, image, words, **kw):
        """constrained_beam_cases.Unit.score_bound's rule: (len - 1) x seq2seq_cases.need(scale)."""
        import seq2seq_cases
        return words * seq2seq_cases.need(self.search(k, D, image, **kw).scale)


def unit(name):
    return [u for u in units() if u.name == name][0]


def con_set():
    import constrained_beam_cases
    return constrained_beam_cases.SETS[CON_SET]


_units = None


def units():
    """Every family of the three case files, each name once, in their order."""
    global _units
    if _units is None:
        fams = {}
        for f in device_beam_cases.families() + att_beam_cases.families() + beam_decode_cases.families():
            fams.setdefault(f.name, f)
        _units = [Unit(f) for f in fams.values()]
    return _units


def is_attention(u):
    return u.name in {f.name for f in att_beam_cases.families()}


# ---- stored logits ---------------------------------------------------------------------------------------------------
TABLE_N, TABLE_T, TABLE_END, TABLE_START = 3, 7, 2, 1
TABLE_CASES = [(2, 2, 37), (4, 2, 37), (6, 3, 37), (16, 4, 37), (16, 16, 37), (6, 2, 1500)]      # (k, D, V)
TABLE_GAP = 1e-3                 # every gap the model's selections rest on, exact ties apart, is above this
TABLE_STRENGTHS = (0.5, 1e4)
FAR, A_, B_, BANNED = 3, 5, 6, 9
TIE_STEP, END_FROM = 2, 3
TABLE_CONSTRAINTS = Constraints(no_repeat_ngram=1, min_words=3, banned=(BANNED,))


def table(k, D, V=37):
    """Logits [T][n k][V], the scripts of the module's docstring."""
    n, T, E_, kp = TABLE_N, TABLE_T, TABLE_END, k // D
    x = torch.randn(T, n * k, V, generator=torch.Generator().manual_seed(31 + k + D + V)) * 6.0
    a, b, c = slice(0, k), slice(k, 2 * k), slice(2 * k, 3 * k)
    x[:, a, E_] = -60.0                                       # image 0
    x[:, a, FAR] = 60.0
    x[TIE_STEP - 1, k:k + kp, A_] = 60.0                      # image 1: group 0's rows, then group 1's
    x[TIE_STEP - 1, k + kp:k + 2 * kp, A_] = x[TIE_STEP - 1, k + kp:k + 2 * kp, B_] = 60.0
    x[:TIE_STEP, b, E_] = -60.0
    x[:END_FROM - 1, c, E_] = -60.0                           # image 2
    x[END_FROM - 1:, c, E_] = 60.0
    return x


def model(k, D, V, strength, tab=None, constraints=None):
    """(the fixed-slot model after TABLE_T steps, the smallest gap its selections rest on)."""
    beam = R.DiverseBeam(TABLE_N, k, D, strength, V, TABLE_START, TABLE_END, constraints)
    gap = R.drive(beam, table(k, D, V) if tab is None else tab)
    return beam, gap
