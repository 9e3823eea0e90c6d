"""The cases of the constrained-beam-search tests (tests/test_constrained_beam_cpu.py, tests/test_constrained_beam_gpu.py).
TEST INFRASTRUCTURE.

End to end, a case is (family, constraint set, k, image): the families of device_beam_cases, att_beam_cases and
beam_decode_cases (each name once) with their KS, IMAGES, MAX_LEN and MARGIN, under four constraint sets
  A  no_repeat_ngram=1      B  no_repeat_ngram=2      C  min_words=4      D  no_repeat_ngram=1, min_words=6, banned=(0, 2)
THE RULE is nbest_cases': a case is admitted only where the constrained fp64 search's margin (constrained_beam_ref) and the
smallest gap of its completed scores both exceed MARGIN. tests/test_constrained_beam_cpu.py asserts that every case is
admitted, so nothing is skipped on the GPU, and that every set changes what the unconstrained search returns (C in every
family but DecoderFactoredLSTM, whose unconstrained captions already have four words).

The stored-logits tables drive capnet_beam_advance_constrained[_traced] and capnet_beam_topk_batched_banned against the
fixed-slot model (constrained_beam_ref.ConstrainedBeam) without a decoder: n = 3 images, 7 steps, normal noise of scale 6
with <end> held far down, one script per image --
  0  word 3 is far ahead on every row at every step: the unconstrained search repeats it forever; under g = 1 and g = 2 it
     must not
  1  the best hypothesis is forced into  a b a c a  (a = 5, b = 6, c = 7) and at step 6 words 6 and 8 are EXACTLY equal and
     far ahead on its row: under g = 2 both b and c are excluded behind a, the lower flat index of the tie is gone and 8
     must win
  2  <end> is far ahead from step 1 on and min_words = 3: every beam completes at step 4 exactly; word 9, banned, is ahead
     even of <end> on every row at every step -- and, left in the rows' log-sum-exp, costs every step about 10 nats
under the two sets TABLE_SETS (g = 1 and g = 2, both with min_words = 3 and banned = (9,))."""
import torch

import att_beam_cases
import beam_decode_cases
import constrained_beam_ref as R
import device_beam_cases
import nbest_ref
import seq2seq_cases
from capnet.beam import Constraints
from device_beam_cases import IMAGES, KS, MARGIN, MAX_LEN, START   # noqa: F401

SETS = {"A": Constraints(no_repeat_ngram=1), "B": Constraints(no_repeat_ngram=2), "C": Constraints(min_words=4),
        "D": Constraints(no_repeat_ngram=1, min_words=6, banned=(0, 2))}
PENALTIES = (0.0, 1.0)
C_UNCHANGED = ("DecoderFactoredLSTM",)       # set C changes nothing there


class Unit:
    """One family: the fp64 searches of its cases, computed once -- search(k, image, set name or None)."""

    def __init__(self, family):
        self.family, self.name, self.V = family, family.name, family.V
        self._search = {}

    def __repr__(self):
        return self.name

    @property
    def end(self):
        return self.family.end

    def search(self, k, image, s):
        if (k, image, s) not in self._search:
            step_fn, state = self.family.initial(k, image)
            if s is None:
                self._search[(k, image, s)] = nbest_ref.nbest_search(step_fn, state, self.V, START, self.end, k, MAX_LEN)
            else:
                self._search[(k, image, s)] = R.constrained_search(step_fn, state, self.V, START, self.end, k, MAX_LEN, SETS[s])
        return self._search[(k, image, s)]

    def cases(self):
        return [(k, i) for k in KS for i in range(IMAGES)]

    def admitted(self, k, image, s, penalty=0.0):
        q = self.search(k, image, s)
        return q.margin > MARGIN and q.gap(penalty) > MARGIN

    def winner(self, k, image, s):
        """The caption the call without nbest returns: the first maximum of the completed scores, [<end>] for none."""
        best = self.search(k, image, s).nbest(0.0)
        return best[0][0] if best else [self.end]

    def changed(self, s):
        """The cases whose completed lists differ from the unconstrained search's."""
        return [(k, i) for k, i in self.cases()
                if [q for _, q in self.search(k, i, s).done] != [q for _, q in self.search(k, i, None).done]]

    def score_bound(self, k, image, s, words):
        """nbest_cases.Unit.score_bound's rule: (len - 1) x seq2seq_cases.need(scale)."""
        return words * seq2seq_cases.need(self.search(k, image, s).scale)


def other_winner(u):
    """The first (set, k, image) of `u`, among its changed cases, whose winner is not the unconstrained search's; None for none."""
    for s in SETS:
        for k, i in u.changed(s):
            if u.winner(k, i, s) != u.winner(k, i, None):
                return s, k, i
    return None


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
TABLE_KS = (1, 3, 5, 16)
TABLE_VS = (37, 1500)            # fewer entries than the workgroup's 1024 threads; the strided loop
WIDE_K = 5                       # the one table at V = 1500
TABLE_GAP = 1e-3                 # every gap the model's selections rest on, exact ties apart, is above this
FAR, A_, B_, C_, TIE, BANNED = 3, 5, 6, 7, 8, 9
TABLE_MIN_WORDS = 3
TABLE_SETS = {"g1": Constraints(no_repeat_ngram=1, min_words=TABLE_MIN_WORDS, banned=(BANNED,)),
              "g2": Constraints(no_repeat_ngram=2, min_words=TABLE_MIN_WORDS, banned=(BANNED,))}
TABLE_CASES = [(k, 37) for k in TABLE_KS] + [(WIDE_K, 1500)]


def table(k, V=37):
    """Logits [T][n k][V], the scripts of the module's docstring."""
    n, T, E_ = TABLE_N, TABLE_T, TABLE_END
    x = torch.randn(T, n * k, V, generator=torch.Generator().manual_seed(23 + k + V)) * 6.0
    x[:, :, E_] = -60.0
    x[:, :, BANNED] = -60.0
    a, b, c = slice(0, k), slice(k, 2 * k), slice(2 * k, 3 * k)
    x[:, a, FAR] = 60.0                                       # image 0
    for t, w in enumerate((A_, B_, A_, C_, A_)):              # image 1
        x[t, b, w] = 60.0
    x[5, b, B_] = x[5, b, TIE] = 60.0
    x[:, c, E_] = 60.0                                        # image 2
    x[:, c, BANNED] = 70.0
    return x


def model(k, V, s, tab=None, constraints=None):
    """(the fixed-slot model after TABLE_T steps under TABLE_SETS[s] -- or under `constraints` --, the smallest gap its
    selections rest on)."""
    beam = R.ConstrainedBeam(TABLE_N, k, V, TABLE_START, TABLE_END, TABLE_SETS[s] if constraints is None else constraints)
    gap = R.drive(beam, table(k, V) if tab is None else tab)
    return beam, gap
