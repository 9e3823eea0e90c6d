"""The cases of the forced-word beam-search tests (tests/test_forced_beam_cpu.py, tests/test_forced_beam_gpu.py).
TEST INFRASTRUCTURE.

End to end, a case is (family, forced set, k, image): the families of device_beam_cases, att_beam_cases and
beam_decode_cases (each name once) with their KS, IMAGES, MAX_LEN and MARGIN, under two forced sets per family (SETS: "one", a
single forced id, and "two", a pair with min_words=2). THE RULE is nbest_cases': a case is admitted only where the forced fp64
search's margin (forced_beam_ref.forced_search: every gap its pool and its allocation rest on) and the smallest gap of its
completed scores both exceed MARGIN. The ids were chosen per family so that every case is admitted and completes a hypothesis
within MAX_LEN; tests/test_forced_beam_cpu.py asserts both, and that in every family a case's unforced winner lacks a forced
word and its forced winner is another caption, so nothing is skipped or vacuous on the GPU.

The stored-logits tables drive capnet_beam_advance_forced and capnet_beam_topk_batched_forced against the fixed-slot model
(forced_beam_ref.ForcedBeam) without a decoder: n = 4 images, 7 steps, <end> = 2, normal noise of scale 6, one script per
image --
  0  the forced word W0 sits at -30 on every row at every step and <end> is far ahead: the plain search never emits W0, the
     forced search must, and its winner pays the word's full cost
  1  W1, a forced word of the sets with two or more, is the far-ahead word of step 2: it enters the pool through the plain
     selection, is the row's missing forced id and the row's best word too, and is taken once, banked by its met count
  2  <end> is held far down and at step 6 words 20 and 21 are EXACTLY equal and far ahead on every row: candidates of one
     bank that tie; the lower flat index wins
  3  <end> is far ahead from step 1 on: no hypothesis completes before every forced word is in; at k = 1 the walk is greedy
     on the highest bank that has a candidate
under TABLE_SETS: F = 1, F = 2, and F = 4 with no_repeat_ngram=1, min_words=3, banned=(9,), where a forced word that was
emitted is excluded and must not come back through the pool."""
import torch

import att_beam_cases
import beam_decode_cases
import device_beam_cases
import forced_beam_ref as R
import nbest_ref
import seq2seq_cases
from capnet.beam import Constraints
from device_beam_cases import IMAGES, KS, MARGIN, MAX_LEN, START   # noqa: F401

PENALTIES = (0.0, 1.0)
# per family (one forced id, a pair): chosen so that every case is admitted (tests/test_forced_beam_cpu.py)
FORCED = {
    "StackedFactoredLSTM-2": (4, (3, 5)), "StackedDecoderRNN-2": (4, (3, 6)), "DecoderRNNAtt": (4, (3, 5)),
    "StackedFactoredLSTMAtt-2": (4, (3, 5)), "DecoderFactoredLSTMAtt": (4, (3, 5)), "StackedDecoderRNNAtt-2": (4, (12, 13)),
    "StackedFactoredLSTMAtt-2-wide": (6, (4, 10)), "DecoderRNNAtt-wide": (4, (3, 5)), "DecoderFactoredLSTM": (4, (3, 5)),
    "DecoderRNN": (5, (3, 8)),
}


def sets(name):
    """The two forced sets of family `name`."""
    one, two = FORCED[name]
    return {"one": Constraints(forced=(one,)), "two": Constraints(min_words=2, forced=two)}


class Unit:
    """One family: the fp64 searches of its cases, computed once -- search(k, image, set name or None)."""

    def __init__(self, family):
        self.family, self.name, self.V = family, family.name, family.V
        self.sets = sets(family.name)
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
                self._search[(k, image, s)] = R.forced_search(step_fn, state, self.V, START, self.end, k, MAX_LEN, self.sets[s])
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

    def score_bound(self, k, image, s, words):
        """nbest_cases.Unit.score_bound's rule: (len - 1) x seq2seq_cases.need(scale)."""
        return words * seq2seq_cases.need(self.search(k, image, s).scale)

    def bites(self):
        """The first (set, k, image) whose unforced winner lacks a forced word and whose forced winner is another caption."""
        for s, c in self.sets.items():
            for k, i in self.cases():
                free = self.winner(k, i, None)
                if R.missing(free, c.forced) and self.winner(k, i, s) != free:
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
TABLE_N, TABLE_T, TABLE_END, TABLE_START = 4, 7, 2, 1
TABLE_KS = (1, 3, 5, 16)
TABLE_VS = (37, 1500)            # fewer entries than the workgroup's 1024 threads; the strided loop
WIDE_K = 5                       # the one table at V = 1500
TABLE_GAP = 1e-3                 # every gap the model's selections rest on, exact ties apart, is above this
W0, W1, W2, W3, TIE_A, TIE_B, BANNED = 10, 11, 12, 13, 20, 21, 9
TIE_STEP = 6
TABLE_SETS = {"F1": Constraints(forced=(W0,)), "F2": Constraints(forced=(W0, W1)),
              "F4": Constraints(no_repeat_ngram=1, min_words=3, banned=(BANNED,), forced=(W0, W1, W2, W3))}
TABLE_CASES = [(k, 37) for k in TABLE_KS] + [(WIDE_K, 1500)]


def table(k, V=37):
    """Logits [T][n k][V], the scripts of the module's docstring."""
    T = TABLE_T         # (the seed: the first from 40 on at which every table's model gap exceeds 2 TABLE_GAP)
    x = torch.randn(T, TABLE_N * k, V, generator=torch.Generator().manual_seed(103 + k + V)) * 6.0
    a, b, c, d = (slice(i * k, (i + 1) * k) for i in range(TABLE_N))
    x[:, a, W0] = -30.0                                       # image 0
    x[:, a, TABLE_END] = 60.0
    x[1, b, W1] = 60.0                                        # image 1
    x[:, c, TABLE_END] = -60.0                                # image 2
    x[TIE_STEP - 1, c, TIE_A] = x[TIE_STEP - 1, c, TIE_B] = 60.0
    x[:, d, TABLE_END] = 60.0                                 # image 3
    return x


def model(k, V, s, tab=None, constraints=None):
    """(the fixed-slot model after TABLE_T steps under TABLE_SETS[s] -- or under `constraints` --, the smallest gap its
    selections rest on)."""
    beam = R.ForcedBeam(TABLE_N, k, V, TABLE_START, TABLE_END, TABLE_SETS[s] if constraints is None else constraints)
    gap = R.drive(beam, table(k, V) if tab is None else tab)
    return beam, gap
