"""Inputs shared by tests/test_seq2seq_constrained_cpu.py (the rule) and tests/test_seq2seq_constrained_gpu.py (the runs):
capnet.seq2seq's constrained beam searches (Seq2Seq.sample_beam_constrained) against their fp64 restatement. TEST INFRASTRUCTURE.

A case is a seq2seq_beam_cases.Case (its shape, parameters, features, <end> and Case.initial(k, r)) under three constraint
sets, each a function of the case alone:
  D  Constraints(no_repeat_ngram=1, min_words=6, banned=(a, b)): a, b the first two distinct words, neither START nor <end>,
     of what the UNCONSTRAINED search returns for sentence 0 at the case's first k -- so the set bans words the model emits
  B  Constraints(no_repeat_ngram=2)
  F  Constraints(forced=(w,)): w the smallest id from 3 up that is not <end> and occurs in no unconstrained winner of the
     case -- so the forced word is never met by accident
The restatement: tests/constrained_beam_ref.constrained_search on Case.initial(k, r) for D and B; for F
tests/forced_beam_ref.forced_search, which is that loop with the forced-word allocation in topk's place (constrained_search
knows nothing of the allocation). What a call returns is the first maximum of the completed scores ([<end>] for none),
`factual` without the seeding START.

THE RULE is seq2seq_beam_cases', on the constrained search: a (case, set) is compared only if the search's margin at every
(k, sentence) exceeds
    max(MARGIN, (MAX_LEN + 1) x seq2seq_cases.need(scale)),    scale = the largest |logit| the case has met,
and, for an emotion case, the encoder's greedy gap exceeds need(scale). Asked on top of it, because the n-best lists are
compared in order: the smallest gap between two completed scores of a search exceeds the same bound.
tests/test_seq2seq_constrained_cpu.py asserts all of it for every (case, set) below, and that every set changes what the
unconstrained search returns on every case; nothing is skipped on the GPU. Seeds: per (shape, set) the first from 0 upwards
that clears the rule at the shape (search())."""
import constrained_beam_ref as R
import forced_beam_ref as FR
import nbest_ref
import seq2seq_beam_cases as BC
import seq2seq_cases as SC
from capnet.beam import Constraints
from device_beam_cases import MARGIN, MAX_LEN, START

SET_NAMES = ("D", "B", "F")


class Unit:
    """One Case: its constraint sets and the fp64 searches of its (set, k, sentence), computed once. set None: the
    unconstrained search."""

    def __init__(self, case):
        self.case, self.name = case, case.name
        self._search, self._sets = {}, None

    def __repr__(self):
        return self.name

    @property
    def end(self):
        return self.case.end

    @property
    def sets(self):
        if self._sets is None:
            end = self.end
            first = [w for w in self.winner(None, self.case.ks[0], 0)[1:] if w not in (START, end)]
            ab = tuple(dict.fromkeys(first))[:2]
            assert len(ab) == 2, "the unconstrained caption of sentence 0 has fewer than two distinct words"
            seen = {w for k, r in self.cells() for w in self.winner(None, k, r)}
            forced = [w for w in range(3, self.case.V) if w != end and w not in seen][0]
            self._sets = {"D": Constraints(no_repeat_ngram=1, min_words=6, banned=ab), "B": Constraints(no_repeat_ngram=2),
                          "F": Constraints(forced=(forced,))}
        return self._sets

    def cells(self):
        return [(k, r) for k in self.case.ks for r in range(self.case.rows)]

    def search(self, s, k, r):
        if (s, k, r) not in self._search:
            c = self.case
            step_fn, state = c.initial(k, r)
            if s is None:
                q = nbest_ref.nbest_search(step_fn, state, c.V, START, self.end, k, MAX_LEN)
            elif self.sets[s].forced:
                q = FR.forced_search(step_fn, state, c.V, START, self.end, k, MAX_LEN, self.sets[s])
            else:
                q = R.constrained_search(step_fn, state, c.V, START, self.end, k, MAX_LEN, self.sets[s])
            self._search[(s, k, r)] = q
        return self._search[(s, k, r)]

    def winner(self, s, k, r):
        """The search's caption, START included: the first maximum of the completed scores, [<end>] for none."""
        best = self.search(s, k, r).nbest(0.0)
        return best[0][0] if best else [self.end]

    def _cut(self, tokens):
        return tokens[1:] if self.case.mode == "factual" and len(tokens) > 1 else tokens

    def reference(self, s, k, r):
        """What sample_beam_constrained(..., sets[s]) returns for sentence r."""
        return self._cut(self.winner(s, k, r))

    def nbest(self, s, k, r):
        """What sample_beam_constrained(..., sets[s], nbest=True) returns for sentence r: [(tokens, score)], best first; `factual`
        without START (every hypothesis has more than one token)."""
        drop = 1 if self.case.mode == "factual" else 0
        return [(q[drop:], sc) for q, sc in self.search(s, k, r).nbest(0.0)]

    def scale(self, s):
        """The largest |logit| on the way to set s's answers: the searches' own and the encoder's greedy pass."""
        qs = [self.search(s, k, r) for k, r in self.cells()]       # (the searches first: Case.scale grows as they run)
        return max([q.scale for q in qs] + [self.case.scale])

    def check(self, s):
        """(the smallest margin, the smallest gap between completed scores, the bound both must exceed, the encoder's greedy
        gap and its bound) of set s over every (k, sentence)."""
        qs = [self.search(s, k, r) for k, r in self.cells()]
        scale = self.scale(s)
        return (min(q.margin for q in qs), min(q.gap(0.0) for q in qs), max(MARGIN, (MAX_LEN + 1) * SC.need(scale)),
                self.case.encoder_gap, SC.need(scale))

    def clears(self, s):
        margin, gap, bound, enc, enc_bound = self.check(s)
        return margin > bound and gap > bound and enc > enc_bound

    def changed(self, s):
        """The (k, sentence) whose completed lists differ from the unconstrained search's."""
        return [(k, r) for k, r in self.cells()
                if [q for _, q in self.search(s, k, r).done] != [q for _, q in self.search(None, k, r).done]]

    def moved(self, s):
        """The (k, sentence) whose returned caption differs from the unconstrained search's."""
        return [(k, r) for k, r in self.cells() if self.winner(s, k, r) != self.winner(None, k, r)]

    def completes(self, s):
        """Whether all but at most one (k, sentence) return a completed caption (a search may end with nothing completed and
        return [<end>]; a case made of those would test little)."""
        done = [len(self.winner(s, k, r)) > 1 for k, r in self.cells()]
        return sum(done) >= len(done) - 1

    def usable(self, s):
        """Whether set s is well-formed here, clears the rule, moves a returned caption and completes()."""
        try:
            self.sets[s].check(self.case.V, self.end, max(self.case.ks), MAX_LEN + 1)
            return bool(self.clears(s) and self.moved(s) and self.completes(s))
        except Exception:     # a set that cannot be formed, a step with fewer than k finite candidates
            return False


def search(E, H, V, L, rows, mode, out_scale, lstm_scale, s, ks=BC.KS, seeds=range(200)):
    """The first seed whose case is usable(s), or None."""
    for seed in seeds:
        if Unit(BC.Case("probe", E, H, V, L, rows, seed, mode, out_scale, lstm_scale, ks)).usable(s):
            return seed
    return None


SHAPES = {
    "small-happy": (12, 64, 37, 2, 3, "happy", 24.0, 3.0),         # two workgroups, the last ragged; two layers
    "small-factual": (12, 64, 37, 2, 3, "factual", 24.0, 3.0),     # step 1 on the feature column
    "e10-l1-sad": (10, 64, 37, 1, 3, "sad", 24.0, 3.0),            # an embedding width off 4 (scalar loads), one layer
    "mid-factual": (30, 128, 211, 1, 3, "factual", 32.0, 3.0),     # seven workgroups, the last ragged, H = 128
    # a hidden size the decode step does not take: capnet.beam.beam_search_device(constraints=) on the composed step
    "h16-happy": (12, 16, 37, 1, 3, "happy", 24.0, 3.0),
}
COMPOSED = ("h16-happy",)
# (shape, set) -> the first seed from 0 upwards that search() admits. Every (shape, set) has a seed of its own: few (seed,
# set) pairs clear the rule at all six (k, sentence), and hardly a seed does so under all three sets at once
SEEDS = {
    ("small-happy", "D"): 20, ("small-happy", "B"): 7, ("small-happy", "F"): 74,
    ("small-factual", "D"): 4, ("small-factual", "B"): 15, ("small-factual", "F"): 129,
    ("e10-l1-sad", "D"): 1, ("e10-l1-sad", "B"): 33, ("e10-l1-sad", "F"): 186,
    ("mid-factual", "D"): 5, ("mid-factual", "B"): 340,          # (F: no seed below 600 is usable at this shape)
    ("h16-happy", "D"): 42, ("h16-happy", "B"): 21, ("h16-happy", "F"): 406,
}

_units = {}


def pairs():
    """Every (Unit, set name) of the tests, one Unit per (shape, seed)."""
    out = []
    for (shape, s), seed in SEEDS.items():
        if (shape, seed) not in _units:
            E, H, V, L, rows, mode, out_scale, lstm_scale = SHAPES[shape]
            _units[(shape, seed)] = Unit(BC.Case("%s-s%d" % (shape, seed), E, H, V, L, rows, seed, mode, out_scale, lstm_scale))
            _units[(shape, seed)].shape = shape
        out.append((_units[(shape, seed)], s))
    return out


def pair_id(p):
    return "%s/%s" % (p[0].name, p[1])


def is_composed(u):
    return u.shape in COMPOSED
