"""The cases of the per-image beam-search tests (tests/test_per_image_beam_cpu.py, tests/test_per_image_beam_gpu.py).
TEST INFRASTRUCTURE.

The oracle is exact: image i of a mixed batch must return what image i returns when searched ALONE under its own entry. So
nothing new is computed here -- an entry is a key into the fp64 searches the forced and the constrained tests already keep
per (family, set, k, image): ("forced", s) -> forced_beam_cases.Unit.search(k, i, s), ("con", s) ->
constrained_beam_cases.Unit.search(k, i, s), None -> the unconstrained search.

End to end, the families, KS, IMAGES = 3, MAX_LEN and MARGIN are forced_beam_cases'. Two assignments per family:
  A  image 0 -> the family's forced set "one", image 1 -> a non-forced set of constrained_beam_cases.SETS (NON_FORCED, per
     family), image 2 -> None
  B  A rotated by one image: image 0 -> None, image 1 -> the forced set, image 2 -> the non-forced set
THE RULE is the existing one: a case (family, k, image, entry) is admitted only where that search's margin and the smallest
gap of its completed scores exceed MARGIN. tests/test_per_image_beam_cpu.py asserts that every case used is admitted, and
that every family has a k at which the winners under A differ from the winners under B and from the winners under each single
entry applied to all three images (telling_k finds it) -- so a table read at the wrong row, or one image's rule leaking to
another, cannot pass. NON_FORCED was chosen per family so that this holds.

Stored logits: forced_beam_cases.table over its TABLE_CASES (n = 4 independent images), under
  first   image 0 -> F1, image 1 -> F2, image 2 -> constrained_beam_cases.TABLE_SETS["g1"], image 3 -> F4
  second  image 0 -> F4, image 1 -> F2, image 2 -> None, image 3 -> F1
The expectation is composed from the existing fixed-slot model (forced_beam_ref.ForcedBeam, which without forced ids is the
constrained model and without anything the plain one) driven over the table under entries[i], of which image i's slice is
taken. The images of those tables are independent, and the smallest gap is taken over the decisions the expectation rests
on -- image i's own under entries[i]: the model is driven with the other three images dead from the start (they select
nothing and add no gap; image i's selections are what they are in the whole model). It must exceed TABLE_GAP, as today. (Over
all four images the model under "g1" at k = 16, V = 37 has a gap of 6.9e-05 -- in image 1, which no assignment puts under
"g1"; image 2's own is 5.4e-03.)"""
import constrained_beam_cases as CC
import forced_beam_cases as FC
import forced_beam_ref as R
from capnet.beam import Constraints, PerImage
from forced_beam_cases import IMAGES, KS, MARGIN, MAX_LEN, PENALTIES, START   # noqa: F401

# the non-forced set of image 1 (assignment A), per family: "A" (no word twice) wherever every case is admitted at both
# penalties -- under "A", StackedDecoderRNNAtt-2 at k = 5, image 1 ranks its two best completed captions 5.6e-05 apart at
# length_penalty 1, below MARGIN; under "B" (no 2-gram twice) every case of that family is admitted
NON_FORCED = {"StackedDecoderRNNAtt-2": "B"}
DEFAULT_NON_FORCED = "A"


def units():
    """(forced_beam_cases' unit, constrained_beam_cases' unit) per family, in forced_beam_cases' order."""
    con = {u.name: u for u in CC.units()}
    return [(u, con[u.name]) for u in FC.units()]


def keys(name, which):
    """The entry keys of family `name` under assignment `which` ("A" or "B"), one per image."""
    a = [("forced", "one"), ("con", NON_FORCED.get(name, DEFAULT_NON_FORCED)), None]
    return a if which == "A" else [a[(i - 1) % IMAGES] for i in range(IMAGES)]


ASSIGNMENTS = ("A", "B")


def entry(fu, key):
    """The capnet.beam.Constraints (or None) of an entry key."""
    if key is None:
        return None
    return fu.sets[key[1]] if key[0] == "forced" else CC.SETS[key[1]]


def per_image(fu, which):
    return PerImage([entry(fu, key) for key in keys(fu.name, which)])


def search(fu, cu, k, image, key):
    """The fp64 search of image `image` alone under entry `key`: the existing tests' own, computed once there."""
    if key is None:
        return fu.search(k, image, None)
    return (fu if key[0] == "forced" else cu).search(k, image, key[1])


def admitted(fu, cu, k, image, key, penalty=0.0):
    q = search(fu, cu, k, image, key)
    return q.margin > MARGIN and q.gap(penalty) > MARGIN


def winner(fu, cu, k, image, key):
    if key is None:
        return fu.winner(k, image, None)
    return (fu if key[0] == "forced" else cu).winner(k, image, key[1])


def winners(fu, cu, k, image_keys):
    return [winner(fu, cu, k, i, key) for i, key in enumerate(image_keys)]


def score_bound(fu, cu, k, image, key, words):
    if key is None:
        return fu.score_bound(k, image, None, words)
    return (fu if key[0] == "forced" else cu).score_bound(k, image, key[1], words)


def telling_k(fu, cu):
    """The first k at which the winners under A, under B and under each single entry for all images are pairwise what the test
    needs: A != B, and neither equals a uniform set's. None for none."""
    a, b = keys(fu.name, "A"), keys(fu.name, "B")
    for k in KS:
        wa, wb = winners(fu, cu, k, a), winners(fu, cu, k, b)
        same = [winners(fu, cu, k, [key] * IMAGES) for key in a]
        if wa != wb and all(wa != w and wb != w for w in same):
            return k
    return None


# ---- stored logits ---------------------------------------------------------------------------------------------------
TABLE_N, TABLE_T, TABLE_END, TABLE_START, TABLE_GAP, TABLE_CASES = FC.TABLE_N, FC.TABLE_T, FC.TABLE_END, FC.TABLE_START, FC.TABLE_GAP, FC.TABLE_CASES
TABLE_ENTRIES = {"F1": FC.TABLE_SETS["F1"], "F2": FC.TABLE_SETS["F2"], "F4": FC.TABLE_SETS["F4"], "g1": CC.TABLE_SETS["g1"], None: None}
TABLE_ASSIGNMENTS = {"first": ("F1", "F2", "g1", "F4"), "second": ("F4", "F2", None, "F1")}


def table_per_image(which):
    return PerImage([TABLE_ENTRIES[key] for key in TABLE_ASSIGNMENTS[which]])


_models = {}


def table_model(k, V, key, image):
    """(the fixed-slot model of image `image` driven under TABLE_ENTRIES[key] over the table -- the other images dead --, the
    smallest gap its selections rest on), once per (k, V, key, image)."""
    if (k, V, key, image) not in _models:
        c = TABLE_ENTRIES[key]
        beam = R.ForcedBeam(TABLE_N, k, V, TABLE_START, TABLE_END, Constraints() if c is None else c)
        for other in range(TABLE_N):
            if other != image:
                beam.live[other] = 0
        _models[(k, V, key, image)] = (beam, R.drive(beam, FC.table(k, V)))
    return _models[(k, V, key, image)]


class Composed:
    """What a mixed batch must do on the stored logits: image i behaves as image i of the model driven under its own entry.
    The read-only view of n models the tests compare against."""

    def __init__(self, k, V, which):
        self.k, self.V, self.names = k, V, TABLE_ASSIGNMENTS[which]
        self.models = [table_model(k, V, key, i)[0] for i, key in enumerate(self.names)]
        self.gap = min(table_model(k, V, key, i)[1] for i, key in enumerate(self.names))

    def _rows(self, per_model, width):
        """Image i's slice [i width, (i + 1) width) of model i's flat per-row list."""
        out = []
        for i, m in enumerate(self.models):
            out += per_model(m)[i * width:(i + 1) * width]
        return out

    def outputs(self, step):
        """(next_words [n k], parent_rows [n k]) of `step`."""
        k = self.k
        return (self._rows(lambda m: m.outputs[step][0], k), self._rows(lambda m: m.outputs[step][1], k))

    def completed(self, i):
        return self.models[i].completed(i)

    def finish(self):
        return [m.finish()[i] for i, m in enumerate(self.models)]

    def nbest(self, penalty):
        return [m.nbest(penalty)[i] for i, m in enumerate(self.models)]

    def winner_rows(self, T):
        return [m.winner_rows(T)[i] for i, m in enumerate(self.models)]

    def nbest_rows(self, T, penalty):
        return [m.nbest_rows(T, penalty)[i] for i, m in enumerate(self.models)]


class HostBeam(R.ForcedBeam):
    """The host loops' bookkeeping under a rule per image: ForcedBeam whose ban lists and met masks are those of each
    image's own entry (None: nothing banned, mask 0)."""

    def __init__(self, k, V, which):
        super().__init__(TABLE_N, k, V, TABLE_START, TABLE_END, None)
        self.entries = [TABLE_ENTRIES[key] or Constraints() for key in TABLE_ASSIGNMENTS[which]]

    def bans(self, step, i, rows):
        return [R.excluded(self.seqs[i][r], step, self.end, self.entries[i]) for r in range(rows)]

    def met(self, i, rows):
        return [sum(1 << f for f, w in enumerate(self.entries[i].forced) if w in self.seqs[i][r][1:]) for r in range(rows)]
