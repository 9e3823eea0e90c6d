"""Inputs shared by tests/test_excluded_sample_cpu.py (the margin rule, the binding condition) and
tests/test_excluded_sample_gpu.py (the runs). TEST INFRASTRUCTURE.

The families are sample_random_cases.families(), 2 images x 3 samples, MAX_LEN = 12 steps, every family at top_k 0 and 5 with
the temperatures in turn; the two exclusion sets alternate over them (both sets meet both top_k):
  A = Constraints(no_repeat_ngram=1)                                   no word twice (<start> counts)
  D = Constraints(no_repeat_ngram=2, min_words=6, banned=(two ids))    no bigram twice, six words at least, two banned words
and one case draws from the nucleus (top_p = 0.9, an attention decoder: the one call's logits block), one carries the greedy
row (greedy=True; the restatement is that of the drawn rows).

Per case and stream seed: the UNEXCLUDED restatement on that seed gives the end token -- sample_random_cases.early_end's, the
fourth word of its row 0, so min_words = 6 has something to forbid -- and D's banned ids: the first two distinct words other
than that end token that it draws inside a cut caption (scanning step by step, row by row). The case's seed is the first from
0 upwards for which the EXCLUDED restatement clears the margin rule at every row and step (excluded_sample_ref.clears:
sample_random_ref's key gap and k-th / (k + 1)-th gap among the allowed words, nucleus_ref's rule where top_p < 1) and the
unexcluded one violates the set in a cut caption; the rejected seeds are noted beside each case.
"""
import excluded_sample_ref as XR
import sample_random_cases as SC
from capnet.beam import Constraints
from device_beam_cases import MAX_LEN, START

IMAGES, SAMPLES = SC.IMAGES, SC.SAMPLES

# case id -> the stream seed where it is not 0, with what the earlier seeds missed
SEEDS = {
    "DecoderFactoredLSTMAtt-p4-factual-k5-A": 1,             # seed 0: the 5th / 6th allowed logits 1.46e-4 apart < 1.69e-4
    "StackedFactoredLSTMAtt-2-p49-factual-k5-A": 1,          # seed 0: 1.35e-4 < 1.64e-4
    "StackedFactoredLSTMAtt-2-p49-happy-k5-A": 1,            # seed 0: 9.65e-5 < 1.78e-4
    # seeds 0..67: nucleus_ref's rule (c) at some row and step -- a cumulative mass within 4 TOL_STEP scale / T (about 4.3e-4,
    # relative) of top_p: mass ratios -4e-7 .. 3.8e-4 -- at 17 of them also the edge gap (4e-6 .. 2.0e-4 < 2.1e-4), at two the key gap
    "DecoderRNNAtt-p4-k0-D-p0.9": 68,
}


def _cases():
    out = []
    names = [c["family"] for c in SC.IMAGE_CASES if c["top_k"] == 0]
    for f, name in enumerate(names):
        for j, top_k in enumerate((0, 5)):
            which = "A" if (f + j) % 2 == 0 else "D"
            cid = "%s-k%d-%s" % (name, top_k, which)
            out.append(dict(id=cid, family=name, T=(1.0, 0.5, 2.0)[(2 * f + j) % 3], top_k=top_k, top_p=1.0, set=which, greedy=False))
    out.append(dict(id="DecoderRNNAtt-p4-k0-D-p0.9", family="DecoderRNNAtt-p4", T=1.0, top_k=0, top_p=0.9, set="D", greedy=False))
    # (the family and set for which, on the CPU, the greedy caption of both images under D reaches <end> within MAX_LEN words --
    # where the width-1 beam then completes -- and differs from the unexcluded one: test_excluded_sample_cpu.py asserts it)
    out.append(dict(id="DecoderRNNAtt-p4-k0-D-greedy", family="DecoderRNNAtt-p4", T=1.0, top_k=0, top_p=1.0, set="D", greedy=True))
    for c in out:
        c["seed"] = SEEDS.get(c["id"], 0)
    return out


CASES = _cases()


def banned_pair(ids, end):
    """The first two distinct words other than `end` inside a cut caption of the unexcluded restatement `ids`."""
    found = []
    for t in range(ids.shape[1]):
        for r in range(ids.shape[0]):
            w = int(ids[r][t])
            if end not in [int(v) for v in ids[r][:t]] and w != end and w not in found:
                found.append(w)
                if len(found) == 2:
                    return tuple(found)
    raise AssertionError("fewer than two distinct words drawn")


def build(case, seed):
    """The references of one case on stream seed `seed`: dict(end, c, plain=(ids, logp, Trace) of the unexcluded restatement,
    excl=(ids, logp, Trace) of the excluded one)."""
    fam = SC.families()[case["family"]]
    args = (fam.initial, IMAGES, SAMPLES, MAX_LEN, START)
    plain = XR.family_sampled(*args, fam.V, case["T"], seed, case["top_k"], None, case["top_p"])
    end = SC.early_end(plain[0])
    c = Constraints(no_repeat_ngram=1) if case["set"] == "A" else \
        Constraints(no_repeat_ngram=2, min_words=6, banned=banned_pair(plain[0], end))
    excl = XR.family_sampled(*args, end, case["T"], seed, case["top_k"], c, case["top_p"])
    return dict(end=end, c=c, plain=plain, excl=excl)


def binding(ref):
    """(violations of the set in the unexcluded restatement's cut captions, in the excluded one's): the first must not be
    empty, the second must be."""
    def of(ids, logp):
        cut = XR.R.cut(ids, logp, IMAGES, SAMPLES, START, ref["end"])
        return [v for img in cut for q, _ in img for v in XR.violations(q, ref["end"], ref["c"])]
    return of(*ref["plain"][:2]), of(*ref["excl"][:2])


def admitted(case, ref):
    """What keeps `ref` from serving as the case's reference (empty: admitted)."""
    fails = XR.clears(ref["excl"][2], case["T"], case["top_k"], case["top_p"])
    before, after = binding(ref)
    if not before:
        fails.append("the unexcluded restatement does not violate the set")
    if after:
        fails.append("the excluded restatement violates the set: %s" % after[:3])
    return fails


def greedy_captions(case, ref):
    """Per image (the greedy caption under the case's set, the unexcluded one): excluded_sample_ref.greedy_caption's triples."""
    fam = SC.families()[case["family"]]
    return [(XR.greedy_caption(fam.initial, i, MAX_LEN, START, ref["end"], ref["c"]),
             XR.greedy_caption(fam.initial, i, MAX_LEN, START, ref["end"], None)) for i in range(IMAGES)]


_refs = {}


def reference(case):
    """build(case, its seed) -- computed once and left unchanged."""
    if case["id"] not in _refs:
        _refs[case["id"]] = build(case, case["seed"])
    return _refs[case["id"]]
