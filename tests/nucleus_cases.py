"""Inputs shared by tests/test_nucleus_cpu.py (the margin rule) and tests/test_nucleus_gpu.py (the runs). TEST
INFRASTRUCTURE.

A nucleus decode feeds every draw back, so a GPU run and the fp64 restatement agree token for token only while, at every row
and step, tests/nucleus_ref.py's margin rule holds: the key gap among the kept entries, the logit gap across the nucleus'
edge, the distance of every cumulative mass from top_p, and with top_k > 0 the k-th / (k + 1)-th logit gap. The CPU test
asserts it for every case below; the GPU test then compares ids exactly and skips nothing. The stream seeds are the first
from 0 upwards for which the restatement clears the rule (the rejected ones are noted beside each case).

The models, features and shapes are those of tests/sample_random_cases.py: the image families (V = 37 / 97, 2 images x 3
samples, MAX_LEN steps, attention maps of 4 and 49 pixels), each at top_k 0 and 5 with top_p 0.5 / 0.9 and the temperatures
in turn, and capnet.seq2seq at V 8192 with 1 row, top_k 5.

NOT admitted, because no stream seed clears the rule (80 tried for each; the search is the restatement alone, on the CPU):
  * capnet.seq2seq without top_k, r1_l3_v8192 (V 8192, 1 row) and r12_l2_v7411 (V 7411, 12 rows), at top_p 0.5 and 0.9 and
    T 1.0 / 0.5 (and 0.25 / 0.125, tried beyond the listed temperatures): the models' distributions are wide, the nucleus is
    up to 7010 words, and the logits on the two sides of its edge lie 1e-7 .. 2e-4 apart against a need of 2.5e-4 .. 3e-3 --
    rule (b) fails at every step of every seed, and rule (c) with it (mass ratio 3e-7 .. 2e-5 against 5e-4 .. 6e-3).
  * r12_l2_v7411 with top_k 5 (top_p 0.5 / 0.9, T 0.5 / 1.0): 480 draws must clear the k-th / (k + 1)-th rule AND rule (c);
    seeds 0 .. 79 each fail one of them at some row and step (sample_random_cases found its one 12-row top_k case at seed 40
    without rule (c)).
tests/test_nucleus_gpu.py covers those shapes otherwise: nucleus_rows alone against the restatement on exact logits up to V
12289, and the 12-row V 7411 decode as bit-equality of the one-call and composed routes.
"""
import nucleus_ref as N
import sample_random_cases as SC
from device_beam_cases import MAX_LEN, START

IMAGES, SAMPLES = SC.IMAGES, SC.SAMPLES

# ---- capnet.seq2seq: name -> dict(greedy: the seq2seq_cases case whose model it is, T, top_k, top_p, seed) ------------------
SEQ2SEQ = {
    "r1_l3_v8192_k5_p5": dict(greedy="r1_l3_v8192", T=0.5, top_k=5, top_p=0.5, seed=0),
    "r1_l3_v8192_k5_p9": dict(greedy="r1_l3_v8192", T=1.0, top_k=5, top_p=0.9, seed=0),
}

_seq_refs = {}


def seq2seq_reference(name, seed=None, on_logits=None):
    """(greedy case dict, fp64 params, fp64 features, sampling case dict, (ids, logp, final (h, c), Trace, the encoder's
    greedy (margin, scale) or None)) -- computed once (seed / on_logits given: computed afresh, not kept)."""
    if name in _seq_refs and seed is None and on_logits is None:
        return _seq_refs[name]
    s = SEQ2SEQ[name]
    c, p, feats = SC.SC.greedy_case(s["greedy"])
    ref = N.seq2seq_sample_random(p, c["layers"], c["steps"], feats, 1, c["mode"], s["T"], s["seed"] if seed is None else seed,
                                  s["top_k"], s["top_p"], on_logits)
    if seed is None and on_logits is None:
        _seq_refs[name] = (c, p, feats, s, ref)
    return c, p, feats, s, ref


# ---- the image decoders -------------------------------------------------------------------------------------------------
# (family, top_k) -> the stream seed where it is not 0. Every seed below it was rejected by rule (c), a cumulative mass too
# close to top_p at some row and step (at a few seeds the logit gap across the edge failed too); no other rule rejected one
SEEDS = {("DecoderFactoredLSTM", 5): 16, ("StackedFactoredLSTM-3", 0): 10, ("DecoderFactoredLSTMAtt-p4-factual", 0): 1,
         ("StackedFactoredLSTMAtt-2-p4-factual", 0): 2, ("DecoderFactoredLSTMAtt-p4-happy", 0): 2,
         ("StackedFactoredLSTMAtt-2-p4-happy", 0): 7, ("StackedFactoredLSTMAtt-2-p4-happy", 5): 15,
         ("DecoderFactoredLSTMAtt-p49-factual", 0): 1, ("StackedFactoredLSTMAtt-2-p49-factual", 5): 5,
         ("StackedFactoredLSTMAtt-2-p49-happy", 0): 10}
IMAGE_CASES = []


def _image_cases():
    names = sorted({c["family"] for c in SC.IMAGE_CASES}, key=[c["family"] for c in SC.IMAGE_CASES].index)
    i = 0
    for name in names:
        for top_k in (0, 5):
            # every family sees both top_p values: DecoderRNN and DecoderRNNAtt on 4 pixels (V = 37) take 0.9 without top_k, the
            # others 0.5 -- at 0.9 the factored ones' nucleus is 60 to 80 near-equal words of 97, some cumulative mass lands
            # inside rule (c)'s band at about every eighth draw, and no seed from 0 to 59 clears 72 draws (DecoderRNNAtt on
            # 49 pixels: none from 0 to 79)
            T, top_p = (1.0, 0.5, 2.0)[i % 3], (0.5, 0.9)[(top_k == 0) == (name in ("DecoderRNN", "DecoderRNNAtt-p4"))]
            IMAGE_CASES.append(dict(id="%s-k%d-p%g" % (name, top_k, top_p), family=name, T=T, top_k=top_k, top_p=top_p,
                                    seed=SEEDS.get((name, top_k), 0)))
            i += 1


_image_cases()
_img_refs = {}


def image_reference(case, seed=None, on_logits=None):
    """(ids [6, MAX_LEN], logp, Trace) of the restatement for one of IMAGE_CASES -- computed once (seed / on_logits given:
    computed afresh, not kept)."""
    if case["id"] in _img_refs and seed is None and on_logits is None:
        return _img_refs[case["id"]]
    fam = SC.families()[case["family"]]
    ref = N.family_sampled(fam.initial, IMAGES, SAMPLES, MAX_LEN, START, case["T"], case["seed"] if seed is None else seed,
                           case["top_k"], case["top_p"], on_logits)
    if seed is None and on_logits is None:
        _img_refs[case["id"]] = ref
    return ref
