"""Inputs shared by tests/test_greedy_row_cpu.py (the margin rule) and tests/test_greedy_row_gpu.py (the runs): sampled
decodes that carry a greedy row per image (sample_random(greedy=True)). TEST INFRASTRUCTURE.

Four tiny decoders (V 37, H 64, the smallest hidden size the fused step takes; 8 steps): a plain factored stack, a stack of
LSTM cells, a one-layer and a two-layer attention decoder. Three shapes, the smallest that can still go wrong: 1 image x 1
sample (two rows, one of each kind), 3 x 5 (18 rows: past the 16-row tile) and 2 x 15 (16 rows per image, the attention
step's limit). The options -- top_k 0 / 5, top_p 1 / 0.9, T 1 / 0.7 -- are spread over the twelve (family, shape) pairs so
that every family and every shape meets both values of each (OPTIONS).

As in sample_random_cases, a GPU run agrees with the fp64 restatement token for token only where every row and step
clears the margin rule (greedy_row_ref.clears: sample_random_ref's and nucleus_ref's rules for the drawn rows and the
truncations, and for a greedy row the best two scaled logits more than 2 TOL_STEP max|logit| / T apart). SEEDS holds, per
case, the first stream seed from 0 upwards whose restatement clears it; first_seed() is the search and the CPU test runs
it again. A case for which no seed below SEARCH clears the rule is dropped (DROPPED, with the reason); coverage() is what
the CPU test asserts of the rest.
"""
import att_beam_cases
import greedy_row_ref as G
import sample_random_ref as R
from device_beam_cases import START, families as device_families

STEPS = 8
SEARCH = 64
SHAPES = ((1, 1), (3, 5), (2, 15))
# (top_k, top_p, T) per family (rows, in FAMILIES' order) and shape (columns). A nucleus without top_k (top_k 0, top_p 0.9) sits
# at the small shapes: over V 37 words some cumulative mass of some row and step lies too near top_p for nucleus_ref's mass
# rule once a decode has hundreds of draws (no seed below SEARCH cleared it at 3 x 5 or 2 x 15 on the plain stacks, nor at
# 3 x 5 on the one-layer attention decoder, which were first laid out that way); the
# top_p = 1e-6 self-check of the GPU test covers that draw at every shape without a restatement.
OPTIONS = (((0, 0.9, 0.7), (5, 1.0, 1.0), (0, 1.0, 1.0)),
           ((0, 0.9, 1.0), (5, 0.9, 0.7), (0, 1.0, 0.7)),
           ((5, 1.0, 0.7), (0, 1.0, 1.0), (5, 0.9, 1.0)),
           ((0, 0.9, 0.7), (5, 0.9, 1.0), (0, 1.0, 1.0)))
FAMILIES = ("StackedFactoredLSTM-2", "StackedDecoderRNN-2", "DecoderFactoredLSTMAtt-1-v37", "StackedFactoredLSTMAtt-2-v37")

_families = None


def families():
    """{name: Family}: device_beam_cases' two plain stacks and two attention decoders built here at V 37 on maps of 4 pixels."""
    global _families
    if _families is None:
        from capnet.model_att import DecoderFactoredLSTMAtt
        from capnet.stacked_att import StackedFactoredLSTMAtt
        fams = [f for f in device_families() if f.name in FAMILIES]
        fams.append(att_beam_cases._factored_att("DecoderFactoredLSTMAtt-1-v37", DecoderFactoredLSTMAtt, 1, "factual", 41, A=32, E=24,
                                                 H=64, F=32, V=37, Cf=512, P=4))
        fams.append(att_beam_cases._factored_att("StackedFactoredLSTMAtt-2-v37", StackedFactoredLSTMAtt, 2, "happy", 43, A=32, E=24,
                                                 H=64, F=32, V=37, Cf=512, P=4))
        _families = {f.name: f for f in fams}
        assert sorted(_families) == sorted(FAMILIES)
    return _families


def make(fam, dev):
    """The family's decoder on `dev` in eval mode, decoding STEPS words."""
    dec = fam.make()
    dec.max_seq_length = STEPS
    return dec.to(dev).eval()


CASES = []
for _fi, _name in enumerate(FAMILIES):
    for _si, (_n, _m) in enumerate(SHAPES):
        _k, _p, _T = OPTIONS[_fi][_si]
        CASES.append(dict(id="%s-n%d-m%d-k%d-p%g-T%g" % (_name, _n, _m, _k, _p, _T), family=_name, n=_n, m=_m, top_k=_k, top_p=_p,
                          T=_T))

# case id -> the first seed that clears the rule (first_seed; tests/test_greedy_row_cpu.py repeats the search). The rejected ones:
#   StackedFactoredLSTM-2 1 x 1, top_p 0.9: seeds 0 .. 2, a cumulative mass within 4.2e-5 .. 3.5e-4 (relative) of top_p (bound 3.5e-4)
#   StackedDecoderRNN-2 3 x 5, top_k 5, top_p 0.9: seed 0, mass ratio 8.4e-5 (bound 4.3e-4)
#   DecoderFactoredLSTMAtt-1-v37 2 x 15, top_k 5, top_p 0.9: seeds 0 .. 8, mass ratio about 2.8e-4 (bound 4.4e-4), at seeds 1 and
#   4 also the 5th / 6th logits 1.0e-4 and 2.4e-5 apart (bound 2.2e-4)
SEEDS = {c["id"]: 0 for c in CASES}
SEEDS.update({"StackedFactoredLSTM-2-n1-m1-k0-p0.9-T0.7": 3, "StackedDecoderRNN-2-n3-m5-k5-p0.9-T0.7": 1,
              "DecoderFactoredLSTMAtt-1-v37-n2-m15-k5-p0.9-T1": 9})
# case id -> why no seed below SEARCH serves
DROPPED = {}

_refs = {}


def restate(case, seed):
    fam = families()[case["family"]]
    return G.family_sampled(fam.initial, case["n"], case["m"], STEPS, START, case["T"], seed, case["top_k"], case["top_p"])


def first_seed(case, limit=SEARCH):
    """(the first seed in [0, limit) whose restatement clears the margin rule or None, {rejected seed: what failed})."""
    rejected = {}
    inv_T = R.inv_temperature(case["T"])
    for seed in range(limit):
        fails = G.clears(restate(case, seed)[2], inv_T, case["top_k"], case["top_p"])
        if not fails:
            return seed, rejected
        rejected[seed] = fails
    return None, rejected


def live_cases():
    return [c for c in CASES if c["id"] not in DROPPED]


def reference(case):
    """(ids [n (m + 1), STEPS], logp, Trace) of the restatement at the case's seed -- computed once."""
    if case["id"] not in _refs:
        _refs[case["id"]] = restate(case, SEEDS[case["id"]])
    return _refs[case["id"]]


def greedy_rows(case):
    """The physical rows of the greedy captions."""
    return [i * (case["m"] + 1) + case["m"] for i in range(case["n"])]


def end_token(case):
    """An end token that the greedy caption of image 0 reaches at its fourth word, so that it completes."""
    return int(reference(case)[0][greedy_rows(case)[0]][3])


def coverage(cases):
    """What must remain after dropping: every family, every shape and both values of every option."""
    return dict(family={c["family"] for c in cases}, shape={(c["n"], c["m"]) for c in cases}, top_k={c["top_k"] for c in cases},
                top_p={c["top_p"] for c in cases}, T={c["T"] for c in cases},
                family_options={(c["family"], o, c[o]) for c in cases for o in ("top_k", "top_p", "T")})
