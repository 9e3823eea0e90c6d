"""Inputs shared by tests/test_sample_random_cpu.py (the margin rule) and tests/test_sample_random_gpu.py (the runs).
TEST INFRASTRUCTURE.

A sampled decode feeds every draw back, so a GPU run and the fp64 restatement agree token for token only while, at every
row and step, the best and second-best keys (scaled logit + Gumbel noise) are further apart than the error a key may carry:
sample_random_ref.need(max |logit|, 1 / T) = 2 (TOL_STEP max|logit| / T + TOL_G). With top_k > 0 the k-th and (k + 1)-th
logits must also be 2 TOL_STEP max|logit| apart, or the two sides may draw among different candidates. The CPU test asserts
both for every case below, every row and every step; the GPU test then compares ids exactly. The stream seeds are the first
from 0 upwards for which the restatement clears the rule (the rejected ones are noted beside each case).

capnet.seq2seq cases take the parameters and features of seq2seq_cases' greedy cases of the same shape (linear.weight x 32,
LSTM matrices x 2), whose encoder pass is known to clear the greedy margin -- an emotion mode runs it first. top_k = 5 at 12
rows needs a long search: the 5th / 6th-logit condition is one on the model's logits along the path, 480 draws have to clear
a bound of ~1.1e-3 and each misses it with probability ~1e-2 whatever the stream seed; one such case is kept (seed 40), the
other top_k cases have 1 row (40 draws). The image decoders (V = 37 / 97, 72 draws) carry top_k = 5 at every shape.
"""
import torch

import att_beam_cases
import beam_decode_cases
import sample_random_ref as R
import seq2seq_cases as SC
import stacked_decode_ref
from device_beam_cases import MAX_LEN, START, Family, _load

# ---- capnet.seq2seq: name -> dict(greedy: the seq2seq_cases case whose model it is, T, top_k, seed) ---------------------------
SEQ2SEQ = {
    "r1_l3_v8192": dict(greedy="r1_l3_v8192", T=1.0, top_k=5, seed=0),
    "r12_l1_v8192": dict(greedy="r12_l1_v8192", T=1.0, top_k=0, seed=1),            # seed 0: key gap 9.3e-4 < 1.14e-3
    # seeds 0..39: the 5th / 6th logits 1e-5 .. 8e-4 apart (bound 1.1e-3) at some row and step, or (35) the key gap 8.1e-4
    "r12_l1_v8192_k5": dict(greedy="r12_l1_v8192", T=1.0, top_k=5, seed=40),
    "r12_l2_v7411": dict(greedy="r12_l2_v7411", T=0.5, top_k=0, seed=0),
    "happy_r12_l3_v8192": dict(greedy="happy_r12_l3_v8192", T=2.0, top_k=0, seed=0),
    "sad_r1_l2_v7411": dict(greedy="sad_r1_l2_v7411", T=1.0, top_k=5, seed=0),
}

_seq_refs = {}


def seq2seq_reference(name):
    """(greedy case dict, fp64 params, fp64 features, sampling case dict, (ids, logp, final (h, c), Trace, the encoder's
    greedy (margin, scale) or None)) -- computed once. The decoders' start token is 1."""
    if name not in _seq_refs:
        s = SEQ2SEQ[name]
        c, p, feats = SC.greedy_case(s["greedy"])
        ref = R.seq2seq_sample_random(p, c["layers"], c["steps"], feats, 1, c["mode"], s["T"], s["seed"], s["top_k"])
        _seq_refs[name] = (c, p, feats, s, ref)
    return _seq_refs[name]


# ---- the image decoders: 2 images x 3 samples, MAX_LEN steps -------------------------------------------------------------
IMAGES, SAMPLES = 2, 3


def _stacked_factored3():
    from capnet.stacked import StackedFactoredLSTM
    E, H, F, V, L = 12, 64, 32, 37, 3
    p = stacked_decode_ref.decode_params(StackedFactoredLSTM(E, H, F, V, L), seed=19)
    return Family("StackedFactoredLSTM-3", lambda: _load(StackedFactoredLSTM(E, H, F, V, L), p), p, V, {"mode": "sad"},
                  lambda: torch.zeros(3, E),
                  lambda k, i: (stacked_decode_ref._step_fn(p, "sad", L), stacked_decode_ref._zeros(p, k, L)))


def _att_families():
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model_att import DecoderRNNAtt
    from capnet.stacked_att import StackedFactoredLSTMAtt
    out = []
    for P in (4, 49):
        for mode in ("factual", "happy"):
            out.append(att_beam_cases._factored_att("DecoderFactoredLSTMAtt-p%d-%s" % (P, mode), DecoderFactoredLSTMAtt, 1, mode, 1,
                                                    A=32, E=24, H=64, F=32, V=97, Cf=512, P=P))
            out.append(att_beam_cases._factored_att("StackedFactoredLSTMAtt-2-p%d-%s" % (P, mode), StackedFactoredLSTMAtt, 2, mode,
                                                    28, A=32, E=24, H=64, F=32, V=97, Cf=512, P=P))
        out.append(att_beam_cases._rnn_att("DecoderRNNAtt-p%d" % P, DecoderRNNAtt, 1, 121, A=16, E=12, H=64, V=37, Cf=512, P=P))
    return out


_families = None


def families():
    """{name: Family}: DecoderFactoredLSTM and DecoderRNN (beam_decode_cases'), StackedFactoredLSTM at 3 layers, and the
    three attention decoders on maps of 4 and 49 pixels, the factored ones in `factual` and in one emotion."""
    global _families
    if _families is None:
        fams = beam_decode_cases.families() + [_stacked_factored3()] + _att_families()
        _families = {f.name: f for f in fams}
    return _families


# (family, T, top_k) -> the stream seed; every family at top_k 0 and 5, the temperatures in turn
SEEDS = {("StackedFactoredLSTMAtt-2-p49-factual", 5): 1}      # seed 0: the 5th / 6th logits 1.07e-4 apart < 1.64e-4
IMAGE_CASES = []


def _image_cases():
    names = ["DecoderFactoredLSTM", "DecoderRNN", "StackedFactoredLSTM-3"]
    for P in (4, 49):
        for mode in ("factual", "happy"):
            names += ["DecoderFactoredLSTMAtt-p%d-%s" % (P, mode), "StackedFactoredLSTMAtt-2-p%d-%s" % (P, mode)]
        names.append("DecoderRNNAtt-p%d" % P)
    i = 0
    for name in names:
        for top_k in (0, 5):
            T = (1.0, 0.5, 2.0)[i % 3]
            IMAGE_CASES.append(dict(id="%s-k%d" % (name, top_k), family=name, T=T, top_k=top_k, seed=SEEDS.get((name, top_k), 0)))
            i += 1


_image_cases()
_img_refs = {}


def image_reference(case):
    """(ids [6, MAX_LEN], logp, Trace) of the restatement for one of IMAGE_CASES -- computed once."""
    if case["id"] not in _img_refs:
        fam = families()[case["family"]]
        _img_refs[case["id"]] = R.family_sampled(fam.initial, IMAGES, SAMPLES, MAX_LEN, START, case["T"], case["seed"], case["top_k"])
    return _img_refs[case["id"]]


def early_end(ids):
    """An end token that cuts the restatement's row 0 after its fourth word."""
    return int(ids[0][3])
