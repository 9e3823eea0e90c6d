"""Inputs shared by tests/test_seq2seq_styles_cpu.py (margins) and tests/test_seq2seq_styles_gpu.py (the runs) of
Seq2Seq.sample_styles. TEST INFRASTRUCTURE.

Parameters and features are built exactly as seq2seq_cases.greedy_case builds them (make_params at seed 1000 + seed with
linear.weight x 32 and the LSTM matrices x 2, features from generator seed 2000 + seed times 0.5, start token 1). The
seeds are the first from 0 upwards at which ALL FOUR modes clear seq2seq_cases.need(scale) at every row and step of the
fp64 restatement (tests/seq2seq_ref.py); the CPU test asserts that, and that every row's ids differ between any two
emotions, so the GPU test compares ids exactly and a kernel that used one group's embedding or projection for every
group cannot pass. (At 12 rows with V = 8192 and two layers no seed below 40 clears all four modes: there is no such case
against the restatement; the GPU test runs that size against sample(mode=...) only, where no margin is needed.)

Seq2Seq does not forward max_seq_length: a case with fewer than 40 steps sets it on the encoder and the three decoders.
"""
import functools

import torch

import seq2seq_cases as SC
import seq2seq_ref as SR

MODES = ("factual", "happy", "sad", "angry")
START = 1

# name -> dict(E, H, V, layers, rows, steps, seed)
CASES = {}


def _add(E, H, V, layers, rows, steps, seed):
    CASES["e%d_h%d_v%d_l%d_r%d" % (E, H, V, layers, rows)] = dict(E=E, H=H, V=V, layers=layers, rows=rows, steps=steps, seed=seed)


_add(20, 64, 211, 3, 16, 12, 3)        # a full 16-row tile per group, V off 32, E below one k group
_add(30, 128, 211, 1, 7, 12, 1)        # E off 4 (scalar x loads), a ragged tile
_add(300, 512, 7411, 2, 1, 40, 0)      # odd V, one row
_add(300, 512, 8192, 3, 2, 40, 1)
_add(300, 512, 8192, 1, 3, 40, 0)
_add(300, 512, 1000, 2, 16, 20, 7)     # full size, a full tile


def make_case(c):
    """(fp64 params, fp64 features [rows, E]) of a case dict."""
    p = SR.make_params(SC.shapes(c["E"], c["H"], c["V"], c["layers"]), seed=1000 + c["seed"], out_scale=32.0, lstm_scale=2.0)
    g = torch.Generator().manual_seed(2000 + c["seed"])
    feats = torch.randn(c["rows"], c["E"], generator=g, dtype=torch.float64) * 0.5
    return p, feats


def case(name):
    """(case dict, fp64 params, fp64 features [rows, E])."""
    c = CASES[name]
    return (c,) + make_case(c)


@functools.lru_cache(maxsize=None)
def reference(name):
    """{mode: (ids [rows, steps], the smallest top-1 / top-2 gap on the mode's path -- the encoder's pass included --, the
    largest |logit| met)} of the restatement: SR.seq2seq_sample per mode, the encoder's loop computed once. Computed once
    per process; callers must not change what they get."""
    c, p, feats = case(name)
    L, steps = c["layers"], c["steps"]
    ids, states, margin, scale = SR.greedy(p, "encoder", L, steps, features=feats)
    out = {"factual": (ids, margin, scale)}
    for m in SR.EMOTIONS:
        ids_m, _, m2, s2 = SR.greedy(p, "decoder_" + m, L, steps, start_token=START, states=states)
        out[m] = (ids_m, min(margin, m2), max(scale, s2))
    return out


def set_steps(model, steps):
    for mod in (model.encoder, model.decoder_happy, model.decoder_sad, model.decoder_angry):
        mod.max_seq_length = steps
    return model
