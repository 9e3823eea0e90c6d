"""Inputs shared by tests/test_seq2seq_cpu.py (margins) and tests/test_seq2seq_gpu.py (the runs). TEST INFRASTRUCTURE.

A greedy decode feeds every argmax back, so a GPU run and the fp64 restatement decode the same tokens only while the two
best logits of every row and step are further apart than the fp32 error of a logit. The CPU test asserts that for every
case below (all rows, all steps; none is skipped), with the bound `need(scale)`; the GPU test then compares ids exactly.

At torch's default initial values the greedy path of a full-size model settles where the logits are nearly flat (gaps of
1e-6 .. 1e-4), so the full-size cases scale linear.weight by 32 and the LSTM weight matrices by 2, and take the seeds
that a search on the CPU found (the first seed from 0 upwards whose smallest gap clears the bound at all 40 steps).
"""
import torch

import seq2seq_ref as SR

TOL_STEP = 3e-5          # a decode step's relative error bound (tests/test_stacked_decode_gpu.py)
E_FULL, H_FULL = 300, 512


def need(scale):
    """Twice the error a logit may carry: 2 x TOL_STEP x the largest |logit| on the path."""
    return 2 * TOL_STEP * scale


def shapes(E, H, V, L):
    out = {}
    for m in ("encoder", "decoder_happy", "decoder_sad", "decoder_angry"):
        out[m + ".embed.weight"] = (V, E)
        for l in range(L):
            out["%s.lstm.weight_ih_l%d" % (m, l)] = (4 * H, E if l == 0 else H)
            out["%s.lstm.weight_hh_l%d" % (m, l)] = (4 * H, H)
            out["%s.lstm.bias_ih_l%d" % (m, l)] = (4 * H,)
            out["%s.lstm.bias_hh_l%d" % (m, l)] = (4 * H,)
        out[m + ".linear.weight"] = (V, H)
        out[m + ".linear.bias"] = (V,)
    return out


# name -> dict(E, H, V, layers, rows, seed, steps, mode)
GREEDY = {}


def _add(name, V, layers, rows, seed, steps=40, mode="factual", E=E_FULL, H=H_FULL):
    GREEDY[name] = dict(E=E, H=H, V=V, layers=layers, rows=rows, seed=seed, steps=steps, mode=mode)


_add("r1_l3_v8192", 8192, 3, 1, 0)
_add("r12_l1_v8192", 8192, 1, 12, 0)
_add("r12_l2_v7411", 7411, 2, 12, 0)
_add("r64_l3_v8192", 8192, 3, 64, 11)              # seeds 0..10: gaps of 1e-5 .. 2e-4, below the bound
_add("happy_r12_l3_v8192", 8192, 3, 12, 6, mode="happy")   # seeds 0..5: 5e-5 .. 4.5e-4
_add("sad_r1_l2_v7411", 7411, 2, 1, 0, mode="sad")


def greedy_case(name):
    """(case dict, fp64 params, fp64 features [rows, E])."""
    c = GREEDY[name]
    p = SR.make_params(shapes(c["E"], c["H"], c["V"], c["layers"]), seed=1000 + c["seed"], out_scale=32.0, lstm_scale=2.0)
    g = torch.Generator().manual_seed(2000 + c["seed"])
    feats = torch.randn(c["rows"], c["E"], generator=g, dtype=torch.float64) * 0.5
    return c, p, feats


def greedy_reference(name):
    """(ids, smallest gap, largest |logit|, encoder final states) of the restatement. The decoders' start token is 1."""
    c, p, feats = greedy_case(name)
    return SR.seq2seq_sample(p, c["layers"], c["steps"], feats, 1, c["mode"])


# ---- full-size training cases: name -> dict(V, layers, B, T, seed, mode, p) ---------------------------------------------
TRAIN = {}
TOL_LOGITS = 2e-5


def _train(name, V, layers, B, T, seed, mode="factual", p=0.0):
    TRAIN[name] = dict(E=E_FULL, H=H_FULL, V=V, layers=layers, B=B, T=T, seed=seed, mode=mode, p=p)


_train("b12_l3_v8192", 8192, 3, 12, 9, 0)
_train("b64_l2_v7411", 7411, 2, 64, 9, 0)
_train("b64_l1_v8192", 8192, 1, 64, 9, 0)
_train("happy_b12_l3_v7411", 7411, 3, 12, 9, 0, mode="happy")
_train("drop22_b12_l3", 8192, 3, 12, 9, 0, p=0.22)
_train("drop50_happy_b12_l3", 7411, 3, 12, 9, 0, mode="happy", p=0.5)


def train_case(name):
    """(case, fp64 params, features [B, E], (tokens [B, T], lengths), targets [B, T], tf_mask of the module's steps):
    mixed teacher forcing, the first step forced, steps 2 and T - 2 free running. In `factual` the lengths count the
    feature column's step too (lengths <= T, targets = the tokens); in an emotion mode targets = the next tokens."""
    c = TRAIN[name]
    p = SR.make_params(shapes(c["E"], c["H"], c["V"], c["layers"]), seed=3000 + c["seed"], out_scale=8.0)
    g = torch.Generator().manual_seed(4000 + c["seed"])
    B, T, V = c["B"], c["T"], c["V"]
    feats = torch.randn(B, c["E"], generator=g, dtype=torch.float64) * 0.5
    lengths = sorted([int(v) for v in torch.randint(2, T + 1, (B,), generator=g)], reverse=True)
    lengths[0] = T
    seq = torch.randint(3, V, (B, T + 1), generator=g)
    tokens, targets = seq[:, :T].contiguous(), (seq[:, :T] if c["mode"] == "factual" else seq[:, 1:]).contiguous()
    tf = [bool(v) for v in (torch.rand(T, generator=g) < 0.6)]
    tf[0], tf[2], tf[T - 2] = True, False, False
    return c, p, feats, (tokens, lengths), targets, tf
