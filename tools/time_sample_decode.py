"""Time sampled decoding (sample_random) three ways and append one JSON line per cell to profiles/time_sample_decode.jsonl:
the one-call route (capnet_sample_decode / capnet_att_sample_decode), the composed route (CAPNET_NO_FUSED_SAMPLE=1: the
decode step, ops.linear and ops.sample_rows -- or torch.topk and ops.sample_pick -- launch by launch from Python) and the
greedy / beam decode of the same shape on the same commit, the floor: sampling adds two logf and one hash per logit and the
log-sum-exp.

Wall ms per call (host clock around the call, ended by a synchronise), the variants alternated, `--reps` times each in one
process after `--warmup` untimed rounds; per variant the median and the (min, max) of the repeats. The one-call route is
timed at EVERY row count (capnet.decode.FUSED_SAMPLE_MAX_ROWS and FUSED_ATT_SAMPLE_MAX_ROWS are lifted for the
measurement): the constants are set from these
numbers -- the largest measured row count at which the one-call median beats the composed median by more than the spread
(the larger of the two ranges) at every layer count and top_k.
Cells:
  seq   capnet.seq2seq's EncoderRNN.sample_random at E 300, H 512, V 8192, 40 steps: rows 1 / 12 / 64 x layers 1 / 3 x top_k
        0 / 5; the floor is EncoderRNN.sample (greedy) at its own default route
  att   DecoderFactoredLSTMAtt at BASELINE configs[3]'s sizes (attention 512, embedding 300, hidden 512, factored 1024, maps
        of 2048 channels) on 7 x 7, 12 images x 5 samples, 20 steps, top_k 0 / 5; the yardstick is sample_batch(one_call=True)
        at k = 5 (a beam search: the same step on the same 60 rows, plus its bookkeeping)
  att_rows  the same decoder at 60 / 72 / 96 physical rows: 12 x 5, 12 x 5 with the greedy row of sample_random(greedy=True)
        and 12 x 7 with it, top_k 0 / 5 x top_p 1 / 0.9 -- what FUSED_ATT_SAMPLE_MAX_ROWS / FUSED_ATT_NUCLEUS_MAX_ROWS are set from
Every route of a cell must return the same tokens where the restatement's margins allow; random weights do not guarantee
that, so the tool reports "same_tokens" and does not fail on it.

usage: python tools/time_sample_decode.py [--cells seq,att,att_rows] [--rows 1,12,64] [--layers 1,3] [--reps R] [--warmup W]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import capnet  # noqa: E402,F401
from capnet import decode  # noqa: E402
from capnet.model_att import DecoderFactoredLSTMAtt  # noqa: E402
from capnet.seq2seq import Seq2Seq  # noqa: E402

E, H, V = 300, 512, 8192
OUT = os.path.join(ROOT, "profiles", "time_sample_decode.jsonl")


def _set_fused(fused):
    if fused:
        os.environ.pop(decode.FUSED_SAMPLE_OFF, None)
    else:
        os.environ[decode.FUSED_SAMPLE_OFF] = "1"


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def compare(variants, reps, warmup):
    """variants: name -> (fused or None, fn). -> ({name: {median, min, max}}, {name: the last result})."""
    ms, last = {k: [] for k in variants}, {}
    for it in range(warmup + reps):
        for name, (fused, fn) in variants.items():
            if fused is not None:
                _set_fused(fused)
            t, last[name] = _timed(fn)
            if it >= warmup:
                ms[name].append(t)
    _set_fused(True)
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            for k, v in ms.items()}, last


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def cell_seq(a, dev):
    for L in [int(x) for x in a.layers.split(",")]:
        torch.manual_seed(L)
        enc = Seq2Seq(E, H, V, L).to(dev).eval().encoder
        for rows in [int(x) for x in a.rows.split(",")]:
            feats = torch.randn(rows, E, device=dev) * 0.5
            for top_k in (0, 5):
                kw = dict(temperature=1.0, top_k=top_k, seed=7)
                res, last = compare({"one_call": (True, lambda: enc.sample_random(feats, **kw)),
                                     "composed": (False, lambda: enc.sample_random(feats, **kw)),
                                     "greedy": (None, lambda: enc.sample(feats))}, a.reps, a.warmup)
                emit({"tool": "time_sample_decode", "cell": "seq", "E": E, "H": H, "V": V, "steps": 40, "layers": L, "rows": rows,
                      "top_k": top_k, "reps": a.reps, "ms": res,
                      "same_tokens": bool(torch.equal(last["one_call"][0], last["composed"][0]))})


def cell_att(a, dev):
    A, F, CF, n, m, steps = 512, 1024, 2048, 12, 5, 20
    torch.manual_seed(3)
    dec = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=steps).to(dev).eval()
    feats = torch.rand(n, 7, 7, CF, device=dev)
    for top_k in (0, 5):
        kw = dict(samples=m, temperature=1.0, top_k=top_k, seed=7)
        res, last = compare({"one_call": (True, lambda: dec.sample_random(feats, 1, V, **kw)),
                             "composed": (False, lambda: dec.sample_random(feats, 1, V, **kw)),
                             "beam_one_call": (None, lambda: dec.sample_batch(feats, 1, V, k=m, one_call=True))}, a.reps, a.warmup)
        tokens = {k: [q for img in last[k] for q, _ in img] for k in ("one_call", "composed")}
        emit({"tool": "time_sample_decode", "cell": "att", "decoder": "DecoderFactoredLSTMAtt", "A": A, "E": E, "H": H, "F": F, "V": V,
              "C": CF, "P": 49, "images": n, "samples": m, "steps": steps, "top_k": top_k, "reps": a.reps, "ms": res,
              "same_tokens": tokens["one_call"] == tokens["composed"]})


def cell_att_rows(a, dev):
    """The attention decoder of cell `att` at 60, 72 and 96 physical rows: 12 images x 5 samples, the same with the greedy row
    (12 x 6: capnet.train.self_critical_step's greedy baseline) and 12 x 7 with it (12 x 8); top_k 0 / 5 x top_p 1 / 0.9."""
    A, F, CF, n, steps = 512, 1024, 2048, 12, 20
    torch.manual_seed(3)
    dec = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=steps).to(dev).eval()
    feats = torch.rand(n, 7, 7, CF, device=dev)
    for m, greedy in ((5, False), (5, True), (7, True)):
        for top_k in (0, 5):
            for top_p in (1.0, 0.9):
                kw = dict(samples=m, temperature=1.0, top_k=top_k, top_p=top_p, seed=7, greedy=greedy)
                res, last = compare({"one_call": (True, lambda: dec.sample_random(feats, 1, V, **kw)),
                                     "composed": (False, lambda: dec.sample_random(feats, 1, V, **kw))}, a.reps, a.warmup)
                tokens = {k: [q for img in last[k] for q, _ in img] for k in ("one_call", "composed")}
                emit({"tool": "time_sample_decode", "cell": "att_rows", "decoder": "DecoderFactoredLSTMAtt", "A": A, "E": E, "H": H,
                      "F": F, "V": V, "C": CF, "P": 49, "images": n, "samples": m, "greedy": greedy, "rows": n * (m + greedy),
                      "steps": steps, "top_k": top_k, "top_p": top_p, "reps": a.reps, "ms": res,
                      "same_tokens": tokens["one_call"] == tokens["composed"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="seq,att")
    ap.add_argument("--layers", default="1,3")
    ap.add_argument("--rows", default="1,12,64")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    # the one-call route at every row count: the constants come from this table
    decode.FUSED_SAMPLE_MAX_ROWS = decode.FUSED_ATT_SAMPLE_MAX_ROWS = decode.FUSED_ATT_NUCLEUS_MAX_ROWS = 1 << 30
    for cell in a.cells.split(","):
        {"seq": cell_seq, "att": cell_att, "att_rows": cell_att_rows}[cell](a, dev)


if __name__ == "__main__":
    main()
