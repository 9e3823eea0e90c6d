"""Time what the n-best lists cost -- print ONE JSON line and append it to profiles/time_nbest.jsonl.

Wall ms per sample_batch (host clock around the call, ended by a synchronise), the variants alternated in one process,
`--reps` (25) times each after 2 untimed calls of each; per variant the median and the spread (max - min) of the repeats.
k = 5, V = 8192, max_seq_length = 20, tools/time_att_alphas.py's cells and sizes (attention 512, embedding 300, hidden 512,
factored 1024, feature maps of 2048 channels), <end> biased far down: every beam runs all 21 steps in every variant. Per
cell:
  plain         sample_batch(one_call=True)                                       the search and its winner
  nbest         sample_batch(one_call=True, nbest=True)                           + capnet_beam_nbest and its one copy
  nbest_alphas  sample_batch(one_call=True, nbest=True, return_alphas=True)       the search records its maps, then
                                                                                  capnet_beam_nbest_traced + one gather over n k rows
Cells: fa = DecoderFactoredLSTMAtt, sfa2 = StackedFactoredLSTMAtt with 2 layers; each at 12 images on a 7 x 7 map and at
64 images on a 14 x 14 map (--shapes). nbest - plain is the cost of the keyword. With <end> biased away nothing completes:
the lists come back empty, but the ranking launch, the gather over all n k x 21 rows (zeros) and the copy are all paid,
which is what is timed. The call without the keyword must not have changed: --plain-only times `plain` alone and uses
nothing this keyword added, so the same file runs on the commit before it; compare its `plain` with this commit's.

usage: python tools/time_nbest.py [--cells fa,sfa2] [--shapes 12x7,64x14] [--reps R] [--plain-only] [--label TEXT]
On a shared GPU run one cell per process, each under its own time limit, chained so that a failure ends the chain:
  timeout -k 10 300 python tools/time_nbest.py --cells fa && timeout -k 10 300 python tools/time_nbest.py --cells sfa2
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
from capnet import ops  # noqa: E402
from capnet.model_att import DecoderFactoredLSTMAtt  # noqa: E402
from capnet.stacked_att import StackedFactoredLSTMAtt  # noqa: E402

A, E, H, F, V, CF, K, MAXLEN = 512, 300, 512, 1024, 8192, 2048, 5, 20
START, END = 1, 2
UNTIMED = 2


def _variants(dec, feats, plain_only):
    kw = dict(k=K, mode="factual", one_call=True)
    out = {"plain": lambda: dec.sample_batch(feats, START, END, **kw)}
    if not plain_only:
        out["nbest"] = lambda: dec.sample_batch(feats, START, END, nbest=True, **kw)
        out["nbest_alphas"] = lambda: dec.sample_batch(feats, START, END, nbest=True, return_alphas=True, **kw)[0]
    return out


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def cell_result(dec, feats, reps, plain_only):
    variants = _variants(dec, feats, plain_only)
    first = {}
    for name, fn in variants.items():                # untimed: allocator, weight folds, code objects, the workspaces
        for _ in range(UNTIMED):
            first[name] = _time(fn)[1]
    runs = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            runs[name].append(_time(fn)[0])
    out = {}
    for name, v in runs.items():
        out[name] = round(statistics.median(v), 3)
        out[name + "_spread"] = round(max(v) - min(v), 3)
    same = True
    if not plain_only:
        out["nbest_minus_plain"] = round(out["nbest"] - out["plain"], 3)
        out["nbest_alphas_minus_plain"] = round(out["nbest_alphas"] - out["plain"], 3)
        winners = [hyps[0][0] if hyps else [END] for hyps in first["nbest"]]
        same = winners == first["plain"] and first["nbest_alphas"] == first["nbest"]
    out["longest_sequence"], out["same_sequences"] = max(len(s) for s in first["plain"]), bool(same)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="fa,sfa2")
    ap.add_argument("--shapes", default="12x7,64x14")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_nbest.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nbest: needs the GPU")
    dev = torch.device("cuda:0")
    result = {}
    for cell in args.cells.split(","):
        torch.manual_seed(len(cell))
        if cell == "fa":
            dec = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=MAXLEN)
        elif cell == "sfa2":
            dec = StackedFactoredLSTMAtt(A, E, H, F, V, 2, feature_size=CF, dropout=0.0, max_seq_length=MAXLEN)
        else:
            raise SystemExit("time_nbest: unknown cell %r" % cell)
        dec = dec.to(dev).eval()
        with torch.no_grad():
            dec.C.bias[END] = -100.0
        for shape in args.shapes.split(","):
            n, side = (int(v) for v in shape.split("x"))
            feats = torch.rand(n, side * side, CF, device=dev)
            result["%s_n%d_p%d" % (cell, n, side * side)] = cell_result(dec, feats, args.reps, args.plain_only)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_nbest", "label": args.label, "plain_only": args.plain_only, "A": A, "E": E, "H": H, "F": F,
                       "V": V, "C": CF, "k": K, "max_seq_length": MAXLEN, "reps": args.reps, "untimed": UNTIMED,
                       "ms_per_call": result})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    bad = [name for name, r in result.items() if not r["same_sequences"]]
    if bad:
        raise SystemExit("time_nbest: the variants disagree in %s" % ", ".join(bad))


if __name__ == "__main__":
    main()
