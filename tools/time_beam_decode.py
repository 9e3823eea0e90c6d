"""Time sample_batch three ways -- the beam bookkeeping on the host (the default), on_device=True (capnet.beam.
beam_search_device: a Python loop of launches) and one_call=True (capnet_beam_decode: the same launches from one C call,
the parent rows read by the decode step itself) -- print ONE JSON line and append it to profiles/time_beam_decode.jsonl.

Wall ms per sample_batch (host clock around the call, ended by a synchronise), the variants alternated, `--reps` times
each in one process after one untimed call of each; per variant the median and the (min, max) of the repeats. k = 5,
V = 8192, max_seq_length = 20, the cell of BASELINE configs[4] (embedding 300, hidden 512, factored 1024). Cells:
  sf1, sf3   StackedFactoredLSTM with 1 and 3 layers at 1, 12 and 64 images, <end> biased far down: every beam runs all
             21 steps in every variant
  early      StackedFactoredLSTM, 1 layer, 12 images, <end> biased far UP: every beam has ended after step 2, where the host
             loop stops; on_device and one_call run with poll_every=4
  fl         the reference's one-layer DecoderFactoredLSTM at 12 images, <end> biased far down: host and on_device run the
             composed chain, one_call the folded one
Every variant of a cell must return the same sequences: the tool exits non-zero otherwise.

usage: python tools/time_beam_decode.py [--cells sf1,sf3,early,fl] [--images 1,12,64] [--reps R]
On a shared GPU run one cell per process, each under its own time limit, chained so that a failure ends the chain:
  timeout -k 10 300 python tools/time_beam_decode.py --cells sf1 && timeout -k 10 300 python tools/time_beam_decode.py --cells sf3 && ...
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
from capnet.model import DecoderFactoredLSTM  # noqa: E402
from capnet.stacked import StackedFactoredLSTM  # noqa: E402

E, H, F, V, K, MAXLEN = 300, 512, 1024, 8192, 5, 20
START, END = 1, 2


def _bias_end(dec, value):
    with torch.no_grad():
        dec.C.bias[END] = value


def _time(dec, feats, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seqs = dec.sample_batch(feats, START, END, k=K, mode="factual", **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, seqs


def compare(dec, feats, reps, variants):
    """{name: median ms, name_range: [min, max]} of sample_batch under each of `variants` (name -> keywords), alternated;
    "same_sequences": whether all variants returned the same."""
    want, same = None, True
    for kw in variants.values():                      # untimed: allocator, weight folds, code objects, the workspace
        _, seqs = _time(dec, feats, **kw)
        want = want or seqs
        same = same and seqs == want
    runs = {name: [] for name in variants}
    for _ in range(reps):
        for name, kw in variants.items():
            runs[name].append(_time(dec, feats, **kw)[0])
    out = {}
    for name, v in runs.items():
        out[name] = round(statistics.median(v), 3)
        out[name + "_range"] = [round(min(v), 3), round(max(v), 3)]
    out["longest_sequence"], out["same_sequences"] = max(len(s) for s in want), same
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="sf1,sf3,early,fl")
    ap.add_argument("--images", default="1,12,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_beam_decode.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_beam_decode: needs the GPU")
    dev = torch.device("cuda:0")
    three = {"host": {}, "on_device": {"on_device": True}, "one_call": {"one_call": True}}
    result = {}
    for cell in args.cells.split(","):
        torch.manual_seed(len(cell))
        if cell in ("sf1", "sf3"):
            dec = StackedFactoredLSTM(E, H, F, V, int(cell[2]), max_seq_length=MAXLEN).to(dev).eval()
            _bias_end(dec, -100.0)
            for n in [int(v) for v in args.images.split(",")]:
                result["%s_n%d" % (cell, n)] = compare(dec, torch.zeros(n, E, device=dev), args.reps, three)
        elif cell == "early":
            dec = StackedFactoredLSTM(E, H, F, V, 1, max_seq_length=MAXLEN).to(dev).eval()
            _bias_end(dec, 100.0)
            result["early_n12"] = compare(dec, torch.zeros(12, E, device=dev), args.reps,
                                          {"host": {}, "on_device_poll4": {"on_device": True, "poll_every": 4},
                                           "one_call_poll4": {"one_call": True, "poll_every": 4}})
        elif cell == "fl":
            dec = DecoderFactoredLSTM(E, H, F, V, 1, dropout=0.0, max_seq_length=MAXLEN).to(dev).eval()
            _bias_end(dec, -100.0)
            result["fl_n12"] = compare(dec, torch.zeros(12, E, device=dev), args.reps, three)
        else:
            raise SystemExit("time_beam_decode: unknown cell %r" % cell)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_beam_decode", "E": E, "H": H, "F": F, "V": V, "k": K, "max_seq_length": MAXLEN,
                       "reps": args.reps, "ms_per_sample_batch": result})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    if not all(r["same_sequences"] for r in result.values()):
        raise SystemExit("time_beam_decode: the variants returned different sequences")


if __name__ == "__main__":
    main()
