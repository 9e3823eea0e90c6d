"""Time sample_batch with the beam bookkeeping on the host (the default) against on_device=True (capnet.beam.
beam_search_device) and print ONE JSON line.

Wall ms per sample_batch (host clock around the call, ended by a synchronise), the two paths alternated, `--reps` times
each in one process after one untimed call of each; the median is printed. k = 5, V = 8192, max_seq_length = 20, the cell
of BASELINE configs[4] (embedding 300, hidden 512, factored 1024). Cells:
  sf1, sf3   StackedFactoredLSTM with 1 and 3 layers at 1, 12 and 64 images, <end> biased far down: every beam runs all
             21 steps (the host loop and the fixed-length device loop do the same number of steps)
  att        DecoderFactoredLSTMAtt (attention 512, a 7 x 7 x 2048 map) at 12 images, the same bias
  early      StackedFactoredLSTM, 1 layer, 12 images, <end> biased far UP: every beam has ended after step 2, where the host
             loop stops; on_device runs all 21 steps unless it polls -- timed with poll_every 0 and 4

usage: python tools/time_device_beam.py [--cells sf1,sf3,att,early] [--reps R]
On a shared GPU run one cell per process, each under its own time limit, chained so that a failure ends the chain:
  timeout -k 10 300 python tools/time_device_beam.py --cells sf1 && timeout -k 10 300 python tools/time_device_beam.py --cells sf3 && ...
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
from capnet.model_att import DecoderFactoredLSTMAtt  # noqa: E402
from capnet.stacked import StackedFactoredLSTM  # noqa: E402

E, H, F, V, K, A, P, CF, MAXLEN = 300, 512, 1024, 8192, 5, 512, 49, 2048, 20
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
    """{name: median ms} of sample_batch under each of `variants` (name -> keywords), alternated; "same_sequences": whether
    all variants returned the same (random weights at V = 8192 can hold a near-tie that the two row counts break
    differently)."""
    want, same = None, True
    for kw in variants.values():                      # untimed: allocator, weight folds, code objects
        _, seqs = _time(dec, feats, **kw)
        want = want or seqs
        same = same and seqs == want
    runs = {name: [] for name in variants}
    for _ in range(reps):
        for name, kw in variants.items():
            runs[name].append(_time(dec, feats, **kw)[0])
    out = {name: round(statistics.median(v), 3) for name, v in runs.items()}
    out["longest_sequence"], out["same_sequences"] = max(len(s) for s in want), same
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="sf1,sf3,att,early")
    ap.add_argument("--images", default="1,12,64")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_device_beam: needs the GPU")
    dev = torch.device("cuda:0")
    both = {"host": {}, "on_device": {"on_device": True}}
    result = {}
    for cell in args.cells.split(","):
        torch.manual_seed(len(cell))
        if cell in ("sf1", "sf3"):
            dec = StackedFactoredLSTM(E, H, F, V, int(cell[2]), max_seq_length=MAXLEN).to(dev).eval()
            _bias_end(dec, -100.0)
            for n in [int(v) for v in args.images.split(",")]:
                result["%s_n%d" % (cell, n)] = compare(dec, torch.zeros(n, E, device=dev), args.reps, both)
        elif cell == "att":
            dec = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=MAXLEN).to(dev).eval()
            _bias_end(dec, -100.0)
            result["att_n12"] = compare(dec, torch.rand(12, P, CF, device=dev), args.reps, both)
        elif cell == "early":
            dec = StackedFactoredLSTM(E, H, F, V, 1, max_seq_length=MAXLEN).to(dev).eval()
            _bias_end(dec, 100.0)
            result["early_n12"] = compare(dec, torch.zeros(12, E, device=dev), args.reps,
                                          dict(both, on_device_poll4={"on_device": True, "poll_every": 4}))
        else:
            raise SystemExit("time_device_beam: unknown cell %r" % cell)
        del dec
    print(json.dumps({"tool": "time_device_beam", "E": E, "H": H, "F": F, "V": V, "k": K, "max_seq_length": MAXLEN,
                      "reps": args.reps, "ms_per_sample_batch": result}))


if __name__ == "__main__":
    main()
