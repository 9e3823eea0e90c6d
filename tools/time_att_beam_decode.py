"""Time an attention decoder's sample_batch three ways -- the beam bookkeeping on the host (the default), on_device=True
(capnet.beam.beam_search_device over capnet.decode.att_beam_step: a Python loop of launches on per-row copies of the maps)
and one_call=True (capnet_att_beam_decode: the k beams of an image on one read of its maps, the cell folded or packed for
the fused decode step, no Python per step) -- print ONE JSON line and append it to profiles/time_att_beam_decode.jsonl.

Wall ms per sample_batch (host clock around the call, ended by a synchronise), the variants alternated, `--reps` times
each in one process after one untimed call of each; per variant the median and the (min, max) of the repeats. k = 5,
V = 8192, max_seq_length = 20, BASELINE configs[3]'s sizes (attention 512, embedding 300, hidden 512, factored 1024,
feature maps of 2048 channels), <end> biased far down: every beam runs all 21 steps in every variant. Cells:
  fa7, fa14  DecoderFactoredLSTMAtt on a 7 x 7 / 14 x 14 map at 1, 12 and 64 images (--images)
  rnn        DecoderRNNAtt on a 7 x 7 map at 12 images
  sfa2       StackedFactoredLSTMAtt with 2 layers on a 7 x 7 map at 12 images
on_device=True is the yardstick. A cell whose per-step map copies ([n k, P, A + C] floats, twice: the copy and
index_select's source stay alive together) would not fit in the free memory skips the host and on_device variants and
says so ("skipped"). Every variant of a cell must return the same sequences: the tool exits non-zero otherwise.

usage: python tools/time_att_beam_decode.py [--cells fa7,fa14,rnn,sfa2] [--images 1,12,64] [--reps R]
On a shared GPU run one cell per process, each under its own time limit, chained so that a failure ends the chain:
  timeout -k 10 300 python tools/time_att_beam_decode.py --cells fa7 && timeout -k 10 300 python tools/time_att_beam_decode.py --cells fa14 && ...
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
from capnet.nic_model_att import DecoderRNNAtt  # noqa: E402
from capnet.stacked_att import StackedFactoredLSTMAtt  # noqa: E402

A, E, H, F, V, CF, K, MAXLEN = 512, 300, 512, 1024, 8192, 2048, 5, 20
START, END = 1, 2


def _time(dec, feats, kw, **variant):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seqs = dec.sample_batch(feats, START, END, k=K, **kw, **variant)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, seqs


def compare(dec, feats, kw, reps, variants):
    """{name: median ms, name_range: [min, max]} of sample_batch under each of `variants` (name -> keywords), alternated;
    "same_sequences": whether all variants returned the same."""
    want, same = None, True
    for v in variants.values():                      # untimed: allocator, weight folds, code objects, the workspace
        _, seqs = _time(dec, feats, kw, **v)
        want = want or seqs
        same = same and seqs == want
    runs = {name: [] for name in variants}
    for _ in range(reps):
        for name, v in variants.items():
            runs[name].append(_time(dec, feats, kw, **v)[0])
    out = {}
    for name, v in runs.items():
        out[name] = round(statistics.median(v), 3)
        out[name + "_range"] = [round(min(v), 3), round(max(v), 3)]
    if "on_device" in out:
        out["one_call_over_on_device"] = round(out["one_call"] / out["on_device"], 3)
    out["longest_sequence"], out["same_sequences"] = max(len(s) for s in want), same
    return out


def cell_result(dec, kw, n, side, reps, dev):
    three = {"host": {}, "on_device": {"on_device": True}, "one_call": {"one_call": True}}
    P = side * side
    copies = 2 * n * K * P * (A + CF) * 4
    free = torch.cuda.mem_get_info(dev)[0]
    if copies > 0.8 * free:
        three = {"one_call": {"one_call": True}}
    feats = torch.rand(n, P, CF, device=dev)
    out = compare(dec, feats, kw, reps, three)
    if len(three) == 1:
        out["skipped"] = "host, on_device: %.1f GB of per-step map copies" % (copies / 1e9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="fa7,fa14,rnn,sfa2")
    ap.add_argument("--images", default="1,12,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_att_beam_decode.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_att_beam_decode: needs the GPU")
    dev = torch.device("cuda:0")
    result = {}
    for cell in args.cells.split(","):
        torch.manual_seed(len(cell))
        if cell in ("fa7", "fa14"):
            dec, kw = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=MAXLEN), {"mode": "factual"}
            sides, images = [int(cell[2:])], [int(v) for v in args.images.split(",")]
        elif cell == "rnn":
            dec, kw, sides, images = DecoderRNNAtt(A, E, H, V, 1, feature_size=CF, max_seq_length=MAXLEN), {}, [7], [12]
        elif cell == "sfa2":
            dec, kw = StackedFactoredLSTMAtt(A, E, H, F, V, 2, feature_size=CF, dropout=0.0, max_seq_length=MAXLEN), {"mode": "factual"}
            sides, images = [7], [12]
        else:
            raise SystemExit("time_att_beam_decode: unknown cell %r" % cell)
        dec = dec.to(dev).eval()
        with torch.no_grad():
            (dec.linear if cell == "rnn" else dec.C).bias[END] = -100.0
        for side in sides:
            for n in images:
                result["%s_n%d" % (cell, n)] = cell_result(dec, kw, n, side, args.reps, dev)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_att_beam_decode", "A": A, "E": E, "H": H, "F": F, "V": V, "C": CF, "k": K,
                       "max_seq_length": MAXLEN, "reps": args.reps, "ms_per_sample_batch": result})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    if not all(r["same_sequences"] for r in result.values()):
        raise SystemExit("time_att_beam_decode: the variants returned different sequences")


if __name__ == "__main__":
    main()
