"""Time the three emotion captions of capnet.seq2seq three ways -- `styles`: one sample_styles(modes=happy, sad, angry) call
(the encoder's greedy loop once, then capnet_lstm_greedy_decode_groups: the three decoders as three weight groups of the
same launches), `three`: three sample(mode=m) calls (six greedy loops) and `one`: one sample(mode="happy") call (two
greedy loops) -- print ONE JSON line and append it to profiles/time_seq2seq_styles.jsonl.

Wall ms per call (host clock around `--inner` back-to-back calls ended by a synchronise, divided by their number; the
packing of the LSTM weights is inside every variant), the variants alternated, `--reps` windows each in one process after
`--warmup` untimed windows; per variant the median and the (min, max) of the windows. E = 300, H = 512, V = 8192, 40
steps, cells layers x rows. "grouped": the grouped calls one sample_styles call made (0 where it took the fallback).
The tool times, it does not compare (tests/test_seq2seq_styles_gpu.py does).

--variants one,three also runs on a tree without sample_styles: the same tool times sample(mode=...) before and after
the kernels gained their group arguments.

usage: python tools/time_seq2seq_styles.py [--layers 1,2,3] [--rows 1,12] [--reps R] [--warmup W] [--inner N]
                                           [--variants styles,three,one] [--out FILE]"""
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
from capnet.seq2seq import Seq2Seq  # noqa: E402

E, H, V, STEPS, START = 300, 512, 8192, 40, 1
EMOTIONS = ("happy", "sad", "angry")

VARIANTS = {
    "styles": lambda m, f: m.sample_styles(f, START, modes=EMOTIONS),
    "three": lambda m, f: [m.sample(f, START, mode=e) for e in EMOTIONS],
    "one": lambda m, f: m.sample(f, START, mode="happy"),
}


def _window(fn, model, feats, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn(model, feats)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def compare(model, feats, names, reps, warmup, inner):
    grouped = []
    real = getattr(ops, "lstm_greedy_decode_groups", None)
    if "styles" in names:                 # count the grouped calls of one untimed sample_styles call
        ops.lstm_greedy_decode_groups = lambda *a, **kw: (grouped.append(1), real(*a, **kw))[1]
        VARIANTS["styles"](model, feats)
        ops.lstm_greedy_decode_groups = real
    runs = {n: [] for n in names}
    for it in range(warmup + reps):
        for n in names:
            ms = _window(VARIANTS[n], model, feats, inner)
            if it >= warmup:
                runs[n].append(ms)
    out = {}
    for n, v in runs.items():
        out[n] = round(statistics.median(v), 4)
        out[n + "_range"] = [round(min(v), 4), round(max(v), 4)]
    if "styles" in names and "three" in names:
        out["styles_over_three"] = round(out["styles"] / out["three"], 3)
    if "styles" in names:
        out["grouped"] = len(grouped)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="1,2,3")
    ap.add_argument("--rows", default="1,12")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--variants", default="styles,three,one")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_seq2seq_styles.jsonl"))
    a = ap.parse_args()
    names = a.variants.split(",")
    if any(n not in VARIANTS for n in names):
        raise SystemExit("time_seq2seq_styles: variants are %s" % ", ".join(VARIANTS))
    if not torch.cuda.is_available():
        raise SystemExit("time_seq2seq_styles: needs the GPU")
    dev = torch.device("cuda:0")
    result = {}
    for L in [int(x) for x in a.layers.split(",")]:
        torch.manual_seed(L)
        model = Seq2Seq(E, H, V, L).to(dev).eval()
        for rows in [int(x) for x in a.rows.split(",")]:
            feats = torch.randn(rows, E, device=dev) * 0.5
            result["layers%d_rows%d" % (L, rows)] = compare(model, feats, names, a.reps, a.warmup, a.inner)
        del model
    ops.check_device_errors()
    res = {"tool": "time_seq2seq_styles", "E": E, "H": H, "V": V, "decode_steps": STEPS, "emotions": len(EMOTIONS),
           "reps": a.reps, "inner": a.inner, "ms_per_call": result}
    if a.tag:
        res["tag"] = a.tag
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
