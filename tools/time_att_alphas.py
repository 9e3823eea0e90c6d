"""Time what the attention maps cost -- print ONE JSON line and append it to profiles/time_att_alphas.jsonl.

Wall ms per call (host clock around the call, ended by a synchronise), the variants alternated in one process, `--reps`
(25) times each after 2 untimed calls of each; per variant the median and the spread (max - min) of the repeats. k = 5,
V = 8192, max_seq_length = 20, BASELINE configs[3]'s sizes (attention 512, embedding 300, hidden 512, factored 1024,
feature maps of 2048 channels), <end> biased far down: every beam runs all 21 steps in every variant. Per cell:
  one_call    sample_batch(one_call=True)                                      the search alone
  trace       sample_batch(one_call=True, return_alphas=True)                  the search records its maps
  replay      sample_batch(one_call=True), then capnet.decode.replay_alphas    the maps by replay of the tokens
  styles / styles_trace  (factored cells) sample_styles and sample_styles_alphas with four modes
Cells: fa = DecoderFactoredLSTMAtt, sfa2 = StackedFactoredLSTMAtt with 2 layers; each at 12 images on a 7 x 7 map and at
64 images on a 14 x 14 map (--shapes). trace - one_call is the trace's cost; trace against replay decides the route.
With <end> biased away nothing completes, so the searches return [<end>] and no maps: the trace still pays for its 21
slices and its rows, which is what is timed, but a replay of [<end>] would be free. `replay` therefore replays, per image,
a caption of the greatest length a search can return (start and 21 words, random ones: the cost of a replayed step does
not depend on the word) -- what the replay route pays for captions that run to the end, as the timed searches do.
The variants of a cell must return the same sequences: the tool exits non-zero otherwise. (That recorded and replayed
maps agree is tests/test_att_alphas_gpu.py's matter.)

usage: python tools/time_att_alphas.py [--cells fa,sfa2] [--shapes 12x7,64x14] [--reps R]
On a shared GPU run one cell per process, each under its own time limit, chained so that a failure ends the chain:
  timeout -k 10 300 python tools/time_att_alphas.py --cells fa && timeout -k 10 300 python tools/time_att_alphas.py --cells sfa2
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
from capnet import decode, ops  # noqa: E402
from capnet.model_att import DecoderFactoredLSTMAtt  # noqa: E402
from capnet.stacked_att import StackedFactoredLSTMAtt  # noqa: E402

A, E, H, F, V, CF, K, MAXLEN = 512, 300, 512, 1024, 8192, 2048, 5, 20
START, END = 1, 2
MODES = ("factual", "happy", "sad", "angry")
UNTIMED = 2


def _variants(dec, feats):
    n = feats.shape[0]

    full = torch.randint(3, V, (n, MAXLEN + 1), generator=torch.Generator().manual_seed(n)).tolist()

    def replay():
        step_fn, state = dec._beam(feats, n, K, "factual", True)
        seqs = decode.beam_decode(dec, step_fn, state, n, K, START, END, one_call=True)
        return seqs, decode.replay_alphas(step_fn, state, [[START] + words for words in full], n, K)
    return {
        "one_call": lambda: (dec.sample_batch(feats, START, END, k=K, mode="factual", one_call=True), None),
        "trace": lambda: dec.sample_batch(feats, START, END, k=K, mode="factual", one_call=True, return_alphas=True),
        "replay": replay,
        "styles": lambda: (dec.sample_styles(feats, START, END, k=K, modes=MODES), None),
        "styles_trace": lambda: dec.sample_styles_alphas(feats, START, END, k=K, modes=MODES),
    }


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def cell_result(dec, feats, reps):
    variants = _variants(dec, feats)
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
    out["trace_minus_one_call"] = round(out["trace"] - out["one_call"], 3)
    out["replay_minus_trace"] = round(out["replay"] - out["trace"], 3)
    out["styles_trace_minus_styles"] = round(out["styles_trace"] - out["styles"], 3)
    seqs = first["one_call"][0]
    same = first["trace"][0] == seqs and first["replay"][0] == seqs and first["styles_trace"][0] == first["styles"][0] \
        and first["styles"][0]["factual"] == seqs
    out["longest_sequence"], out["same_sequences"] = max(len(s) for s in seqs), bool(same)
    out["replayed_steps"] = first["replay"][1][0].shape[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="fa,sfa2")
    ap.add_argument("--shapes", default="12x7,64x14")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_att_alphas.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_att_alphas: needs the GPU")
    dev = torch.device("cuda:0")
    result = {}
    for cell in args.cells.split(","):
        torch.manual_seed(len(cell))
        if cell == "fa":
            dec = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=MAXLEN)
        elif cell == "sfa2":
            dec = StackedFactoredLSTMAtt(A, E, H, F, V, 2, feature_size=CF, dropout=0.0, max_seq_length=MAXLEN)
        else:
            raise SystemExit("time_att_alphas: unknown cell %r" % cell)
        dec = dec.to(dev).eval()
        with torch.no_grad():
            dec.C.bias[END] = -100.0
        for shape in args.shapes.split(","):
            n, side = (int(v) for v in shape.split("x"))
            feats = torch.rand(n, side * side, CF, device=dev)
            result["%s_n%d_p%d" % (cell, n, side * side)] = cell_result(dec, feats, args.reps)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_att_alphas", "A": A, "E": E, "H": H, "F": F, "V": V, "C": CF, "k": K,
                       "max_seq_length": MAXLEN, "modes": len(MODES), "reps": args.reps, "untimed": UNTIMED,
                       "ms_per_call": result})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    bad = [name for name, r in result.items() if not r["same_sequences"]]
    if bad:
        raise SystemExit("time_att_alphas: the variants disagree in %s" % ", ".join(bad))


if __name__ == "__main__":
    main()
