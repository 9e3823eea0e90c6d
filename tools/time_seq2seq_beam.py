"""Time capnet.seq2seq.DecoderRNN.sample_beam three ways -- the fused step (fused_topk=True: csrc/vocab_topk.hip and
capnet_beam_advance_topk), the unfused step in the same C call (fused_topk=False: sgemm_splitk's logits block and
capnet_beam_advance) and the fallback loop (CAPNET_NO_FUSED_DECODE_STEP=1: capnet.beam.beam_search_device on the composed
step) -- print ONE JSON line and append it to profiles/time_seq2seq_beam.jsonl.

Wall ms per sample_beam call (host clock around the call, ended by a synchronise), the variants alternated, `--reps` times
each in one process after `--warmup` untimed calls of each; per variant the median and the (min, max) of the repeats, and per
cell `fused_wins`: the fused median is below the unfused median by more than the larger of the two ranges' widths (the
spread). E = 300, H = 512, V = 8192, k = 5, max_seq_length = 20; <end> is biased far down, so no beam completes and every call
runs all 21 steps in every variant (the lists are then [<end>] everywhere: the tool checks that, it does not compare captions
-- tests/test_seq2seq_beam_gpu.py does). The decoder starts from a random state.

capnet.seq2seq.FUSED_TOPK_MAX_ROWS is read off these lines: the largest measured n k at which fused_wins holds at every
layer count, 0 if there is none.

usage: python tools/time_seq2seq_beam.py [--layers 1,2,3] [--sentences 1,3,12,64] [--reps R] [--warmup W] [--variants ...]
On a shared GPU run one layer count per process, each under its own time limit, chained so that a failure ends the chain.
--variants fused,unfused with --reps small is what a kernel trace of one cell wants.
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
from capnet.decode import FUSED_DECODE_OFF  # noqa: E402
from capnet.seq2seq import DecoderRNN  # noqa: E402

E, H, V, K, MAXLEN = 300, 512, 8192, 5, 20
START, END = 1, 2
VARIANTS = {"fused": (True, False), "unfused": (False, False), "fallback": (None, True)}    # (fused_topk, composed loop)


def _time(dec, states, variant):
    fused, composed = VARIANTS[variant]
    if composed:
        os.environ[FUSED_DECODE_OFF] = "1"
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seqs = dec.sample_beam(START, END, states, k=K, fused_topk=fused)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, seqs
    finally:
        os.environ.pop(FUSED_DECODE_OFF, None)


def compare(dec, states, reps, warmup, variants):
    n = states[0].size(1)
    same = True
    for _ in range(warmup):                           # untimed: allocator, packing, code objects, the workspaces
        for name in variants:
            same = same and _time(dec, states, name)[1] == [[END]] * n
    runs = {name: [] for name in variants}
    for _ in range(reps):
        for name in variants:
            runs[name].append(_time(dec, states, name)[0])
    out = {"rows": n * K}
    for name, v in runs.items():
        out[name] = round(statistics.median(v), 3)
        out[name + "_range"] = [round(min(v), 3), round(max(v), 3)]
    if "fused" in runs and "unfused" in runs:
        spread = max(max(runs[x]) - min(runs[x]) for x in ("fused", "unfused"))
        out["spread"] = round(spread, 3)
        out["fused_wins"] = out["unfused"] - out["fused"] > spread
    out["all_end"] = same
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="1,2,3")
    ap.add_argument("--sentences", default="1,3,12,64")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variants", default="fused,unfused,fallback")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_seq2seq_beam.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_seq2seq_beam: needs the GPU")
    dev = torch.device("cuda:0")
    variants = args.variants.split(",")
    if any(v not in VARIANTS for v in variants):
        raise SystemExit("time_seq2seq_beam: variants are %s" % ", ".join(VARIANTS))
    result = {}
    for L in [int(v) for v in args.layers.split(",")]:
        torch.manual_seed(L)
        dec = DecoderRNN(E, H, V, L, dropout=0.0, max_seq_length=MAXLEN).to(dev).eval()
        with torch.no_grad():
            dec.linear.bias[END] = -100.0
        for n in [int(v) for v in args.sentences.split(",")]:
            states = tuple(torch.randn(L, n, H, device=dev) * 0.1 for _ in range(2))
            result["l%d_n%d" % (L, n)] = compare(dec, states, args.reps, args.warmup, variants)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_seq2seq_beam", "E": E, "H": H, "V": V, "k": K, "max_seq_length": MAXLEN, "reps": args.reps,
                       "warmup": args.warmup, "ms_per_sample_beam": result})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    if not all(r["all_end"] for r in result.values()):
        raise SystemExit("time_seq2seq_beam: a variant completed a beam; the cells are not the ones described")


if __name__ == "__main__":
    main()
