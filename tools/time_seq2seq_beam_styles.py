"""Time capnet.seq2seq.Seq2Seq.sample_beam_styles over the three emotions -- one encoder pass and ONE grouped search
(capnet_lstm_beam_decode_groups), with the fused step (fused_topk=True: one capnet_vocab_topk_groups launch per step) and
with the unfused step (fused_topk=False: one sgemm_splitk per decoder per step) -- against what a caller had before it:
three Seq2Seq.sample_beam(mode=...) calls on their default route, each with its own encoder pass. Print ONE JSON line and
append it to profiles/time_seq2seq_beam_styles.jsonl.

Wall ms per variant (host clock around the call or the three calls, ended by a synchronise), the variants alternated,
`--reps` times each in one process after `--warmup` untimed rounds; per variant the median and the (min, max) of the
repeats; per cell the spread (the largest of the variants' range widths) and
  fused_wins    the grouped fused median is below the grouped unfused median by more than the spread,
  grouped_wins  the better grouped median is below the three calls' median by more than the spread.
E = 300, H = 512, V = 8192, k = 5, max_seq_length = 20; <end> is biased far down in every emotion decoder, so no beam
completes and every search runs all 21 steps in every variant (the lists are then [<end>] everywhere: the tool checks that,
it does not compare captions -- tests/test_seq2seq_beam_styles_gpu.py does). It also checks, by a spy on ops, that the
grouped variants made exactly one grouped call and the three calls none.

capnet.seq2seq.FUSED_TOPK_GROUPS_MAX_ROWS is read off these lines: the largest measured rows per decoder (n k) at which
fused_wins holds at every layer count, 0 if there is none.

usage: python tools/time_seq2seq_beam_styles.py [--layers 1,3] [--sentences 1,3,12,64] [--reps R] [--warmup W] [--out FILE]
On a shared GPU run one layer count per process, each under its own time limit, chained so that a failure ends the chain.
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
from capnet.seq2seq import Seq2Seq  # noqa: E402

E, H, V, K, MAXLEN = 300, 512, 8192, 5, 20
START, END = 1, 2
EMOTIONS = ("happy", "sad", "angry")
VARIANTS = ("grouped_fused", "grouped_unfused", "three_calls")


def _time(model, feats, variant):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if variant == "three_calls":
        out = {m: model.sample_beam(feats, START, END, mode=m, k=K) for m in EMOTIONS}
    else:
        out = model.sample_beam_styles(feats, START, END, modes=EMOTIONS, k=K, fused_topk=variant == "grouped_fused")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def compare(model, feats, reps, warmup):
    n = feats.size(0)
    want = {m: [[END]] * n for m in EMOTIONS}
    same = True
    grouped = []
    real = ops.lstm_beam_decode_groups
    ops.lstm_beam_decode_groups = lambda *a, **kw: (grouped.append(1), real(*a, **kw))[1]
    try:
        for _ in range(warmup):                       # untimed: allocator, packing, code objects, the workspaces
            for name in VARIANTS:
                del grouped[:]
                same = same and _time(model, feats, name)[1] == want
                same = same and len(grouped) == (0 if name == "three_calls" else 1)
        runs = {name: [] for name in VARIANTS}
        for _ in range(reps):
            for name in VARIANTS:
                runs[name].append(_time(model, feats, name)[0])
    finally:
        ops.lstm_beam_decode_groups = real
    out = {"rows_per_decoder": n * K}
    for name, v in runs.items():
        out[name] = round(statistics.median(v), 3)
        out[name + "_range"] = [round(min(v), 3), round(max(v), 3)]
    spread = max(max(v) - min(v) for v in runs.values())
    out["spread"] = round(spread, 3)
    out["fused_wins"] = out["grouped_unfused"] - out["grouped_fused"] > spread
    out["grouped_wins"] = out["three_calls"] - min(out["grouped_fused"], out["grouped_unfused"]) > spread
    out["as_described"] = same
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="1,3")
    ap.add_argument("--sentences", default="1,3,12,64")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_seq2seq_beam_styles.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_seq2seq_beam_styles: needs the GPU")
    dev = torch.device("cuda:0")
    result = {}
    for L in [int(v) for v in args.layers.split(",")]:
        torch.manual_seed(L)
        model = Seq2Seq(E, H, V, L, dropout=0.0).to(dev).eval()
        for mod in (model.encoder, model.decoder_happy, model.decoder_sad, model.decoder_angry):
            mod.max_seq_length = MAXLEN
        with torch.no_grad():
            for m in EMOTIONS:
                model._decoder(m).linear.bias[END] = -100.0
        for n in [int(v) for v in args.sentences.split(",")]:
            feats = torch.randn(n, E, device=dev) * 0.5
            result["l%d_n%d" % (L, n)] = compare(model, feats, args.reps, args.warmup)
        del model
    ops.check_device_errors()
    line = json.dumps({"tool": "time_seq2seq_beam_styles", "E": E, "H": H, "V": V, "k": K, "max_seq_length": MAXLEN,
                       "emotions": len(EMOTIONS), "reps": args.reps, "warmup": args.warmup, "ms": result})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    if not all(r["as_described"] for r in result.values()):
        raise SystemExit("time_seq2seq_beam_styles: a beam completed or a variant took another route; the cells are not the "
                         "ones described")


if __name__ == "__main__":
    main()
