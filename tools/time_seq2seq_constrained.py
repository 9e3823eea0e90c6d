"""Time capnet.seq2seq.DecoderRNN.sample_beam with and without constraints, on the fused step (fused_topk=True:
csrc/vocab_topk.hip, under constraints its select-only instance behind one capnet_beam_exclusion_mask launch) and on the
unfused step of the same C call (fused_topk=False: sgemm_splitk's logits block and capnet_beam_advance[_constrained]) -- print
ONE JSON line and append it to profiles/time_seq2seq_constrained.jsonl. Modelled on tools/time_seq2seq_beam.py and
tools/time_constrained_beam.py.

Wall ms per sample_beam call (host clock around the call, ended by a synchronise), the four variants alternated, `--reps`
times each in one process after `--warmup` untimed calls of each; per variant the median and the (min, max) of the repeats.
Per cell:
  fused_cost_us_per_step / unfused_cost_us_per_step: (constrained median - unconstrained median) / 21 steps, and
  *_cost_inside_spread: that difference is within the larger of the two ranges' widths;
  fused_wins: the CONSTRAINED fused median is below the constrained unfused median by more than the spread of those two --
  the crossover capnet.seq2seq.FUSED_TOPK_MAX_ROWS was set at without constraints (tools/time_seq2seq_beam.py).
E = 300, H = 512, V = 8192, k = 5, max_seq_length = 20; the constraint set is "no word twice, min_words = 6, two banned ids".
<end> is biased far down, so no beam completes and every call runs all 21 steps in every variant (the lists are then [<end>]
everywhere: the tool checks that; tests/test_seq2seq_constrained_gpu.py compares captions). The decoder starts from a random
state.
--sample also times sample_random with and without exclude= (the same set) per cell: `sample` / `sample_excl`.

usage: python tools/time_seq2seq_constrained.py [--layers 1,3] [--sentences 1,3,12,64] [--reps R] [--warmup W] [--sample]
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
from capnet.beam import Constraints  # noqa: E402
from capnet.seq2seq import DecoderRNN  # noqa: E402

E, H, V, K, MAXLEN = 300, 512, 8192, 5, 20
START, END = 1, 2
STEPS = MAXLEN + 1
SET = Constraints(no_repeat_ngram=1, min_words=6, banned=(7, 4099))
VARIANTS = {"fused": (True, None), "fused_con": (True, SET), "unfused": (False, None), "unfused_con": (False, SET)}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _beam(dec, states, variant):
    fused, con = VARIANTS[variant]
    return _timed(lambda: dec.sample_beam(START, END, states, k=K, fused_topk=fused, constraints=con))


def _summary(runs):
    out = {}
    for name, v in runs.items():
        out[name] = round(statistics.median(v), 3)
        out[name + "_range"] = [round(min(v), 3), round(max(v), 3)]
    return out


def _spread(runs, a, b):
    return max(max(runs[x]) - min(runs[x]) for x in (a, b))


def compare(dec, states, reps, warmup, sample):
    n = states[0].size(1)
    same = True
    for _ in range(warmup):                           # untimed: allocator, packing, code objects, the workspaces
        for name in VARIANTS:
            same = same and _beam(dec, states, name)[1] == [[END]] * n
    runs = {name: [] for name in VARIANTS}
    for _ in range(reps):
        for name in VARIANTS:
            runs[name].append(_beam(dec, states, name)[0])
    out = {"rows": n * K}
    out.update(_summary(runs))
    for step in ("fused", "unfused"):
        spread = _spread(runs, step, step + "_con")
        cost = out[step + "_con"] - out[step]
        out[step + "_cost_us_per_step"] = round(cost * 1e3 / STEPS, 2)
        out[step + "_cost_inside_spread"] = abs(cost) <= spread
    spread = _spread(runs, "fused_con", "unfused_con")
    out["spread_con"] = round(spread, 3)
    out["fused_wins"] = out["unfused_con"] - out["fused_con"] > spread
    out["all_end"] = same
    if sample:
        draws = {"sample": {}, "sample_excl": {"exclude": SET, "end_token": END}}
        sruns = {name: [] for name in draws}
        for i in range(warmup + reps):
            for name, kw in draws.items():
                ms, _ = _timed(lambda: dec.sample_random(START, states, temperature=1.0, top_k=0, seed=5, **kw))
                if i >= warmup:
                    sruns[name].append(ms)
        out.update(_summary(sruns))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="1,3")
    ap.add_argument("--sentences", default="1,3,12,64")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_seq2seq_constrained.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_seq2seq_constrained: needs the GPU")
    dev = torch.device("cuda:0")
    result = {}
    for L in [int(v) for v in args.layers.split(",")]:
        torch.manual_seed(L)
        dec = DecoderRNN(E, H, V, L, dropout=0.0, max_seq_length=MAXLEN).to(dev).eval()
        with torch.no_grad():
            dec.linear.bias[END] = -100.0
        for n in [int(v) for v in args.sentences.split(",")]:
            states = tuple(torch.randn(L, n, H, device=dev) * 0.1 for _ in range(2))
            result["l%d_n%d" % (L, n)] = compare(dec, states, args.reps, args.warmup, args.sample)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_seq2seq_constrained", "E": E, "H": H, "V": V, "k": K, "max_seq_length": MAXLEN,
                       "constraints": repr(SET), "reps": args.reps, "warmup": args.warmup, "ms_per_call": result})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    if not all(r["all_end"] for r in result.values()):
        raise SystemExit("time_seq2seq_constrained: a variant completed a beam; the cells are not the ones described")


if __name__ == "__main__":
    main()
