"""Time sample_batch on the two device routes (on_device=True and one_call=True) without diversity and under
capnet.beam.Diversity(2, 0.5) and Diversity(3, 0.5) at the same k, print ONE JSON line and append it to
profiles/time_diverse_beam.jsonl.

Wall ms per sample_batch (host clock around the call, ended by a synchronise), the variants alternated, `--reps` times
each in one process after two untimed rounds; per variant the median and the (min, max) of the repeats -- the method of
tools/time_constrained_beam.py. k = 6, V = 8192, max_seq_length = 20, <end> biased far down: every beam of every group runs
all 21 steps in every variant. The cells:
  sf1_n12, sf3_n64   StackedFactoredLSTM with 1 layer at 12 images and 3 layers at 64, BASELINE configs[4]'s cell (embedding
                     300, hidden 512, factored 1024)
  fa7_n12, fa14_n64  DecoderFactoredLSTMAtt on a 7 x 7 map at 12 images and a 14 x 14 map at 64, BASELINE configs[3]'s sizes
                     (attention 512, maps of 2048 channels)
With <end> far down nothing completes and every timed call returns [<end>], so what diversity does is checked first,
untimed, on the same decoder with <end> biased far UP and Constraints(min_words=6), so that every caption has six words:
per image capnet.metrics.distinct_n(., 2) over the D captions of Diversity(D, 0.5, per_group=True) beside that of the first D
entries of the plain n-best at the same k (the mean over the images is reported), both routes must agree, and
diversity=None must return what the call without the keyword returns: the tool exits non-zero otherwise.

--plain-only times the calls WITHOUT the keyword alone: that form also runs on a checkout from before the keyword existed,
which is how the un-diverse times are compared with the parent commit's -- this file copied into a build of the parent, the
two trees alternated process by process in one session, --label naming the tree in the line.

usage: python tools/time_diverse_beam.py [--cells sf1_n12,sf3_n64,fa7_n12,fa14_n64] [--reps R] [--plain-only] [--label TEXT]
On a shared GPU run one cell per process, each under its own time limit, chained so that a failure ends the chain.
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
from capnet.stacked import StackedFactoredLSTM  # noqa: E402

A, E, H, F, V, CF, K, MAXLEN = 512, 300, 512, 1024, 8192, 2048, 6, 20
START, END = 1, 2
ROUTES = {"on_device": {"on_device": True}, "one_call": {"one_call": True}}
GROUPS, STRENGTH, UNTIMED = (2, 3), 0.5, 2


def _time(dec, feats, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seqs = dec.sample_batch(feats, START, END, k=K, mode="factual", **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, seqs


def _set_end(dec, value):
    with torch.no_grad():
        dec.C.bias[END] = value


def diversity_checks(dec, feats):
    """What the groups do in a cell, untimed, with <end> biased far UP under min_words = 6 -> checks and distinct-2 numbers."""
    from capnet.beam import Constraints, Diversity
    from capnet.metrics import distinct_n
    c = Constraints(min_words=6)
    _set_end(dec, 100.0)
    out = {}
    free = {name: _time(dec, feats, dict(kw, constraints=c))[1] for name, kw in ROUTES.items()}
    out["none_is_the_call_without"] = all(_time(dec, feats, dict(kw, constraints=c, diversity=None))[1] == free[name]
                                          for name, kw in ROUTES.items())
    plain = _time(dec, feats, dict(one_call=True, constraints=c, nbest=True))[1]
    for D in GROUPS:
        got = {name: _time(dec, feats, dict(kw, constraints=c, nbest=True, diversity=Diversity(D, STRENGTH, per_group=True)))[1]
               for name, kw in ROUTES.items()}
        caps = [[e[0] for e in hyps if e is not None] for hyps in got["one_call"]]
        out["routes_agree_D%d" % D] = [[e and e[0] for e in h] for h in got["on_device"]] == [[e and e[0] for e in h] for h in got["one_call"]]
        out["every_group_completed_D%d" % D] = all(len(q) == D for q in caps)
        out["six_words_D%d" % D] = all(len(t) == 8 and t[-1] == END for q in caps for t in q)
        out["distinct2_D%d" % D] = round(statistics.mean(distinct_n(q, 2) for q in caps), 4)
        out["distinct2_plain_first%d" % D] = round(statistics.mean(distinct_n([t for t, _ in hyps[:D]], 2) for hyps in plain), 4)
    _set_end(dec, -100.0)
    return out


def compare(dec, feats, reps, plain_only):
    variants = {name: dict(kw) for name, kw in ROUTES.items()}
    checks = {}
    if not plain_only:
        from capnet.beam import Diversity
        checks = diversity_checks(dec, feats)
        for D in GROUPS:
            for name, kw in ROUTES.items():
                variants["%s_D%d" % (name, D)] = dict(kw, diversity=Diversity(D, STRENGTH))
    for _ in range(UNTIMED):       # untimed: allocator, code objects, workspaces
        first = {name: _time(dec, feats, kw)[1] for name, kw in variants.items()}
    checks["timed_routes_agree"] = all(v == first["on_device"] for v in first.values())   # (<end> far down: [<end>] everywhere)
    runs = {name: [] for name in variants}
    for _ in range(reps):
        for name, kw in variants.items():
            runs[name].append(_time(dec, feats, kw)[0])
    out = {}
    for name, v in runs.items():
        out[name] = round(statistics.median(v), 3)
        out[name + "_range"] = [round(min(v), 3), round(max(v), 3)]
    out.update(checks)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="sf1_n12,sf3_n64,fa7_n12,fa14_n64")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_diverse_beam.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_diverse_beam: needs the GPU")
    dev = torch.device("cuda:0")
    result = {}
    for name in args.cells.split(","):
        cell, _, images = name.partition("_n")
        torch.manual_seed(len(cell))
        if cell in ("sf1", "sf3") and images.isdigit():
            dec, side = StackedFactoredLSTM(E, H, F, V, int(cell[2]), max_seq_length=MAXLEN), 0
        elif cell in ("fa7", "fa14") and images.isdigit():
            dec, side = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=MAXLEN), int(cell[2:])
        else:
            raise SystemExit("time_diverse_beam: unknown cell %r" % name)
        dec = dec.to(dev).eval()
        _set_end(dec, -100.0)
        n = int(images)
        feats = torch.rand(n, side * side, CF, device=dev) if side else torch.zeros(n, E, device=dev)
        result[name] = compare(dec, feats, args.reps, args.plain_only)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_diverse_beam", "label": args.label, "plain_only": args.plain_only, "A": A, "E": E, "H": H,
                       "F": F, "V": V, "C": CF, "k": K, "strength": STRENGTH, "max_seq_length": MAXLEN, "reps": args.reps,
                       "untimed_rounds": UNTIMED, "ms_per_sample_batch": result})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    bad = [(cell, name) for cell, r in result.items() for name, v in r.items() if v is False]
    if bad:
        raise SystemExit("time_diverse_beam: failed checks %r" % (bad,))


if __name__ == "__main__":
    main()
