"""Time sample_batch on the two device routes (on_device=True and one_call=True) under
capnet.beam.Constraints(no_repeat_ngram=1, min_words=6) without forced words and with F = 1 and F = 4 of them, and without the
keyword at all; print ONE JSON line and append it to profiles/time_forced_beam.jsonl.

Wall ms per sample_batch (host clock around the call, ended by a synchronise), the variants alternated, `--reps` times each in
one process after one untimed call of each; per variant the median and the (min, max) of the repeats. k = 5, V = 8192,
max_seq_length = 20, <end> biased far down: every beam runs all 21 steps in every variant (under forced words <end> is
excluded or far down: the same). The cells are those of tools/time_constrained_beam.py at one batch size each:
  sf1:12, sf3:64    StackedFactoredLSTM with 1 and 3 layers at 12 and 64 images
  fa7:12, fa14:64   DecoderFactoredLSTMAtt on a 7 x 7 / 14 x 14 map at 12 and 64 images
With <end> far down nothing completes and every timed call returns [<end>], so what the forced words do is checked first,
untimed, on the same decoder with <end> biased far UP (forced_checks): without them every caption is [start, six words,
<end>]; with them every caption on both routes ends in <end> and contains every forced id, and the routes agree: the tool
exits non-zero otherwise.

--plain-only times the variants that exist without the field alone (no keyword; the Constraints without forced words): that
form also runs on a checkout from before the field existed, which is how the unforced times are compared with the parent
commit's -- this file copied into a build of the parent, the two trees alternated process by process in one session, --label
naming the tree in the line.

usage: python tools/time_forced_beam.py [--cells sf1:12,sf3:64,fa7:12,fa14:64] [--reps R] [--plain-only] [--label TEXT]
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
from capnet.beam import Constraints  # noqa: E402
from capnet.model_att import DecoderFactoredLSTMAtt  # noqa: E402
from capnet.stacked import StackedFactoredLSTM  # noqa: E402

A, E, H, F, V, CF, K, MAXLEN = 512, 300, 512, 1024, 8192, 2048, 5, 20
START, END = 1, 2
ROUTES = {"on_device": {"on_device": True}, "one_call": {"one_call": True}}
BASE = dict(no_repeat_ngram=1, min_words=6)
FORCED = {"forced1": (4000,), "forced4": (4000, 4001, 4002, 4003)}


def _time(dec, feats, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seqs = dec.sample_batch(feats, START, END, k=K, mode="factual", **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, seqs


def _set_end(dec, value):
    with torch.no_grad():
        dec.C.bias[END] = value


def forced_checks(dec, feats):
    """What the forced sets do in a cell, untimed, with <end> biased far UP."""
    _set_end(dec, 100.0)
    free = {name: _time(dec, feats, dict(kw, constraints=Constraints(**BASE)))[1] for name, kw in ROUTES.items()}
    checks = {"unforced_is_six_words": all(len(q) == 8 and q[-1] == END for v in free.values() for q in v)}
    for tag, ids in FORCED.items():
        c = Constraints(forced=ids, **BASE)
        got = {name: _time(dec, feats, dict(kw, constraints=c))[1] for name, kw in ROUTES.items()}
        checks[tag + "_kept"] = all(q[-1] == END and set(ids) <= set(q[1:]) and len(set(q)) == len(q) and len(q) >= 8
                                    for v in got.values() for q in v)
        checks[tag + "_routes_agree"] = got["on_device"] == got["one_call"]
        checks[tag + "_changed_captions"] = got["one_call"] != free["one_call"]
    _set_end(dec, -100.0)
    return checks


def compare(dec, feats, reps, plain_only):
    variants, checks = {}, {}
    for name, kw in ROUTES.items():
        variants[name] = dict(kw)
        variants[name + "_constrained"] = dict(kw, constraints=Constraints(**BASE))
    if not plain_only:
        checks = forced_checks(dec, feats)
        for name, kw in ROUTES.items():
            for tag, ids in FORCED.items():
                variants[name + "_" + tag] = dict(kw, constraints=Constraints(forced=ids, **BASE))
    first = {name: _time(dec, feats, kw)[1] for name, kw in variants.items()}     # untimed: allocator, code objects, workspaces
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
    ap.add_argument("--cells", default="sf1:12,sf3:64,fa7:12,fa14:64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_forced_beam.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_forced_beam: needs the GPU")
    dev = torch.device("cuda:0")
    result = {}
    for spec in args.cells.split(","):
        cell, n = spec.split(":")
        n = int(n)
        torch.manual_seed(len(cell))
        if cell in ("sf1", "sf3"):
            dec, side = StackedFactoredLSTM(E, H, F, V, int(cell[2]), max_seq_length=MAXLEN), 0
        elif cell in ("fa7", "fa14"):
            dec, side = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=MAXLEN), int(cell[2:])
        else:
            raise SystemExit("time_forced_beam: unknown cell %r" % cell)
        dec = dec.to(dev).eval()
        _set_end(dec, -100.0)
        feats = torch.rand(n, side * side, CF, device=dev) if side else torch.zeros(n, E, device=dev)
        result["%s_n%d" % (cell, n)] = compare(dec, feats, args.reps, args.plain_only)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_forced_beam", "label": args.label, "plain_only": args.plain_only, "A": A, "E": E, "H": H,
                       "F": F, "V": V, "C": CF, "k": K, "max_seq_length": MAXLEN, "reps": args.reps, "forced": FORCED,
                       "ms_per_sample_batch": result})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    bad = [(cell, name) for cell, r in result.items() for name, v in r.items() if v is False]
    if bad:
        raise SystemExit("time_forced_beam: failed checks %r" % (bad,))


if __name__ == "__main__":
    main()
