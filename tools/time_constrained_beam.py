"""Time sample_batch on the two device routes (on_device=True and one_call=True) without constraints and under
capnet.beam.Constraints(no_repeat_ngram=1, min_words=6, banned=(two ids)) -- tests/constrained_beam_cases' set D, the two ids
being the words the cell's captions use most without the ban, so that the set bites -- print ONE JSON line and append it to
profiles/time_constrained_beam.jsonl.

Wall ms per sample_batch (host clock around the call, ended by a synchronise), the variants alternated, `--reps` times
each in one process after one untimed call of each; per variant the median and the (min, max) of the repeats. k = 5,
V = 8192, max_seq_length = 20, <end> biased far down: every beam runs all 21 steps in every variant. The cells are those of
tools/time_beam_decode.py and tools/time_att_beam_decode.py:
  sf1, sf3   StackedFactoredLSTM with 1 and 3 layers, BASELINE configs[4]'s cell (embedding 300, hidden 512, factored 1024)
  fa7, fa14  DecoderFactoredLSTMAtt on a 7 x 7 / 14 x 14 map, BASELINE configs[3]'s sizes (attention 512, maps of 2048
             channels)
each at 12 and 64 images (--images). With <end> far down nothing completes and every timed call returns [<end>], so what the
set does is checked first, untimed, on the same decoder with <end> biased far UP (constraints_for): the unconstrained
captions are [start, <end>], the constrained ones six distinct unbanned words long on both routes, and constraints=None
returns what the call without the keyword returns: the tool exits non-zero otherwise.

--plain-only times the calls WITHOUT the keyword alone: that form also runs on a checkout from before the keyword existed,
which is how the unconstrained times are compared with the parent commit's -- this file copied into a build of the parent,
the two trees alternated process by process in one session, --label naming the tree in the line.

usage: python tools/time_constrained_beam.py [--cells sf1,sf3,fa7,fa14] [--images 12,64] [--reps R] [--plain-only] [--label TEXT]
On a shared GPU run one cell per process, each under its own time limit, chained so that a failure ends the chain.
"""
import argparse
import collections
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

A, E, H, F, V, CF, K, MAXLEN = 512, 300, 512, 1024, 8192, 2048, 5, 20
START, END = 1, 2
ROUTES = {"on_device": {"on_device": True}, "one_call": {"one_call": True}}


def _time(dec, feats, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seqs = dec.sample_batch(feats, START, END, k=K, mode="factual", **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, seqs


def _set_end(dec, value):
    with torch.no_grad():
        dec.C.bias[END] = value


def _keeps(seqs, c):
    """Whether every caption is [start, min_words words, <end>] without a word twice (g = 1) and without a banned id."""
    return all(len(q) == c.min_words + 2 and q[-1] == END and len(set(q)) == len(q) and not set(q) & set(c.banned) for q in seqs)


def constraints_for(dec, feats):
    """The constraint set of a cell and what it does there, untimed, with <end> biased far UP: unconstrained, every caption
    is [start, <end>]; under min_words = 6 every caption has six words, and the two of them used most (ties to the lower
    id) become `banned` -> (Constraints, checks)."""
    from capnet.beam import Constraints
    _set_end(dec, 100.0)
    free = {name: _time(dec, feats, kw)[1] for name, kw in ROUTES.items()}
    unbanned = _time(dec, feats, dict(one_call=True, constraints=Constraints(no_repeat_ngram=1, min_words=6)))[1]
    counts = collections.Counter(w for q in unbanned for w in q if w not in (START, END))
    banned = tuple(sorted(w for w, _ in sorted(counts.items(), key=lambda t: (-t[1], t[0]))[:2]))
    c = Constraints(no_repeat_ngram=1, min_words=6, banned=banned)
    got = {name: _time(dec, feats, dict(kw, constraints=c))[1] for name, kw in ROUTES.items()}
    checks = {"banned": list(banned),
              "unconstrained_is_start_end": all(q == [START, END] for v in free.values() for q in v),
              "none_is_the_call_without": all(_time(dec, feats, dict(kw, constraints=None))[1] == free[name] for name, kw in ROUTES.items()),
              "constraints_kept": all(_keeps(v, c) for v in got.values()) and _keeps(unbanned, Constraints(1, 6)),
              "routes_agree": got["on_device"] == got["one_call"],
              "the_ban_changed_captions": sum(a != b for a, b in zip(unbanned, got["one_call"])) > 0}
    _set_end(dec, -100.0)
    return c, checks


def compare(dec, feats, reps, plain_only):
    variants = {name: dict(kw) for name, kw in ROUTES.items()}
    checks = {}
    if not plain_only:
        c, checks = constraints_for(dec, feats)
        for name, kw in ROUTES.items():
            variants[name + "_constrained"] = dict(kw, constraints=c)
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
    ap.add_argument("--cells", default="sf1,sf3,fa7,fa14")
    ap.add_argument("--images", default="12,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_constrained_beam.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_constrained_beam: needs the GPU")
    dev = torch.device("cuda:0")
    result = {}
    for cell in args.cells.split(","):
        torch.manual_seed(len(cell))
        if cell in ("sf1", "sf3"):
            dec, side = StackedFactoredLSTM(E, H, F, V, int(cell[2]), max_seq_length=MAXLEN), 0
        elif cell in ("fa7", "fa14"):
            dec, side = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=MAXLEN), int(cell[2:])
        else:
            raise SystemExit("time_constrained_beam: unknown cell %r" % cell)
        dec = dec.to(dev).eval()
        _set_end(dec, -100.0)
        for n in [int(v) for v in args.images.split(",")]:
            feats = torch.rand(n, side * side, CF, device=dev) if side else torch.zeros(n, E, device=dev)
            result["%s_n%d" % (cell, n)] = compare(dec, feats, args.reps, args.plain_only)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_constrained_beam", "label": args.label, "plain_only": args.plain_only, "A": A, "E": E, "H": H,
                       "F": F, "V": V, "C": CF, "k": K, "max_seq_length": MAXLEN, "reps": args.reps,
                       "ms_per_sample_batch": result})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    bad = [(cell, name) for cell, r in result.items() for name, v in r.items() if v is False]
    if bad:
        raise SystemExit("time_constrained_beam: failed checks %r" % (bad,))


if __name__ == "__main__":
    main()
