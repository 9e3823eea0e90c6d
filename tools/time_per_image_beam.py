"""Time the one-call beam search under forced words three ways -- (a) sample_batch with a mixed capnet.beam.PerImage, one
forced word per image and every word different; (b) the same call under ONE shared Constraints(forced=(w,)); (c) n
single-image sample(..., constraints=c_i, one_call=True) calls, the only way to a rule per image before there was a
PerImage -- print ONE JSON line and append it to profiles/time_per_image_beam.jsonl.

Wall ms per variant (host clock around the call -- around all n calls in (c) -- ended by a synchronise), the variants
alternated, `--reps` times each in one process after one untimed call of each; per variant the median and the (min, max) of
the repeats. k = 5, V = 8192, max_seq_length = 20, <end> biased far down: every beam runs all 21 steps in every variant. The
cells are those of tools/time_forced_beam.py:
  sf1:12, sf3:64    StackedFactoredLSTM with 1 and 3 layers at 12 and 64 images
  fa7:12, fa14:64   DecoderFactoredLSTMAtt on a 7 x 7 / 14 x 14 map at 12 and 64 images
With <end> far down nothing completes and every timed call returns [<end>], so what the rules do is checked first, untimed, on
the same decoder with <end> biased far UP (rule_checks): under the mixed set image i's caption ends in <end>, holds ITS word
and is the caption of its own single-image call, and the captions under the shared word are others: the tool exits non-zero
otherwise. (a) and (b) differ by the row load and the workgroup-uniform branch of capnet_beam_advance_rules alone.

usage: python tools/time_per_image_beam.py [--cells sf1:12,sf3:64,fa7:12,fa14:64] [--reps R] [--label TEXT]
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
from capnet.beam import Constraints, PerImage  # noqa: E402
from capnet.model_att import DecoderFactoredLSTMAtt  # noqa: E402
from capnet.stacked import StackedFactoredLSTM  # noqa: E402

A, E, H, F, V, CF, K, MAXLEN = 512, 300, 512, 1024, 8192, 2048, 5, 20
START, END = 1, 2
FIRST_WORD = 4000              # image i is told to say word FIRST_WORD + i


def _sync_ms(t0):
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _batch(dec, feats, constraints):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seqs = dec.sample_batch(feats, START, END, k=K, mode="factual", one_call=True, constraints=constraints)
    return _sync_ms(t0), seqs


def _singles(dec, feats, entries):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seqs = [dec.sample(feats[i:i + 1], START, END, k=K, mode="factual", one_call=True, constraints=c)[0].tolist()
            for i, c in enumerate(entries)]
    return _sync_ms(t0), seqs


def _set_end(dec, value):
    with torch.no_grad():
        dec.C.bias[END] = value


def rule_checks(dec, feats, entries, mixed, shared):
    """What the rules do in a cell, untimed, with <end> biased far UP."""
    _set_end(dec, 100.0)
    got, one, alone = _batch(dec, feats, mixed)[1], _batch(dec, feats, shared)[1], _singles(dec, feats, entries)[1]
    _set_end(dec, -100.0)
    return {"every_image_says_its_word": all(q[-1] == END and c.forced[0] in q[1:] for q, c in zip(got, entries)),
            "mixed_is_the_single_image_calls": got == alone,
            "shared_word_gives_other_captions": one != got and all(shared.forced[0] in q[1:] for q in one)}


def compare(dec, feats, reps):
    n = feats.shape[0]
    entries = [Constraints(forced=(FIRST_WORD + i,)) for i in range(n)]
    mixed, shared = PerImage(entries), entries[0]
    checks = rule_checks(dec, feats, entries, mixed, shared)
    variants = {"per_image": lambda: _batch(dec, feats, mixed), "shared": lambda: _batch(dec, feats, shared),
                "single_calls": lambda: _singles(dec, feats, entries)}
    first = {name: fn()[1] for name, fn in variants.items()}     # untimed: allocator, code objects, workspaces, the rule table
    checks["timed_variants_agree"] = all(v == first["shared"] for v in first.values())   # (<end> far down: [<end>] everywhere)
    runs = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            runs[name].append(fn()[0])
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
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_per_image_beam.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_per_image_beam: needs the GPU")
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
            raise SystemExit("time_per_image_beam: unknown cell %r" % cell)
        dec = dec.to(dev).eval()
        _set_end(dec, -100.0)
        feats = torch.rand(n, side * side, CF, device=dev) if side else torch.zeros(n, E, device=dev)
        result["%s_n%d" % (cell, n)] = compare(dec, feats, args.reps)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_per_image_beam", "label": args.label, "A": A, "E": E, "H": H, "F": F, "V": V, "C": CF, "k": K,
                       "max_seq_length": MAXLEN, "reps": args.reps, "first_word": FIRST_WORD, "ms_per_variant": result})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    bad = [(cell, name) for cell, r in result.items() for name, v in r.items() if v is False]
    if bad:
        raise SystemExit("time_per_image_beam: failed checks %r" % (bad,))


if __name__ == "__main__":
    main()
