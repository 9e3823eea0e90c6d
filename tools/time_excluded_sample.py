"""Time sampled decoding under exclusions (sample_random(exclude=)) against the same call without them IN THE SAME
PROCESS, on the one-call route (capnet_*_sample_decode_excl against capnet_*_sample_decode) and on the composed loop
(CAPNET_NO_FUSED_SAMPLE=1: per step ops.sample_exclusion_mask + ops.mask_logits in front of the draw), and append one JSON line
per cell to profiles/time_excluded_sample.jsonl.

Wall ms per call (host clock around the call, ended by a synchronise), the four variants alternated, `--reps` times each after
`--warmup` untimed rounds; per variant the median and the (min, max) of the repeats, and per route the microseconds per step
the exclusions add (the difference of the medians over the steps).
Cells (the sizes of tools/time_constrained_beam.py: attention 512, embedding 300, hidden 512, factored 1024, V 8192, maps of
2048 channels; 21 steps):
  sf1 / sf3    StackedFactoredLSTM, 1 and 3 layers, 12 images x 1 sample = 12 rows
  fa7 / fa14   DecoderFactoredLSTMAtt, 12 images x 5 samples on 7 x 7 and on 14 x 14
each at top_k 0 and 5. The set is time_constrained_beam.py's D: no word twice, min_words = 6, two banned ids -- the two words
an unexcluded draw of the cell uses most. The tool checks, untimed, that the excluded captions keep the set, and reports
whether both routes drew the same tokens (random weights do not guarantee the margins; it does not fail on that).

usage: python tools/time_excluded_sample.py [--cells sf1,sf3,fa7,fa14] [--reps R] [--warmup W] [--label TEXT]
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
from capnet import decode, ops  # noqa: E402
from capnet.beam import Constraints, banned_words  # noqa: E402
from capnet.model_att import DecoderFactoredLSTMAtt  # noqa: E402
from capnet.stacked import StackedFactoredLSTM  # noqa: E402

A, E, H, F, V, CF, STEPS = 512, 300, 512, 1024, 8192, 2048, 21
START, END = 1, 2
OUT = os.path.join(ROOT, "profiles", "time_excluded_sample.jsonl")


def _set_fused(fused):
    if fused:
        os.environ.pop(decode.FUSED_SAMPLE_OFF, None)
    else:
        os.environ[decode.FUSED_SAMPLE_OFF] = "1"


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _keeps(lists, c):
    """Whether no caption takes a word capnet.beam.banned_words forbids it at that step."""
    return all(q[p] not in banned_words(q[:p], p, END, c) for img in lists for q, _ in img for p in range(1, len(q)))


def compare(dec, feats, m, top_k, reps, warmup):
    kw = dict(samples=m, temperature=1.0, top_k=top_k, seed=7)
    free = dec.sample_random(feats, START, END, **kw)
    counts = collections.Counter(w for img in free for q, _ in img for w in q if w not in (START, END))
    banned = tuple(sorted(w for w, _ in sorted(counts.items(), key=lambda t: (-t[1], t[0]))[:2]))
    c = Constraints(no_repeat_ngram=1, min_words=6, banned=banned)
    variants = {"one_call": (True, {}), "one_call_excluded": (True, {"exclude": c}),
                "composed": (False, {}), "composed_excluded": (False, {"exclude": c})}
    ms, last = {k: [] for k in variants}, {}
    for it in range(warmup + reps):
        for name, (fused, ex) in variants.items():
            _set_fused(fused)
            t, last[name] = _timed(lambda: dec.sample_random(feats, START, END, **kw, **ex))
            if it >= warmup:
                ms[name].append(t)
    _set_fused(True)
    res = {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}
    tokens = {k: [q for img in v for q, _ in img] for k, v in last.items()}
    return {"ms": res, "banned": list(banned),
            "us_per_step_added": {r: round((res[r + "_excluded"]["median"] - res[r]["median"]) * 1e3 / STEPS, 2)
                                  for r in ("one_call", "composed")},
            "excluded_keep_the_set": _keeps(last["one_call_excluded"], c) and _keeps(last["composed_excluded"], c),
            "unexcluded_breaks_the_set": not _keeps(last["one_call"], c),
            "same_tokens": tokens["one_call"] == tokens["composed"],
            "same_tokens_excluded": tokens["one_call_excluded"] == tokens["composed_excluded"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="sf1,sf3,fa7,fa14")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_excluded_sample: needs the GPU")
    dev = torch.device("cuda:0")
    bad = []
    for cell in a.cells.split(","):
        torch.manual_seed(len(cell))
        if cell in ("sf1", "sf3"):
            dec, side, m = StackedFactoredLSTM(E, H, F, V, int(cell[2]), max_seq_length=STEPS), 0, 1
        elif cell in ("fa7", "fa14"):
            dec, side, m = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=STEPS), int(cell[2:]), 5
        else:
            raise SystemExit("time_excluded_sample: unknown cell %r" % cell)
        dec = dec.to(dev).eval()
        feats = torch.rand(12, side * side, CF, device=dev) if side else torch.zeros(12, E, device=dev)
        for top_k in (0, 5):
            rec = {"tool": "time_excluded_sample", "label": a.label, "cell": cell, "rows": 12 * m, "steps": STEPS, "V": V, "top_k": top_k,
                   "reps": a.reps}
            rec.update(compare(dec, feats, m, top_k, a.reps, a.warmup))
            line = json.dumps(rec)
            print(line, flush=True)
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            with open(OUT, "a") as f:
                f.write(line + "\n")
            if not rec["excluded_keep_the_set"]:
                bad.append((cell, top_k))
        del dec
    ops.check_device_errors()
    if bad:
        raise SystemExit("time_excluded_sample: the excluded captions break the set in %r" % (bad,))


if __name__ == "__main__":
    main()
