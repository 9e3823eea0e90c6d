"""Time the captions of a batch of images in all four styles two ways -- `loop`: four sequential sample_batch(mode=m,
one_call=True) calls (capnet_beam_decode / capnet_att_beam_decode once per mode) and `styles`: one sample_styles call
(capnet_beam_decode_groups / capnet_att_beam_decode_groups: the four modes as four weight groups of the same launches) --
print ONE JSON line and append it to profiles/time_style_decode.jsonl.

Wall ms for the four styles (host clock around the calls, ended by a synchronise; the folds of the four modes are inside
both), the two variants alternated, `--reps` times each in one process after one untimed run of each; per variant the
median and the (min, max) of the repeats. k = 5, V = 8192, max_seq_length = 20, <end> biased far down: every beam runs all
21 steps. Cells:
  p1, p3   StackedFactoredLSTM with 1 / 3 layers at BASELINE configs[4]'s sizes (embedding 300, hidden 512, factored 1024)
           at 1, 12 and 64 images (--images)
  a1, a2   StackedFactoredLSTMAtt with 1 / 2 layers at configs[3]'s attention sizes (attention 512, 2048-channel maps) at
           12 images on a 7 x 7 map and 64 images on a 14 x 14 map
No beam completes under that bias, so every caption is the lone <end> in both variants: the tool times, it does not
compare (tests/test_style_decode_gpu.py does). "rows": modes x images x k, "calls": the grouped searches sample_styles
made (more than one where the rows' logits exceed the split-K slab, 0 where it took the loop).

usage: python tools/time_style_decode.py [--cells p1,p3,a1,a2] [--images 1,12,64] [--reps R]
On a shared GPU run one cell per process, each under its own time limit, chained so that a failure ends the chain."""
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
from capnet.stacked import MODES, StackedFactoredLSTM  # noqa: E402
from capnet.stacked_att import StackedFactoredLSTMAtt  # noqa: E402

A, E, H, F, V, CF, K, MAXLEN = 512, 300, 512, 1024, 8192, 2048, 5, 20
START, END = 1, 2


def _loop(dec, feats):
    return {m: dec.sample_batch(feats, START, END, k=K, mode=m, one_call=True) for m in MODES}


def _styles(dec, feats):
    return dec.sample_styles(feats, START, END, k=K)


def _time(fn, dec, feats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(dec, feats)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def compare(dec, feats, reps):
    variants = {"loop": _loop, "styles": _styles}
    calls = []
    real = {name: getattr(ops, name) for name in ("beam_decode", "att_beam_decode")}
    for name, fn in real.items():          # count the grouped searches of the untimed run
        setattr(ops, name, lambda *a, _fn=fn, **kw: (calls.append(kw.get("groups", 1)), _fn(*a, **kw))[1])
    for fn in variants.values():           # untimed: allocator, code objects, workspaces
        _time(fn, dec, feats)
    for name, fn in real.items():
        setattr(ops, name, fn)
    runs = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            runs[name].append(_time(fn, dec, feats)[0])
    out = {}
    for name, v in runs.items():
        out[name] = round(statistics.median(v), 3)
        out[name + "_range"] = [round(min(v), 3), round(max(v), 3)]
    out["styles_over_loop"] = round(out["styles"] / out["loop"], 3)
    out["rows"] = len(MODES) * feats.size(0) * K
    out["calls"] = sum(1 for g in calls if g > 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="p1,p3,a1,a2")
    ap.add_argument("--images", default="1,12,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_style_decode.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_style_decode: needs the GPU")
    dev = torch.device("cuda:0")
    result = {}
    for cell in args.cells.split(","):
        torch.manual_seed(len(cell) + int(cell[1:]))
        if cell in ("p1", "p3"):
            dec = StackedFactoredLSTM(E, H, F, V, int(cell[1:]), max_seq_length=MAXLEN)
            shapes = [(int(v), None) for v in args.images.split(",")]
        elif cell in ("a1", "a2"):
            dec = StackedFactoredLSTMAtt(A, E, H, F, V, int(cell[1:]), feature_size=CF, dropout=0.0, max_seq_length=MAXLEN)
            shapes = [(12, 7), (64, 14)]
        else:
            raise SystemExit("time_style_decode: unknown cell %r" % cell)
        dec = dec.to(dev).eval()
        with torch.no_grad():
            dec.C.bias[END] = -100.0
        for n, side in shapes:
            feats = torch.zeros(n, E, device=dev) if side is None else torch.rand(n, side * side, CF, device=dev)
            result["%s_n%d" % (cell, n)] = compare(dec, feats, args.reps)
        del dec
    ops.check_device_errors()
    line = json.dumps({"tool": "time_style_decode", "A": A, "E": E, "H": H, "F": F, "V": V, "C": CF, "k": K, "modes": len(MODES),
                       "max_seq_length": MAXLEN, "reps": args.reps, "ms_for_four_styles": result})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
