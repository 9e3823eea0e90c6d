"""Time beam-search decoding with the stacked FactoredLSTM (capnet.stacked.StackedFactoredLSTM) and print ONE JSON line.

Two numbers per (layers, images): the decoder's beam step -- every layer's step and the vocabulary projection C over
n k rows, without the host's top-k bookkeeping -- in ms (device events around `--steps` steps), and the wall time of one
sample_batch over n images (host clock around the call, ended by a synchronise). The cell is BASELINE configs[4]'s
(embedding 300, hidden 512, factored 1024), V = 8192, k = 5. Every configuration is timed with the fused step (default)
and with CAPNET_NO_FUSED_DECODE_STEP=1 (the composed step), alternating, `--reps` times each in one process; the median
is printed.

usage: python tools/time_stacked_decode.py [--layers 1,2,3] [--images 1,12,64] [--steps K] [--reps R]
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
from capnet.decode import FUSED_DECODE_OFF  # noqa: E402
from capnet.stacked import StackedFactoredLSTM  # noqa: E402

E, H, F, V, K = 300, 512, 1024, 8192, 5


def _set_fused(fused):
    if fused:
        os.environ.pop(FUSED_DECODE_OFF, None)
    else:
        os.environ[FUSED_DECODE_OFF] = "1"


def time_step(dec, n, steps, fused, dev):
    """ms per decoder beam step over n k rows (the fold is outside the timed window, as in sample_batch)."""
    _set_fused(fused)
    rows = n * K
    g = torch.Generator().manual_seed(rows)
    tokens = torch.randint(3, V, (rows,), generator=g).to(dev)
    state = ((torch.rand(rows, 2 * dec.num_layers, H, generator=g) - 0.5) * 0.5).to(dev)
    with torch.no_grad():
        step, emb = dec._decode_stepper("factual"), dec.B.weight.detach()
        for _ in range(3):
            top, st = step(emb, tokens, state)
            dec.C(top)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            top, st = step(emb, tokens, state)
            dec.C(top)
        e1.record()
        torch.cuda.synchronize()
    if not torch.isfinite(st).all().item():
        raise RuntimeError("non-finite state at layers=%d images=%d" % (dec.num_layers, n))
    return e0.elapsed_time(e1) / steps


def time_sample_batch(dec, n, fused, dev):
    _set_fused(fused)
    feats = torch.zeros(n, E, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seqs = dec.sample_batch(feats, 1, 2, k=K, mode="factual")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, max(len(s) for s in seqs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="1,2,3")
    ap.add_argument("--images", default="1,12,64")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_stacked_decode: needs the GPU")
    dev = torch.device("cuda:0")
    step_ms, sample_ms, lengths = {}, {}, {}
    try:
        for layers in [int(v) for v in args.layers.split(",")]:
            torch.manual_seed(layers)
            dec = StackedFactoredLSTM(E, H, F, V, layers, max_seq_length=20).to(dev).eval()
            for n in [int(v) for v in args.images.split(",")]:
                runs = {}
                for _ in range(args.reps):
                    for fused in (True, False):
                        name = "fused" if fused else "composed"
                        st = time_step(dec, n, args.steps, fused, dev)
                        sb, ln = time_sample_batch(dec, n, fused, dev)
                        runs.setdefault(name, []).append((st, sb, ln))
                for name, r in runs.items():
                    key = "L%d_n%d_%s" % (layers, n, name)
                    step_ms[key] = round(statistics.median(v[0] for v in r), 4)
                    sample_ms[key] = round(statistics.median(v[1] for v in r), 2)
                    lengths[key] = r[0][2]
            del dec
    finally:
        os.environ.pop(FUSED_DECODE_OFF, None)
    print(json.dumps({"tool": "time_stacked_decode", "E": E, "H": H, "F": F, "V": V, "k": K, "steps": args.steps,
                      "reps": args.reps, "ms_per_beam_step": step_ms, "ms_per_sample_batch": sample_ms,
                      "longest_sequence": lengths}))


if __name__ == "__main__":
    main()
