"""Time capnet.seq2seq and print ONE JSON line.

sample: Seq2Seq.sample(mode='factual') at E = 300, H = 512, V = 8192, 40 steps, over layers x rows: wall ms per call
(synchronised), the one-call greedy decode (default) against the composed loop (CAPNET_NO_FUSED_GREEDY=1: entry points
that predate the fused call -- stacked_decode_step, linear, argmax_rows), alternating, `--reps` repeats after `--warmup`;
median and range of each.
train: ms per step (forward, loss, backward, Adam) at B = 64, 12 columns, teacher forcing 0.5, `factual` and `happy`.

usage: python tools/time_seq2seq.py [--layers 1,2,3] [--rows 1,12,64] [--reps R] [--warmup W] [--steps K]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import capnet  # noqa: E402,F401
from capnet import ops  # noqa: E402
from capnet.optim import Adam  # noqa: E402
from capnet.seq2seq import FUSED_GREEDY_OFF, Seq2Seq  # noqa: E402
from capnet.train import CrossEntropyLoss  # noqa: E402

E, H, V = 300, 512, 8192


def _set_fused(fused):
    if fused:
        os.environ.pop(FUSED_GREEDY_OFF, None)
    else:
        os.environ[FUSED_GREEDY_OFF] = "1"


def time_sample(model, rows, reps, warmup, dev):
    feats = torch.randn(rows, E, device=dev) * 0.5
    ms = {"fused": [], "composed": []}
    for it in range(warmup + reps):
        for path in ("fused", "composed"):
            _set_fused(path == "fused")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.sample(feats, 1)
            torch.cuda.synchronize()
            if it >= warmup:
                ms[path].append((time.perf_counter() - t0) * 1e3)
    _set_fused(True)
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            for k, v in ms.items()}


def time_train(model, mode, steps, warmup, dev):
    B, T = 64, 12
    g = torch.Generator().manual_seed(1)
    feats = (torch.randn(B, E, generator=g) * 0.5).to(dev)
    lengths = sorted([int(v) for v in torch.randint(4, T + 1, (B,), generator=g)], reverse=True)
    seq = torch.randint(3, V, (B, T + 1), generator=g).to(dev)
    src, tgt = seq[:, :T].contiguous(), (seq[:, :T] if mode == "factual" else seq[:, 1:]).contiguous()
    params = list(model.parameters()) if mode == "factual" else list(getattr(model, "decoder_" + mode).parameters())
    opt, crit = Adam(params, lr=2e-4), CrossEntropyLoss()
    targets = ops.packed_targets(tgt, lengths)
    random.seed(0)
    for it in range(warmup + steps):
        if it == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        model.zero_grad()
        out = model(feats, (src, lengths), (src, lengths), teacher_forcing_ratio=0.5, mode=mode)
        crit(out, targets).backward()
        opt.step()
    torch.cuda.synchronize()
    ops.check_device_errors()
    return round((time.perf_counter() - t0) * 1e3 / steps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="1,2,3")
    ap.add_argument("--rows", default="1,12,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"tool": "time_seq2seq", "E": E, "H": H, "V": V, "decode_steps": 40, "reps": a.reps, "sample_ms": {},
           "train_ms_per_step": {}}
    for L in [int(x) for x in a.layers.split(",")]:
        torch.manual_seed(L)
        model = Seq2Seq(E, H, V, L).to(dev)
        model.eval()
        for rows in [int(x) for x in a.rows.split(",")]:
            res["sample_ms"]["layers%d_rows%d" % (L, rows)] = time_sample(model, rows, a.reps, a.warmup, dev)
        model.train()
        for mode in ("factual", "happy"):
            res["train_ms_per_step"]["layers%d_%s" % (L, mode)] = time_train(model, mode, a.steps, a.warmup, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
