"""Time the stacked attention decoder's train step (capnet.stacked_att.StackedFactoredLSTMAtt) and print ONE JSON line.

One step = forward, loss (cross entropy + the alphas term), backward, the gradient clamp and Adam, through
capnet.train.train_step_att with the image features precomputed (the trunk is not timed). The cell is BASELINE's
attention cell (attention 512, embedding 300, hidden 512, factored 512, feature map 14 x 14 x 2048), V = 8192, teacher
forcing 0.5 (one fixed mask per step, the same for every configuration). Every (layers, rows) is timed with the fused
upper step (default) and with CAPNET_NO_FUSED_UPPER_STEP=1 (the composed step), in one process.

usage: python tools/time_stacked_att.py [--layers 1,2,3] [--rows 12,96] [--steps K] [--warmup W] [--no-compare]
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import capnet  # noqa: E402,F401
from capnet.optim import Adam  # noqa: E402
from capnet.stacked_att import StackedFactoredLSTMAtt  # noqa: E402
from capnet.train import CrossEntropyLoss, train_step_att  # noqa: E402

A, E, H, F, C, P, V = 512, 300, 512, 512, 2048, 196, 8192
FUSED_OFF = "CAPNET_NO_FUSED_UPPER_STEP"


class FixedFeatures(nn.Module):
    """The encoder of train_step_att: the precomputed feature map."""

    def __init__(self, feats):
        super().__init__()
        self.feats = feats

    def forward(self, images):
        return self.feats


def time_config(layers, rows, steps, warmup, fused, dev):
    torch.manual_seed(layers * 1000 + rows)
    dec = StackedFactoredLSTMAtt(A, E, H, F, V, layers, feature_size=C).to(dev).train()
    opt = Adam(list(dec.parameters()), lr=2e-4)
    g = torch.Generator().manual_seed(rows)
    lengths = sorted([int(v) for v in torch.randint(10, 21, (rows,), generator=g)], reverse=True)
    captions = torch.randint(3, V, (rows, max(lengths)), generator=g).to(dev)
    enc = FixedFeatures((torch.rand(rows, 14, 14, C, generator=g) * 0.5).to(dev))
    crit = CrossEntropyLoss()
    rnd = random.Random(7)
    masks = [[rnd.random() < 0.5 for _ in range(max(lengths) - 1)] for _ in range(warmup + steps)]
    if fused:
        os.environ.pop(FUSED_OFF, None)
    else:
        os.environ[FUSED_OFF] = "1"
    try:
        for k in range(warmup):
            train_step_att(enc, dec, opt, crit, None, captions, lengths, 5.0, tf_mask=masks[k])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(steps):
            loss = train_step_att(enc, dec, opt, crit, None, captions, lengths, 5.0, tf_mask=masks[warmup + k])
        e1.record()
        torch.cuda.synchronize()
    finally:
        os.environ.pop(FUSED_OFF, None)
    if not torch.isfinite(loss).item():
        raise RuntimeError("non-finite loss at layers=%d rows=%d" % (layers, rows))
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="1,2,3")
    ap.add_argument("--rows", default="12,96")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-compare", action="store_true", help="time the default (fused) step only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_stacked_att: needs the GPU")
    dev = torch.device("cuda:0")
    res = {}
    for layers in [int(v) for v in args.layers.split(",")]:
        for rows in [int(v) for v in args.rows.split(",")]:
            for fused in ((True,) if args.no_compare else (True, False)):
                key = "L%d_B%d_%s" % (layers, rows, "fused" if fused else "composed")
                res[key] = round(time_config(layers, rows, args.steps, args.warmup, fused, dev), 3)
    print(json.dumps({"tool": "time_stacked_att", "unit": "ms per decoder train step", "V": V, "tf": 0.5,
                      "steps": args.steps, "warmup": args.warmup, "ms": res}))


if __name__ == "__main__":
    main()
