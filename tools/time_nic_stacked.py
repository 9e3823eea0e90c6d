"""Time the stacked NIC decoders (capnet.nic_stacked) and print ONE JSON line.

Train step = forward, loss, backward, the gradient clamp and Adam, through capnet.train.train_step (StackedDecoderRNN:
embedding 300, hidden 512, B = 64 images, features [B, 300] precomputed) or train_step_att (StackedDecoderRNNAtt:
attention 512, embedding 300, hidden 512, feature map 14 x 14 x 2048 precomputed, 12 and 96 rows), V = 8192, teacher
forcing 0.5 (one fixed mask per step). Beam step (plain stack) = every layer's step and the vocabulary projection over
n k rows (device events around `--steps` steps) and the wall time of one sample_batch over n images, each with the fused
step (default) and with CAPNET_NO_FUSED_DECODE_STEP=1 (the composed step), alternating, `--reps` times; medians printed.

usage: python tools/time_nic_stacked.py [--layers 1,2,3] [--images 1,12,64] [--steps K] [--warmup W] [--reps R]
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
import torch.nn as nn  # noqa: E402

import capnet  # noqa: E402,F401
from capnet.decode import FUSED_DECODE_OFF, cell_stepper  # noqa: E402
from capnet.nic_stacked import StackedDecoderRNN, StackedDecoderRNNAtt  # noqa: E402
from capnet.optim import Adam  # noqa: E402
from capnet.train import CrossEntropyLoss, train_step, train_step_att  # noqa: E402

A, E, H, C, P, V, K = 512, 300, 512, 2048, 196, 8192, 5


class FixedFeatures(nn.Module):
    """The encoder of train_step / train_step_att: the precomputed features."""

    def __init__(self, feats):
        super().__init__()
        self.feats = feats

    def forward(self, images):
        return self.feats


def _set_fused(fused):
    if fused:
        os.environ.pop(FUSED_DECODE_OFF, None)
    else:
        os.environ[FUSED_DECODE_OFF] = "1"


def time_train(layers, rows, att, steps, warmup, dev):
    torch.manual_seed(layers * 1000 + rows)
    if att:
        dec = StackedDecoderRNNAtt(A, E, H, V, layers, feature_size=C).to(dev).train()
    else:
        dec = StackedDecoderRNN(E, H, V, layers).to(dev).train()
    opt = Adam(list(dec.parameters()), lr=2e-4)
    g = torch.Generator().manual_seed(rows)
    lengths = sorted([int(v) for v in torch.randint(10, 21, (rows,), generator=g)], reverse=True)
    captions = torch.randint(3, V, (rows, max(lengths)), generator=g).to(dev)
    shape = (rows, 14, 14, C) if att else (rows, E)
    enc = FixedFeatures((torch.rand(shape, generator=g) * 0.5).to(dev))
    crit, rnd = CrossEntropyLoss(), random.Random(7)
    n_tf = max(lengths) - 1 if att else max(lengths)
    masks = [[rnd.random() < 0.5 for _ in range(n_tf)] for _ in range(warmup + steps)]
    fn = train_step_att if att else train_step

    def one(k):
        return fn(enc, dec, opt, crit, None, captions, lengths, 5.0, tf_mask=masks[k])
    for k in range(warmup):
        one(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(steps):
        loss = one(warmup + k)
    e1.record()
    torch.cuda.synchronize()
    if not torch.isfinite(loss).all().item():
        raise RuntimeError("non-finite loss at layers=%d rows=%d" % (layers, rows))
    return e0.elapsed_time(e1) / steps


def time_step(dec, n, steps, fused, dev):
    _set_fused(fused)
    rows = n * K
    g = torch.Generator().manual_seed(rows)
    tokens = torch.randint(3, V, (rows,), generator=g).to(dev)
    state = ((torch.rand(rows, 2 * dec.num_layers, H, generator=g) - 0.5) * 0.5).to(dev)
    with torch.no_grad():
        step, emb = cell_stepper(dec._cells(), E, H), dec.embed.weight.detach()
        for _ in range(3):
            top, st = step(emb, tokens, state)
            dec.linear(top)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            top, st = step(emb, tokens, state)
            dec.linear(top)
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
    seqs = dec.sample_batch(feats, 1, 2, k=K)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, max(len(s) for s in seqs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="1,2,3")
    ap.add_argument("--images", default="1,12,64")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nic_stacked: needs the GPU")
    dev = torch.device("cuda:0")
    layers = [int(v) for v in args.layers.split(",")]
    train_ms = {}
    for L in layers:
        train_ms["plain_L%d_B64" % L] = round(time_train(L, 64, False, args.steps, args.warmup, dev), 3)
        for rows in (12, 96):
            train_ms["att_L%d_rows%d" % (L, rows)] = round(time_train(L, rows, True, args.steps, args.warmup, dev), 3)
    step_ms, sample_ms, lengths = {}, {}, {}
    try:
        for L in layers:
            torch.manual_seed(L)
            dec = StackedDecoderRNN(E, H, V, L, max_seq_length=20).to(dev).eval()
            for n in [int(v) for v in args.images.split(",")]:
                runs = {}
                for _ in range(args.reps):
                    for fused in (True, False):
                        name = "fused" if fused else "composed"
                        st = time_step(dec, n, 50, fused, dev)
                        sb, ln = time_sample_batch(dec, n, fused, dev)
                        runs.setdefault(name, []).append((st, sb, ln))
                for name, r in runs.items():
                    key = "L%d_n%d_%s" % (L, n, name)
                    step_ms[key] = round(statistics.median(v[0] for v in r), 4)
                    sample_ms[key] = round(statistics.median(v[1] for v in r), 2)
                    lengths[key] = r[0][2]
            del dec
    finally:
        os.environ.pop(FUSED_DECODE_OFF, None)
    print(json.dumps({"tool": "time_nic_stacked", "A": A, "E": E, "H": H, "C": C, "V": V, "k": K, "tf": 0.5,
                      "ms_per_train_step": train_ms, "ms_per_beam_step": step_ms, "ms_per_sample_batch": sample_ms,
                      "longest_sequence": lengths}))


if __name__ == "__main__":
    main()
