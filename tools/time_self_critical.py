"""Time one self-critical step (capnet.train.self_critical_step) and its parts, and append one JSON line per baseline to
profiles/time_self_critical.jsonl. A record; nothing is chosen by these numbers.

DecoderFactoredLSTMAtt at BASELINE configs[3]'s attention sizes (attention 512, embedding 300, hidden 512, factored 1024,
maps of 2048 channels, V 8192) on 7 x 7 maps, 12 images x 5 samples, 20 steps, reward = capnet.train.bleu_reward against
three random references per image (plus a hash of the tokens, so that the advantages are not all 0), capnet.optim.Adam.
Timed, each on its own with the inputs the step would give it:
  sample     decoder.sample_random(samples=5)                      the exploration
  baseline   decoder.sample_batch(k=1)                             the greedy caption ('greedy' only)
  reward     the host metric on every drawn caption (and the greedy ones)
  policy     capnet.train.policy_step on the drawn captions        pack, teacher-forced forward, loss, backward, clamp + Adam
  step       the whole self_critical_step
Wall ms per call (host clock around the call, ended by a synchronise), the parts alternated, `--reps` times each in one
process after `--warmup` untimed rounds; per part the median and the (min, max) of the repeats. The parameters move between
repeats (the optimiser steps), the shapes do not: the seed of the draw is fixed and an untrained decoder rarely draws <end>.

--routes: `host` is the above. `device`: reward = capnet.train.DeviceBleuReward (add-one BLEU), the step's device route -- one
decode with the greedy caption as one more row ('greedy'), the rewards of all rows from one ops.bleu_rows launch, the
advantages formed on the device; its parts: sample (sample_random(greedy=..., device=True)), reward (the launch, the
advantages and a synchronise), policy, step. `host_smooth`: the host route with the same add-one BLEU as a plain function.
For these two the decoder's output bias prefers sixteen words and the references are made of them, so that rewards differ
between captions without the hash. `device_cider` / `host_cider`: the same two routes with CIDEr-D
(capnet.train.DeviceCiderReward: ops.cider_rows on the device; the same object called as a host function), the same decoder
with the same bias and the same references; the corpus is the 12 images' references plus 400 seeded random reference sets
over the same words, so that the idf values are not all equal and the tables have thousands of keys. The routes named in one
run are alternated, part by part, in one process.

usage: python tools/time_self_critical.py [--baselines greedy,mean] [--routes host,host_smooth,device,host_cider,device_cider]
                                          [--reps R] [--warmup W]
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
from capnet import metrics, train  # noqa: E402
from capnet.model_att import DecoderFactoredLSTMAtt  # noqa: E402
from capnet.optim import Adam  # noqa: E402

A, E, H, F, V, CF = 512, 300, 512, 1024, 8192, 2048
IMAGES, SAMPLES, STEPS, START, END = 12, 5, 20, 1, 2
OUT = os.path.join(ROOT, "profiles", "time_self_critical.jsonl")


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


_corpora = {}


def _corpus(refs_near):
    """The CIDEr-D corpus of the *_cider routes: the images' references and 400 random reference sets over the same words."""
    if "c" not in _corpora:
        g = torch.Generator().manual_seed(2)
        more = [[[START] + torch.randint(4, 20, (12,), generator=g).tolist() + [END] for _ in range(3)] for _ in range(400)]
        _corpora["c"] = metrics.CiderCorpus(list(refs_near) + more)
    return _corpora["c"]


def _route(route, baseline, dev, refs_host, refs_near):
    """(parts, after) of one route: parts name -> fn, timed in order; after(t, outs) times what needs the parts' results (the
    reward and the policy step) and returns the packed rows."""
    torch.manual_seed(3)
    dec = DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=CF, dropout=0.0, max_seq_length=STEPS).to(dev).train()
    feats = torch.rand(IMAGES, 7, 7, CF, device=dev)
    opt = Adam(dec.parameters(), lr=1e-4)
    kw = dict(samples=SAMPLES, seed=7)
    greedy = baseline == "greedy"
    if route == "host":
        bleu = train.bleu_reward(refs_host)

        def reward(i, tokens):
            # BLEU's host cost, plus a hash of the tokens: an untrained decoder's BLEU is 0 for every caption, and rows of
            # advantage 0 would take the gradient kernel's short path
            return bleu(i, tokens) + (sum(tokens) % 97) / 97.0
    else:
        # host_smooth / device: the same add-one BLEU on both, and a decoder that prefers the references' sixteen words, so
        # that the rewards differ between captions without a hash (which the device route has no place for)
        with torch.no_grad():
            dec.C.bias[4:20] += 9.0
        if route.endswith("_cider"):
            scorer = train.DeviceCiderReward(refs_near, _corpus(refs_near), device=dev)
        else:
            scorer = train.DeviceBleuReward(refs_near, smooth=1, device=dev)
        reward = scorer if route.startswith("device") else (lambda i, tokens: scorer(i, tokens))
    step = lambda: train.self_critical_step(dec, opt, feats, reward, START, END, 5.0, baseline=baseline, **kw)   # noqa: E731
    if route.startswith("device"):
        parts = {"sample": lambda: dec.sample_random(feats, START, END, greedy=greedy, device=True, **kw), "step": step}

        def after(t, outs):
            drawn, ids, _ = outs["sample"]
            m = SAMPLES + greedy

            def score():
                r = scorer.rows(ids, START, END, m)[0].double().view(-1, m)
                if greedy:
                    return (r[:, :SAMPLES] - r[:, SAMPLES:]).reshape(-1).float()
                return (r - (r.sum(1, keepdim=True) - r) / (SAMPLES - 1)).reshape(-1).float()
            t["reward"], adv = _timed(score)
            drawn = [row[:SAMPLES] for row in drawn]
            t["policy"], _ = _timed(lambda: train.policy_step(dec, opt, feats, drawn, adv, 5.0))
            return sum(len(q) - 1 for row in drawn for q, _ in row)
        return parts, after
    parts = {"sample": lambda: dec.sample_random(feats, START, END, **kw),
             "baseline": lambda: dec.sample_batch(feats, START, END, k=1), "step": step}
    if not greedy:
        del parts["baseline"]

    def after(t, outs):
        drawn = outs["sample"]
        t0 = time.perf_counter()
        rewards = [[reward(i, q) for q, _ in row] for i, row in enumerate(drawn)]
        if greedy:
            base = [[reward(i, [int(w) for w in q])] * SAMPLES for i, q in enumerate(outs["baseline"])]
        else:
            base = train.mean_baseline(rewards)
        t["reward"] = (time.perf_counter() - t0) * 1e3
        adv = [r - b for rr, bb in zip(rewards, base) for r, b in zip(rr, bb)]
        t["policy"], _ = _timed(lambda: train.policy_step(dec, opt, feats, drawn, adv, 5.0))
        return sum(len(q) - 1 for row in drawn for q, _ in row)
    return parts, after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baselines", default="greedy,mean")
    ap.add_argument("--routes", default="host", help="host (bleu_reward + a hash, as DESIGN 4ah), host_smooth, device, host_cider, "
                    "device_cider; the routes of one run are alternated, part by part, in one process")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    refs_host = [[torch.randint(4, V, (12,), generator=g).tolist() for _ in range(3)] for _ in range(IMAGES)]
    refs_near = [[[START] + torch.randint(4, 20, (12,), generator=g).tolist() + [END] for _ in range(3)] for _ in range(IMAGES)]
    routes = a.routes.split(",")
    for baseline in a.baselines.split(","):
        built = {r: _route(r, baseline, dev, refs_host, refs_near) for r in routes}
        ms = {r: {} for r in routes}
        words = {}
        for it in range(a.warmup + a.reps):
            for r in routes:
                parts, after = built[r]
                t, outs = {}, {}
                for name, fn in parts.items():
                    t[name], outs[name] = _timed(fn)
                words[r] = after(t, outs)
                if it >= a.warmup:
                    for k, v in t.items():
                        ms[r].setdefault(k, []).append(v)
        for r in routes:
            rec = {"tool": "time_self_critical", "decoder": "DecoderFactoredLSTMAtt", "A": A, "E": E, "H": H, "F": F, "V": V, "C": CF,
                   "P": 49, "images": IMAGES, "samples": SAMPLES, "steps": STEPS, "baseline": baseline, "route": r,
                   "alternated_with": [x for x in routes if x != r], "packed_rows": words[r], "reps": a.reps,
                   "ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                          for k, v in ms[r].items()}}
            line = json.dumps(rec)
            print(line, flush=True)
            with open(OUT, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
