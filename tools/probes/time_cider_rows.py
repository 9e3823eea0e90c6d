"""What the binary searches cost inside ops.cider_rows: kernel-only times, hip events around 200 back-to-back
launches, of ops.bleu_rows, ops.cider_rows with tools/time_self_critical.py's corpus (the 12 images' references plus 400
random reference sets) and ops.cider_rows with a table of three keys, where every search ends after one or two steps -- the
difference of the last two is the lookups. 72 and 60 rows of 20 steps, median of 7 rounds, the three alternated. A record: one
JSON line on stdout and appended to profiles/time_cider_rows.jsonl.

usage: python tools/probes/time_cider_rows.py"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import capnet  # noqa
from capnet import metrics, train, ops
START, END, IMAGES, STEPS = 1, 2, 12, 20
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(1)
_ = [[torch.randint(4, 8192, (12,), generator=g).tolist() for _ in range(3)] for _ in range(IMAGES)]    # (the tool's draws, in its order)
refs = [[[START] + torch.randint(4, 20, (12,), generator=g).tolist() + [END] for _ in range(3)] for _ in range(IMAGES)]
g2 = torch.Generator().manual_seed(2)
more = [[[START] + torch.randint(4, 20, (12,), generator=g2).tolist() + [END] for _ in range(3)] for _ in range(400)]
big = metrics.CiderCorpus(refs + more)
tiny = metrics.CiderCorpus([[[START, END]], [[START, 4, END]]])
out = {"tool": "time_cider_rows", "keys": [k.shape[0] for k, _ in big.tables()], "tiny_keys": [k.shape[0] for k, _ in tiny.tables()]}
for m in (6, 5):
    ids = torch.randint(4, 20, (IMAGES * m, STEPS), generator=torch.Generator().manual_seed(3)).to(dev)
    bleu = train.DeviceBleuReward(refs, smooth=1, device=dev)
    cb, ct = train.DeviceCiderReward(refs, big, device=dev), train.DeviceCiderReward(refs, tiny, device=dev)
    fns = {"bleu_rows": lambda: bleu.rows(ids, START, END, m), "cider_rows": lambda: cb.rows(ids, START, END, m),
           "cider_rows_tiny_table": lambda: ct.rows(ids, START, END, m)}
    res = {k: [] for k in fns}
    for rep in range(7):
        for k, fn in fns.items():
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / 200 * 1e3)
    out["rows_%d" % (IMAGES * m)] = {k: {"median_us": round(sorted(v)[3], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in res.items()}
    st = cb.rows(ids, START, END, m)[2].cpu()
    out["known_of_distinct_%d" % (IMAGES * m)] = [int(st[:, 5:].sum()), int(st[:, 1:5].sum())]
ops.check_device_errors()
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "time_cider_rows.jsonl"), "a") as f:
    f.write(json.dumps(out) + "\n")
