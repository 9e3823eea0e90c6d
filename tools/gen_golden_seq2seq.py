"""Generates tests/golden/seq2seq_tiny.npz and tests/golden/seq2seq_state_dict_keys.json by running the REFERENCE's own
seq2seq/model.py classes (EncoderRNN, DecoderRNN, Seq2Seq) on the CPU.

Runs only where the reference tree is present: it imports seq2seq/model.py verbatim, with an empty stub for the absent
torchvision package (touched only inside EncoderCNN.__init__, which is never constructed here). Nothing of the reference is
copied: only inputs, parameters and outputs are stored.

Per num_layers in (1, 3), E = 12, H = 16, V = 37, B = 4, dropout = 0:
  L{n}.param.<state_dict key>                 torch's constructor defaults under torch.manual_seed(n)
  L{n}.case.<mode>_tf{10,00,05}.*             Seq2Seq.forward + CrossEntropyLoss + backward in train():
      seed, ratio, draws (the random.random() values the forward consumed: the encoder's steps, then the decoder's),
      logits (packed), loss, grad.<key> of EVERY parameter that got a gradient
  L{n}.states_tf{10,00,05}.{h,c}              EncoderRNN.forward's returned states under the factual case's draws
  L{n}.sample.factual.{ids,h,c}               Seq2Seq.sample / EncoderRNN.sample on all B rows
  L{n}.sample.happy.ids                       Seq2Seq.sample(mode='happy') on row 0 alone (the reference's
                                              DecoderRNN.sample only works for one row)
Shared inputs: features, src, src_lengths (factual targets = pack(src)), dst_in, dst_tgt, dst_lengths, start_token.
"""
import importlib.util
import json
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CAPNET_REFERENCE", "")   # the reference checkout
OUT = os.path.join(ROOT, "tests", "golden")

E, H, V, B, T = 12, 16, 37, 4, 6
SRC_LENGTHS = [6, 5, 3, 2]          # b_last = 1 < B
DST_LENGTHS = [6, 4, 4, 2]
START = 1
CASES = (("tf10", 100, 1.0), ("tf00", 101, 0.0), ("tf05", 7, 0.5))


def load_ref():
    for stub in ("torchvision", "torchvision.models"):
        if stub not in sys.modules:
            sys.modules[stub] = types.ModuleType(stub)
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    spec = importlib.util.spec_from_file_location("ref_seq2seq_model", os.path.join(REF, "seq2seq", "model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def draws(seed, n):
    random.seed(seed)
    return np.array([random.random() for _ in range(n)], dtype=np.float64)


def main():
    if not os.path.isfile(os.path.join(REF, "seq2seq", "model.py")):
        sys.exit("usage: gen_golden_seq2seq.py <reference checkout>   (or CAPNET_REFERENCE=<reference checkout>)")
    ref = load_ref()
    g = torch.Generator().manual_seed(0)
    features = torch.randn(B, E, generator=g) * 0.5
    src = torch.randint(3, V, (B, T), generator=g)
    dst = torch.randint(3, V, (B, T + 1), generator=g)
    dst[:, 0] = START
    dst_in, dst_tgt = dst[:, :-1].contiguous(), dst[:, 1:].contiguous()
    arrays = {"dims": np.array([E, H, V, B, T]), "features": features.numpy(), "src": src.numpy(),
              "src_lengths": np.array(SRC_LENGTHS), "dst_in": dst_in.numpy(), "dst_tgt": dst_tgt.numpy(),
              "dst_lengths": np.array(DST_LENGTHS), "start_token": np.array(START)}
    keys = {}
    crit = nn.CrossEntropyLoss()
    for L in (1, 3):
        torch.manual_seed(L)
        model = ref.Seq2Seq(E, H, V, L, dropout=0.0)
        keys[str(L)] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        pre = "L%d." % L
        for k, v in model.state_dict().items():
            arrays[pre + "param." + k] = v.numpy().copy()
        model.train()
        for mode in ("factual", "happy"):
            for tag, seed, ratio in CASES:
                model.zero_grad()
                random.seed(seed)
                if mode == "factual":
                    out = model(features, (src, SRC_LENGTHS), teacher_forcing_ratio=ratio)
                    targets = pack_padded_sequence(src, SRC_LENGTHS, batch_first=True)[0]
                    n_draws = SRC_LENGTHS[0]
                else:
                    out = model(features, (src, SRC_LENGTHS), (dst_in, DST_LENGTHS), teacher_forcing_ratio=ratio, mode=mode)
                    targets = pack_padded_sequence(dst_tgt, DST_LENGTHS, batch_first=True)[0]
                    n_draws = SRC_LENGTHS[0] + DST_LENGTHS[0]
                loss = crit(out, targets)
                loss.backward()
                c = "%scase.%s_%s." % (pre, mode, tag)
                arrays[c + "seed"] = np.array(seed)
                arrays[c + "ratio"] = np.array(ratio)
                arrays[c + "draws"] = draws(seed, n_draws)
                arrays[c + "logits"] = out.detach().numpy().copy()
                arrays[c + "loss"] = loss.detach().numpy().copy()
                for k, p in model.named_parameters():
                    if p.grad is not None:
                        arrays[c + "grad." + k] = p.grad.detach().numpy().copy()
                if mode == "factual":
                    random.seed(seed)
                    with torch.no_grad():
                        _, (h, cc) = model.encoder(features, src, SRC_LENGTHS, ratio)
                    arrays["%sstates_%s.h" % (pre, tag)] = h.numpy().copy()
                    arrays["%sstates_%s.c" % (pre, tag)] = cc.numpy().copy()
        model.eval()
        with torch.no_grad():
            ids, (h, cc) = model.encoder.sample(features)
            assert torch.equal(ids, model.sample(features, START))
            arrays[pre + "sample.factual.ids"] = ids.numpy().copy()
            arrays[pre + "sample.factual.h"] = h.numpy().copy()
            arrays[pre + "sample.factual.c"] = cc.numpy().copy()
            arrays[pre + "sample.happy.ids"] = model.sample(features[:1], START, mode="happy").numpy().copy()
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "seq2seq_tiny.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
    path = os.path.join(OUT, "seq2seq_state_dict_keys.json")
    with open(path, "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")
    print("wrote %s" % path)


if __name__ == "__main__":
    main()
