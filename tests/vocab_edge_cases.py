"""Inputs of the vocabulary kernels' edge tests (vocab_argmax, vocab_sample; vocab_topk uses its own lifted inputs): the
sizes at which the code the three kernels share takes a path the other kernel tests do not reach. TEST INFRASTRUCTURE.

  wide     V = 8225 = 258 workgroups of 32 entries. A lane of the last arriver takes four workgroups per pass of its loop,
           so workgroups 256 and 257 are the loop's SECOND pass. Some rows' winners are lifted into those two workgroups
           (entries 8200 and 8224), the others stay where the random logits put them.
  one-wg   V = 32: one workgroup, the last arriver is the only arriver.
  h1024    H = 1024: the one-row-tile instantiation (16 rows per pass), rows 17 and 33, one group and two.

The rules are those of the kernels' own tests: an argmax row is compared where its fp64 gap exceeds 2 TOL_STEP max|logit|
(tests/test_seq2seq_gpu.py), a drawn row where its key gap exceeds sample_random_ref.need, and all but at most one row of
a launch must be such rows. tests/test_vocab_edges_cpu.py asserts that in fp64 for every case below."""
import torch

import sample_random_ref as R

TOL_STEP = 3e-5
TEMPS = (0.5, 1.0, 2.0)
WIDE_V, WIDE_COLS = 8225, (8224, 8200)      # workgroups 257 and 256

# (name, H, V, rows per group, groups)
ARGMAX = [("wide", 64, WIDE_V, 1, 1), ("wide", 64, WIDE_V, 17, 1), ("one-wg", 64, 32, 1, 1), ("one-wg", 64, 32, 17, 1),
          ("h1024", 1024, 37, 17, 1), ("h1024", 1024, 37, 33, 1), ("h1024", 1024, 37, 17, 2), ("h1024", 1024, 37, 33, 2)]
# (name, H, V, rows)
SAMPLE = [("wide", 64, WIDE_V, 1), ("wide", 64, WIDE_V, 17), ("one-wg", 64, 32, 1), ("one-wg", 64, 32, 17)]


def case_id(c):
    return "-".join(str(x) for x in c)


def argmax_inputs(name, H, V, rows, groups):
    """-> (h [groups rows, H], [W_g [V, H]], [b_g [V]], [fp64 logits of block g]). wide: row r's winner is entry 8224
    (r % 3 == 0), entry 8200 (r % 3 == 1) or wherever the random logits put it (r % 3 == 2)."""
    g = torch.Generator().manual_seed(1000 * H + V + 7 * rows + groups)
    h = torch.rand(groups * rows, H, generator=g) * 2 - 1
    Ws = [torch.randn(V, H, generator=g) / H ** 0.5 for _ in range(groups)]
    bs = [torch.randn(V, generator=g) * 0.1 for _ in range(groups)]
    if name == "wide":
        h[:, 0] = torch.tensor([(1.0, -1.0, 0.0)[r % 3] for r in range(groups * rows)])
        for W in Ws:
            W[:, 0] = 0.0
            W[WIDE_COLS[0], 0], W[WIDE_COLS[1], 0] = 8.0, -8.0
    logits = [h[i * rows:(i + 1) * rows].double() @ Ws[i].double().t() + bs[i].double() for i in range(groups)]
    return h, Ws, bs, logits


def argmax_clear(logits):
    """The rows whose argmax fp32 must agree on (the rule of test_vocab_argmax_matches_composed_and_fp64)."""
    top2 = logits.topk(2, 1)[0]
    return (top2[:, 0] - top2[:, 1]) > 2 * TOL_STEP * logits.abs().max()


def sample_inputs(name, H, V, rows):
    """-> (h [rows, H], W [V, H], b [V], fp64 logits). wide: the 33 entries of workgroups 256 and 257 are lifted by 4, about
    a fifth of a row's probability at T = 1, so both passes of the merge hold winners and the sum needs both."""
    g = torch.Generator().manual_seed(3 * V + H + rows)
    W = torch.randn(V, H, generator=g) * (2.0 / H ** 0.5)
    b = torch.randn(V, generator=g) * 0.1
    h = torch.rand(rows, H, generator=g) * 2 - 1
    if name == "wide":
        b[8192:] += 4.0
    return h, W, b, (h.double() @ W.double().t() + b.double()).numpy()


def sample_launches(name, H, V, rows):
    """The launches of one case: (temperature, inv_T, seed, step) -- every temperature at three steps."""
    out = []
    for T in TEMPS:
        for step in (1, 2, 3):
            out.append((T, R.inv_temperature(T), V + rows, 10 * step + int(2 * T)))
    return out


def sample_clear(d, inv_T):
    return d["key_gaps"] > R.need(d["scale"], inv_T)
