"""Inputs shared by tests/test_policy_cpu.py and tests/test_policy_gpu.py. TEST INFRASTRUCTURE.

KERNEL: the loss kernels' shapes, name -> (lengths, V). N = sum(lengths) rows: 1 (one row, one word), 7 (a caption of one
word), 40 and 300 (more rows than the final sum's 256 threads; 24 steps); V: 1, 203 (less than one 256-thread stride), 257
(one past it), 1000, 8192. advantages(): both signs, exact zeros, and a positive sum well away from 0 so that the signed loss
is not a difference of nearly equal numbers (the loss is compared relatively).

DECODERS: the eight image decoders at the sizes of the existing decoder tests, (B, V, A, E, F, H, P), with what T3 needs of
each: the class, its fp64 forward with every step teacher forced, whether the image is an input, a mode other than factual
where the class has modes.
"""
import torch

import nic_stacked_ref
import stacked_att_ref
from oracle import decoders_ref as D

KERNEL = {
    "n1_v1": ([1], 1),
    "n7_v203": ([4, 2, 1], 203),
    "n7_v257": ([4, 2, 1], 257),
    "n40_v1000": ([9, 8, 7, 6, 5, 3, 1, 1], 1000),
    "n300_v8192": (list(range(24, 0, -1)), 8192),
}
IDENTITY = ("n1_v1", "n7_v203", "n40_v1000", "n300_v8192")       # T1's shapes; T2 runs all of KERNEL

_PATTERN = (1.5, 0.0, -0.25, 0.75, 2.0, 0.0, -0.5, 1.0)


def advantages(B):
    """[B] floats: _PATTERN repeated -- a zero at captions 1, 5, ..., negatives at 2, 6, ...; a single caption gets -0.75."""
    return [-0.75] if B == 1 else [_PATTERN[b % len(_PATTERN)] for b in range(B)]


def kernel_inputs(name):
    """(logits [N, V] fp32, targets [N], lengths) of a KERNEL case, seeded by its shape."""
    lengths, V = KERNEL[name]
    N = sum(lengths)
    g = torch.Generator().manual_seed(1000 * N + V)
    return torch.randn(N, V, generator=g) * 3.0, torch.randint(0, V, (N,), generator=g), lengths


SIZES = {                       # (B, V, A, E, F, H, P)
    "b5": (5, 203, 24, 20, 24, 28, 9),
    "b1": (1, 203, 24, 20, 24, 28, 9),
    "b20": (20, 203, 72, 68, 64, 64, 9),
    "b12_full": (12, 1000, 512, 300, 512, 512, 196),
}


def _classes():
    from capnet.model import DecoderFactoredLSTM
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model import DecoderRNN
    from capnet.nic_model_att import DecoderRNNAtt
    from capnet.nic_stacked import StackedDecoderRNN, StackedDecoderRNNAtt
    from capnet.stacked import StackedFactoredLSTM
    from capnet.stacked_att import StackedFactoredLSTMAtt
    return {
        # name: (make(V, A, E, F, H, Cf), forward(p, inputs, lengths, features, tf_mask) -> logits, attention, mode)
        "DecoderFactoredLSTM": (
            lambda V, A, E, F, H, Cf: DecoderFactoredLSTM(E, H, F, V, 1, dropout=0.0),
            lambda p, c, l, f, tf: D.factored_lstm_forward(p, c, l, None, tf, mode="happy"), False, "happy"),
        "StackedFactoredLSTM": (
            lambda V, A, E, F, H, Cf: StackedFactoredLSTM(E, H, F, V, 2, dropout=0.0),
            lambda p, c, l, f, tf: D.stacked_factored_lstm_forward(p, c, l, None, tf, mode="sad", num_layers=2), False, "sad"),
        "DecoderRNN": (
            lambda V, A, E, F, H, Cf: DecoderRNN(E, H, V, 1, dropout=0.0),
            lambda p, c, l, f, tf: D.lstm_forward(p, c, l, None, tf), False, None),
        "StackedDecoderRNN": (
            lambda V, A, E, F, H, Cf: StackedDecoderRNN(E, H, V, 2, dropout=0.0),
            lambda p, c, l, f, tf: nic_stacked_ref.stacked_lstm_forward(p, c, l, None, tf, 2), False, None),
        "DecoderFactoredLSTMAtt": (
            lambda V, A, E, F, H, Cf: DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=Cf, dropout=0.0),
            lambda p, c, l, f, tf: D.factored_att_forward(p, c, l, f, tf, mode="angry")[0], True, "angry"),
        "StackedFactoredLSTMAtt": (
            lambda V, A, E, F, H, Cf: StackedFactoredLSTMAtt(A, E, H, F, V, 2, feature_size=Cf, dropout=0.0),
            lambda p, c, l, f, tf: stacked_att_ref.stacked_factored_att_forward(p, c, l, f, tf, mode="happy", num_layers=2)[0],
            True, "happy"),
        "DecoderRNNAtt": (
            lambda V, A, E, F, H, Cf: DecoderRNNAtt(A, E, H, V, 1, feature_size=Cf, dropout=0.0),
            lambda p, c, l, f, tf: D.lstm_att_forward(p, c, l, f, tf)[0], True, None),
        "StackedDecoderRNNAtt": (
            lambda V, A, E, F, H, Cf: StackedDecoderRNNAtt(A, E, H, V, 2, feature_size=Cf, dropout=0.0),
            lambda p, c, l, f, tf: nic_stacked_ref.stacked_lstm_att_forward(p, c, l, f, tf, 2)[0], True, None),
    }


DECODERS = ("DecoderFactoredLSTM", "StackedFactoredLSTM", "DecoderRNN", "StackedDecoderRNN", "DecoderFactoredLSTMAtt",
            "StackedFactoredLSTMAtt", "DecoderRNNAtt", "StackedDecoderRNNAtt")
STEP_CASES = [(d, s) for d in DECODERS for s in ("b5", "b1", "b20")] + [("DecoderFactoredLSTMAtt", "b12_full")]


def decoder_case(name, size):
    """(decoder on the CPU with its parameters loaded, fp64 parameters, forward, attention, mode, token lists in a shuffled
    caller's order, features [B, P, Cf] aligned with them (None for a plain decoder), advantages in the caller's order)."""
    from capnet import synthetic
    make, forward, att, mode = _classes()[name]
    B, V, A, E, F, H, P = SIZES[size]
    Cf = 512 if P < 100 else 2048
    dec = make(V, A, E, F, H, Cf)
    p = synthetic.decoder_state(dec.state_dict(), seed=B, bias_range=0.05)
    dec.load_state_dict(p)
    _, captions, lengths = synthetic.make_batch(B, V, seed=40 + B, images=False, min_len=4, max_len=11)
    g = torch.Generator().manual_seed(B)
    feats = torch.randn(B, P, Cf, generator=g).abs() * 0.5 if att else None       # post-ReLU-like maps
    shuffle = torch.randperm(B, generator=g).tolist()                            # the caller's order is not the sorted one
    tokens = [captions[r, :lengths[r]].tolist() for r in shuffle]
    return dec, {k: v.double() for k, v in p.items()}, forward, att, mode, tokens, feats, advantages(B)
