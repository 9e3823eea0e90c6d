"""The randomly parametrised attention decoders on which tests/test_att_beam_decode_gpu.py compares one_call=True (the
whole search in capnet_att_beam_decode: the k beams of an image on one read of its maps, the cell folded or packed for
the fused decode step) with the default host path (the composed step on per-row maps), and the fp64 restatement of each.
TEST INFRASTRUCTURE.

The fold, the beam-aware attention kernels and the wide decode step change the arithmetic, so a case is compared only
where the restatement's beam_margin exceeds device_beam_cases.MARGIN; the seeds below are chosen so that every (k, image)
has it, which tests/test_att_beam_decode_cpu.py asserts -- no case is skipped on the GPU. Two families have K = round16(E
+ C) + H above 2048 (C = 2048): layer 0 then runs on the wide kernel of the decode-step family."""
import torch

import nic_stacked_ref
import stacked_decode_ref
from device_beam_cases import IMAGES, KS, MARGIN, MAX_LEN, START, Family, _factored_att_initial, _load   # noqa: F401
from device_beam_cases import families as device_families


def _randn_features(P, Cf):
    return torch.randn(IMAGES, P, Cf, generator=torch.Generator().manual_seed(7), dtype=torch.float64).abs() * 0.5


def _rand_features(P, Cf):
    return torch.rand(IMAGES, P, Cf, generator=torch.Generator().manual_seed(122), dtype=torch.float64)


def _factored_att(name, cls, L, mode, seed, A, E, H, F, V, Cf, P):
    make = lambda: cls(A, E, H, F, V, L, feature_size=Cf, dropout=0.0)   # noqa: E731
    p = stacked_decode_ref.decode_params(make(), seed=seed)
    f = _randn_features(P, Cf)
    return Family(name, lambda: _load(make(), p), p, V, {"mode": mode}, lambda: f.float(),
                  lambda k, i: _factored_att_initial(p, L, k, f[i:i + 1], mode))


def _rnn_att(name, cls, L, seed, A, E, H, V, Cf, P):
    make = lambda: cls(A, E, H, V, L, feature_size=Cf)   # noqa: E731
    p = nic_stacked_ref.decode_params(make(), seed=seed)
    f = _rand_features(P, Cf)
    return Family(name, lambda: _load(make(), p), p, V, {}, lambda: f.float(),
                  lambda k, i: nic_stacked_ref._initial(p, L, k, f[i:i + 1]))


def _new_families():
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.nic_model_att import DecoderRNNAtt
    from capnet.nic_stacked import StackedDecoderRNNAtt
    from capnet.stacked_att import StackedFactoredLSTMAtt
    return [
        _factored_att("DecoderFactoredLSTMAtt", DecoderFactoredLSTMAtt, 1, "happy", 1, A=32, E=24, H=64, F=32, V=97, Cf=512, P=9),
        _rnn_att("StackedDecoderRNNAtt-2", StackedDecoderRNNAtt, 2, 1, A=16, E=12, H=64, V=37, Cf=512, P=6),
        _factored_att("StackedFactoredLSTMAtt-2-wide", StackedFactoredLSTMAtt, 2, "sad", 5, A=20, E=12, H=64, F=32, V=97, Cf=2048,
                      P=5),
        _rnn_att("DecoderRNNAtt-wide", DecoderRNNAtt, 1, 2, A=20, E=12, H=64, V=37, Cf=2048, P=5),
    ]


WIDE = ("StackedFactoredLSTMAtt-2-wide", "DecoderRNNAtt-wide")
_new = None


def new_families():
    """The four families this file adds."""
    global _new
    if _new is None:
        _new = _new_families()
    return _new


def families():
    """new_families() and the two attention families of device_beam_cases."""
    return new_families() + [f for f in device_families() if f.name in ("DecoderRNNAtt", "StackedFactoredLSTMAtt-2")]
