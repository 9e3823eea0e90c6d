"""The one-layer reference decoders on which tests/test_beam_decode_gpu.py compares one_call=True (the chain folded into
the fused decode step, the whole search in one C call) with the default host path (the composed chain), and the fp64
restatement of each from oracle.decoders_ref's cells. TEST INFRASTRUCTURE.

The fold changes the arithmetic, so a case is compared only where the restatement's beam_margin exceeds
device_beam_cases.MARGIN; the seeds below are chosen so that every (k, image) has it, which
tests/test_beam_decode_cpu.py asserts -- no case is skipped on the GPU. <end> is chosen as device_beam_cases.Family
chooses it: the fifth token of the greedy decode."""
import torch

import nic_stacked_ref
import stacked_decode_ref
from device_beam_cases import IMAGES, Family, _load

E, H, F, V = 12, 64, 32, 37
MODE = "happy"


def _factored():
    from capnet.model import DecoderFactoredLSTM
    p = stacked_decode_ref.decode_params(DecoderFactoredLSTM(E, H, F, V, 1), seed=32)
    return Family("DecoderFactoredLSTM", lambda: _load(DecoderFactoredLSTM(E, H, F, V, 1), p), p, V, {"mode": MODE},
                  lambda: torch.zeros(IMAGES, E),
                  lambda k, i: (stacked_decode_ref._step_fn(p, MODE, 1), stacked_decode_ref._zeros(p, k, 1)))


def _rnn():
    from capnet.nic_model import DecoderRNN
    p = nic_stacked_ref.decode_params(DecoderRNN(E, H, V, 1), seed=42)
    return Family("DecoderRNN", lambda: _load(DecoderRNN(E, H, V, 1), p), p, V, {},
                  lambda: torch.zeros(IMAGES, E), lambda k, i: nic_stacked_ref._initial(p, 1, k))


_families = None


def families():
    global _families
    if _families is None:
        _families = [_factored(), _rnn()]
    return _families
