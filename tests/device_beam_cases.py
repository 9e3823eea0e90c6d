"""The randomly parametrised decoders on which tests/test_device_beam_gpu.py compares on_device=True with the host
bookkeeping, and the fp64 restatement of each (step_fn, initial state of one image). TEST INFRASTRUCTURE.

The fixed-slot search runs its products on n k rows, the host loop on the live rows, and capnet_sgemm picks its kernel
by size: logits may differ in the last bit. A case is therefore compared only where the restatement's beam_margin
exceeds MARGIN (the rule of tests/test_stacked_decode_gpu.py); the seeds below are chosen so that every case has it,
which tests/test_device_beam_cpu.py asserts -- no case is skipped on the GPU."""
import torch
import torch.nn.functional as Fn

import nic_stacked_ref
import stacked_decode_ref
from device_beam_ref import beam_margin
from oracle import decoders_ref as D
from stacked_att_ref import layer_params

MARGIN = 1e-4
MAX_LEN = 12
START = 1
KS = (3, 5)
IMAGES = 3


def _lin(p, name, x):
    return Fn.linear(x, p[name + ".weight"], p[name + ".bias"])


def _factored_att_initial(p, num_layers, k, features, mode):
    """(step_fn, state) of StackedFactoredLSTMAtt.sample on ONE image, as tests/stacked_att_ref.greedy_decode steps."""
    feat = features.reshape(1, -1, features.size(-1))
    feat = feat.expand(k, feat.size(1), feat.size(2))
    mean = feat.mean(dim=1)
    tags = [""] + [str(l) for l in range(1, num_layers)]
    hs = tuple(_lin(p, "init_h" + t, mean) for t in tags)
    cs = tuple(_lin(p, "init_c" + t, mean) for t in tags)
    lp = [p] + [layer_params(p, l) for l in range(1, num_layers)]
    L = num_layers

    def step_fn(prev_words, state):
        hs, cs, f = list(state[:L]), list(state[L:2 * L]), state[2 * L]
        awe, _ = D.attention_step(p, D.MODE_ATT[mode], f, hs[0])
        awe = torch.sigmoid(_lin(p, "f_beta", hs[0])) * awe
        x = torch.cat([p["B.weight"][prev_words].squeeze(1), awe], dim=1)
        for l in range(L):
            hs[l], cs[l] = D.factored_step(lp[l], x, hs[l], cs[l], mode)
            x = hs[l]
        return _lin(p, "C", x), tuple(hs + cs) + (f,)
    return step_fn, hs + cs + (feat,)


class Family:
    """name; make() -> the decoder (CPU, parameters loaded, max_seq_length MAX_LEN); V; kw: sample's extra keywords;
    features(): [IMAGES, ...] float32; initial(k, image) -> the restatement's (step_fn, state); end: the fifth token of
    image 0's greedy decode, so that beams complete."""

    def __init__(self, name, make, params, V, kw, features, initial):
        self.name, self.make, self.params, self.V, self.kw, self.features, self.initial = name, make, params, V, kw, features, initial
        self._end = None

    @property
    def end(self):
        if self._end is None:
            step_fn, state = self.initial(1, 0)
            words = torch.LongTensor([[START]])
            for _ in range(5):
                logits, state = step_fn(words, state)
                words = logits.argmax(1, keepdim=True)
            self._end = int(words)
        return self._end

    def margin(self, k, image):
        step_fn, state = self.initial(k, image)
        return beam_margin(step_fn, state, self.V, START, self.end, k, MAX_LEN)

    def reference(self, k, image):
        from oracle import beam_ref
        step_fn, state = self.initial(k, image)
        return beam_ref._beam(step_fn, state, self.V, START, self.end, k, MAX_LEN)[0].tolist()


def _load(dec, p):
    dec.load_state_dict({k: v.float() for k, v in p.items()})
    dec.max_seq_length = MAX_LEN
    return dec


def _stacked_factored():
    from capnet.stacked import StackedFactoredLSTM
    E, H, F, V, L = 12, 64, 32, 37, 2
    p = stacked_decode_ref.decode_params(StackedFactoredLSTM(E, H, F, V, L), seed=9)
    return Family("StackedFactoredLSTM-2", lambda: _load(StackedFactoredLSTM(E, H, F, V, L), p), p, V, {"mode": "angry"},
                  lambda: torch.zeros(IMAGES, E),
                  lambda k, i: (stacked_decode_ref._step_fn(p, "angry", L), stacked_decode_ref._zeros(p, k, L)))


def _stacked_rnn():
    from capnet.nic_stacked import StackedDecoderRNN
    E, H, V, L = 12, 64, 37, 2
    p = nic_stacked_ref.decode_params(StackedDecoderRNN(E, H, V, L), seed=112)
    return Family("StackedDecoderRNN-2", lambda: _load(StackedDecoderRNN(E, H, V, L), p), p, V, {},
                  lambda: torch.zeros(IMAGES, E), lambda k, i: nic_stacked_ref._initial(p, L, k))


def _rnn_att():
    from capnet.nic_model_att import DecoderRNNAtt
    A, E, H, V, Cf, P = 16, 12, 64, 37, 512, 6
    p = nic_stacked_ref.decode_params(DecoderRNNAtt(A, E, H, V, 1, feature_size=Cf), seed=121)
    f = torch.rand(IMAGES, P, Cf, generator=torch.Generator().manual_seed(122), dtype=torch.float64)
    return Family("DecoderRNNAtt", lambda: _load(DecoderRNNAtt(A, E, H, V, 1, feature_size=Cf), p), p, V, {},
                  lambda: f.float(), lambda k, i: nic_stacked_ref._initial(p, 1, k, f[i:i + 1]))


def _stacked_factored_att():
    from capnet.stacked_att import StackedFactoredLSTMAtt
    s = dict(A=32, E=24, H=64, F=32, V=97, Cf=512, P=9)
    make = lambda: StackedFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], 2, feature_size=s["Cf"], dropout=0.0)   # noqa: E731
    p = stacked_decode_ref.decode_params(make(), seed=28)
    f = torch.randn(IMAGES, s["P"], s["Cf"], generator=torch.Generator().manual_seed(7), dtype=torch.float64).abs() * 0.5
    return Family("StackedFactoredLSTMAtt-2", lambda: _load(make(), p), p, s["V"], {"mode": "factual"},
                  lambda: f.float(), lambda k, i: _factored_att_initial(p, 2, k, f[i:i + 1], "factual"))


_families = None


def families():
    global _families
    if _families is None:
        _families = [_stacked_factored(), _stacked_rnn(), _rnn_att(), _stacked_factored_att()]
    return _families
