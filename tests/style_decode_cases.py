"""The randomly parametrised factored decoders on which tests/test_style_decode_gpu.py compares sample_styles (every
mode in one grouped search) with sample_batch(mode=m, one_call=True) mode by mode, and the fp64 restatement of each
(mode, k, image). TEST INFRASTRUCTURE.

The grouped search makes its vocabulary projection over modes x images x k rows, the single-mode search over images x k,
and the product picks its kernel by size: logits may differ in the last bit. A case is therefore compared only where the
restatement's beam_margin exceeds device_beam_cases.MARGIN; the seeds below are chosen so that every (mode, k, image) has
it, which tests/test_style_decode_cpu.py asserts -- no case is skipped on the GPU. <end> is the fifth token of the
FACTUAL greedy decode of image 0, for every mode of a family: the modes of one call share their end token.

The stacked classes carry the seeded parameters; the one-layer reference classes load the one-layer stacked parameters,
whose key sets equal theirs (asserted here)."""
import torch

import stacked_decode_ref
from device_beam_cases import IMAGES, KS, MARGIN, MAX_LEN, START, _factored_att_initial, _load   # noqa: F401
from device_beam_ref import beam_margin

MODES = ("factual", "happy", "sad", "angry")
PLAIN = dict(E=12, H=64, F=32, V=37)
ATT = dict(A=32, E=24, H=64, F=32, V=97, Cf=512, P=9)


class StyleFamily:
    """name; make() -> the decoder (CPU, parameters loaded, max_seq_length MAX_LEN); V; features(): [IMAGES, ...] float32;
    initial(mode, k, image) -> the restatement's (step_fn, state); distinct: the least number of different captions
    among the four modes at any (k, image)."""

    def __init__(self, name, make, params, V, features, initial, distinct):
        self.name, self.make, self.params, self.V, self.features, self.initial = name, make, params, V, features, initial
        self.distinct = distinct
        self._end, self._ref = None, {}

    @property
    def end(self):
        if self._end is None:
            step_fn, state = self.initial("factual", 1, 0)
            words = torch.LongTensor([[START]])
            for _ in range(5):
                logits, state = step_fn(words, state)
                words = logits.argmax(1, keepdim=True)
            self._end = int(words)
        return self._end

    def margin(self, mode, k, image):
        step_fn, state = self.initial(mode, k, image)
        return beam_margin(step_fn, state, self.V, START, self.end, k, MAX_LEN)

    def reference(self, mode, k, image):
        """The fp64 beam search's token list, computed once per (mode, k, image)."""
        key = (mode, k, image)
        if key not in self._ref:
            from oracle import beam_ref
            step_fn, state = self.initial(mode, k, image)
            self._ref[key] = beam_ref._beam(step_fn, state, self.V, START, self.end, k, MAX_LEN)[0].tolist()
        return self._ref[key]


def _same_keys(cls_module, p, name):
    assert set(cls_module.state_dict().keys()) == set(p.keys()), name + ": the one-layer key sets differ"


def _plain(L, seed, distinct):
    from capnet.model import DecoderFactoredLSTM
    from capnet.stacked import StackedFactoredLSTM
    s = PLAIN
    make = lambda: StackedFactoredLSTM(s["E"], s["H"], s["F"], s["V"], L)   # noqa: E731
    p = stacked_decode_ref.decode_params(make(), seed=seed)
    feats = lambda: torch.zeros(IMAGES, s["E"])    # noqa: E731
    initial = lambda mode, k, i: (stacked_decode_ref._step_fn(p, mode, L), stacked_decode_ref._zeros(p, k, L))   # noqa: E731
    out = [StyleFamily("StackedFactoredLSTM-%d" % L, lambda: _load(make(), p), p, s["V"], feats, initial, distinct)]
    if L == 1:
        single = lambda: DecoderFactoredLSTM(s["E"], s["H"], s["F"], s["V"], 1)   # noqa: E731
        _same_keys(single(), p, "DecoderFactoredLSTM")
        out.append(StyleFamily("DecoderFactoredLSTM", lambda: _load(single(), p), p, s["V"], feats, initial, distinct))
    return out


def _att(L, seed, distinct):
    from capnet.model_att import DecoderFactoredLSTMAtt
    from capnet.stacked_att import StackedFactoredLSTMAtt
    s = ATT
    make = lambda: StackedFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], L, feature_size=s["Cf"], dropout=0.0)   # noqa: E731
    p = stacked_decode_ref.decode_params(make(), seed=seed)
    f = torch.randn(IMAGES, s["P"], s["Cf"], generator=torch.Generator().manual_seed(7), dtype=torch.float64).abs() * 0.5
    feats = lambda: f.float()    # noqa: E731
    initial = lambda mode, k, i: _factored_att_initial(p, L, k, f[i:i + 1], mode)   # noqa: E731
    out = [StyleFamily("StackedFactoredLSTMAtt-%d" % L, lambda: _load(make(), p), p, s["V"], feats, initial, distinct)]
    if L == 1:
        single = lambda: DecoderFactoredLSTMAtt(s["A"], s["E"], s["H"], s["F"], s["V"], 1, feature_size=s["Cf"], dropout=0.0)   # noqa: E731
        _same_keys(single(), p, "DecoderFactoredLSTMAtt")
        out.append(StyleFamily("DecoderFactoredLSTMAtt", lambda: _load(single(), p), p, s["V"], feats, initial, distinct))
    return out


_families = None


def families():
    """StackedFactoredLSTM (1 and 2 layers), DecoderFactoredLSTM, StackedFactoredLSTMAtt (1 and 2 layers),
    DecoderFactoredLSTMAtt. The plain ones give four different captions at every (k, image), the attention ones at
    least three."""
    global _families
    if _families is None:
        _families = _plain(1, 214, 4) + _plain(2, 240, 4) + _att(1, 220, 3) + _att(2, 204, 3)
    return _families


def family(name):
    return next(f for f in families() if f.name == name)


NAMES = ("StackedFactoredLSTM-1", "DecoderFactoredLSTM", "StackedFactoredLSTM-2", "StackedFactoredLSTMAtt-1",
         "DecoderFactoredLSTMAtt", "StackedFactoredLSTMAtt-2")
