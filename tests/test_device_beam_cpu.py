"""Beam search with device-side bookkeeping, the part that needs no GPU: the fixed-slot algorithm (tests/device_beam_ref.py,
the model capnet_beam_advance is held to bit for bit in tests/test_device_beam_gpu.py) returns the reference loop's
sequences; the new entries are declared; the decoder cases of the GPU test have the margin its comparison needs."""
import pytest
import torch
import torch.nn.functional as Fn

from capnet import _lib
from device_beam_cases import KS, IMAGES, MARGIN, families
from device_beam_ref import DeviceBeam, run
from oracle import beam_ref, decoders_ref as D

V, H, E, START, END, MAX_LEN = 11, 4, 4, 1, 2, 6
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
SITUATIONS = {"several completions in one step", "nothing completed", "all beams complete before the last step",
              "the winner is not the first completion"}


def _params(seed):
    """A tiny LSTMCell decoder in oracle.beam_ref.sample_lstm's parameter style; the <end> logit is biased by seed so
    that beams finish early, late or never."""
    g = torch.Generator().manual_seed(seed)

    def u(*shape):
        return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1)
    p = {"embed.weight": u(V, E), "lstm.weight_ih": u(4 * H, E), "lstm.weight_hh": u(4 * H, H), "lstm.bias_ih": u(4 * H) * 0.1,
         "lstm.bias_hh": u(4 * H) * 0.1, "linear.weight": u(V, H) * 8.0, "linear.bias": u(V) * 0.5}
    p["linear.bias"][END] += (-1.0, 0.0, 1.0)[seed % 3]
    return p


def _reference(p, k):
    """oracle.beam_ref.sample_lstm on fp64 parameters (its own zero state is f32)."""
    def step_fn(prev_words, state):
        h, c = D.lstmcell_step(p, p["embed.weight"][prev_words].squeeze(1), state[0], state[1])
        return Fn.linear(h, p["linear.weight"], p["linear.bias"]), (h, c)
    z = torch.zeros(k, H, dtype=torch.float64)
    return beam_ref._beam(step_fn, (z, z.clone()), V, START, END, k, MAX_LEN)[0].tolist()


def _fixed_slot_search(p, k):
    """sample_lstm's search on the fixed-slot model: all k rows take every step, the state follows parent_rows, the
    top-k is float64 torch on the rows the model asks for."""
    beam = DeviceBeam(1, k, V, START, END)
    box = {"state": (torch.zeros(k, H, dtype=torch.float64), torch.zeros(k, H, dtype=torch.float64))}

    def step_topk(step, words, rows):
        h, c = box["state"]
        if step > 1:
            h, c = h[rows], c[rows]
        prev = torch.tensor([START] * k if words is None else words)
        h, c = D.lstmcell_step(p, p["embed.weight"][prev], h, c)
        box["state"] = (h, c)
        logp = Fn.log_softmax(Fn.linear(h, p["linear.weight"], p["linear.bias"]), dim=1)
        prev_scores = torch.tensor(beam.scores[0], dtype=torch.float64)

        def topk(image, nrows, kk):
            flat = (prev_scores[:nrows, None] + logp[:nrows]).reshape(-1)
            s, ix = flat.topk(kk, 0, True, True)
            return s.tolist(), ix.tolist()
        return topk
    out = run(beam, MAX_LEN + 1, step_topk)
    return out[0], beam.events(MAX_LEN + 1)


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("seed", SEEDS)
def test_fixed_slot_model_returns_the_reference_sequences(seed, k):
    p = _params(seed)
    got, _ = _fixed_slot_search(p, k)
    assert got == _reference(p, k)


def test_seed_list_contains_every_situation():
    seen = set()
    for seed in SEEDS:
        for k in (1, 3, 5):
            seen |= _fixed_slot_search(_params(seed), k)[1]
    assert seen == SITUATIONS


def test_a_dead_image_asks_for_no_top_k():
    """Once no beam is live a step changes nothing (what poll_every relies on): dead slots report <end> and their row."""
    beam = DeviceBeam(1, 3, V, START, END)
    assert beam.advance(1, lambda i, r, kk: ([0.0, -1.0, -2.0], [END, END, END]))[0] == [END] * 3 and beam.live_total == 0
    assert beam.advance(2, None) == ([END] * 3, [0, 1, 2])
    assert beam.finish() == [[START, END]]


def test_new_entries_are_declared():
    for name in ("capnet_beam_state_bytes", "capnet_beam_init", "capnet_beam_advance", "capnet_beam_finish", "capnet_beam_live"):
        assert name in _lib.SIGNATURES, name


def test_state_size_and_argument_checks_need_no_gpu():
    import capnet
    lib = capnet.lib()
    assert lib.capnet_beam_state_bytes(4, 5, 21) == 4 * (4 + 2 * 4 + 3 * 20 + 3 * 20 * 23)
    assert lib.capnet_beam_state_bytes(4, 17, 21) == 0 and lib.capnet_beam_state_bytes(4, 0, 21) == 0
    assert lib.capnet_beam_advance(None, None, 16, 16, 1, 3, 6, 1, END, None, None, None) != 0
    assert b"null" in lib.capnet_last_error()


@pytest.mark.parametrize("family", families(), ids=lambda f: f.name)
def test_decoder_cases_have_the_margin(family):
    """Every (k, image) the GPU test compares is well-posed in fp64: none is skipped there."""
    for k in KS:
        for i in range(IMAGES):
            assert family.margin(k, i) > MARGIN, (k, i)
