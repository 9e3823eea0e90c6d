"""capnet.stacked.StackedFactoredLSTM decoding without a GPU: the fp64 restatement (tests/stacked_decode_ref.py) reduces
to the reference's beam search with one layer, the fold identity the fused kernel computes with, the decoding methods,
and the C entry point's argument checks."""
import ctypes as C
import os

import pytest
import torch

import capnet
from capnet import _lib
from capnet.stacked import MODES, StackedFactoredLSTM
from oracle import beam_ref
from stacked_decode_ref import decode_params, folded_step, greedy_path, sample_stacked, stacked_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", MODES)
def test_restatement_with_one_layer_is_the_reference_beam_search(mode):
    E, H, F, V = 6, 10, 7, 23
    p = decode_params(StackedFactoredLSTM(E, H, F, V, 1), seed=11)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)                      # sample_factored's zero state takes the default dtype
    try:
        end = greedy_path(p, 1, 1, 5, mode)[4]
        for k in (1, 3, 5):
            want = beam_ref.sample_factored(p, H, 1, end, k=k, mode=mode, max_seq_length=20)
            got = sample_stacked(p, 1, 1, end, k=k, mode=mode, max_seq_length=20)
            assert got.tolist() == want.tolist(), k
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES)
def test_folded_step_is_the_chain_step(layers, mode):
    E, H, F, rows = 13, 16, 24, 9
    p = decode_params(StackedFactoredLSTM(E, H, F, 31, layers), seed=20 + layers)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(rows, E, generator=g, dtype=torch.float64) * 2 - 1
    hs = [torch.rand(rows, H, generator=g, dtype=torch.float64) - 0.5 for _ in range(layers)]
    cs = [torch.rand(rows, H, generator=g, dtype=torch.float64) - 0.5 for _ in range(layers)]
    top_a, ha, ca = stacked_step(p, x, hs, cs, mode, layers)
    top_b, hb, cb = folded_step(p, x, hs, cs, mode, layers)
    assert torch.equal(top_a, ha[-1]) and torch.equal(top_b, hb[-1])
    for l in range(layers):
        assert (ha[l] - hb[l]).abs().max().item() <= 1e-12 * max(ha[l].abs().max().item(), 1.0), l
        assert (ca[l] - cb[l]).abs().max().item() <= 1e-12 * max(ca[l].abs().max().item(), 1.0), l


def test_stacked_decoder_decodes():
    for name in ("sample", "sample_batch", "forward_step"):
        assert hasattr(StackedFactoredLSTM, name), name


def test_decoding_checks_the_mode_before_any_launch():
    dec = StackedFactoredLSTM(6, 64, 8, 11, 2)                  # on the CPU: a launch would raise CapnetError
    with pytest.raises(ValueError):
        dec.sample(torch.zeros(1, 6), 1, 2, mode="cheerful")
    with pytest.raises(ValueError):
        dec.sample_batch(torch.zeros(2, 6), 1, 2, mode="cheerful")
    with pytest.raises(ValueError):
        dec.forward_step(torch.zeros(3, 6), torch.zeros(3, 4, 64), "cheerful")


def test_entry_point_is_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "capnet.h")).read()
    assert "capnet_stacked_decode_step(" in src
    assert "capnet_stacked_decode_step" in _lib.SIGNATURES
    assert hasattr(capnet.lib(), "capnet_stacked_decode_step")
    assert capnet.lib().capnet_abi_version() == 1


def _call(nlayers=2, rows=5, E=300, H=512, V=37, tokens=8, x=16, w=(32, 48), b=(64, 80), sin=96, sout=112, top=128,
          err=144):
    """Argument checks only: every pointer is a fake, 16-B aligned address, never dereferenced on the host."""
    lib = capnet.lib()
    arr = (C.c_void_p * 2)
    return lib.capnet_stacked_decode_step(nlayers, rows, E, H, V, tokens, x, arr(*w), arr(*b), sin, sout, top, err,
                                          None), lib.capnet_last_error().decode()


def test_entry_point_checks_arguments_without_a_gpu():
    rc, msg = _call(x=None)
    assert rc < 0 and "null" in msg
    rc, msg = _call(sout=None)
    assert rc < 0 and "null" in msg
    rc, msg = _call(w=(32, None))
    assert rc < 0 and "layer 1" in msg
    rc, msg = _call(err=None)
    assert rc < 0 and "err_flag" in msg
    rc, msg = _call(rows=0)
    assert rc < 0 and "rows 0" in msg
    rc, msg = _call(H=500)
    assert rc < 0 and "unsupported" in msg and "H=500" in msg
    rc, msg = _call(E=2000)                                     # round16(E) + H > 2048
    assert rc < 0 and "unsupported" in msg
    rc, msg = _call(nlayers=0)
    assert rc < 0 and "layers" in msg
    rc, msg = _call(sout=96)
    assert rc < 0 and "differ" in msg
    rc, msg = _call(sin=100)
    assert rc < 0 and "alignment" in msg
