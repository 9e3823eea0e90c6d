"""capnet.nic_stacked without a GPU: parameter names and order, the fp64 restatement of the stack against torch's own
nn.LSTM(num_layers), and the argument checks of the new C entry point and of the sequence Functions."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence

import capnet
from capnet import _lib, ops
from capnet.nic_model import DecoderRNN
from capnet.nic_model_att import DecoderRNNAtt
from capnet.nic_stacked import StackedDecoderRNN, StackedDecoderRNNAtt
from nic_stacked_ref import decode_params, stacked_lstm_forward, stacked_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")))


def _kv(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def test_one_layer_has_the_reference_keys():
    assert _kv(StackedDecoderRNN(300, 512, 1000, 1)) == KEYS["nic.DecoderRNN(300,512,1000,1)"]
    assert _kv(StackedDecoderRNNAtt(512, 300, 512, 1000, 1)) == KEYS["nic.DecoderRNNAtt(512,300,512,1000,1)"]
    assert list(StackedDecoderRNN(30, 64, 100, 1).state_dict()) == list(DecoderRNN(30, 64, 100, 1).state_dict())
    assert list(StackedDecoderRNNAtt(16, 30, 64, 100, 1, feature_size=32).state_dict()) == \
        list(DecoderRNNAtt(16, 30, 64, 100, 1, feature_size=32).state_dict())


@pytest.mark.parametrize("layers", [2, 3])
def test_upper_layers_are_named_and_shaped_after_the_reference(layers):
    E, H, V, A, Cf = 30, 64, 100, 16, 48
    plain = _kv(StackedDecoderRNN(E, H, V, layers))
    assert plain[:len(KEYS["nic.DecoderRNN(300,512,1000,1)"])] == _kv(DecoderRNN(E, H, V, 1))
    want = []
    for l in range(1, layers):
        want += [["lstm%d.weight_ih" % l, [4 * H, H]], ["lstm%d.weight_hh" % l, [4 * H, H]],
                 ["lstm%d.bias_ih" % l, [4 * H]], ["lstm%d.bias_hh" % l, [4 * H]]]
    assert plain[len(_kv(DecoderRNN(E, H, V, 1))):] == want
    att = _kv(StackedDecoderRNNAtt(A, E, H, V, layers, feature_size=Cf))
    n0 = len(_kv(DecoderRNNAtt(A, E, H, V, 1, feature_size=Cf)))
    assert att[:n0] == _kv(DecoderRNNAtt(A, E, H, V, 1, feature_size=Cf))
    want = []
    for l in range(1, layers):
        want += [["init_h%d.weight" % l, [H, Cf]], ["init_h%d.bias" % l, [H]], ["init_c%d.weight" % l, [H, Cf]],
                 ["init_c%d.bias" % l, [H]], ["lstm%d.weight_ih" % l, [4 * H, H]], ["lstm%d.weight_hh" % l, [4 * H, H]],
                 ["lstm%d.bias_ih" % l, [4 * H]], ["lstm%d.bias_hh" % l, [4 * H]]]
    assert att[n0:] == want


def test_init_follows_the_reference_decoders():
    dec = StackedDecoderRNN(12, 32, 50, 3)
    assert float(dec.lstm2.bias_ih.abs().max()) == 0.0 and float(dec.linear.bias.abs().max()) == 0.0
    assert float(dec.embed.weight.abs().max()) <= 0.1 and float(dec.linear.weight.abs().max()) <= 0.1
    bound = (6.0 / (4 * 32 + 32)) ** 0.5                      # xavier_uniform on [4H, H]
    assert float(dec.lstm1.weight_hh.abs().max()) <= bound
    att = StackedDecoderRNNAtt(16, 12, 32, 50, 2, feature_size=24)
    assert float(att.init_c1.bias.abs().max()) == 0.0 and float(att.lstm1.bias_hh.abs().max()) == 0.0


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_restatement_is_torch_lstm(layers):
    """Teacher forcing, no dropout: the restated stack's logits equal linear(nn.LSTM(num_layers=L)) on the packed
    sequence of [feature, embed(w_0), ...], in fp64."""
    E, H, V, B = 7, 9, 23, 5
    p = decode_params(StackedDecoderRNN(E, H, V, layers), seed=5 + layers)
    lengths = [6, 6, 4, 3, 1]
    g = torch.Generator().manual_seed(1)
    captions = torch.randint(0, V, (B, max(lengths)), generator=g)
    feats = torch.rand(B, E, generator=g, dtype=torch.float64) - 0.5
    got = stacked_lstm_forward(p, captions, lengths, feats, [True] * max(lengths), layers)
    lstm = nn.LSTM(E, H, num_layers=layers, batch_first=True).double()
    with torch.no_grad():
        for l in range(layers):
            src = "lstm" if l == 0 else "lstm%d" % l
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(lstm, "%s_l%d" % (n, l)).copy_(p["%s.%s" % (src, n)])
    x = torch.cat([feats.unsqueeze(1), p["embed.weight"][captions]], 1)[:, :max(lengths)]
    out, _ = lstm(pack_padded_sequence(x, lengths, batch_first=True))
    want = nn.functional.linear(out.data, p["linear.weight"], p["linear.bias"])
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)


def test_restated_step_is_torch_lstm_step():
    E, H, rows, layers = 5, 8, 4, 3
    p = decode_params(StackedDecoderRNN(E, H, 11, layers), seed=2)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(rows, E, generator=g, dtype=torch.float64)
    hs = [torch.rand(rows, H, generator=g, dtype=torch.float64) for _ in range(layers)]
    cs = [torch.rand(rows, H, generator=g, dtype=torch.float64) for _ in range(layers)]
    top, h2, c2 = stacked_step(p, x, hs, cs, layers)
    lstm = nn.LSTM(E, H, num_layers=layers).double()
    with torch.no_grad():
        for l in range(layers):
            src = "lstm" if l == 0 else "lstm%d" % l
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(lstm, "%s_l%d" % (n, l)).copy_(p["%s.%s" % (src, n)])
    out, (hn, cn) = lstm(x.unsqueeze(0), (torch.stack(hs), torch.stack(cs)))
    assert torch.allclose(top, out[0], atol=1e-12)
    for l in range(layers):
        assert torch.allclose(h2[l], hn[l], atol=1e-12) and torch.allclose(c2[l], cn[l], atol=1e-12)


def test_new_entry_point_is_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "capnet.h")).read()
    assert "capnet_stacked_decode_step_cell(" in src
    assert "capnet_stacked_decode_step_cell" in _lib.SIGNATURES
    assert hasattr(capnet.lib(), "capnet_stacked_decode_step_cell")
    assert capnet.lib().capnet_abi_version() == 1


def _call(cell=1, nlayers=2, rows=5, E=300, H=512, V=37, tokens=8, x=16, w=(32, 48), b=(64, 80), sin=96, sout=112,
          top=128, err=144):
    """Argument checks only: every pointer is a fake, 16-B aligned address, never dereferenced on the host."""
    lib = capnet.lib()
    arr = (C.c_void_p * 2)
    return lib.capnet_stacked_decode_step_cell(cell, nlayers, rows, E, H, V, tokens, x, arr(*w), arr(*b), sin, sout, top,
                                               err, None), lib.capnet_last_error().decode()


def test_new_entry_point_checks_arguments_without_a_gpu():
    rc, msg = _call(cell=2)
    assert rc < 0 and "cell 2" in msg
    rc, msg = _call(cell=-1)
    assert rc < 0 and "cell" in msg
    rc, msg = _call(nlayers=0)
    assert rc < 0 and "layers" in msg
    rc, msg = _call(x=None)
    assert rc < 0 and "null" in msg
    rc, msg = _call(sout=None)
    assert rc < 0 and "null" in msg
    rc, msg = _call(w=(32, None))
    assert rc < 0 and "layer 1" in msg
    rc, msg = _call(H=500)
    assert rc < 0 and "unsupported" in msg
    rc, msg = _call(sin=100)
    assert rc < 0 and "alignment" in msg
    rc, msg = _call(w=(32, 52))
    assert rc < 0 and "aligned" in msg


def test_stacked_lstm_entries_check_null_weights_without_a_gpu():
    lib = capnet.lib()
    dims = _lib.int_array([4, 6, 5, 14, 12, 0, 16, 37, 0, 1])
    rc = lib.capnet_seq_forward_stacked(dims, 2, None, None, None, None, None, (C.c_void_p * 64)(), None, None, 0.0, 0,
                                        0, None, None, None, None, None, None)
    assert rc != 0 and b"null" in lib.capnet_last_error()


def test_sequence_functions_check_weight_counts():
    """The CPU tensors would be refused only at the first launch: the counts are checked before."""
    with pytest.raises(capnet.CapnetError):
        ops.SeqFn.apply(dict(cell=ops.CELL_LSTM, num_layers=2), torch.zeros(2, 3, dtype=torch.int64), None,
                        torch.zeros(5, 4), torch.zeros(5, 8), torch.zeros(5))
    # (the CUDA check comes first for CPU tensors; the count check is reached through _seq_args on a CUDA-free path)
    cfg = dict(cell=ops.CELL_LSTM, num_layers=2, batch_sizes=[2, 2], tf_mask=[True, True], hidden_size=8)
    with pytest.raises(capnet.CapnetError, match="LSTM cell 4"):
        ops.SeqFn.forward(_Ctx(), cfg, _Cuda(torch.zeros(2, 2, dtype=torch.int64)), None, *[_Cuda(torch.zeros(1))] * 3,
                          *[_Cuda(torch.zeros(1))] * 4)
    cfg["attention_size"] = 4
    with pytest.raises(capnet.CapnetError, match="16 \\+ 8"):
        ops.AttSeqFn.forward(_Ctx(), cfg, _Cuda(torch.zeros(2, 2, dtype=torch.int64)), _Cuda(torch.zeros(1)),
                             *[_Cuda(torch.zeros(1))] * 3, *[_Cuda(torch.zeros(1))] * 16)
    with pytest.raises(capnet.CapnetError, match="stacks 1 to 8"):
        ops.SeqFn.forward(_Ctx(), dict(cfg, num_layers=9), _Cuda(torch.zeros(2, 2, dtype=torch.int64)), None,
                          *[_Cuda(torch.zeros(1))] * 3)


class _Ctx:
    pass


class _Cuda(torch.Tensor):
    """A CPU tensor that passes the operators' device check (no launch is reached in these tests)."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True
