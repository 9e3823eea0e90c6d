"""capnet.stacked_att without a GPU: the CPU restatement of the stacked attention decoder reduces to the reference's
attention decoder with one layer, the module's parameter registration, and the new C-ABI entry points."""
import json
import os
import random

import torch

import capnet
from capnet import _lib
from capnet.stacked_att import StackedFactoredLSTMAtt
from oracle import decoders_ref as D
from stacked_att_ref import layer_params, stacked_factored_att_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")))
ATT_KEY = "stylenet.DecoderFactoredLSTMAtt(512,300,512,512,1000,1)"


def _kv(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def _params(dec, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: ((torch.rand(v.shape, generator=g) * 2 - 1) * (0.3 if v.dim() > 1 else 0.05)).double()
            for k, v in dec.state_dict().items()}


def test_restatement_with_one_layer_is_the_attention_decoder():
    A, E, H, F, V, Cf, P, B = 8, 6, 10, 7, 23, 12, 5, 4
    dec = StackedFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=Cf, dropout=0.0)
    p = _params(dec, 3)
    g = torch.Generator().manual_seed(5)
    lengths = [6, 5, 5, 2]
    captions = torch.randint(0, V, (B, max(lengths)), generator=g)
    feats = torch.rand(B, P, Cf, generator=g, dtype=torch.float64)
    random.seed(2)
    tf = [random.random() < 0.5 for _ in range(max(lengths))]
    targets = D.packed_targets(captions, lengths)
    for mode in ("factual", "sad"):
        pa = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        pb = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        la, aa = stacked_factored_att_forward(pa, captions, lengths, feats, tf, mode, num_layers=1)
        lb, ab = D.factored_att_forward(pb, captions, lengths, feats, tf, mode)
        D.att_loss(la, aa, targets).backward()
        D.att_loss(lb, ab, targets).backward()
        assert torch.allclose(la, lb, rtol=1e-13, atol=0) and torch.allclose(aa, ab, rtol=1e-13, atol=0)
        for k in p:
            assert (pa[k].grad is None) == (pb[k].grad is None), k
            if pa[k].grad is not None:
                assert torch.allclose(pa[k].grad, pb[k].grad, rtol=1e-12, atol=1e-15), k


def test_restatement_upper_layers_read_their_own_parameters():
    A, E, H, F, V, Cf, P, B = 8, 6, 10, 7, 23, 12, 5, 3
    dec = StackedFactoredLSTMAtt(A, E, H, F, V, 2, feature_size=Cf, dropout=0.0)
    p = {k: v.requires_grad_(True) for k, v in _params(dec, 4).items()}
    assert sorted(layer_params(p, 1)) == sorted(k for k in p if k[0] in "VSUW" and k[1] == "_")
    captions = torch.randint(0, V, (B, 4), generator=torch.Generator().manual_seed(1))
    feats = torch.rand(B, P, Cf, dtype=torch.float64)
    logits, alphas = stacked_factored_att_forward(p, captions, [4, 3, 2], feats, [True, False, True, True], "happy", 2)
    logits.sum().backward()
    for k in ("init_h1.weight", "init_c1.bias", "V1_i.weight", "S1_happy_c.weight", "U1_o.bias", "W1_f.weight"):
        assert p[k].grad is not None and float(p[k].grad.abs().max()) > 0, k
    for k in ("S1_fi.weight", "S1_sad_i.weight", "S_fi.weight"):
        assert p[k].grad is None, k


def test_one_layer_has_the_reference_state_dict_keys_in_order():
    assert _kv(StackedFactoredLSTMAtt(512, 300, 512, 512, 1000, 1)) == KEYS[ATT_KEY]


def test_two_layers_add_exactly_the_layer_one_keys():
    H, F, Cf = 32, 24, 64
    ref = [k for k, _ in KEYS[ATT_KEY]]
    dec = StackedFactoredLSTMAtt(16, 12, H, F, 50, 2, feature_size=Cf)
    keys = list(dec.state_dict().keys())
    assert keys[:len(ref)] == ref
    extra = keys[len(ref):]
    want = {"init_h1.weight": [H, Cf], "init_h1.bias": [H], "init_c1.weight": [H, Cf], "init_c1.bias": [H]}
    for g in "ifoc":
        want.update({"U1_%s.weight" % g: [H, F], "U1_%s.bias" % g: [H], "S1_f%s.weight" % g: [F, F], "S1_f%s.bias" % g: [F],
                     "V1_%s.weight" % g: [F, H], "V1_%s.bias" % g: [F], "W1_%s.weight" % g: [H, H], "W1_%s.bias" % g: [H]})
        for emo in ("happy", "sad", "angry"):
            want.update({"S1_%s_%s.weight" % (emo, g): [F, F], "S1_%s_%s.bias" % (emo, g): [F]})
    assert sorted(extra) == sorted(want)
    sd = dec.state_dict()
    for k, shape in want.items():
        assert list(sd[k].shape) == shape, k
    assert len(keys) == len(set(keys))


def test_initialisation_follows_the_attention_decoder():
    dec = StackedFactoredLSTMAtt(16, 12, 32, 24, 50, 3, feature_size=64)
    dec.requires_grad_(False)
    assert float(dec.C.bias.abs().max()) == 0.0 and float(dec.C.weight.abs().max()) <= 0.1
    assert float(dec.B.weight.abs().max()) <= 0.1
    assert float(dec.init_h2.bias.abs().max()) == 0.0 and float(dec.V2_i.weight.abs().max()) > 0.0
    assert float(dec.W1_c.bias.abs().max()) == 0.0


def test_new_entry_points_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "capnet.h")).read()
    lib = capnet.lib()
    for name in ("capnet_att_seq_forward_stacked", "capnet_att_seq_backward_stacked", "capnet_att_stacked_saved_floats",
                 "capnet_att_stacked_saved_ints", "capnet_att_stacked_fwd_scratch_floats",
                 "capnet_att_stacked_bwd_scratch_floats"):
        assert name + "(" in src, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_stacked_entry_points_check_arguments_without_a_gpu():
    lib = capnet.lib()
    dims = _lib.int_array([4, 6, 5, 14, 12, 16, 16, 37, 16, 4, 512, 1])       # the LSTMCell: not stackable
    rc = lib.capnet_att_seq_forward_stacked(dims, 2, None, None, None, None, None, None, None, None, 0.0, 0, 0, None, None,
                                            None, None, None, None, None)
    assert rc != 0
    dims = _lib.int_array([4, 6, 5, 14, 12, 16, 16, 37, 16, 4, 512, 0])
    # an upper layer's saved rows carry its initial state in front of the packed rows
    assert lib.capnet_att_stacked_saved_floats(dims, 1) > lib.capnet_seq_saved_floats(
        _lib.int_array([4, 6, 5, 14, 16, 16, 16, 37, 0, 0]))
    assert lib.capnet_att_stacked_saved_floats(dims, 0) == lib.capnet_att_saved_floats(dims)
    assert lib.capnet_att_stacked_bwd_scratch_floats(dims, 2) > lib.capnet_att_stacked_bwd_scratch_floats(dims, 1)
