"""Every decoder family at long captions: one training step (forward, loss, backward) against the fp64 oracle at 65 to
128 steps, where the suite otherwise stops at 24 (tests/long_cases.py holds the cases, tests/test_long_inputs_cpu.py the
host-side proof of which branch each reaches).

* DecoderFactoredLSTM / nic DecoderRNN at H = 512 (the persistent kernel, csrc/lstm_persist.hip: steps >= 64 read the
  second metadata register), exactly 128 steps and 97, teacher forcing all / none / mixed, the launch-per-step path on
  the same inputs as a control.
* The attention decoders at A = 512, where att_datt1_kernel holds 29 steps in LDS at a time: samples alive for 100, 59,
  58, 30, 29 and 5 steps in one launch (4, 3, 2, 2, 1, 1 trips), at <= 16 rows and at 20, with a small-A control.
* The four stacked families at 2 and 3 layers beyond 64 steps; the stacked attention decoders' own cap (127 steps run,
  128 are refused on the host).
* Dropout p = 0.5 for one long case per family, with the very masks the kernels draw (tests/test_dropout_gpu.py).

Bounds: each family's short-test bounds (long_cases.TOL). The logits / alphas bound is max(that, 3 x the distance of
the same oracle run in float32 from the float64 one on the case), the rule of tests/test_lstm_persist_gpu.py; both
distances are printed. Scheduled sampling feeds an argmax back: before anything is compared, every fed-back row of the
oracle must be clear of a tie by twice what the logits bound lets through."""
import pytest
import torch

import capnet
from capnet import ops
from capnet._lib import lib
from helpers import rel_err
import long_cases as LC
from test_dropout_gpu import _Case

pytestmark = pytest.mark.gpu

_ORACLE = {}


@pytest.fixture(params=[-1, 1], ids=["chain-3-products", "chain-1-product"])
def chain(request):
    old = lib().capnet_att_set_chain_mode(request.param)
    yield request.param
    lib().capnet_att_set_chain_mode(old)


def _run_case(dev, name, tag=""):
    lc = LC.LongCase(name)
    lc.dec.to(dev).train()
    c = _Case(lc.dec, lc.params, lc.forward, lc.captions, lc.lengths, lc.feats, lc.tf, att=lc.att,
              num_layers=lc.num_layers, **lc.kw)
    old = lib().capnet_lstm_persist_set_mode(1) if lc.per_step else None     # what CAPNET_NO_PERSISTENT_LSTM=1 sets
    try:
        seed = c.product(dev, lc.seed_k)
    finally:
        if old is not None:
            lib().capnet_lstm_persist_set_mode(old)
    key = _key(lc)
    if key not in _ORACLE:                    # the same for both chain forms and for the per-step control
        masks = lc.masks()
        if lc.p > 0:
            assert seed == LC.pin_dropout_seed(lc.seed_k)
        ref = c.oracle(**masks)
        e_f = rel_err(lc.oracle_logits(torch.float32), ref["logits"])
        _ORACLE[key] = (ref, e_f)
    c.ref, e_f = _ORACLE[key]
    tol = max(lc.tol_logits, 3 * e_f)
    margin, rows, scale = LC.fed_back_margin(c.ref["logits"], lc.lengths, lc.tf)
    print("%s%s: %d steps, %d rows; fp32 oracle %.2e from fp64, logits bound %.1e; %d fed-back rows, margin %.2e"
          % (name, tag, lc.steps, sum(lc.lengths), e_f, tol, rows, margin))
    assert rows == 0 or margin > 2 * tol * scale, (name, margin, 2 * tol * scale)
    c.compare(name + tag, tol, lc.tol_grad)
    return lc


def _key(lc):
    like = LC.CASES[lc.name]["like"]
    return like or lc.name


PLAIN_CASES = [n for n, c in LC.CASES.items() if c["family"] in ("factored", "nic")]
ATT_CASES = [n for n, c in LC.CASES.items() if c["family"] == "factored_att"]
NIC_ATT_CASES = [n for n, c in LC.CASES.items() if c["family"] == "nic_att"]
STACKED_CASES = [n for n, c in LC.CASES.items() if "stacked" in c["family"]]


@pytest.mark.parametrize("name", PLAIN_CASES)
def test_plain_decoders_at_long_captions(dev, name):
    lc = _run_case(dev, name)
    assert lc.dims["H"] == 512 and lc.steps >= 65
    if "_128_" in name:
        assert lc.steps == LC.MAX_STEPS


@pytest.mark.parametrize("name", ATT_CASES)
def test_factored_attention_decoder_at_long_captions(dev, chain, name):
    lc = _run_case(dev, name, " chain %d" % chain)
    trips = sorted({LC.datt1_trips(l, lc.dims["A"], lc.steps) for l in lc.lengths})
    if lc.dims["A"] == 512:
        assert trips[:3] == [1, 2, 3] and trips[-1] >= 4
    else:
        assert trips == [1]


@pytest.mark.parametrize("name", NIC_ATT_CASES)
def test_nic_attention_decoder_at_long_captions(dev, name):
    lc = _run_case(dev, name)
    trips = sorted({LC.datt1_trips(l, lc.dims["A"], lc.steps) for l in lc.lengths})
    assert (trips[:3] == [1, 2, 3] and trips[-1] >= 4) if lc.dims["A"] == 512 else trips == [1]


@pytest.mark.parametrize("name", STACKED_CASES)
def test_stacked_decoders_at_long_captions(dev, name):
    lc = _run_case(dev, name)
    assert lc.steps > 64 and lc.layers in (2, 3)
    if name.endswith("_127_steps"):
        assert lc.steps + 1 == LC.MAX_STEPS


@pytest.mark.parametrize("family", ["stacked_att", "nic_stacked_att"])
def test_stacked_attention_refuses_128_steps(dev, family):
    """The stacked attention decoders keep one more row table entry than steps: 127 steps run
    (test_stacked_decoders_at_long_captions), 128 are refused by the host-side check before any device work."""
    d = LC.TINY_ATT
    dec = LC._decoder(family, d, 2, 0.0).to(dev).train()
    lengths = [128, 5]
    captions = LC._captions(lengths, d["V"], 1).to(dev)
    feats = torch.zeros(2, d["P"], d["Cf"], device=dev)
    with pytest.raises(capnet.CapnetError):
        dec(captions, lengths, feats, tf_mask=[True] * 128)
    ops.check_device_errors()
