"""capnet.decode.beam_decode's one route ladder (one call on a PlainStack, one call on an AttStack, beam_search_device, the
host loops) under every combination of one_call, on_device, nbest and return_alphas, with CAPNET_NO_FUSED_DECODE_STEP unset
(one_call=True is the one C call) and set to 1 (one_call=True is on_device=True): entry 0 of the n-best list at penalty 0
is the caption of the call without nbest, the tokens with return_alphas are those without it, and every route gives the
fp64 restatement's caption. One plain and one attention family, the smallest of their case modules, 2 images, k = 3: every
(k, image) of both has the margin (tests/test_beam_decode_cpu.py, tests/test_att_beam_decode_cpu.py), so nothing is skipped.
return_alphas is a keyword of the attention decoders only."""
import itertools

import pytest
import torch

from att_beam_cases import families as att_families
from beam_decode_cases import families as plain_families
from capnet import ops
from device_beam_cases import START

pytestmark = pytest.mark.gpu

N, K = 2, 3
FAMILIES = [plain_families()[0], [f for f in att_families() if f.name == "DecoderRNNAtt"][0]]
_want = {}


def _reference(family):
    if family.name not in _want:
        _want[family.name] = [family.reference(K, i) for i in range(N)]
    return _want[family.name]


@pytest.mark.parametrize("composed", [False, True], ids=["fused", "CAPNET_NO_FUSED_DECODE_STEP=1"])
@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.name)
def test_every_keyword_combination_takes_its_route_to_the_same_captions(dev, monkeypatch, family, composed):
    if composed:
        monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
    else:
        monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    dec = family.make().to(dev).eval()
    feats, end, kw = family.features()[:N].to(dev), family.end, family.kw
    att = "Att" in family.name
    want = _reference(family)
    for one_call, on_device in itertools.product((False, True), repeat=2):
        route = dict(one_call=one_call, on_device=on_device, **kw)
        plain = dec.sample_batch(feats, START, end, k=K, **route)
        assert plain == want, route
        one = dec.sample(feats[:1], START, end, k=K, **route)
        assert one.dtype == torch.int64 and one.device.type == "cuda" and one.cpu().tolist() == [want[0]], route
        best = dec.sample_batch(feats, START, end, k=K, nbest=True, **route)
        assert [hyps[0][0] for hyps in best] == plain, route
        assert all(isinstance(sc, float) for hyps in best for _, sc in hyps), route
        best1 = dec.sample(feats[:1], START, end, k=K, nbest=True, **route)
        assert best1[0][0].dtype == torch.int64 and best1[0][0].cpu().tolist() == [plain[0]], route
        if not att:
            continue
        P = feats.shape[1]
        seqs, maps = dec.sample_batch(feats, START, end, k=K, return_alphas=True, **route)
        assert seqs == plain and [tuple(m.shape) for m in maps] == [(len(q) - 1, P) for q in seqs], route
        one, m1 = dec.sample(feats[:1], START, end, k=K, return_alphas=True, **route)
        assert one.cpu().tolist() == [plain[0]] and tuple(m1.shape) == (len(plain[0]) - 1, P), route
        lists, maps = dec.sample_batch(feats, START, end, k=K, nbest=True, return_alphas=True, **route)
        assert [[q for q, _ in hyps] for hyps in lists] == [[q for q, _ in hyps] for hyps in best], route
        assert [[tuple(m.shape) for m in ms] for ms in maps] == [[(len(q) - 1, P) for q, _ in hyps] for hyps in lists], route
        lists1, maps1 = dec.sample(feats[:1], START, end, k=K, nbest=True, return_alphas=True, **route)
        assert [q.cpu().tolist() for q, _ in lists1] == [q.cpu().tolist() for q, _ in best1], route
        assert [tuple(m.shape) for m in maps1] == [(q.shape[1] - 1, P) for q, _ in best1], route
    ops.check_device_errors()
