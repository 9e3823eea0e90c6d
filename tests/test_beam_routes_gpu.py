"""Which C entries each beam-search route calls, cell by cell: routes (host loop on one image, host loop on a batch,
on_device, one_call) x options (nothing, an inactive Constraints(), min_words, a forced word, one team, two teams, two
teams under constraints, nbest, return_alphas). The existing tests compare tokens, scores and maps; they cannot see an
inactive Constraints() start taking the constrained kernel, or return_alphas fall from the recording entry to replay,
since the results stay equal. This test sees the calls themselves.

A recording proxy stands in for the loaded library object for the duration of a cell. It forwards every call and notes
the names of the capnet_*beam* and capnet_alpha_gather calls -- the size and offset queries (*_bytes, *_offset) apart:
most are asked once per shape and then cached, so whether a cell makes them depends on what ran before it; the ordered list of distinct names must equal
tests/beam_routes_expected.json. That table was recorded ONCE from a build of the commit before the selection-step
refactor, by running this file with CAPNET_RECORD_BEAM_ROUTES=<path of the table to write>; no normal run sets it, and
it is never recorded from the code under test.

Every cell's result is also compared with the host loop's for the same option. Tokens, lengths and nesting: exact.
Scores: 2 (len - 1) x seq2seq_cases.need(scale) -- the siblings' rule against fp64, doubled since both sides are fp32 here
-- with scale the bound on any logit of the decoder (|h| < 1 for an LSTM's output, so |logit| <= max over the rows of
sum |C| + |b|). Maps: 2 x att_alpha_cases.BOUND, for the same reason.
Shapes: the smallest of the case modules -- 2 images, k = 4, 2 teams, V = 37, 7 steps, <end> the fifth token of a greedy
decode so that beams complete."""
import json
import os

import pytest
import torch

import diverse_beam_cases as DC
from att_alpha_cases import BOUND, row_error
from capnet import _lib
from capnet.beam import Constraints, Diversity
from diverse_beam_cases import START
from seq2seq_cases import need

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "beam_routes_expected.json")
RECORD = os.environ.get("CAPNET_RECORD_BEAM_ROUTES")
UNITS = ("StackedFactoredLSTM-2", "DecoderRNNAtt")       # a plain stack, an attention decoder
N, K, STEPS = 2, 4, 7
QUERIES = ("_bytes", "_offset")
ROUTES = (("host_one", None), ("host_batch", {}), ("on_device", dict(on_device=True)), ("one_call", dict(one_call=True)))
OPTIONS = (("nothing", {}),
           ("inactive", dict(constraints=Constraints())),
           ("min_words", dict(constraints=Constraints(min_words=2))),
           ("forced", None),                      # Constraints(forced=(w,)), w the first word that is neither <start> nor <end>
           ("one_team", dict(diversity=Diversity(1, 0.5))),
           ("teams", dict(diversity=Diversity(2, 0.5))),
           ("teams_min_words", dict(diversity=Diversity(2, 0.5), constraints=Constraints(min_words=2))),
           ("nbest", dict(nbest=True)),
           ("alphas", dict(return_alphas=True)))


class Recorder:
    """Forwards every attribute to the library; notes the distinct beam entries in the order of their first call."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == "capnet_alpha_gather" or (name.startswith("capnet_") and "beam" in name and not name.endswith(QUERIES)):
            def noted(*a):
                if name not in self.names:
                    self.names.append(name)
                return fn(*a)
            return noted
        return fn


def _plain(x):
    """A result as nested lists: token tensors become lists (a [1, L] tensor its row), maps double tensors on the CPU."""
    if isinstance(x, torch.Tensor):
        if x.is_floating_point():
            return x.detach().cpu().double()
        return x[0].tolist() if x.dim() == 2 and x.size(0) == 1 else x.tolist()
    if isinstance(x, (list, tuple)):
        return [_plain(e) for e in x]
    return x


def _same(got, want, bound, what):
    if isinstance(want, torch.Tensor):
        assert isinstance(got, torch.Tensor) and tuple(got.shape) == tuple(want.shape), what
        assert row_error(got, want) < 2 * BOUND, what
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), (what, got, want)
        if len(want) == 2 and isinstance(want[1], float):                       # (tokens, score)
            assert got[0] == want[0] and abs(got[1] - want[1]) <= 2 * (len(want[0]) - 1) * bound, (what, got, want)
        else:
            for g, w in zip(got, want):
                _same(g, w, bound, what)
    else:
        assert got == want, (what, got, want)


def _first_image(batch, opts):
    """What sample() on image 0 returns, out of sample_batch's result."""
    return [batch[0][0], batch[1][0]] if opts.get("return_alphas") else batch[0]


def _logit_bound(dec):
    p = dec.state_dict()
    name = "C" if "C.weight" in p else "linear"
    w, b = p[name + ".weight"], p.get(name + ".bias")
    return float((w.abs().sum(1) + (b.abs() if b is not None else 0.0)).max())


@pytest.mark.parametrize("name", UNITS)
def test_every_cell_calls_the_entries_of_the_table(dev, monkeypatch, name):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    u = DC.unit(name)
    dec = u.family.make().to(dev).eval()
    dec.max_seq_length = STEPS
    feats, end, kw = u.family.features()[:N].to(dev), u.end, u.family.kw
    forced = dict(constraints=Constraints(forced=(min(w for w in range(3, u.V) if w not in (START, end)),)))
    bound = need(_logit_bound(dec))
    lib = _lib.lib()
    seen, results = {}, {}
    for oname, opts in OPTIONS:
        opts = forced if opts is None else opts
        if opts.get("return_alphas") and not DC.is_attention(u):
            continue
        for rname, route in ROUTES:
            rec = Recorder(lib)
            monkeypatch.setattr(_lib, "_lib", rec)
            if route is None:
                got = dec.sample(feats[:1], START, end, k=K, **opts, **kw)
            else:
                got = dec.sample_batch(feats, START, end, k=K, **opts, **route, **kw)
            monkeypatch.setattr(_lib, "_lib", lib)
            seen["%s/%s/%s" % (name, rname, oname)] = rec.names
            results[rname, oname] = _plain(got)
        host = results["host_batch", oname]
        _same(results["host_one", oname], _first_image(host, opts), bound, (name, "host_one", oname))
        for rname in ("on_device", "one_call"):
            _same(results[rname, oname], host, bound, (name, rname, oname))
    assert any(len(t) > 2 and t[-1] == end for t in results["host_batch", "nothing"])      # beams did complete
    if RECORD:
        table = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        table.update(seen)
        with open(RECORD, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    table = json.load(open(TABLE))
    assert sorted(k for k in table if k.startswith(name + "/")) == sorted(seen)
    for cell, names in seen.items():
        assert names == table[cell], (cell, names, table[cell])
