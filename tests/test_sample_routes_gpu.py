"""Which C entries each sampled-decoding route calls, cell by cell: units (a plain stack, an attention decoder,
capnet.seq2seq) x routes (default, CAPNET_NO_FUSED_SAMPLE=1, CAPNET_NO_FUSED_DECODE_STEP=1) x options (nothing, top_k, top_p,
both, an explicit top_p=1.0, greedy=True, greedy=True under a nucleus, an inactive Constraints(), an active exclusion set, an
active set under a nucleus, under top_k and with the greedy row). The sibling tests compare tokens and log-probabilities
with the fp64 restatements; they cannot see an explicit top_p=1.0 or an inactive Constraints() start taking the nucleus or
the _excl entry, or a greedy row fall from the one call to the composed loop, since the results stay equal. This test sees
the calls themselves, as tests/test_beam_routes_gpu.py does for the searches.

A recording proxy stands in for the loaded library object for the duration of a cell. It forwards every call and notes
the ordered distinct names of the capnet_* calls made, the size queries (*_bytes) apart; the list must equal
tests/sample_routes_expected.json. That table was recorded ONCE from a build of the commit before the sampling entries were
merged, by running this file with CAPNET_RECORD_SAMPLE_ROUTES=<path of the table to write>; no normal run sets it, and it is
never recorded from the code under test.

Every cell takes its decoder, stream seed and options from a case of sample_random_cases, nucleus_cases, greedy_row_cases
or excluded_sample_cases (CELLS), whose margins the CPU tests have cleared, so the three routes must return the same tokens;
logp agrees within 2 x sample_random_ref.logp_tol per word, the rule of the sibling tests between routes. A unit has no
cell where no case has the option: capnet.seq2seq has neither greedy nor exclude and no admitted nucleus case without
top_k, the plain stacks no exclusion case under a nucleus or with the greedy row. The explicit top_p=1.0 and the inactive
set run on the `nothing` case and must make its calls. The greedy_row_cases cells run, as in test_greedy_row_gpu, with the
row limits of the one call raised to 64, so that the _greedy entries are reached at the cases' 18 and 32 rows.
Shapes: those of the case modules -- 2 images x 3 samples, 12 steps, V 37 (greedy_row_cases: 3 x 5 and 2 x 15 on 8 steps;
capnet.seq2seq: 1 and 12 rows, 40 steps, V 8192)."""
import json
import os

import pytest
import torch

import excluded_sample_cases as XC
import greedy_row_cases as GC
import nucleus_cases as NC
import sample_random_cases as SC
import sample_random_ref as R
import test_greedy_row_gpu as TG
import test_sample_random_gpu as TS
from capnet import _lib, decode, ops
from capnet.beam import Constraints
from capnet.decode import FUSED_DECODE_OFF, FUSED_SAMPLE_OFF

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sample_routes_expected.json")
RECORD = os.environ.get("CAPNET_RECORD_SAMPLE_ROUTES")
ROUTES = (("default", None), ("no_fused_sample", FUSED_SAMPLE_OFF), ("no_fused_step", FUSED_DECODE_OFF))
# unit -> (option, case module, case id, keywords on top of the case's own)
CELLS = {
    "plain": (("nothing", "sample", "DecoderRNN-k0", {}),
              ("top_k", "sample", "DecoderRNN-k5", {}),
              ("top_p", "nucleus", "DecoderRNN-k0-p0.9", {}),
              ("top_k_top_p", "nucleus", "DecoderRNN-k5-p0.5", {}),
              ("top_p_1.0", "sample", "DecoderRNN-k0", dict(top_p=1.0)),
              ("greedy", "greedy", "StackedFactoredLSTM-2-n3-m5-k5-p1-T1", {}),
              ("greedy_top_p", "greedy", "StackedDecoderRNN-2-n3-m5-k5-p0.9-T0.7", {}),
              ("inactive", "sample", "DecoderRNN-k0", dict(exclude=Constraints())),
              ("active", "excluded", "DecoderRNN-k0-D", {}),
              ("active_top_k", "excluded", "DecoderRNN-k5-A", {})),
    "att": (("nothing", "sample", "DecoderRNNAtt-p4-k0", {}),
            ("top_k", "sample", "DecoderRNNAtt-p4-k5", {}),
            ("top_p", "nucleus", "DecoderRNNAtt-p4-k0-p0.9", {}),
            ("top_k_top_p", "nucleus", "DecoderRNNAtt-p4-k5-p0.5", {}),
            ("top_p_1.0", "sample", "DecoderRNNAtt-p4-k0", dict(top_p=1.0)),
            ("greedy", "greedy", "DecoderFactoredLSTMAtt-1-v37-n3-m5-k0-p1-T1", {}),
            ("greedy_top_p", "greedy", "DecoderFactoredLSTMAtt-1-v37-n2-m15-k5-p0.9-T1", {}),
            ("inactive", "sample", "DecoderRNNAtt-p4-k0", dict(exclude=Constraints())),
            ("active", "excluded", "DecoderRNNAtt-p4-k0-D", {}),
            ("active_top_p", "excluded", "DecoderRNNAtt-p4-k0-D-p0.9", {}),
            ("active_top_k", "excluded", "DecoderRNNAtt-p4-k5-A", {}),
            ("active_greedy", "excluded", "DecoderRNNAtt-p4-k0-D-greedy", {})),
    "seq2seq": (("nothing", "seq2seq", "r12_l1_v8192", {}),
                ("top_k", "seq2seq", "r1_l3_v8192", {}),
                ("top_k_top_p", "seq2seq_nucleus", "r1_l3_v8192_k5_p9", {}),
                ("top_p_1.0", "seq2seq", "r12_l1_v8192", dict(top_p=1.0))),
}
SAME_AS_NOTHING = ("top_p_1.0", "inactive")


class Recorder:
    """Forwards every attribute to the library; notes the distinct capnet_* calls in the order of their first call."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("capnet_") and not name.endswith("_bytes"):
            def noted(*a):
                if name not in self.names:
                    self.names.append(name)
                return fn(*a)
            return noted
        return fn


def _by_id(cases, cid):
    return [c for c in cases if c["id"] == cid][0]


def _image(module, cid, dev):
    """(run(**extra) -> the lists of sample_random, the case's logp tolerance per word) for an image-decoder case."""
    if module == "greedy":
        case = _by_id(GC.CASES, cid)
        fam = GC.families()[case["family"]]
        dec, f, tr = GC.make(fam, dev), fam.features()[:case["n"]].to(dev), GC.reference(case)[2]
        kw = dict(samples=case["m"], temperature=case["T"], top_k=case["top_k"], seed=GC.SEEDS[cid], greedy=True, **fam.kw)
        end = GC.end_token(case)
    else:
        cases = {"sample": SC.IMAGE_CASES, "nucleus": NC.IMAGE_CASES, "excluded": XC.CASES}[module]
        case = _by_id(cases, cid)
        fam = SC.families()[case["family"]]
        dec, f = fam.make().to(dev).eval(), fam.features()[:SC.IMAGES].to(dev)
        kw = dict(samples=SC.SAMPLES, temperature=case["T"], top_k=case["top_k"], seed=case["seed"], **fam.kw)
        if module == "excluded":
            ref = XC.reference(case)
            tr, end = ref["excl"][2], ref["end"]
            kw.update(exclude=ref["c"], **({"greedy": True} if case["greedy"] else {}))
        else:
            tr = (SC if module == "sample" else NC).image_reference(case)[2]
            end = fam.V                                      # never drawn: all MAX_LEN words
    if case.get("top_p", 1.0) < 1.0:
        kw["top_p"] = case["top_p"]
    return (lambda **extra: dec.sample_random(f, SC.START, end, **kw, **extra)), R.logp_tol(tr.scale, R.inv_temperature(case["T"]))


def _seq2seq(module, name, dev):
    """The same for a capnet.seq2seq case: run(**extra) -> (ids, logp)."""
    c, p, feats, s, ref = (SC if module == "seq2seq" else NC).seq2seq_reference(name)
    m, f = TS._seq_model(p, c, dev), feats.float().to(dev)
    kw = dict(temperature=s["T"], top_k=s["top_k"], seed=s["seed"], **({"top_p": s["top_p"]} if "top_p" in s else {}))
    return (lambda **extra: m.sample_random(f, 1, mode=c["mode"], **kw, **extra)), R.logp_tol(ref[3].scale, R.inv_temperature(s["T"]))


def _same(got, want, tol, what):
    if isinstance(want, tuple):                              # capnet.seq2seq: (ids, logp) [rows, steps]
        assert torch.equal(got[0], want[0]), what
        assert (got[1].double() - want[1].double()).abs().max().item() <= 2 * tol, what
    else:
        TS._same_lists(got, want, 2 * tol)


@pytest.mark.parametrize("unit", sorted(CELLS))
def test_every_cell_calls_the_entries_of_the_table(dev, monkeypatch, unit):
    lib = _lib.lib()
    seen = {}
    for option, module, cid, extra in CELLS[unit]:
        run, tol = (_seq2seq if module.startswith("seq2seq") else _image)(module, cid, dev)
        with monkeypatch.context() as mp:
            if module == "greedy":
                for name in TG.LIMITS:
                    mp.setattr(decode, name, 64)
            results = {}
            for route, env in ROUTES:
                mp.delenv(FUSED_SAMPLE_OFF, raising=False)
                mp.delenv(FUSED_DECODE_OFF, raising=False)
                if env:
                    mp.setenv(env, "1")
                rec = Recorder(lib)
                mp.setattr(_lib, "_lib", rec)
                results[route] = run(**extra)
                mp.setattr(_lib, "_lib", lib)
                seen["%s/%s/%s" % (unit, route, option)] = rec.names
        for route, _ in ROUTES[1:]:
            _same(results[route], results["default"], tol, (unit, route, option))
    ops.check_device_errors()
    for option in SAME_AS_NOTHING:
        for route, _ in ROUTES:
            cell = "%s/%s/%s" % (unit, route, option)
            assert cell not in seen or seen[cell] == seen["%s/%s/nothing" % (unit, route)], cell
    if RECORD:
        table = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        table.update(seen)
        with open(RECORD, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    table = json.load(open(TABLE))
    assert sorted(k for k in table if k.startswith(unit + "/")) == sorted(seen)
    for cell, names in seen.items():
        assert names == table[cell], (cell, names, table[cell])
