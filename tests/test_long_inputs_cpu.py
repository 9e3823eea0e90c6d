"""Host-side proof that the inputs of the long-caption and attention-shape GPU tests reach the branches they are meant
for, and that the scheduled-sampling cases are well posed. Nothing here needs a GPU.

* att_datt1_kernel's chunk loop: at A = 512 it holds 29 steps at a time, and the attention batches make workgroups of
  ONE launch take 1, 2, 3 and >= 4 trips; the small-A control takes one.
* lstm_persist_kernel's second metadata register: steps >= 64 are run, the cap of 128 is reached exactly, and runs of
  teacher-forced steps restart past step 64.
* att_context_fwd_kernel's quarters: which of {full 14-sweep, clamped tail, empty quarter} every P of the list gives.
* A fed-back token is an argmax: for every row that is fed back the fp64 oracle's top-1 / top-2 margin exceeds twice
  the error the logits comparison lets through, so the GPU run and the oracle decode the same sequence."""
import pytest
import torch

import long_cases as LC
from test_lstm_persist_gpu import CASES as PERSIST_CASES, SEGMENT_CASES


def test_t_chunk_and_trip_counts():
    assert LC.t_chunk(512) == 29
    for lengths in (LC.LATT6, LC.LATT20):
        trips = sorted({LC.datt1_trips(l, 512, max(lengths)) for l in lengths})
        assert trips[:3] == [1, 2, 3] and trips[-1] >= 4, trips
        assert {29, 30, 58, 59} <= set(lengths) and max(lengths) > 87 and min(lengths) < 10
    assert LC.t_chunk(24) >= max(LC.LATT6)
    assert {LC.datt1_trips(l, 24, max(LC.LATT6)) for l in LC.LATT6} == {1}
    assert len(LC.LATT6) <= 16 and 17 <= len(LC.LATT20) <= 64


def test_step_counts_of_the_long_cases():
    assert max(LC.L128) == LC.MAX_STEPS
    assert 65 <= max(LC.L97) <= 100
    assert max(LC.LSTACK) > 64 and max(LC.L127) + 1 == LC.MAX_STEPS
    for name, c in LC.CASES.items():
        assert c["lengths"] == sorted(c["lengths"], reverse=True), name
        T = max(c["lengths"])
        assert T >= 65, name
        if c["tf"] == "mixed":
            tf = LC.tf_mask("mixed", T, c["seed"])
            starts = LC.segment_starts(tf)
            assert any(t > 64 for t in starts) and any(t < 64 for t in starts), (name, starts)
            assert not all(tf) and any(tf)
    families = {c["family"] for c in LC.CASES.values()}
    assert families == set(LC.TOL)
    for fam in families:                                  # one long case with dropout on per family
        assert any(c["family"] == fam and c["p"] == 0.5 for c in LC.CASES.values()), fam
    for fam in ("stacked", "nic_stacked", "stacked_att", "nic_stacked_att"):
        assert {c["layers"] for c in LC.CASES.values() if c["family"] == fam} >= {2, 3}


def test_persistent_kernel_cases_reach_the_second_register():
    steps = {len(bs) for bs in PERSIST_CASES.values()}
    assert {64, 65, 100, 128} <= steps
    assert any(len(bs) > 64 and len(set(bs)) == 1 and bs[0] <= 16 for bs in PERSIST_CASES.values())
    assert any(len(bs) == 128 and set(bs) == {64} for bs in PERSIST_CASES.values())
    shrink = [bs for bs in PERSIST_CASES.values() if bs[0] == 128 and bs[-1] == 1]
    assert shrink
    for bs in shrink:
        cuts = [t for t in range(1, len(bs)) if bs[t] < bs[t - 1]]
        assert any(t < 64 for t in cuts) and any(t > 64 for t in cuts) and 64 in cuts
    for bs in PERSIST_CASES.values():
        assert all(1 <= b <= 128 for b in bs) and bs == sorted(bs, reverse=True) and len(bs) <= LC.MAX_STEPS
    t0s = set()
    for name, segs in SEGMENT_CASES:
        bs = PERSIST_CASES[name]
        assert segs[0][0] == 0 and segs[-1][1] == len(bs)
        assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        t0s |= {s[0] for s in segs}
    assert {63, 64, 65, 127} <= t0s


def test_map_sizes_cover_every_path_of_the_context_sweep():
    want = {
        1: {"clamped tail", "empty quarter"}, 2: {"clamped tail", "empty quarter"}, 3: {"clamped tail", "empty quarter"},
        4: {"clamped tail"}, 5: {"clamped tail", "empty quarter"}, 13: {"clamped tail"}, 14: {"clamped tail"},
        15: {"clamped tail"}, 16: {"clamped tail"}, 49: {"clamped tail"}, 55: {"full 14-sweep", "clamped tail"},
        56: {"full 14-sweep"}, 57: {"full 14-sweep", "clamped tail"}, 64: {"full 14-sweep", "clamped tail"},
        196: {"full 14-sweep", "clamped tail"}, 197: {"full 14-sweep", "clamped tail"},
        256: {"full 14-sweep", "clamped tail"}, 441: {"full 14-sweep", "clamped tail"}, 784: {"full 14-sweep"},
    }
    assert sorted(want) == LC.P_LIST
    seen = set()
    for P in LC.P_LIST:
        assert LC.context_classes(P) == want[P], (P, LC.context_classes(P))
        seen |= want[P]
        q = LC.context_quarters(P)
        assert sum(max(0, b - a) for a, b in q) == P
        tp = LC.tail_pixels(P)
        assert tp[-1] == P - 1 and all(0 <= p < P for p in tp)
    assert seen == {"full 14-sweep", "clamped tail", "empty quarter"}
    # quarters that are an exact multiple of 14, a quarter shorter than 14 that is not 3, many full sweeps
    assert [b - a for a, b in LC.context_quarters(56)] == [14] * 4
    assert [b - a for a, b in LC.context_quarters(784)] == [196] * 4 and 196 % 14 == 0
    assert [b - a for a, b in LC.context_quarters(49)] == [13, 13, 13, 10]
    assert LC.context_quarters(5)[3][1] <= LC.context_quarters(5)[3][0]
    # the backward kernels sweep all of P 14 at a time: multiples of 14 (no tail) and everything else
    assert {P % 14 == 0 for P in LC.P_LIST} == {True, False}


@pytest.mark.parametrize("name", [n for n, c in LC.CASES.items() if c["tf"] != "all" and not c["like"]])
def test_fed_back_argmax_margins(name):
    """Twice the logits tolerance times the largest logit is twice the error the GPU comparison would let through: a
    fed-back row whose two best logits are closer than that could decode another token on the GPU and make the two
    runs different sequences. Every fed-back row is checked; none is dropped."""
    c = LC.LongCase(name)
    logits = c.oracle_logits()
    margin, rows, scale = LC.fed_back_margin(logits, c.lengths, c.tf)
    need = 2 * c.tol_logits * scale
    print("%s: %d fed-back rows, smallest margin %.3e, needed %.3e (largest logit %.3f)" % (name, rows, margin, need, scale))
    assert rows > 0
    assert margin > need, (name, margin, need)
