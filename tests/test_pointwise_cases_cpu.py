"""The table of tests/pointwise_cases.py checked without a device: every entry has rows and every row an entry; for every
row a plain float32 torch computation of the operation stays within BOUND x magnitude of the float64 reference (the bound
is achievable, and the inputs are chosen so that the reference alone meets it -- where this fails the row is wrong, not
the bound); the properties the GPU test relies on hold in the references themselves; and the host-side refusals of the
family, which return before anything touches a device."""
import ctypes

import pytest
import torch

import capnet
import pointwise_cases as PC

BOUND = 2e-6                                               # tests/test_pointwise_views_gpu.py's
X, Y, S1, T1, S2, OUT, TGT, ERR = (0x100000 * k for k in range(1, 9))     # plain integers as addresses, 16-B aligned


@pytest.fixture(scope="module")
def lib():
    return capnet.lib()


def test_every_entry_has_rows_and_every_row_an_entry():
    assert all(PC.of(e) for e in PC.ENTRIES)
    assert sum(len(PC.of(e)) for e in PC.ENTRIES) == len(PC.CASES)
    assert set(PC.ENTRY) == set(PC.ENTRIES)


def worst_ratio(got, ref, mag, floor=0.0):
    ok = torch.isfinite(ref)
    assert bool(torch.isfinite(got.double()[ok]).all())
    return float(((got.double() - ref).abs()[ok] / (BOUND * mag[ok] + floor).clamp_min(1e-300)).max()) if bool(ok.any()) else 0.0


def adam_rounds32(c, r):
    """The float32 oracle's state carried over the row's rounds; each round is measured against the float64 update of that
    round's own float32 state, as the GPU test measures the kernel."""
    worst = 0.0
    p, m, v = r["p"], r["m"], r["v"]
    for k in range(c.rounds):
        nxt = [], [], []
        for i in range(c.count):
            step = r["step"][i] + k
            _, ref = PC.adam_reference(p[i], r["g"][k][i], m[i], v[i], step, c.clip)
            got = PC.adam32(p[i], r["g"][k][i], m[i], v[i], step, c.clip)
            for j, name in enumerate(("p", "m", "v")):
                if c.numel[i]:
                    worst = max(worst, worst_ratio(got[name], *ref[name]))
                nxt[j].append(got[name])
        p, m, v = nxt
    return worst


@pytest.mark.parametrize("entry", [e for e in PC.ENTRIES if e not in PC.EXACT])
def test_float32_torch_stays_within_the_bound_of_the_float64_reference(entry):
    worst, over = 0.0, {}
    for c in PC.of(entry):
        r = PC.reference(c)
        if entry == PC.ADAM:
            ratios = {"p/m/v": adam_rounds32(c, r)}
        else:
            got = PC.oracle32(c, r)
            ratios = {name: worst_ratio(got[name], ref, mag, PC.ABS_FLOOR.get(name, 0.0)) for name, (ref, mag) in r["out"].items()}
        worst = max([worst] + list(ratios.values()))
        if max(ratios.values()) > 1.0:
            over[c.name] = ratios
    print("fp32 torch / bound, worst over %-24s %.3f" % (entry, worst))
    assert not over, over


def test_the_references_hold_what_the_rows_are_there_for():
    for c in PC.of(PC.XENT):
        r = PC.reference(c)
        assert all(bool(torch.isfinite(ref).all()) for ref, _ in r["out"].values()), c.name
        assert bool(torch.isfinite(r["x"][torch.arange(c.N), r["t"]]).all()), c.name
        if c.kind == "s80" and c.V > 5:
            assert float(r["x"].max()) > 89.0, c.name              # expf(x) alone overflows
        if c.kind == "neginf" and c.V > 5:
            assert bool(torch.isinf(r["x"]).any()), c.name
    xent = PC.of(PC.XENT)
    assert {c.kind for c in xent} == {"s1", "s80", "off1e4", "neginf"} and {c.ld - c.V for c in xent} == {0, 3}
    assert {(c.N, c.V) for c in xent} >= {(N, V) for N in (1, 3, 37) for V in (1, 5, 255, 256, 257, 1031)}
    for c in PC.of(PC.FINALIZE):
        r = PC.reference(c)
        if c.C >= 16:
            assert float(r["raw_var"][0]) < 0.0, c.name            # the column that clamps: scale = gamma / sqrt(eps)
            g0 = float(r["gamma"][0]) if c.affine else 1.0
            assert abs(float(r["out"]["scale"][0][0]) - g0 / PC.BN_EPS ** 0.5) <= 1e-12 * abs(g0) / PC.BN_EPS ** 0.5, c.name
    for c in PC.of(PC.ADD_RELU):
        if c.plain:
            continue
        r = PC.reference(c)
        neg = PC.negative_rows(c)
        assert bool((r["pre_relu"][neg] < 0).all()) and bool((r["out"]["out"][0][neg] == 0).all()), c.name
        assert bool((r["s1"] < 0).any()) or c.C == 4, c.name
    for c in PC.of(PC.BN1D):
        r = PC.reference(c)
        if c.mode != "eval" and (c.C >= 3 or c.B == 1):
            col = 1 if c.C >= 3 else 0
            assert torch.equal(r["out"]["y"][0][:, col], r["beta"].double()[col].expand(c.B)), c.name
    assert {1, 40, 41, 83} == {c.count for c in PC.of(PC.ADAM)} == {c.count for c in PC.of(PC.PACK)}
    for c in PC.of(PC.ADAM) + PC.of(PC.PACK):
        assert set(c.numel) - {0} <= set(PC.NUMELS), c.name
    assert set(PC.NUMELS) <= {n for c in PC.of(PC.ADAM) for n in c.numel}
    zeros = {i for c in PC.of(PC.ADAM) if c.count == 83 for i, n in enumerate(c.numel) if n == 0}
    assert {0, 40, 41, 82} <= zeros
    assert {(c.clip, c.write_grad) for c in PC.of(PC.ADAM)} >= {(0.5, 1), (0.5, 0), (0.0, 1), (0.0, 0)}
    assert {c.skip for c in PC.of(PC.ADAM)} == {"null", "zero", "set"}
    assert {c.tiles for c in PC.of(PC.FINALIZE)} == {1, 16, 17, 127, 128, 129, 256, 257, 512, 513, 1025}
    assert {c.C for c in PC.of(PC.FINALIZE)} == {1, 16, 17, 50, 96}
    assert {(c.affine, c.running) for c in PC.of(PC.FINALIZE)} == {(a, b) for a in (True, False) for b in (True, False)}
    # the rows past a grid cap are past it
    assert any(c.B * c.P > 512 * 256 for c in PC.of(PC.ATT)) and any(c.B * c.steps * c.P > 1024 * 256 for c in PC.of(PC.ATT))
    assert any(c.n > 4096 * 256 for c in PC.of(PC.CLAMP))
    assert any(c.rows * (c.C // 4) > 2 * 8192 * 256 for c in PC.of(PC.ADD_RELU))
    assert any(c.B * ((c.H - 1) // 2 + 1) * ((c.W - 1) // 2 + 1) * (c.C // 4) > 8192 * 256 for c in PC.of(PC.MAXPOOL))
    assert any(c.B * c.OUT * c.OUT * (c.C // 4) > 8192 * 256 for c in PC.of(PC.UPSAMPLE))
    # float4 kernels only on 16-B windows; every scalar entry also one float off
    for e in PC.ENTRIES:
        offs = {c.off for c in PC.of(e)}
        assert offs <= ({0, 4} if e in PC.FLOAT4 else {0, 1}), e
        if e not in (PC.ADAM, PC.PACK):                    # (those two put every tensor at both offsets inside each row)
            assert len(offs) == 2, e


def test_the_tie_rule_of_topk_counts_what_it_says():
    x = torch.tensor([[1.0, 2.0, 2.0, 2.0, 0.0]])
    assert PC.topk_count(x, torch.tensor([1]), 1) == 1     # nothing larger, no equal value in front
    assert PC.topk_count(x, torch.tensor([3]), 2) == 0     # two equal values with a lower index beat it
    assert PC.topk_count(x, torch.tensor([3]), 3) == 1
    assert PC.topk_count(x, torch.tensor([5]), 5) == 0     # a bad target counts nothing


# ---- host-side refusals: non-zero status and a message, before any device is touched ----

def refused(lib, status, who):
    msg = lib.capnet_last_error() or b""
    return status != 0 and who.encode() in msg


def test_bn_add_relu_refusals(lib):
    assert refused(lib, lib.capnet_bn_add_relu(Y, S1, T1, None, None, None, OUT, 3, 6, None), "bn_add_relu")       # C % 4
    assert refused(lib, lib.capnet_bn_add_relu(Y, S1, T1, X, S2, None, OUT, 3, 8, None), "bn_add_relu")            # s2 alone
    assert refused(lib, lib.capnet_bn_add_relu(Y, S1, T1, X, None, S2, OUT, 3, 8, None), "bn_add_relu")            # t2 alone


def test_bn_finalize_refusals(lib):
    args = lambda tiles, C, count: (X, Y, tiles, C, count, None, None, None, None, 0.1, 1e-5, S1, T1, None)
    for bad in ((0, 16, 7), (-1, 16, 7), (4, 0, 7), (4, -16, 7), (4, 16, 0), (4, 16, -7)):
        assert refused(lib, lib.capnet_bn_finalize(*args(*bad)), "bn_finalize"), bad


def test_clamp_refuses_lo_above_hi(lib):
    assert refused(lib, lib.capnet_clamp(X, 16, 0.5, -0.5, None), "clamp")


def test_clamp_adam_refuses_a_step_below_one(lib):
    ptrs = lambda a: (ctypes.c_void_p * 2)(a, a + 0x1000)
    numel = (ctypes.c_long * 2)(16, 16)
    for steps in ((0, 1), (-3, 1)):                        # the first tensor: the table is checked as it is filled
        st = (ctypes.c_int * 2)(*steps)
        assert refused(lib, lib.capnet_clamp_adam(2, ptrs(X), ptrs(Y), ptrs(S1), ptrs(T1), numel, st, 2e-4, 0.9, 0.999, 1e-8, 0.5,
                                                  1, None, None), "clamp_adam"), steps
    one = lambda a: (ctypes.c_void_p * 1)(a)
    assert refused(lib, lib.capnet_clamp_adam(1, one(X), one(Y), one(S1), one(T1), (ctypes.c_long * 1)(16), (ctypes.c_int * 1)(-2),
                                              2e-4, 0.9, 0.999, 1e-8, 0.5, 1, None, None), "clamp_adam")


def test_topk_correct_refuses_a_short_leading_dimension(lib):
    assert refused(lib, lib.capnet_topk_correct(X, 36, 4, 37, TGT, 5, OUT, ERR, None), "topk_correct")


def test_xent_refusals(lib):
    assert refused(lib, lib.capnet_xent_fwd(X, 37, 0, 37, TGT, Y, S1, T1, ERR, None), "xent_fwd")                  # N <= 0
    assert refused(lib, lib.capnet_xent_fwd(X, 37, -4, 37, TGT, Y, S1, T1, ERR, None), "xent_fwd")
    assert refused(lib, lib.capnet_xent_fwd(X, 36, 4, 37, TGT, Y, S1, T1, ERR, None), "xent_fwd")                  # ld < V
    assert refused(lib, lib.capnet_xent_bwd(X, 36, 4, 37, TGT, Y, S1, OUT, 37, None), "xent_bwd")                  # ld < V
    assert refused(lib, lib.capnet_xent_bwd(X, 37, 4, 37, TGT, Y, S1, OUT, 36, None), "xent_bwd")                  # ldd < V
