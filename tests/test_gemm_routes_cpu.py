"""Which kernel the f32 GEMM family gives each row of tests/gemm_cases.py, asked of the dispatchers' own plan functions
(capnet_sgemm_route, capnet_sgemm_splitk_route: host code, no device). The expected routes in the table are written by
hand from the conditions in csrc/gemm_f32.hip, gemm_dma.hip and gemm_b3.hip; a changed threshold fails here."""
import ctypes

import pytest

import capnet
import gemm_cases as G

# plain integers as addresses: 16-B aligned bases, the row's offsets in floats added
PA, PB, PC, PBIAS, PWS, PCTR = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000


def addresses(case):
    return (PA + 4 * case.a.off, PB + 4 * case.b.off, PC + 4 * case.c.off, PBIAS + 4 * case.bias_off, PWS, PCTR)


ROUTED = [c for c in G.CASES if c.entry in ("sgemm", "splitk", "fused", "batched")]


@pytest.fixture(scope="module")
def lib():
    return capnet.lib()


def test_every_row_takes_the_route_the_table_names(lib):
    wrong = []
    for case in ROUTED:
        route, detail = G.query_route(lib, case, *addresses(case))
        if route != case.route or detail[0] != case.loader:
            wrong.append((case.name, "route", G.route_name(route) if route >= 0 else route, "loader", detail[0], "expected",
                          G.route_name(case.route), case.loader, lib.capnet_last_error()))
        elif not route & G.FELL and route in (G.ROWS16, G.SKINNY64, G.SKINNY128, G.KLOOP_SPLITK, G.B3_SPLITK):
            if detail[1:3] != [case.splits, case.chunk]:
                wrong.append((case.name, "splits, chunk", detail[1:3], "expected", [case.splits, case.chunk]))
    assert not wrong, wrong[:10]


def test_tile_counts_reported(lib):
    by_name = {c.name: c for c in ROUTED}
    expect = {"generic64-01-67x130x35-vec0-b1a0": 2 * 3, "generic128-10-129x66x15-odd-b0a1": 2 * 1,
              "generic6432-11-65x33x17-off1-b1a1": 2 * 1, "auto-nt_dma-lda=K": 2 * 32, "auto-b3-01": 12 * 16,
              "auto-tile128": 16 * 24, "rows16-16x8192x1028-tb1": 128, "skinny-128x4096x256-tb0": 2 * 64,
              "skinny-batch4-17x68x132-tb1": 2 * 4, "kloop-splitk-10-vec": 3 * 2, "b3-splitk-00": 2 * 8}
    for name, tiles in expect.items():
        _, detail = G.query_route(lib, by_name[name], *addresses(by_name[name]))
        assert detail[3] == tiles, (name, detail)


def test_direct_b3_rows_are_eligible(lib):
    rows = [c for c in G.CASES if c.entry == "b3"]
    assert rows
    for case in rows:
        a = G.operand_args(case, *addresses(case)[:4])
        assert lib.capnet_sgemm_b3_eligible(*a[:12], *a[13:]) == 1, case.name


def test_table_covers_every_route_layout_and_loader_form():
    have = {(c.route, c.ta, c.tb, c.loader) for c in ROUTED}
    assert not G.REQUIRED - have, sorted(G.REQUIRED - have)
    # the generic kernel: every tile x layout x loader form on every shape and epilogue of the issue
    for tile, route in G.GENERIC_ROUTE.items():
        for ta, tb in G.LAYOUTS:
            for shape in G.GENERIC_SHAPES:
                for form in ("vec0", "vec4", "odd", "off1"):
                    for bias, acc in G.EPILOGUES:
                        n = "generic%d-%d%d-%dx%dx%d-%s-b%da%d" % ((tile, ta, tb) + shape + (form, bias, acc))
                        assert any(c.name == n and c.route == route for c in G.GENERIC), n


def test_planners_agree_on_rows_that_fall_through(lib):
    fell = [c for c in ROUTED if c.route & G.FELL]
    assert len(fell) >= 10
    for case in fell:
        route, detail = G.query_route(lib, case, *addresses(case))
        assert route & G.FELL, case.name
        direct = case._replace(entry="sgemm", force_tile=0)
        r2, d2 = G.query_route(lib, direct, *addresses(direct))
        assert (route & ~G.FELL, detail) == (r2, d2), case.name


def test_route_queries_refuse_what_the_calls_refuse(lib):
    d = (ctypes.c_int * 4)()
    assert lib.capnet_sgemm_route(0, 0, -1, 4, 4, PA, 4, PB, 4, PC, 4, None, 0, 1, 0, 0, 0, 0, 0, d) < 0
    assert b"negative" in lib.capnet_last_error()
    assert lib.capnet_sgemm_route(0, 0, 4, 4, 4, PA, 3, PB, 4, PC, 4, None, 0, 1, 0, 0, 0, 0, 0, d) < 0
    assert b"leading dimension too small" in lib.capnet_last_error()
    assert lib.capnet_sgemm_route(0, 0, 4, 4, 4, PA, 4, PB, 4, PC, 4, None, 0, 1, 0, 0, 0, 0, 96, d) < 0
    assert b"unknown tile" in lib.capnet_last_error()
    assert lib.capnet_sgemm_route(0, 0, 0, 4, 4, None, 4, None, 4, None, 4, None, 0, 1, 0, 0, 0, 0, 0, None) == G.NONE
    # the split-K entry hands a bad product to sgemm, whose refusal it returns
    assert lib.capnet_sgemm_splitk_route(0, 0, 4, 4, 4, PA, 3, PB, 4, PC, 4, None, 0, 1, 0, 0, 0, 0, None, 0, None, 0, d) < 0
    assert lib.capnet_sgemm_splitk_route(0, 1, 17, 68, 132, PA, 132, None, 132, PC, 68, None, 0, 1, 0, 0, 0, 0, PWS, 1 << 20,
                                         None, 0, d) < 0
    assert b"null operand" in lib.capnet_last_error()
