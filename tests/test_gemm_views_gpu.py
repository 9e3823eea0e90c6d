"""Every row of tests/gemm_cases.py on the device: the f32 GEMM family and its reducers on views into wider buffers
(padded leading dimensions, offset bases, strided batch members), against float64.

Inputs sit in buffers whose every float outside the operand's window is NaN -- padding columns, one slack row and more in
front and behind, the gaps between batch members, the floats in front of an offset base -- so a read outside the window
shows in the result. Outputs and workspaces sit in buffers filled with a sentinel bit pattern that must survive outside
the window. Per row: (1) |got - ref| <= 2e-6 (|A| . |B| + |bias| + |C0|) per element, (2) finite inside the window,
(3) nothing outside it changed, (4) counters back at zero, (5) bit identity with the same call on dense copies wherever
the dispatcher reports the same route and plan for both."""
import ctypes
import functools

import pytest
import torch

import gemm_cases as G
from capnet._lib import current_stream, lib
from helpers import SENTINEL, Window as FencedWindow

pytestmark = pytest.mark.gpu

BOUND = 2e-6
WS_TAIL = 64
WORST = {}                             # route -> worst |got - ref| / (BOUND * magnitude) seen so far


def note(route, ratio):
    WORST[route] = max(WORST.get(route, 0.0), ratio)


def report(routes):
    for r in sorted(routes):
        print("worst error / bound on %-16s %.3f" % (r, WORST[r]))


@functools.lru_cache(maxsize=None)
def problem(M, N, K, batch):
    """Logical operands of a shape, shared by every row that uses it: A [batch][M][K], B [batch][K][N], bias, C0, and the
    float64 product and magnitude."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + 7 * K + batch)
    A = torch.randn(batch, M, K, generator=g)
    B = torch.randn(batch, K, N, generator=g)
    bias = torch.randn(batch, N, generator=g)
    C0 = torch.randn(batch, M, N, generator=g)
    return A, B, bias, C0, A.double() @ B.double(), A.double().abs() @ B.double().abs()


def Window(values, view, dev, poison_bits=None):
    """values [batch][rows][cols] placed at (ld, off, stride) inside a flat device buffer with slack around it
    (helpers.Window with one whole row and more on either side)."""
    batch, rows, cols = values.shape
    ld, off, stride = view
    assert ld >= cols and (batch == 1 or stride >= cols)
    return FencedWindow(values, (stride, ld, 1), dev, off=off, pre=G.up4(ld) + 4, post=ld + 4, fill_bits=poison_bits)


def ws_used(case):
    if case.route in (G.SKINNY64, G.SKINNY128, G.KLOOP_SPLITK, G.B3_SPLITK) or (case.route == G.ROWS16 and case.splits > 1):
        return case.splits * case.M * case.N * case.batch
    return 0


def run(case, dev):
    """One call of the row's entry on the row's views. Returns (result [batch][M][N] on the CPU or None, route query,
    failures)."""
    L = lib()
    A, B, bias, C0, _, _ = problem(case.M, case.N, case.K, case.batch)
    va, vb, vc = G.resolved(case)
    wa = Window(A.transpose(1, 2) if case.ta else A, va, dev)
    wb = Window(B.transpose(1, 2) if case.tb else B, vb, dev)
    nan = torch.full_like(C0, float("nan"))
    slabs = case.entry in ("splitk_slabs", "rows16_slabs")
    wc = None if slabs else Window(C0 if case.accumulate else nan, vc, dev, SENTINEL)
    bvals = bias if case.sbias else bias[:1]
    wbias = Window(bvals.reshape(1, 1, -1), G.View(bvals.numel(), case.bias_off, 0), dev)
    ws = ctr = None
    if case.ws:
        ws = torch.full((case.ws + WS_TAIL,), SENTINEL, dtype=torch.int32, device=dev)
    if case.counters:
        ctr = torch.zeros(case.counters, dtype=torch.int32, device=dev)
    pws, pctr = (ws.data_ptr() if case.ws else None), (ctr.data_ptr() if case.counters else None)
    args = G.operand_args(case, wa.ptr, wb.ptr, wc.ptr if wc else None, wbias.ptr)
    s = current_stream()
    query, n_slabs = None, ctypes.c_int(-1)
    if case.entry == "sgemm":
        query = G.query_route(L, case, wa.ptr, wb.ptr, wc.ptr, wbias.ptr, pws, pctr)
        rc = L.capnet_sgemm(*args, case.force_tile, s)
    elif case.entry == "b3":
        rc = L.capnet_sgemm_b3(*args, pws, case.ws, s)
    elif case.entry == "splitk":
        assert case.batch == 1 and not case.counters
        query = G.query_route(L, case, wa.ptr, wb.ptr, wc.ptr, wbias.ptr, pws, pctr)
        rc = L.capnet_sgemm_splitk(*args[:13], pws, case.ws, s)
    elif case.entry == "fused":
        assert case.batch == 1
        query = G.query_route(L, case, wa.ptr, wb.ptr, wc.ptr, wbias.ptr, pws, pctr)
        rc = L.capnet_sgemm_splitk_fused(*args[:13], pws, case.ws, pctr, case.counters, s)
    elif case.entry == "batched":
        query = G.query_route(L, case, wa.ptr, wb.ptr, wc.ptr, wbias.ptr, pws, pctr)
        rc = L.capnet_sgemm_splitk_batched(*args, pws, case.ws, pctr, case.counters, s)
    else:
        fn = L.capnet_sgemm_splitk_slabs if case.entry == "splitk_slabs" else L.capnet_sgemm_rows16_slabs
        rc = fn(case.tb, case.M, case.N, case.K, wa.ptr, va.ld, wb.ptr, vb.ld, pws, case.ws, ctypes.byref(n_slabs), s)
    torch.cuda.synchronize()
    bad = []
    if rc != 0:
        return None, query, ["status %d: %s" % (rc, L.capnet_last_error())]
    if not (wa.unchanged() and wb.unchanged() and wbias.unchanged()):
        bad.append("an input changed")
    if slabs:
        if n_slabs.value != case.splits:
            return None, query, ["n_slabs %d, expected %d" % (n_slabs.value, case.splits)]
        used = case.splits * case.M * case.N
        got = ws[:used].view(torch.float32).view(case.splits, 1, case.M, case.N).sum(0).cpu() if used else None
        query = (case.route, [n_slabs.value])
    else:
        used = ws_used(case)
        got = wc.inside().cpu()
        if not wc.outside_unchanged():
            bad.append("C changed outside its window")
    if ws is not None and not bool((ws[used:] == SENTINEL).all()):
        bad.append("workspace written past its %d used floats" % used)
    if ctr is not None and int(ctr.abs().sum()) != 0:
        bad.append("counters not back at zero")
    return got, query, bad


def check_case(case, dev):
    got, query, bad = run(case, dev)
    if got is None:                                           # refused, or a slabs entry that rightly did nothing
        return bad
    A, B, bias, C0, prod, mag = problem(case.M, case.N, case.K, case.batch)
    ref, m = prod.clone(), mag.clone()
    slabs = case.entry in ("splitk_slabs", "rows16_slabs")
    if case.bias and not slabs:
        b = (bias if case.sbias else bias[:1].expand(case.batch, -1)).double()[:, None, :]
        ref, m = ref + b, m + b.abs()
    if case.accumulate and not slabs:
        ref, m = ref + C0.double(), m + C0.double().abs()
    if not bool(torch.isfinite(got).all()):
        bad.append("non-finite result (%d elements)" % int((~torch.isfinite(got)).sum()))
        return bad
    ratio = float(((got.double() - ref).abs() / (BOUND * m)).max())
    note(G.route_name(case.route), ratio)
    if ratio > 1.0:
        bad.append("error %.3f of the bound" % ratio)
    # the same product on dense copies: the same bits wherever the dispatcher plans it the same way
    d = G.dense(case)
    if case.entry == "b3" and any(x % 4 for x in (d.N,) + tuple(e[1] for e in G.extents(d.ta, d.tb, d.M, d.N, d.K))):
        return bad                          # gemm_b3 takes no dense copy of this row: its rows would not be 16-B
    got_d, query_d, bad_d = run(d, dev)
    if got_d is None:
        bad.append("dense call failed: %s" % bad_d)
    elif query is None or query == query_d:
        if not torch.equal(got.view(torch.int32), got_d.view(torch.int32)):
            bad.append("differs from the dense call (%d elements)" % int((got != got_d).sum()))
    return bad


def run_rows(rows, dev):
    failures = {}
    for case in rows:
        bad = check_case(case, dev)
        if bad:
            failures[case.name] = bad
    report({G.route_name(c.route) for c in rows if G.route_name(c.route) in WORST})
    assert not failures, (len(failures), list(failures.items())[:8])


@pytest.mark.parametrize("tile", [64, 128, 6432])
def test_generic_kernel_on_views(dev, tile):
    """gemm_f32_kernel at one tile: four layouts x (two vector, two scalar loader forms) x five ragged shapes x four
    epilogues, and the batched rows."""
    run_rows([c for c in G.GENERIC if c.force_tile == tile], dev)


def test_auto_routing_and_b3_on_views(dev):
    run_rows(G.AUTO, dev)


@pytest.mark.parametrize("group", ["rows16", "skinny", "deny", "fell", "kloop", "b3-splitk"])
def test_splitk_family_on_views(dev, group):
    rows = [c for c in G.SPLITK if c.name.startswith(group)]
    assert rows
    run_rows(rows, dev)


def test_groups_cover_the_splitk_rows():
    groups = ("rows16", "skinny", "deny", "fell", "kloop", "b3-splitk")
    assert all(sum(c.name.startswith(g) for g in groups) == 1 for c in G.SPLITK)


def test_slabs_entries_on_views(dev):
    """capnet_sgemm_splitk_slabs / capnet_sgemm_rows16_slabs: the slabs sum to the product; a shape that does not qualify
    reports no slabs and leaves the workspace untouched (run() checks it past the used floats: all of it)."""
    run_rows(G.SLABS, dev)


def reduce_ref32(slab, bias, out0):
    """(((0 + v0) + v1) ...) + bias, then out + that, in fp32 on the CPU."""
    s = torch.zeros_like(slab[0])
    for v in slab:
        s = s + v
    if bias is not None:
        s = s + bias
    return s if out0 is None else out0 + s


@pytest.mark.parametrize("count,M,N,ldc", G.REDUCE)
def test_reduce_slabs_is_a_fixed_order_fp32_sum(dev, count, M, N, ldc):
    L = lib()
    g = torch.Generator().manual_seed(count * 31 + N)
    slab = torch.randn(count, M, N, generator=g)
    bias = torch.randn(N, generator=g)
    out0 = torch.randn(1, M, N, generator=g)
    slab_d, bias_d = slab.to(dev), bias.to(dev)
    for use_bias, acc in G.EPILOGUES:
        wc = Window(out0 if acc else torch.full_like(out0, float("nan")), G.View(ldc, 0, M * ldc), dev, SENTINEL)
        rc = L.capnet_reduce_slabs(slab_d.data_ptr(), count, M, N, wc.ptr, ldc, bias_d.data_ptr() if use_bias else None,
                                   int(acc), current_stream())
        assert rc == 0, L.capnet_last_error()
        torch.cuda.synchronize()
        want = reduce_ref32(slab, bias if use_bias else None, out0[0] if acc else None)
        assert torch.equal(wc.inside().cpu()[0].view(torch.int32), want.view(torch.int32)), (use_bias, acc)
        assert wc.outside_unchanged()


def colsum_ref32(x, r0, r1):
    """colsum_kernel's order: row lane l of 32 sums rows r0 + l, r0 + l + 32, ... ; the lanes are then added 0, 1, ... 31."""
    acc = torch.zeros(32, x.shape[1])
    for base in range(r0, r1, 32):
        blk = x[base:min(base + 32, r1)]
        acc[:len(blk)] = acc[:len(blk)] + blk
    t = torch.zeros(x.shape[1])
    for k in range(32):
        t = t + acc[k]
    return t


@pytest.mark.parametrize("rows,C,ld,ws_floats", G.COLSUM)
def test_colsum_on_views(dev, rows, C, ld, ws_floats):
    L = lib()
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(1, rows, C, generator=g)
    out0 = torch.randn(1, 1, C, generator=g)
    wx = Window(x, G.View(ld, 0, rows * ld), dev)
    chunked = ws_floats >= 4 * C and rows > 4096
    for acc in (False, True):
        wo = Window(out0 if acc else torch.full_like(out0, float("nan")), G.View(C, 0, C), dev, SENTINEL)
        ws = torch.full((ws_floats + WS_TAIL,), SENTINEL, dtype=torch.int32, device=dev)
        rc = L.capnet_colsum_ws(wx.ptr, ld, rows, C, wo.ptr, int(acc), ws.data_ptr() if ws_floats else None, ws_floats,
                                current_stream())
        assert rc == 0, L.capnet_last_error()
        torch.cuda.synchronize()
        got = wo.inside().cpu().view(-1)
        mag = x[0].double().abs().sum(0) + (out0.view(-1).double().abs() if acc else 0)
        ref = x[0].double().sum(0) + (out0.view(-1).double() if acc else 0)
        assert bool(torch.isfinite(got).all())
        ratio = float(((got.double() - ref).abs() / (BOUND * mag)).max())
        note("colsum", ratio)
        assert ratio <= 1.0, ratio
        if chunked:     # four chunks of 1250 rows, added by the slab reducer in chunk order
            parts = torch.stack([colsum_ref32(x[0], r0, min(rows, r0 + 1250)) for r0 in range(0, rows, 1250)])
            want = reduce_ref32(parts, None, out0.view(-1) if acc else None)
            used = 4 * C
        else:
            t = colsum_ref32(x[0], 0, rows)
            want = out0.view(-1) + t if acc else t
            used = 0
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), int((got != want).sum())
        assert wo.outside_unchanged() and wx.unchanged()
        assert bool((ws[used:] == SENTINEL).all())
    report({"colsum"})


def test_new_entries_refuse_bad_arguments_and_write_nothing(dev):
    L = lib()
    s = current_stream()
    M, N, K = 16, 68, 260
    z = torch.zeros(1, M, K), torch.zeros(1, N, K), torch.zeros(1, M, N)
    wa, wb = Window(z[0], G.View(K, 0, 0), dev), Window(z[1], G.View(K, 0, 0), dev)
    wc = Window(z[2], G.View(N, 0, 0), dev, SENTINEL)
    ws = torch.full((1 << 16,), SENTINEL, dtype=torch.int32, device=dev)
    ctr = torch.zeros(16, dtype=torch.int32, device=dev)
    n = ctypes.c_int(-7)
    pa, pb, pc, pw, pk = wa.ptr, wb.ptr, wc.ptr, ws.data_ptr(), ctr.data_ptr()
    refused = [
        ("bad argument", L.capnet_sgemm_splitk_batched, (0, 1, -1, N, K, pa, K, pb, K, pc, N, None, 0, 1, 0, 0, 0, 0, pw, 1 << 16,
                                                          pk, 16, s)),
        ("bad argument", L.capnet_sgemm_splitk_batched, (0, 1, M, N, K, None, K, pb, K, pc, N, None, 0, 1, 0, 0, 0, 0, pw, 1 << 16,
                                                          pk, 16, s)),
        ("leading dimension too small", L.capnet_sgemm_splitk_batched, (0, 1, M, N, K, pa, K - 4, pb, K, pc, N, None, 0, 1, 0, 0,
                                                                         0, 0, pw, 1 << 16, pk, 16, s)),
        ("leading dimension too small", L.capnet_sgemm_splitk_batched, (0, 1, M, N, K, pa, K, pb, K, pc, N - 4, None, 0, 1, 0, 0,
                                                                         0, 0, pw, 1 << 16, pk, 16, s)),
        ("bad argument", L.capnet_sgemm_splitk_slabs, (1, M, N, K, pa, K, None, K, pw, 1 << 16, ctypes.byref(n), s)),
        ("bad argument", L.capnet_sgemm_splitk_slabs, (1, M, N, K, pa, K, pb, K, pw, 1 << 16, None, s)),
        ("leading dimension too small", L.capnet_sgemm_splitk_slabs, (1, M, N, K, pa, K, pb, K - 4, pw, 1 << 16, ctypes.byref(n), s)),
        ("bad argument", L.capnet_sgemm_rows16_slabs, (1, M, -N, K, pa, K, pb, K, pw, 1 << 16, ctypes.byref(n), s)),
        ("leading dimension too small", L.capnet_sgemm_rows16_slabs, (1, M, N, K, pa, K - 4, pb, K, pw, 1 << 16, ctypes.byref(n), s)),
        ("bad argument", L.capnet_reduce_slabs, (pw, 0, M, N, pc, N, None, 0, s)),
        ("bad argument", L.capnet_reduce_slabs, (None, 2, M, N, pc, N, None, 0, s)),
        ("leading dimension too small", L.capnet_reduce_slabs, (pw, 2, M, N, pc, N - 1, None, 0, s)),
        ("bad argument", L.capnet_colsum_ws, (pa, K, M, 0, pc, 0, pw, 1 << 16, s)),
        ("bad argument", L.capnet_colsum_ws, (pa, K, M, K, None, 0, pw, 1 << 16, s)),
        ("leading dimension too small", L.capnet_colsum_ws, (pa, K - 1, M, K, pc, 0, pw, 1 << 16, s)),
    ]
    for what, fn, a in refused:
        assert fn(*a) != 0, (what, fn.__name__)
        assert what.encode() in L.capnet_last_error(), (what, L.capnet_last_error())
    torch.cuda.synchronize()
    assert n.value == -7
    assert torch.equal(wc.buf.view(torch.int32), wc.before.view(torch.int32))
    assert bool((ws == SENTINEL).all()) and int(ctr.abs().sum()) == 0
