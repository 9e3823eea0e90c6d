"""tests/step_cases.py checked without a GPU: the rows are well-formed, every template arm the launchers can pick is hit
(asked of the library's own route queries, capnet_lstm_step_fused_route and capnet_stacked_decode_route, which the
launchers consume), the refusals are pinned as accepted / refused pairs, a plain float32 restatement of every row stays
inside the row's bounds (so the bounds can be met), and five deliberately wrong references land at least 10 bounds away
on every row they apply to (so the rows can see those classes of error)."""
import ctypes as C
import functools

import pytest
import torch

import capnet
import step_cases as SC


def _lib():
    return capnet.lib()


def fused_route(b, H):
    d = (C.c_int * 4)()
    return tuple(d) if _lib().capnet_lstm_step_fused_route(b, H, d) else None


def decode_route(E, H, xvec):
    d = (C.c_int * 2)()
    r = _lib().capnet_stacked_decode_route(E, H, int(xvec), d)
    return (("narrow", "wide")[r - 1],) + tuple(d) if r else None


def layer_routes(row):
    """(kind, NJ, TM, cell, gather) of every launch of a DECODE / WIDE row."""
    out = []
    for l in range(row.L):
        if l == 0:
            E = row.E + (SC.ATT_C if row.entry == SC.WIDE else 0)
            xvec = E % 4 == 0 and row.xoff == 0
        else:
            E, xvec = row.H, True
        r = decode_route(E, row.H, xvec)
        assert r is not None, (row, l)
        out.append(r + (row.cell, row.parents is not None))
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    row = SC.BY_NAME[name]
    inp = SC.inputs(row)
    return row, inp, SC.reference(row, inp)


def test_rows_are_well_formed():
    names = [r.name for r in SC.ROWS]
    assert len(set(names)) == len(names)
    for r in SC.ROWS:
        assert r.entry in SC.FAMILIES and r.cell in (0, 1)
    for r in SC.FUSED_ROWS:
        assert fused_route(r.b, r.H) is not None and r.gap in (0, 12)
    for r in SC.DECODE_ROWS + SC.WIDE_ROWS:
        assert 1 <= r.L <= 3 and r.groups in (1, 2, 3, 8) and r.groups * r.rpg <= 49, r
        assert r.centry in ("step", "cell", "gather", "groups", "tables") if r.entry == SC.DECODE else r.k <= 16
        if r.entry == SC.DECODE:
            assert (r.centry == "step") <= (r.cell == 0 and r.parents is None and r.groups == 1)
            assert (r.centry == "cell") <= (r.parents is None and r.groups == 1)
            assert (r.centry == "gather") <= (r.parents is not None and r.groups == 1)
            assert (r.centry == "tables") == (r.src == "tables")
    for r in SC.UPPER_ROWS:
        assert _lib().capnet_lstm_upper_step is not None and 1 <= r.b <= 16
    # every value the issue lists appears
    assert {r.H for r in SC.FUSED_ROWS} == {16, 48, 64, 96, 112, 144, 256, 272, 320, 512}
    assert {r.b for r in SC.FUSED_ROWS} == {1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64}
    assert {r.rpg for r in SC.DECODE_ROWS if r.groups == 1} >= {1, 15, 16, 17, 31, 32, 33, 48, 49}
    assert {r.rpg for r in SC.DECODE_ROWS if r.centry in ("groups", "tables")} == {1, 5, 16, 17, 33}
    assert {r.groups for r in SC.DECODE_ROWS} == {1, 2, 3, 8} and {r.L for r in SC.DECODE_ROWS} == {1, 2, 3}
    assert {r.parents for r in SC.DECODE_ROWS} == {None, "id", "perm", "repeat"}
    assert {r.rpg for r in SC.WIDE_ROWS} == {1, 16, 17, 33, 49} and {r.groups for r in SC.WIDE_ROWS} == {1, 2}
    assert {(r.H, r.b) for r in SC.UPPER_ROWS} >= {(64, 1), (128, 5), (256, 15), (512, 5), (1024, 16)}
    assert {r.H for r in SC.UPPER_ROWS} == {64, 128, 256, 512, 1024} and {r.b for r in SC.UPPER_ROWS} == {1, 5, 15, 16}
    for r in SC.DECODE_ROWS:                     # the parents are what the row says they are
        p = SC.inputs(r)["parents"] if r.H <= 128 else None
        if p is not None and r.parents == "perm":
            assert sorted(p.tolist()) == list(range(r.groups * r.rpg)) and (r.rpg == 1 or (p != torch.arange(len(p))).any())
        if p is not None and r.parents == "repeat" and r.rpg > 1:
            assert len(set(p.tolist())) < len(p)


def test_every_route_is_hit():
    want_fused = {(ngw, mt, halves, xcd, cell) for ngw in (1, 2, 4, 8) for mt, halves in ((1, 1), (2, 1), (2, 2))
                  for xcd in (0, 1) for cell in (0, 1)}
    # what the predicate admits, from the library itself: every b in 1..64 and H % 16 == 0 in 16..512
    admitted = {fused_route(b, H) for b in range(1, 65) for H in range(16, 513, 16)}
    assert {a + (c,) for a in admitted for c in (0, 1)} == want_fused
    hit = {}
    for r in SC.FUSED_ROWS:
        hit.setdefault(fused_route(r.b, r.H) + (r.cell,), []).append(r.name)
    assert set(hit) == want_fused, sorted(want_fused - set(hit))
    print("step_fused (NGW, MT, halves, xcd map, cell): %d arms, rows per arm %s" % (len(hit), sorted(len(v) for v in hit.values())))

    narrow = {("narrow", nj, 1 if nj == 16 else 2) for nj in (2, 4, 6, 8, 12, 16)}
    wide = {("wide", 12, 2), ("wide", 16, 2)}
    admitted = {decode_route(E, H, x) for H in (64, 128, 256, 512, 1024) for E in range(1, 4097) for x in (0, 1)} - {None}
    assert admitted == narrow | wide
    hit = {}
    for r in SC.DECODE_ROWS + SC.WIDE_ROWS:
        for lr in layer_routes(r):
            hit.setdefault(lr, []).append(r.name)
    want = {a + (c, g) for a in narrow | wide for c in (0, 1) for g in (False, True)}
    assert set(hit) == want, sorted(want - set(hit))
    for k in sorted(hit):
        print("decode %-6s NJ %2d TM %d cell %d gather %d: %d launches" % (k + (len(hit[k]),)))
    for r in SC.WIDE_ROWS:
        assert layer_routes(r)[0][0] == "wide"
    for r in SC.DECODE_ROWS:
        assert all(lr[0] == "narrow" for lr in layer_routes(r))
    # the scalar x path in both forms, and the vector path
    assert any(r.E % 4 and r.src == "rows" for r in SC.DECODE_ROWS) and any(r.E % 4 == 0 and r.xoff for r in SC.DECODE_ROWS)
    up = {(r.H, r.cell) for r in SC.UPPER_ROWS if not r.dropout}
    assert up == {(H, c) for H in (64, 128, 256, 512, 1024) for c in (0, 1)}
    print("upper step (H, cell): %d arms; dropout rows %d" % (len(up), sum(r.dropout for r in SC.UPPER_ROWS)))


def _host_pointer():
    """A 16-B aligned host address with 1 KiB behind it. It is never dereferenced: every call below is refused before any
    launch, and the accepted twin of a refusal is asked of the route queries only."""
    buf = (C.c_float * 264)()
    return buf, (C.addressof(buf) + 15) // 16 * 16


def test_refusals_in_pairs():
    L = _lib()
    err = lambda: L.capnet_last_error().decode()
    # step-fused: H % 16, H > 512, b > 64
    for ok, bad in (((1, 16), (1, 24)), ((64, 512), (64, 528)), ((64, 64), (65, 64)), ((1, 16), (0, 16))):
        assert fused_route(*ok) is not None and L.capnet_lstm_step_fused_supported(*ok) == 1
        assert fused_route(*bad) is None and L.capnet_lstm_step_fused_supported(*bad) == 0
    keep_alive, p = _host_pointer()
    assert L.capnet_lstm_step_fused(p, p, p, 4 * 24, p, p, p, 1, 24, 0, None) != 0 and "unsupported" in err()
    assert L.capnet_lstm_step_fused(p + 4, p, p, 64, p, p, p, 1, 16, 0, None) != 0 and "alignment" in err()
    assert L.capnet_lstm_step_fused(p, p + 4, p, 64, p, p, p, 1, 16, 0, None) != 0 and "alignment" in err()
    # decode: K > 2048 needs f32x4 rows; K > 4096 never
    assert decode_route(1984, 64, 0) == ("narrow", 16, 1) and decode_route(1985, 64, 0) is None
    assert decode_route(1988, 64, 1) == ("wide", 12, 2)
    assert decode_route(3072, 1024, 1) == ("wide", 16, 2) and decode_route(3073, 1024, 1) is None
    assert decode_route(12, 64, 0) is not None and decode_route(12, 96, 0) is None and decode_route(0, 64, 0) is None
    one = (C.c_void_p * 1)(p)

    def step(entry, **kw):
        d = dict(cell=0, L=1, groups=1, rpg=2, E=12, H=64, V=5, tok=None, x=p, w=one, b=one, sin=p, par=None, sout=p + 256, top=p,
                 err=p)
        d.update(kw)
        if entry == "gather":
            return L.capnet_stacked_decode_step_gather(d["cell"], d["L"], d["rpg"], d["E"], d["H"], d["V"], d["tok"], d["x"], d["w"],
                                                       d["b"], d["sin"], d["par"], d["sout"], d["top"], d["err"], None)
        f = L.capnet_stacked_decode_step_groups if entry == "groups" else L.capnet_stacked_decode_step_tables
        return f(d["cell"], d["L"], d["groups"], d["rpg"], d["E"], d["H"], d["V"], d["tok"], d["x"], d["w"], d["b"], d["sin"],
                 d["par"], d["sout"], d["top"], d["err"], None)

    # each refusal names its reason; its accepted twin differs in that one argument and is refused by nothing before
    # the launch (no device here: asked of the route query instead)
    assert step("gather", E=1985) != 0 and "unsupported" in err()
    assert step("gather", sout=p) != 0 and "must differ" in err()
    assert step("gather", sin=p + 4) != 0 and "alignment" in err()
    assert step("gather", sout=p + 260) != 0 and "alignment" in err()
    assert step("gather", w=(C.c_void_p * 1)(p + 4)) != 0 and "aligned" in err()
    assert step("gather", par=p, err=None) != 0 and "err_flag" in err()
    assert step("gather", tok=p, err=None) != 0 and "err_flag" in err()
    assert step("groups", groups=0) != 0 and "groups 0" in err()
    assert step("groups", groups=9) != 0 and "groups 9" in err()
    # tables stay on the narrow kernel: E + H <= 2048 is the entry's own bound (stacked_decode_supported)
    tabs = (C.c_void_p * 8)(*([p] * 8))
    assert step("tables", x=tabs, tok=p, E=1985) != 0 and "unsupported" in err()
    assert step("tables", x=tabs, tok=None) != 0 and "token ids" in err()
    assert step("tables", x=tabs, tok=p, groups=9) != 0 and "groups 9" in err()
    # the upper step: rows, hidden size, alignment
    up = lambda b, H, xin=p: L.capnet_lstm_upper_step(xin, p, p, p, p, p, p, p, p, p, b, H, 0, 0.0, 0, 1, 0, 0, None)
    assert up(17, 64) != 0 and "unsupported" in err()
    assert up(16, 96) != 0 and "unsupported" in err()
    assert up(16, 64, p + 4) != 0 and "alignment" in err()
    assert L.capnet_lstm_upper_step(p, p, p, p, p, p, p, p, p, p, 16, 64, 0, 0.0, 0, 1, 0, 2, None) != 0 and "cell" in err()


def _ratio(got, ref, bound, exact=True):
    """Worst |got - ref| / bound. A bound of 0 (df with c_prev NULL: the value is an exact 0) asks for equality."""
    assert torch.isfinite(got).all() and (bound >= 0).all()
    err = (got.double() - ref).abs()
    assert not exact or bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300)).max())


WORST32 = {}


@pytest.mark.parametrize("name", [r.name for r in SC.ROWS])
def test_float32_restatement_is_inside_the_bounds(name):
    row, inp, ref = _case(name)
    o32 = SC.oracle32(row, inp)
    for k, (r, bnd) in ref.items():
        assert r.shape == bnd.shape == o32[k].shape and torch.isfinite(r).all()
        q = _ratio(o32[k], r, bnd)
        WORST32[(row.entry, k)] = max(WORST32.get((row.entry, k), 0.0), q)
        assert q <= 1.0, (name, k, q)
    print("float32 restatement, worst error / bound so far on %s: %s" % (
        row.entry, "  ".join("%s %.3f" % (k, v) for (e, k), v in sorted(WORST32.items()) if e == row.entry)))


@pytest.mark.parametrize("wrong", SC.WRONG)
def test_wrong_references_are_far_outside(wrong):
    n, least = 0, None
    for row in SC.ROWS:
        if not SC.applies(row, wrong):
            continue
        _, inp, ref = _case(row.name)
        bad = SC.reference(row, inp, wrong=wrong)
        far = max(_ratio(bad[k][0], r, bnd, exact=False) for k, (r, bnd) in ref.items())
        assert far >= 10.0, (row.name, wrong, far)
        least = far if least is None else min(least, far)
        n += 1
    assert n > 0
    print("wrong reference %-7s: %d rows, the nearest lands %.0f bounds away" % (wrong, n, least))
