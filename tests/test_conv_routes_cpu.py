"""The host-side decisions of the convolution family, asked of the library without a device: the eligibility predicates
(capnet_conv_v2_eligible ... capnet_conv_stem_f16x3_eligible, the functions the launchers and the trunk apply) at their
limits, and the tile / slab / statistics-row counts of every row of tests/conv_cases.py.

Every limit is a hand-written pair: a row the predicate accepts AT the limit and one it refuses just past it. A changed
limit fails here; so does a row of the GPU table that its kernel would refuse."""
import ctypes

import pytest

import capnet
import conv_cases as CC

X, S1, T1, RES = 0x100000, 0x200000, 0x300000, 0x400000        # plain integers as addresses, 16-B aligned


@pytest.fixture(scope="module")
def lib():
    return capnet.lib()


def dense(B, H, W, Cin):
    return (H * W * Cin, W * Cin, Cin, 1)


def check_pairs(fn, pairs):
    wrong = []
    for what, ok, no in pairs:
        if fn(*ok) != 1:
            wrong.append((what, "refused at the limit", ok))
        if fn(*no) != 0:
            wrong.append((what, "accepted past the limit", no))
    assert not wrong, wrong


def test_conv_v2_eligible_limits(lib):
    # (x, sxb, sxh, sxw, sxc, B, Cin, Cout, in_scale, in_shift)
    check_pairs(lib.capnet_conv_v2_eligible, [
        ("base off by 4 bytes", (X, 1568, 224, 32, 1, 2, 32, 64, None, None), (X + 4, 1568, 224, 32, 1, 2, 32, 64, None, None)),
        ("pixel stride % 4", (X, 1800, 256, 36, 1, 2, 32, 64, None, None), (X, 1800, 256, 34, 1, 2, 32, 64, None, None)),
        ("row stride % 4", (X, 1800, 228, 32, 1, 2, 32, 64, None, None), (X, 1800, 226, 32, 1, 2, 32, 64, None, None)),
        ("image stride % 4", (X, 1572, 224, 32, 1, 2, 32, 64, None, None), (X, 1570, 224, 32, 1, 2, 32, 64, None, None)),
        ("channel stride 1", (X, 1568, 224, 32, 1, 2, 32, 64, None, None), (X, 1568, 224, 32, 2, 2, 32, 64, None, None)),
        ("Cin % 16", (X, 784, 112, 16, 1, 2, 16, 64, None, None), (X, 1176, 168, 24, 1, 2, 24, 64, None, None)),
        ("Cout % 64", (X, 1568, 224, 32, 1, 2, 32, 128, None, None), (X, 1568, 224, 32, 1, 2, 32, 96, None, None)),
        ("fold vectors 16-B aligned", (X, 1568, 224, 32, 1, 2, 32, 64, S1, T1), (X, 1568, 224, 32, 1, 2, 32, 64, S1 + 4, T1)),
        ("fold shift 16-B aligned", (X, 1568, 224, 32, 1, 2, 32, 64, S1, T1), (X, 1568, 224, 32, 1, 2, 32, 64, S1, T1 + 8)),
        ("2^31 bytes of input", (X, 2 ** 28 - 4, 224, 32, 1, 2, 32, 64, None, None), (X, 2 ** 28, 224, 32, 1, 2, 32, 64, None, None)),
    ])


def test_conv1x1_dma_eligible_limits(lib):
    # (x, sxb, sxh, sxw, sxc, B, H, W, Cin, Cout, stride)
    check_pairs(lib.capnet_conv1x1_dma_eligible, [
        ("base off by 4 bytes", (X, 784, 112, 16, 1, 2, 7, 7, 16, 64, 1), (X + 4, 784, 112, 16, 1, 2, 7, 7, 16, 64, 1)),
        ("pixel stride % 4", (X, 1000, 140, 20, 1, 2, 7, 7, 16, 64, 1), (X, 1000, 140, 18, 1, 2, 7, 7, 16, 64, 1)),
        ("row stride % 4", (X, 1000, 116, 16, 1, 2, 7, 7, 16, 64, 1), (X, 1000, 114, 16, 1, 2, 7, 7, 16, 64, 1)),
        ("image stride % 4", (X, 788, 112, 16, 1, 2, 7, 7, 16, 64, 1), (X, 786, 112, 16, 1, 2, 7, 7, 16, 64, 1)),
        ("Cin % 16", (X, 784, 112, 16, 1, 2, 7, 7, 16, 64, 2), (X, 1176, 168, 24, 1, 2, 7, 7, 24, 64, 2)),
        ("Cout % 64", (X, 784, 112, 16, 1, 2, 7, 7, 16, 192, 1), (X, 784, 112, 16, 1, 2, 7, 7, 16, 96, 1)),
        ("2^32 bytes of input", (X, 2 ** 29 - 4, 112, 16, 1, 2, 7, 7, 16, 64, 1), (X, 2 ** 29, 112, 16, 1, 2, 7, 7, 16, 64, 1)),
        # 2^24 - 1 / 2^24 images of one pixel (the predicate does not ask for dense strides: the images overlap)
        ("2^24 rows", (X, 4, 16, 16, 1, 2 ** 24 - 1, 1, 1, 16, 64, 1), (X, 4, 16, 16, 1, 2 ** 24, 1, 1, 16, 64, 1)),
        ("2^32 bytes of output", (X, 4, 16, 16, 1, 2 ** 23 - 1, 1, 1, 16, 128, 1), (X, 4, 16, 16, 1, 2 ** 23, 1, 1, 16, 128, 1)),
    ])


def test_conv_f16x3_eligible_limits(lib):
    # (x, sxb, sxh, sxw, sxc, B, H, W, Cin, Cout, k, stride, pad, in_scale, in_shift)
    d64, d96 = dense(2, 7, 7, 64), dense(2, 7, 7, 96)
    check_pairs(lib.capnet_conv_f16x3_eligible, [
        ("base off by 4 bytes", (X,) + d64 + (2, 7, 7, 64, 64, 3, 1, 1, None, None), (X + 4,) + d64 + (2, 7, 7, 64, 64, 3, 1, 1, None, None)),
        ("pixel stride % 4", (X, 4000, 520, 72, 1, 2, 7, 7, 64, 64, 3, 1, 1, None, None),
         (X, 4000, 520, 70, 1, 2, 7, 7, 64, 64, 3, 1, 1, None, None)),
        ("row stride % 4", (X, 4000, 460, 64, 1, 2, 7, 7, 64, 64, 3, 1, 1, None, None),
         (X, 4000, 462, 64, 1, 2, 7, 7, 64, 64, 3, 1, 1, None, None)),
        ("image stride % 4", (X, 3156, 448, 64, 1, 2, 7, 7, 64, 64, 1, 1, 0, None, None),
         (X, 3158, 448, 64, 1, 2, 7, 7, 64, 64, 1, 1, 0, None, None)),
        ("Cin % 64", (X,) + d64 + (2, 7, 7, 64, 64, 1, 1, 0, None, None), (X,) + d96 + (2, 7, 7, 96, 64, 1, 1, 0, None, None)),
        ("Cout % 64", (X,) + d64 + (2, 7, 7, 64, 128, 1, 2, 0, None, None), (X,) + d64 + (2, 7, 7, 64, 96, 1, 2, 0, None, None)),
        ("k = 3 comes with pad 1", (X,) + d64 + (2, 7, 7, 64, 64, 3, 2, 1, None, None), (X,) + d64 + (2, 7, 7, 64, 64, 3, 2, 0, None, None)),
        ("k = 1 comes with pad 0", (X,) + d64 + (2, 7, 7, 64, 64, 1, 1, 0, None, None), (X,) + d64 + (2, 7, 7, 64, 64, 1, 1, 1, None, None)),
        ("folded Cin <= 512 (kFoldMaxH)", (X,) + dense(2, 7, 7, 512) + (2, 7, 7, 512, 64, 1, 1, 0, S1, T1),
         (X,) + dense(2, 7, 7, 576) + (2, 7, 7, 576, 64, 1, 1, 0, S1, T1)),
        ("Cin 576 without a fold", (X,) + dense(2, 7, 7, 576) + (2, 7, 7, 576, 64, 1, 1, 0, None, None),
         (X,) + dense(2, 7, 7, 608) + (2, 7, 7, 608, 64, 1, 1, 0, None, None)),
        ("fold vectors 16-B aligned", (X,) + d64 + (2, 7, 7, 64, 64, 3, 1, 1, S1, T1), (X,) + d64 + (2, 7, 7, 64, 64, 3, 1, 1, S1, T1 + 4)),
        ("2^31 bytes of input", (X, 2 ** 28 - 4, 448, 64, 1, 2, 7, 7, 64, 64, 3, 1, 1, None, None),
         (X, 2 ** 28, 448, 64, 1, 2, 7, 7, 64, 64, 3, 1, 1, None, None)),
        ("2^24 rows", (X, 4, 64, 64, 1, 2 ** 24 - 1, 1, 1, 64, 64, 1, 1, 0, None, None),
         (X, 4, 64, 64, 1, 2 ** 24, 1, 1, 64, 64, 1, 1, 0, None, None)),
        ("2^32 bytes of output", (X, 4, 64, 64, 1, 2 ** 23 - 1, 1, 1, 64, 128, 1, 1, 0, None, None),
         (X, 4, 64, 64, 1, 2 ** 23, 1, 1, 64, 128, 1, 1, 0, None, None)),
    ])


def test_conv3x3_patch_eligible_limits(lib):
    # (x, sxb, sxh, sxw, sxc, B, H, W, Cin, Cout, k, stride, pad, in_scale, in_shift)
    def a(B, H, W, Cin, Cout, x=X, k=3, stride=1, pad=1, s=None, t=None, st=None):
        return (x,) + (st or dense(B, H, W, Cin)) + (B, H, W, Cin, Cout, k, stride, pad, s, t)
    check_pairs(lib.capnet_conv3x3_patch_eligible, [
        ("base off by 4 bytes", a(2, 7, 7, 32, 64), a(2, 7, 7, 32, 64, x=X + 4)),
        ("W <= 59 (128 + 2 W + 2 <= 248 patch pixels)", a(1, 3, 59, 32, 64), a(1, 3, 60, 32, 64)),
        ("W >= 3", a(2, 3, 3, 32, 64), a(2, 3, 2, 32, 64)),
        ("H >= 3", a(2, 3, 3, 32, 64), a(2, 2, 3, 32, 64)),
        ("Cin % 32", a(2, 7, 7, 32, 64), a(2, 7, 7, 48, 64)),
        ("Cout % 64", a(2, 7, 7, 32, 128), a(2, 7, 7, 32, 96)),
        ("stride 1 only", a(2, 7, 7, 32, 64), a(2, 7, 7, 32, 64, stride=2)),
        ("3x3 only", a(2, 7, 7, 32, 64), a(2, 7, 7, 32, 64, k=1, pad=0)),
        ("dense pixels", a(2, 7, 7, 32, 64), a(2, 7, 7, 32, 64, st=(7 * 7 * 40, 7 * 40, 40, 1))),
        ("dense rows", a(2, 7, 7, 32, 64), a(2, 7, 7, 32, 64, st=(7 * 236, 236, 32, 1))),
        ("dense images", a(2, 7, 7, 32, 64), a(2, 7, 7, 32, 64, st=(1568 + 20, 224, 32, 1))),
        ("fold vectors 16-B aligned", a(2, 7, 7, 32, 64, s=S1, t=T1), a(2, 7, 7, 32, 64, s=S1 + 4, t=T1)),
        ("2^24 rows", a(2 ** 20 - 1, 4, 4, 32, 64), a(2 ** 20, 4, 4, 32, 64)),
        ("2^31 elements of the larger tensor", a(2 ** 19 - 1, 4, 4, 32, 256), a(2 ** 19, 4, 4, 32, 256)),
    ])


def test_conv1x1_areg_eligible_limits(lib):
    # (x, M, Cin, Cout, bn, in_scale, in_shift)
    check_pairs(lib.capnet_conv1x1_areg_eligible, [
        ("base off by 4 bytes", (X, 300, 64, 64, 64, None, None), (X + 4, 300, 64, 64, 64, None, None)),
        ("Cin 256 is the largest", (X, 300, 256, 128, 128, None, None), (X, 300, 512, 128, 128, None, None)),
        ("Cin 64 / 128 / 256 only", (X, 300, 128, 128, 128, None, None), (X, 300, 96, 128, 128, None, None)),
        ("tile width 64 / 128", (X, 300, 64, 256, 128, None, None), (X, 300, 64, 256, 256, None, None)),
        ("Cout % bn", (X, 300, 64, 192, 64, None, None), (X, 300, 64, 192, 128, None, None)),
        ("at least one row", (X, 1, 64, 64, 64, None, None), (X, 0, 64, 64, 64, None, None)),
        ("fold vectors 16-B aligned", (X, 300, 64, 64, 64, S1, T1), (X, 300, 64, 64, 64, S1, T1 + 4)),
        ("2^24 rows", (X, 2 ** 24 - 1, 64, 64, 64, None, None), (X, 2 ** 24, 64, 64, 64, None, None)),
        ("2^31 elements of the larger tensor", (X, 2 ** 23 - 1, 256, 128, 128, None, None), (X, 2 ** 23, 256, 128, 128, None, None)),
    ])


def test_conv1x1_tail_eligible_limits(lib):
    # (y3, res, M, Cin, Cout)
    check_pairs(lib.capnet_conv1x1_tail_eligible, [
        ("y3 off by 4 bytes", (X, RES, 300, 64, 64), (X + 4, RES, 300, 64, 64)),
        ("identity off by 4 bytes", (X, RES, 300, 64, 64), (X, RES + 4, 300, 64, 64)),
        ("Cin / 32 a power of two", (X, RES, 300, 128, 64), (X, RES, 300, 96, 64)),
        ("Cin 32 is the smallest", (X, RES, 300, 32, 64), (X, RES, 300, 16, 64)),
        ("Cin 2048 / 1536", (X, RES, 300, 2048, 64), (X, RES, 300, 1536, 64)),
        ("Cout % 64", (X, RES, 300, 64, 192), (X, RES, 300, 64, 96)),
        ("at least one row", (X, RES, 1, 64, 64), (X, RES, 0, 64, 64)),
        ("2^24 rows", (X, RES, 2 ** 24 - 1, 32, 64), (X, RES, 2 ** 24, 32, 64)),
        ("2^31 elements of the larger tensor", (X, RES, 2 ** 22 - 1, 512, 256), (X, RES, 2 ** 22, 512, 256)),
    ])


def test_conv_stem_f16x3_eligible_limits(lib):
    # (x, sxb, sxc, sxh, sxw, B, H, W, Cin, Cout, k, stride, pad)
    def a(B, H, W, x=X, st=None, sxw=1, Cin=3, Cout=64, k=7, stride=2, pad=3):
        sxb, sxc, sxh = st or (3 * H * W, H * W, W)
        return (x, sxb, sxc, sxh, sxw, B, H, W, Cin, Cout, k, stride, pad)
    check_pairs(lib.capnet_conv_stem_f16x3_eligible, [
        ("base off by 4 bytes", a(2, 7, 8), a(2, 7, 8, x=X + 4)),
        ("W % 4", a(2, 7, 12), a(2, 7, 10, st=(3 * 7 * 12, 7 * 12, 12))),
        ("H >= 7", a(2, 7, 8), a(2, 6, 8)),
        ("W >= 8", a(2, 7, 8), a(2, 7, 4)),
        ("unit stride along W", a(2, 7, 8), a(2, 7, 8, sxw=2)),
        ("row stride % 4", a(2, 7, 8, st=(3 * 7 * 12, 7 * 12, 12)), a(2, 7, 8, st=(3 * 7 * 12, 7 * 12, 10))),
        ("channel stride % 4", a(2, 7, 8, st=(3 * 60, 60, 8)), a(2, 7, 8, st=(3 * 60, 58, 8))),
        ("image stride % 4", a(2, 7, 8, st=(172, 56, 8)), a(2, 7, 8, st=(170, 56, 8))),
        ("the 7x7 / 2 / pad 3 stem only", a(2, 7, 8), a(2, 7, 8, k=3, pad=1)),
        ("3 -> 64 channels only", a(2, 7, 8), a(2, 7, 8, Cin=4)),
        ("2^31 floats of input", a(2, 7, 8, st=(2 ** 30 - 4, 56, 8)), a(2, 7, 8, st=(2 ** 30, 56, 8))),
        # (the limit of 2^24 segments cannot be met: at the narrowest map, 4 outputs a row, 2^23 segments already fill
        #  the 2^31 output elements)
        ("2^31 elements of output", a(2 ** 21 - 1, 7, 8), a(2 ** 21, 7, 8)),
    ])


# ---- the table itself ----

def eligible(lib, c):
    """What the row's own launcher asks of the row's operand on the row's view."""
    sxb, sxh, sxw, sxc = CC.strides(c)
    s, t = (S1, T1) if c.pre else (None, None)
    M = CC.rows_m(c)
    if c.kernel == CC.GENERIC:
        return 1                                       # the generic kernel takes every operand
    if c.kernel == CC.KMAJOR:
        return lib.capnet_conv_v2_eligible(X, sxb, sxh, sxw, sxc, c.B, c.Cin, c.Cout, s, t) and M < 2 ** 24
    if c.kernel == CC.DMA:
        return lib.capnet_conv1x1_dma_eligible(X, sxb, sxh, sxw, sxc, c.B, c.H, c.W, c.Cin, c.Cout, c.stride)
    if c.kernel in (CC.H3_1X1, CC.H3, CC.H3_SCALED):
        return lib.capnet_conv_f16x3_eligible(X, sxb, sxh, sxw, sxc, c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, c.pad, s, t)
    if c.kernel == CC.PATCH:
        return lib.capnet_conv3x3_patch_eligible(X, sxb, sxh, sxw, sxc, c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, c.pad, s, t)
    if c.kernel == CC.AREG:
        return lib.capnet_conv1x1_areg_eligible(X, M, c.Cin, c.Cout, c.bn, s, t)
    if c.kernel == CC.TAIL:
        return lib.capnet_conv1x1_tail_eligible(X, RES, M, c.Cin, c.Cout)
    return lib.capnet_conv_stem_f16x3_eligible(X, sxb, sxc, sxh, sxw, c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, c.pad)


def test_every_gpu_row_is_eligible_for_its_kernel_on_its_own_view(lib):
    refused = [c.name for c in CC.CASES if not eligible(lib, c)]
    assert not refused, refused
    # ... and the tile widths are ones the launchers take
    for c in CC.CASES:
        if c.kernel in (CC.H3_1X1, CC.H3, CC.H3_SCALED, CC.AREG):
            assert c.bn in (64, 128) and c.Cout % c.bn == 0, c.name
        if c.kernel in (CC.PATCH, CC.TAIL):
            assert c.bn in (64, 128, 256) and c.Cout % c.bn == 0, c.name


def test_rows_stay_small():
    for c in CC.CASES:
        assert CC.rows_m(c) <= 5000 and c.Cin <= 512, c.name


def test_table_covers_every_instantiation():
    have = {CC.arm(c) for c in CC.CASES}
    need = set()
    for tile in (0, 64, 128, 12864):
        need |= {(CC.GENERIC, "nchw", tile), (CC.GENERIC, "nhwc", tile)}
        for k, stride in ((3, 1), (3, 2), (1, 1), (1, 2)):
            assert any(a[:3] == (CC.KMAJOR, k, stride) and a[4] == tile for a in have), (k, stride, tile)
    need |= {(CC.DMA, stride, stats) for stride in (1, 2) for stats in (True, False)}
    for kernel, k in ((CC.H3_1X1, 1), (CC.H3, 3)):
        for bn in (64, 128):
            for pre in (True, False):
                assert any(a[:4] == (kernel, k, bn, pre) for a in have), (kernel, bn, pre)
        for stride in (1, 2):
            assert any(a[0] == kernel and a[1] == k and a[4] == stride for a in have), (kernel, stride)
    need |= {(CC.PATCH, shared, bn) for shared in (0, 1) for bn in (64, 128, 256)}
    need |= {(CC.AREG, cin, pre) for cin in (64, 128, 256) for pre in (True, False)}
    need |= {(CC.TAIL, bn, ds) for bn in (64, 128, 256) for ds in (True, False)}
    assert not need - have, sorted(need - have, key=str)
    rows = CC.CASES
    km = CC.of(CC.KMAJOR)
    assert any(c.pre for c in km) and any(not c.pre for c in km) and any(c.slab > 0 for c in km)
    assert any((c.B, c.H, c.W, c.Cin, c.Cout) == (23, 14, 14, 64, 256) for c in km)
    h3 = [c for c in rows if c.kernel in (CC.H3_1X1, CC.H3)]
    assert {(9, 11), (7, 7)} <= {(c.H, c.W) for c in h3 if c.k == 3}
    assert {1, 2} <= {c.epi for c in h3} and any(c.in_exp for c in CC.of(CC.H3_SCALED))
    pt = CC.of(CC.PATCH)
    assert {(5, 3, 3), (2, 9, 11)} <= {(c.B, c.H, c.W) for c in pt} and any(c.W == 59 for c in pt)
    for kernel in (CC.AREG, CC.TAIL):
        assert {1, 129, 300} <= {c.B for c in CC.of(kernel)}, kernel
    assert {0, 1} <= {c.relu for c in CC.of(CC.AREG)}
    assert {32, 64, 256, 512} <= {c.Cin for c in CC.of(CC.TAIL)}
    st = CC.of(CC.STEM)
    assert {(7, 8), (40, 264)} <= {(c.H, c.W) for c in st} and {0, 1} <= {c.stats for c in st}
    # every kernel has a dense row; every instantiation of a kernel that takes strides has a `gaps` row
    for kernel in CC.KERNELS:
        assert any(c.view == "dense" for c in CC.of(kernel)), kernel
    for kernel in CC.STRIDED:
        missing = {CC.arm(c) for c in CC.of(kernel)} - {CC.arm(c) for c in CC.of(kernel) if c.view == "gaps"}
        assert not missing, sorted(missing, key=str)


def test_tile_slab_and_statistics_row_counts(lib):
    wrong = []
    for c in CC.CASES:
        M = CC.rows_m(c)
        if c.kernel == CC.GENERIC:
            got = lib.capnet_conv_tiles_m(M, c.Cout, c.tile)
        elif c.kernel == CC.KMAJOR:
            got = lib.capnet_conv_kmajor_tiles_m(M, c.Cout, CC.k_rows(c), c.tile)
            slab = lib.capnet_conv_kmajor_slab_floats(M, c.Cout, CC.k_rows(c), c.tile)
            if slab != c.slab:
                wrong.append((c.name, "slab floats", slab, "expected", c.slab))
        elif c.kernel == CC.STEM:
            got = lib.capnet_conv_stem_f16x3_part_rows(c.B, c.H, c.W)
        else:
            got = lib.capnet_conv1x1_tiles_m(M)
        if c.stats and got != c.tiles:
            wrong.append((c.name, "statistics rows", got, "expected", c.tiles))
    assert not wrong, wrong
    # the K-sliced row's plan: {tile, tiles, whole tiles, K-slices, k-tiles per slice}
    plan = (ctypes.c_int * 5)()
    c = CC.BY_NAME["kmajor-tail-sliced-dense"]
    lib.capnet_conv_kmajor_plan(CC.rows_m(c), c.Cout, CC.k_rows(c), c.tile, plan)
    assert list(plan) == [64, 568, 512, 4, 18]
    c = CC.BY_NAME["kmajor-tail-unsliced-dense"]
    lib.capnet_conv_kmajor_plan(CC.rows_m(c), c.Cout, CC.k_rows(c), c.tile, plan)
    assert list(plan) == [64, 284, 284, 1, 36]
