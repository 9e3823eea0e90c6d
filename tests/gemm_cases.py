"""The case table of the f32 GEMM family (csrc/gemm_f32.hip, gemm_dma.hip, gemm_b3.hip) and its two reducers: one row per
branch of the dispatchers, at the smallest shape at which that branch can still go wrong. tests/test_gemm_routes_cpu.py
asks the library which kernel each row is given (no GPU), tests/test_gemm_views_gpu.py runs every row on padded, offset
views against float64.

The expected route, loader form and split of a row are written here BY HAND from the conditions in the source; nothing in
this file is recorded from the library. When a dispatch condition changes on purpose, the rows it moves are edited with it.

Pure Python (no torch): the CPU test needs only integers."""
from collections import namedtuple

# CAPNET_ROUTE_* of include/capnet.h
NONE, G64, G128, G6432, NT_DMA, B3, ROWS16, SKINNY64, SKINNY128, KLOOP_SPLITK, B3_SPLITK = range(11)
FELL = 64
ROUTE_NAMES = {NONE: "none", G64: "generic64", G128: "generic128", G6432: "generic6432", NT_DMA: "nt_dma", B3: "b3",
               ROWS16: "rows16", SKINNY64: "skinny64", SKINNY128: "skinny128", KLOOP_SPLITK: "kloop_splitk",
               B3_SPLITK: "b3_splitk"}
VEC, SCALAR = 1, 0


def route_name(r):
    return ("fell>" if r & FELL else "") + ROUTE_NAMES[r & ~FELL]


# A view of an operand inside a wider buffer: leading dimension (None: the extent itself), base offset in floats from a
# 16-B aligned address, batch stride (None: rows * ld, members one after the other).
View = namedtuple("View", "ld off stride", defaults=(None, 0, None))

# entry: sgemm | b3 (capnet_sgemm_b3) | splitk | fused (capnet_sgemm_splitk_fused) | batched (capnet_sgemm_splitk_batched)
#        | splitk_slabs | rows16_slabs
# sbias: batch stride of the bias (N: one bias per member, 0: shared); bias_off: floats from a 16-B aligned address
# ws / counters: floats / ints handed to the entry (0: none)
# route, loader: what the row must be given; splits, chunk: the cut of K where the route has one (chunk: sub, kc or
# kchunk); for the two slabs entries, splits is the n_slabs the call must report (0: the shape does not qualify)
Case = namedtuple("Case", "name entry ta tb M N K batch a b c bias sbias bias_off accumulate force_tile ws counters "
                          "route loader splits chunk")


def up4(x):
    return (x + 3) // 4 * 4


def odd_ld(extent):
    return extent + 1 if (extent + 1) % 4 else extent + 2


def extents(ta, tb, M, N, K):
    """(rows, contiguous extent) of A and B as stored."""
    return ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))


def mk(name, entry, ta, tb, M, N, K, route, loader=VEC, batch=1, a=View(), b=View(), c=View(), bias=False, sbias=None,
       bias_off=0, accumulate=False, force_tile=0, ws=0, counters=0, splits=1, chunk=0):
    if sbias is None:
        sbias = N
    return Case(name, entry, int(ta), int(tb), M, N, K, batch, a, b, c, bias, sbias, bias_off, accumulate, force_tile, ws,
                counters, route, loader, splits, chunk)


def resolved(case):
    """The row with every default of its views filled in: (a, b, c) as (ld, off, stride)."""
    (ar, ac), (br, bc) = extents(case.ta, case.tb, case.M, case.N, case.K)
    out = []
    for v, rows, cols in ((case.a, ar, ac), (case.b, br, bc), (case.c, case.M, case.N)):
        ld = cols if v.ld is None else v.ld
        out.append(View(ld, v.off, rows * ld if v.stride is None else v.stride))
    return out


def dense(case):
    """The same product on dense contiguous operands (what summation order must not differ from)."""
    sep = case.c.stride is None or case.c.stride != case.N      # members of C: separate matrices / column blocks
    c = View() if sep else View(case.N * case.batch, 0, case.N)
    return case._replace(a=View(), b=View(), c=c, bias_off=0)


def operand_args(case, pa, pb, pc, pbias):
    """The operand part of every entry's argument list, from the operands' addresses: transA .. accumulate, batch and the
    four strides (all 0 for a single product)."""
    a, b, c = resolved(case)
    one = case.batch == 1
    return [case.ta, case.tb, case.M, case.N, case.K, pa, a.ld, pb, b.ld, pc, c.ld, pbias if case.bias else None,
            int(case.accumulate), case.batch, 0 if one else a.stride, 0 if one else b.stride, 0 if one else c.stride,
            0 if one else case.sbias]


def query_route(lib, case, pa, pb, pc, pbias, pws, pctr):
    """(route, [loader, splits, chunk, tiles]) the library gives the row: capnet_sgemm_route for the sgemm entry,
    capnet_sgemm_splitk_route for the split-K entries (the addresses are looked at for null and alignment only)."""
    import ctypes
    detail = (ctypes.c_int * 4)(-1, -1, -1, -1)
    args = operand_args(case, pa, pb, pc, pbias)
    if case.entry == "sgemm":
        r = lib.capnet_sgemm_route(*args, case.force_tile, detail)
    else:
        assert case.entry in ("splitk", "fused", "batched")
        r = lib.capnet_sgemm_splitk_route(*args, pws if case.ws else None, case.ws, pctr if case.counters else None,
                                          case.counters, detail)
    return r, list(detail)


LAYOUTS = [(0, 1), (0, 0), (1, 0), (1, 1)]
EPILOGUES = [(True, False), (False, True), (True, True), (False, False)]       # (bias, accumulate)
GENERIC_SHAPES = [(1, 1, 1), (3, 5, 2), (65, 33, 17), (67, 130, 35), (129, 66, 15)]
GENERIC_ROUTE = {64: G64, 128: G128, 6432: G6432}


def _generic_rows():
    rows = []
    for tile in (64, 128, 6432):
        for ta, tb in LAYOUTS:
            for M, N, K in GENERIC_SHAPES:
                (_, ac), (_, bc) = extents(ta, tb, M, N, K)
                # vec: 16-B rows and bases (ld = roundup4(extent) + 4, base offsets 0 and 4 floats); odd: ld = extent + 1
                # (+ 2 where that is a multiple of 4: extents 3, 15, 35, 67 -- the form is the one whose rows are not 16-B);
                # off1: ld % 4 == 0 but the base one float past a 16-B boundary
                forms = [("vec0", View(up4(ac) + 4, 0), View(up4(bc) + 4, 0), VEC),
                         ("vec4", View(up4(ac) + 4, 4), View(up4(bc) + 4, 4), VEC),
                         ("odd", View(odd_ld(ac), 0), View(odd_ld(bc), 0), SCALAR),
                         ("off1", View(up4(ac) + 4, 1), View(up4(bc) + 4, 1), SCALAR)]
                for fname, a, b, loader in forms:
                    for bias, acc in EPILOGUES:
                        rows.append(mk("generic%d-%d%d-%dx%dx%d-%s-b%da%d" % (tile, ta, tb, M, N, K, fname, bias, acc),
                                       "sgemm", ta, tb, M, N, K, GENERIC_ROUTE[tile], loader, a=a, b=b, c=View(N + 3, 1),
                                       bias=bias, accumulate=acc, force_tile=tile))
    # batched: three members; strides a multiple of 4 (vector loads) and not (scalar); C members as column blocks of one
    # matrix (stride N) and as separate matrices; one bias per member and a shared one
    M, N, K = 65, 33, 17
    for tile in (64, 128, 6432):
        for ta, tb in LAYOUTS:
            (ar, ac), (br, bc) = extents(ta, tb, M, N, K)
            lda, ldb = up4(ac) + 4, up4(bc) + 4
            for sname, sa, sb, loader in (("s4", ar * lda + 8, br * ldb + 4, VEC), ("s1", ar * lda + 5, br * ldb + 4, SCALAR),
                                          ("s2", ar * lda + 8, br * ldb + 2, SCALAR)):
                for cname, c in (("cols", View(3 * N + 2, 0, N)), ("mats", View(N + 4, 0, M * (N + 4) + 7))):
                    for sbias in (N, 0):
                        rows.append(mk("generic%d-%d%d-batch3-%s-%s-sb%d" % (tile, ta, tb, sname, cname, sbias), "sgemm",
                                       ta, tb, M, N, K, GENERIC_ROUTE[tile], loader, batch=3, a=View(lda, 0, sa),
                                       b=View(ldb, 0, sb), c=c, bias=True, sbias=sbias, accumulate=(sbias == 0),
                                       force_tile=tile))
    return rows


def _auto_rows():
    rows = []
    # nt_dma: !ta, tb, one member, no accumulation, M > 64, ceil(M/128) * (N/64) >= 64 (here 2 * 32), N % 64 == 0,
    # K % 16 == 0, ldb == K, ldc == N, lda % 4 == 0, 16-B aligned A and B
    M, N, K = 129, 2048, 32
    rows.append(mk("auto-nt_dma-lda=K", "sgemm", 0, 1, M, N, K, NT_DMA, bias=True))
    rows.append(mk("auto-nt_dma-lda=K+4", "sgemm", 0, 1, M, N, K, NT_DMA, a=View(K + 4)))
    # ... pushed back to the generic kernel (2 * 16 tiles of 128 < 384: the 64 tile) by accumulation and by ldb != K
    rows.append(mk("auto-nt_dma-denied-accumulate", "sgemm", 0, 1, M, N, K, G64, bias=True, accumulate=True))
    rows.append(mk("auto-nt_dma-denied-ldb=K+4", "sgemm", 0, 1, M, N, K, G64, b=View(K + 4)))
    # b3 at its threshold: 12 * 16 = 192 tiles of 128, 1536 * 2048 * 80 = 2.52e8 multiply-adds, every extent % 4 == 0
    for ta, tb in LAYOUTS:
        rows.append(mk("auto-b3-%d%d" % (ta, tb), "sgemm", ta, tb, 1536, 2048, 80, B3, bias=True, accumulate=bool(ta)))
    # one k less: 2.49e8 multiply-adds (K % 4 != 0 is admitted by b3 in this layout), 192 tiles < 384: the 64 tile
    rows.append(mk("auto-b3-below-2.5e8", "sgemm", 1, 0, 1536, 2048, 79, G64))
    # the 128 tile by itself: 16 * 24 = 384 tiles of 128; 2.5e7 multiply-adds keep it off b3
    rows.append(mk("auto-tile128", "sgemm", 1, 0, 2048, 3072, 4, G128, bias=True))
    # gemm_b3 directly on padded views: K % 4 != 0 where no operand is K-contiguous, M % 4 != 0 and N % 4 != 0 where both are
    for ta, tb, M, N, K in ((1, 0, 260, 132, 301), (0, 1, 261, 133, 300)):
        (_, ac), (_, bc) = extents(ta, tb, M, N, K)
        rows.append(mk("b3-direct-%d%d-%dx%dx%d" % (ta, tb, M, N, K), "b3", ta, tb, M, N, K, B3, a=View(up4(ac) + 4),
                       b=View(up4(bc) + 4), c=View(up4(N) + 4), bias=True, accumulate=True))
    return rows


def _splitk_rows():
    rows = []
    BIG = 1 << 21
    # ---- rows16 (counters, M <= 16, N % 4 == 0, 16-B rows of C): (sub, splits) from the cost rule 2.2 sub (+ 3.5 + 0.25
    # splits when split) over chunks of 256 k, the grid held to 256 workgroups:
    #   K = 64: one chunk (1, 1); K = 260: two chunks, 4.4 < 6.2 (2, 1); K = 1028, 2 tiles: 5 chunks, 6.95 at (1, 5);
    #   K = 1028, 128 tiles: splits 5 and 3 overfill the chip, (3, 2) costs 10.6 < 11 -- its last split owns 2 chunks
    plans = {(4, 64): (1, 1), (68, 260): (2, 1), (68, 1028): (1, 5), (8192, 1028): (3, 2)}
    for M in (1, 16):
        for (N, K), (sub, splits) in plans.items():
            for tb in (1, 0):
                (_, _), (_, bc) = extents(0, tb, M, N, K)
                rows.append(mk("rows16-%dx%dx%d-tb%d" % (M, N, K, tb), "fused", 0, tb, M, N, K, ROWS16, a=View(K + 8, 4),
                               b=View(bc + 4), c=View(N + 4), bias=(M == 16), accumulate=(tb == 1), ws=BIG, counters=128,
                               splits=splits, chunk=sub))
    # four members (the gates): A members column blocks of one matrix, outputs column blocks of C
    for (N, K), (sub, splits) in (((68, 260), (2, 1)), ((68, 1028), (1, 5))):
        for tb in (1, 0):
            (br, bc) = extents(0, tb, 16, N, K)[1]
            rows.append(mk("rows16-batch4-16x%dx%d-tb%d" % (N, K, tb), "batched", 0, tb, 16, N, K, ROWS16, batch=4,
                           a=View(4 * K + 4, 0, K), b=View(bc + 4, 0, br * (bc + 4) + 8), c=View(4 * N + 4, 0, N), bias=True,
                           accumulate=(tb == 0), ws=BIG, counters=128, splits=splits, chunk=sub))
    # ---- skinny (M <= 128, one K chunk per workgroup): kc = 64 while tiles * ceil(K/128) < 200, else 128
    for tb in (1, 0):
        (_, bc) = extents(0, tb, 17, 68, 132)[1]
        # 2 tiles * 2 < 200: kc = 64, chunks of 64, 64 and 4 k (one k-quad)
        rows.append(mk("skinny-17x68x132-tb%d" % tb, "splitk", 0, tb, 17, 68, 132, SKINNY64, a=View(136, 4), b=View(bc + 4),
                       c=View(72), bias=True, accumulate=(tb == 1), ws=BIG, splits=3, chunk=64))
        rows.append(mk("skinny-128x4x64-tb%d" % tb, "splitk", 0, tb, 128, 4, 64, SKINNY64, a=View(68), b=View(up4(extents(
            0, tb, 128, 4, 64)[1][1]) + 4), c=View(5, 1), bias=(tb == 0), ws=BIG, splits=1, chunk=64))
        # 2 * 64 tiles * 2 >= 200: kc = 128
        rows.append(mk("skinny-128x4096x256-tb%d" % tb, "splitk", 0, tb, 128, 4096, 256, SKINNY128, b=View(extents(
            0, tb, 128, 4096, 256)[1][1] + 4), bias=True, accumulate=(tb == 0), ws=BIG, splits=2, chunk=128))
        # kc = 64 needs 3 * 17 * 68 = 3468 floats, kc = 128 needs 2312: a workspace of 3000 takes kc = 128
        rows.append(mk("skinny-17x68x132-ws3000-tb%d" % tb, "splitk", 0, tb, 17, 68, 132, SKINNY128, a=View(136),
                       b=View(bc + 4), c=View(72), bias=True, ws=3000, splits=2, chunk=128))
        # the four gates: 2 tiles * 4 members * 2 < 200: kc = 64
        (br, bc) = extents(0, tb, 17, 68, 132)[1]
        rows.append(mk("skinny-batch4-17x68x132-tb%d" % tb, "batched", 0, tb, 17, 68, 132, SKINNY64, batch=4,
                       a=View(4 * 132 + 4, 0, 132), b=View(bc + 4, 0, br * (bc + 4) + 4), c=View(4 * 68 + 4, 0, 68), bias=True,
                       accumulate=(tb == 1), ws=BIG, splits=3, chunk=64))
    # ---- what denies the skinny path: the product goes to sgemm (2 tiles of 128: the 64 tile), one row per condition
    deny = [
        ("transA", mk("", "splitk", 1, 0, 17, 68, 132, FELL | G64, a=View(20), ws=BIG)),
        ("K%4", mk("", "splitk", 0, 1, 17, 68, 134, FELL | G64, a=View(136), b=View(136), ws=BIG)),
        ("K<64", mk("", "splitk", 0, 1, 17, 68, 60, FELL | G64, ws=BIG)),
        ("N<4", mk("", "splitk", 0, 1, 17, 3, 132, FELL | G64, ws=BIG)),
        ("lda%4", mk("", "splitk", 0, 1, 17, 68, 132, FELL | G64, SCALAR, a=View(133), ws=BIG)),
        ("A-misaligned", mk("", "splitk", 0, 1, 17, 68, 132, FELL | G64, SCALAR, a=View(136, 1), ws=BIG)),
        ("B-misaligned", mk("", "splitk", 0, 0, 17, 68, 132, FELL | G64, SCALAR, b=View(72, 2), ws=BIG)),
        ("ldb%4", mk("", "splitk", 0, 0, 17, 68, 132, FELL | G64, SCALAR, b=View(70), ws=BIG)),
        ("tb0-N%4", mk("", "splitk", 0, 0, 17, 70, 132, FELL | G64, b=View(72), ws=BIG)),
        ("M>128", mk("", "splitk", 0, 1, 129, 68, 132, FELL | G64, ws=BIG)),
        ("no-ws", mk("", "splitk", 0, 1, 17, 68, 132, FELL | G64, bias=True, accumulate=True)),
        # below kc = 128's 2312 floats
        ("ws-too-small", mk("", "splitk", 0, 1, 17, 68, 132, FELL | G64, ws=2000)),
        # members of C that are separate matrices / a shared bias: not the gates' column blocks
        ("batch-sC", mk("", "batched", 0, 1, 17, 68, 132, FELL | G64, batch=4, c=View(72, 0, 17 * 72), bias=True, ws=BIG)),
        ("batch-sBias", mk("", "batched", 0, 1, 17, 68, 132, FELL | G64, batch=4, c=View(4 * 68, 0, 68), bias=True, sbias=0,
                           ws=BIG)),
        ("batch-sA%4", mk("", "batched", 0, 1, 17, 68, 132, FELL | G64, SCALAR, batch=4, a=View(136, 0, 17 * 136 + 2),
                          c=View(4 * 68, 0, 68), ws=BIG)),
        # rows16 denied, skinny taken: 2 tiles * 3 < 200 -> kc = 64, 5 chunks of K = 260
        ("rows16-C-misaligned", mk("", "fused", 0, 1, 16, 68, 260, SKINNY64, c=View(72, 1), bias=True, ws=BIG, counters=128,
                                   splits=5, chunk=64)),
        ("rows16-ldc%4", mk("", "fused", 0, 1, 16, 68, 260, SKINNY64, c=View(70), ws=BIG, counters=128, splits=5, chunk=64)),
        ("rows16-bias-misaligned", mk("", "fused", 0, 0, 16, 68, 260, SKINNY64, bias=True, bias_off=1, accumulate=True, ws=BIG,
                                      counters=128, splits=5, chunk=64)),
        ("rows16-M>16", mk("", "fused", 0, 1, 17, 68, 260, SKINNY64, bias=True, ws=BIG, counters=128, splits=5, chunk=64)),
        ("rows16-counters", mk("", "fused", 0, 1, 16, 68, 260, SKINNY64, bias=True, ws=BIG, counters=1, splits=5, chunk=64)),
        ("rows16-no-counters", mk("", "splitk", 0, 1, 16, 68, 260, SKINNY64, ws=BIG, splits=5, chunk=64)),
        # rows16's 5 slabs need 5440 floats, skinny's 17 (kc = 64) or 9 (kc = 128) slabs more: 3000 sends it to sgemm
        ("rows16-ws-too-small", mk("", "fused", 0, 1, 16, 68, 1028, FELL | G64, bias=True, ws=3000, counters=128)),
    ]
    rows += [c._replace(name="deny-" + n) for n, c in deny]
    # ---- fall-through lands on every kernel sgemm chooses by itself
    rows.append(mk("fell-nt_dma", "splitk", 0, 1, 129, 2048, 32, FELL | NT_DMA, bias=True, ws=BIG))
    rows.append(mk("fell-b3", "splitk", 0, 1, 1536, 2048, 80, FELL | B3, bias=True, ws=BIG))
    rows.append(mk("fell-tile128", "splitk", 1, 0, 2048, 3072, 4, FELL | G128, ws=BIG))
    # ---- k-loop split-K (M > 128, fewer than 256 tiles of 64, K >= 1024, off b3: 9.0e6 multiply-adds):
    # 3 * 2 tiles -> min(1024 / 6, K / 256) = 4 slabs of roundup16(ceil(1030 / 4)) = 272 k, the last of 214
    M, N, K = 129, 68, 1030
    for ta, tb in LAYOUTS:
        (_, ac), (_, bc) = extents(ta, tb, M, N, K)
        rows.append(mk("kloop-splitk-%d%d-vec" % (ta, tb), "splitk", ta, tb, M, N, K, KLOOP_SPLITK, VEC, a=View(up4(ac) + 4, 4),
                       b=View(up4(bc) + 4), c=View(N + 4), bias=bool(tb), accumulate=bool(ta), ws=BIG, splits=4, chunk=272))
        rows.append(mk("kloop-splitk-%d%d-odd" % (ta, tb), "splitk", ta, tb, M, N, K, KLOOP_SPLITK, SCALAR, a=View(ac + 1),
                       b=View(up4(bc) + 4), c=View(N + 3, 1), bias=bool(ta), accumulate=bool(tb), ws=BIG, splits=4, chunk=272))
    # K one short of 1024: no slabs
    rows.append(mk("kloop-splitk-K1023", "splitk", 1, 0, 129, 68, 1023, FELL | G64, a=View(132), ws=BIG))
    # a workspace with room for three slabs of 129 * 68 only: 3 slabs of roundup16(ceil(1030 / 3)) = 352 k
    rows.append(mk("kloop-splitk-ws3", "splitk", 1, 0, M, N, K, KLOOP_SPLITK, VEC, a=View(132), ws=3 * 129 * 68 + 100, splits=3,
                   chunk=352))
    # ---- b3 split-K (M > 128, K >= 512, 2.51e8 multiply-adds): 2 * 8 tiles of 128, 58 steps of 32 k ->
    # min(ceil(512 / 16), 58 / 8) = 7 slabs of ceil(58 / 7) = 9 steps (288 k), the last of 4
    for ta, tb in LAYOUTS:
        rows.append(mk("b3-splitk-%d%d" % (ta, tb), "splitk", ta, tb, 132, 1024, 1856, B3_SPLITK, c=View(1028), bias=bool(ta),
                       accumulate=bool(tb), ws=BIG, splits=7, chunk=288))
    return rows


def _slabs_rows():
    rows = []
    BIG = 1 << 17
    for tb in (1, 0):
        bc = extents(0, tb, 17, 68, 132)[1][1]
        rows.append(mk("splitk_slabs-17x68x132-tb%d" % tb, "splitk_slabs", 0, tb, 17, 68, 132, SKINNY64, a=View(136, 4),
                       b=View(bc + 4), ws=BIG, splits=3, chunk=64))
        bc = extents(0, tb, 16, 68, 1028)[1][1]
        # 2 tiles * 5 chunks <= 256 workgroups: one chunk each
        rows.append(mk("rows16_slabs-16x68x1028-tb%d" % tb, "rows16_slabs", 0, tb, 16, 68, 1028, ROWS16, a=View(1032, 4),
                       b=View(bc + 4), ws=BIG, splits=5, chunk=1))
    # 128 tiles: 5 and 3 slabs overfill 256 workgroups, 3 chunks each leave 2 slabs
    rows.append(mk("rows16_slabs-1x8192x1028", "rows16_slabs", 0, 1, 1, 8192, 1028, ROWS16, ws=BIG, splits=2, chunk=3))
    # shapes that do not qualify: n_slabs = 0, the workspace untouched
    rows.append(mk("splitk_slabs-none-N%4", "splitk_slabs", 0, 0, 17, 70, 132, NONE, b=View(72), ws=BIG, splits=0))
    rows.append(mk("splitk_slabs-none-ws", "splitk_slabs", 0, 1, 17, 68, 132, NONE, ws=2000, splits=0))
    rows.append(mk("rows16_slabs-none-M17", "rows16_slabs", 0, 1, 17, 68, 1028, NONE, ws=BIG, splits=0))
    rows.append(mk("rows16_slabs-none-lda", "rows16_slabs", 0, 1, 16, 68, 1028, NONE, a=View(1029), ws=BIG, splits=0))
    return rows


GENERIC = _generic_rows()
AUTO = _auto_rows()
SPLITK = _splitk_rows()
SLABS = _slabs_rows()
CASES = GENERIC + AUTO + SPLITK + SLABS
assert len({c.name for c in CASES}) == len(CASES)

# reduce_slabs: (count, M, N, ldc); every row runs with and without bias and accumulation. The kernel sums 8 slabs at a
# time, then the rest; 2048 workgroups of 256 walk more than 524288 elements in a second pass.
REDUCE = [(1, 5, 37, 41), (7, 5, 37, 41), (8, 5, 37, 41), (9, 5, 37, 41), (17, 5, 37, 41), (2, 2, 262147, 262151)]
# colsum: (rows, C, ld, workspace floats); with a workspace and more than 4096 rows: min(32, rows / 1024) = 4 chunks of 1250
# rows. Every row runs with and without accumulation.
COLSUM = [(1, 1, 1, 0), (300, 1, 1, 0), (257, 33, 40, 0), (5000, 70, 72, 0), (5000, 70, 72, 4 * 70),
          (5000, 70, 72, 4 * 70 - 1)]            # (the last: a workspace one float short of four chunks -- unchunked)

# Every (route, transA, transB, loader form) the two dispatchers can produce; tests/test_gemm_routes_cpu.py holds the table
# to it.
REQUIRED = set()
for _ta, _tb in LAYOUTS:
    for _r in (G64, G128, G6432, KLOOP_SPLITK):
        REQUIRED |= {(_r, _ta, _tb, VEC), (_r, _ta, _tb, SCALAR)}
    REQUIRED |= {(B3, _ta, _tb, VEC), (B3_SPLITK, _ta, _tb, VEC)}
for _tb in (0, 1):
    REQUIRED |= {(ROWS16, 0, _tb, VEC), (SKINNY64, 0, _tb, VEC), (SKINNY128, 0, _tb, VEC)}
REQUIRED |= {(NT_DMA, 0, 1, VEC), (FELL | NT_DMA, 0, 1, VEC), (FELL | B3, 0, 1, VEC), (FELL | G128, 1, 0, VEC),
             (FELL | G64, 0, 1, VEC), (FELL | G64, 0, 0, VEC), (FELL | G64, 1, 0, VEC), (FELL | G64, 0, 1, SCALAR),
             (FELL | G64, 0, 0, SCALAR)}
