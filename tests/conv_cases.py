"""The case table of the convolution family (csrc/conv_f32.hip, conv_f32_v2.hip, gemm_dma.hip, conv_f16x3.hip,
conv3x3_patch.hip, conv1x1_areg.hip, conv_stem.hip): one named row per kernel, template arm, view form and edge, at the
smallest shape at which that arm can still go wrong. tests/test_conv_routes_cpu.py asks the library's predicates and
planners about every row (no GPU); tests/test_conv_views_gpu.py runs every row on fenced views against float64.

Rows are written BY HAND, the expected statistics rows (`tiles`) and slab floats (`slab`) included: tiles is
ceil(M / tile rows) -- 128 rows everywhere except the 64 x 64 tile of the two f32 kernels (which their automatic choice,
tile 0, picks at all of these sizes except for the generic kernel at Cout <= 64, where it is 128 x 64) and the stem,
whose rows are one per workgroup: min(B * OH * ceil(OW / 128), 512).

View forms: `dense` -- the kernel's dense strides; `gaps` -- a gap behind every pixel, row and image (strides() below),
only where the kernel's predicate takes strides. Whatever the form, the operand starts behind a fence, never at the start
of its allocation.

The operands, the float64 reference and the magnitude of a row come from reference(case), on the CPU."""
import functools
from collections import namedtuple

GENERIC, KMAJOR, DMA, H3_1X1, H3, H3_SCALED, PATCH, AREG, TAIL, STEM = (
    "generic", "kmajor", "dma", "f16x3_1x1", "f16x3", "f16x3_scaled", "patch", "areg", "tail", "stem")
KERNELS = (GENERIC, KMAJOR, DMA, H3_1X1, H3, H3_SCALED, PATCH, AREG, TAIL, STEM)
ENTRY = {GENERIC: "capnet_conv2d_fwd", KMAJOR: "capnet_conv2d_fwd_kmajor", DMA: "capnet_conv1x1_fwd_dma",
         H3_1X1: "capnet_conv1x1_fwd_f16x3", H3: "capnet_conv2d_fwd_f16x3", H3_SCALED: "capnet_conv2d_fwd_f16x3_scaled",
         PATCH: "capnet_conv3x3_fwd_patch", AREG: "capnet_conv1x1_fwd_areg", TAIL: "capnet_conv1x1_fwd_tail",
         STEM: "capnet_conv_stem_fwd_f16x3"}
STRIDED = (GENERIC, KMAJOR, DMA, H3_1X1, H3, H3_SCALED, STEM)        # kernels whose predicate takes strides

# view: dense | gaps.  nchw: the operand is [B][Cin][H][W] (the stem and the generic kernel's stem form), else NHWC.
# tile: the f32 kernels' tile argument.  bn: the split-f16 kernels' tile width.  pre: a folded BatchNorm on the input
# (in_scale / in_shift, some scales negative), relu: relu_in.  stats: part_sum / part_sq requested.
# epi: 0 none, 1 out_scale + out_shift + residual + ReLU, 2 out_scale + out_shift alone.  in_exp: power-of-two prescale.
# shared: the patch kernel's shared_chip.  ds: the tail kernel's identity has its own BatchNorm (s2 / t2).
# AREG and TAIL rows are [M][Cin] matrices: B = M, H = W = 1.
# tiles: rows of part_sum / part_sq the call writes (0: no statistics).  slab: capnet_conv_kmajor_slab_floats.
Case = namedtuple("Case", "name kernel view nchw B H W Cin Cout k stride pad tile bn pre relu stats epi in_exp shared ds "
                          "tiles slab")


def row(name, kernel, view, B, H, W, Cin, Cout, k=1, stride=1, pad=0, tile=0, bn=0, pre=0, relu=0, stats=1, epi=0,
        in_exp=0, shared=0, ds=0, tiles=0, slab=0, nchw=0):
    assert view in ("dense", "gaps") and (view == "dense" or kernel in STRIDED)
    assert not (stats and epi) and (tiles > 0) == bool(stats)
    return Case(name + "-" + view, kernel, view, nchw, B, H, W, Cin, Cout, k, stride, pad, tile, bn, pre, relu, stats, epi,
                in_exp, shared, ds, tiles, slab)


def out_hw(c):
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def rows_m(c):
    oh, ow = out_hw(c)
    return c.B * oh * ow


def strides(c, view=None):
    """(sxb, sxh, sxw, sxc) in floats."""
    gaps = (view or c.view) == "gaps"
    if c.nchw:
        sxh = c.W + 4 if gaps else c.W
        sxc = c.H * sxh + 8 if gaps else c.H * sxh
        sxb = c.Cin * sxc + 12 if gaps else c.Cin * sxc
        return sxb, sxh, 1, sxc
    sxw = c.Cin + 8 if gaps else c.Cin
    sxh = c.W * sxw + 12 if gaps else c.W * sxw
    sxb = c.H * sxh + 20 if gaps else c.H * sxh
    return sxb, sxh, sxw, 1


def dense(c):
    return c._replace(view="dense", name=c.name[:-len(c.view)] + "dense")


def k_rows(c):
    """Rows of the f32 kernels' weight images: KH KW Cin, for the generic kernel padded to a multiple of 16."""
    n = c.k * c.k * c.Cin
    return (n + 15) // 16 * 16 if c.kernel == GENERIC else n


G, K, D = GENERIC, KMAJOR, DMA
CASES = [
    # ---- capnet_conv2d_fwd: the 7x7 / 2 / pad 3 NCHW stem form (gather loader), M = 3 x 9 x 10 = 270
    row("generic-stem-t0", G, "dense", 3, 18, 20, 3, 64, 7, 2, 3, tile=0, tiles=3, nchw=1),
    row("generic-stem-t64", G, "dense", 3, 18, 20, 3, 64, 7, 2, 3, tile=64, tiles=5, nchw=1),
    row("generic-stem-t128", G, "dense", 3, 18, 20, 3, 64, 7, 2, 3, tile=128, tiles=3, nchw=1),
    row("generic-stem-t12864", G, "dense", 3, 18, 20, 3, 64, 7, 2, 3, tile=12864, tiles=3, nchw=1),
    row("generic-stem-t0", G, "gaps", 3, 18, 20, 3, 64, 7, 2, 3, tile=0, tiles=3, nchw=1),
    row("generic-stem-t64", G, "gaps", 3, 18, 20, 3, 64, 7, 2, 3, tile=64, tiles=5, nchw=1),
    row("generic-stem-t128", G, "gaps", 3, 18, 20, 3, 64, 7, 2, 3, tile=128, tiles=3, nchw=1),
    row("generic-stem-t12864", G, "gaps", 3, 18, 20, 3, 64, 7, 2, 3, tile=12864, tiles=3, nchw=1),
    # ... and 3x3 / 2 on NHWC with a fold (vector loader; Cout = 96 leaves the 128-wide tile ragged), M = 3 x 5 x 6 = 90
    row("generic-3x3s2-fold-t0", G, "dense", 3, 9, 11, 32, 96, 3, 2, 1, tile=0, pre=1, relu=1, tiles=2),
    row("generic-3x3s2-fold-t64", G, "dense", 3, 9, 11, 32, 96, 3, 2, 1, tile=64, pre=1, relu=1, tiles=2),
    row("generic-3x3s2-fold-t128", G, "dense", 3, 9, 11, 32, 96, 3, 2, 1, tile=128, pre=1, relu=1, tiles=1),
    row("generic-3x3s2-fold-t12864", G, "dense", 3, 9, 11, 32, 96, 3, 2, 1, tile=12864, pre=1, relu=1, tiles=1),
    row("generic-3x3s2-fold-t0", G, "gaps", 3, 9, 11, 32, 96, 3, 2, 1, tile=0, pre=1, relu=1, tiles=2),
    row("generic-3x3s2-fold-t64", G, "gaps", 3, 9, 11, 32, 96, 3, 2, 1, tile=64, pre=1, relu=1, tiles=2),
    row("generic-3x3s2-fold-t128", G, "gaps", 3, 9, 11, 32, 96, 3, 2, 1, tile=128, pre=1, relu=1, tiles=1),
    row("generic-3x3s2-fold-t12864", G, "gaps", 3, 9, 11, 32, 96, 3, 2, 1, tile=12864, pre=1, relu=1, tiles=1),
    # ... and the gather loader on NHWC (Cin = 24 is no multiple of 16), no fold
    row("generic-3x3s1-cin24-t64", G, "dense", 3, 5, 6, 24, 64, 3, 1, 1, tile=64, tiles=2),
    row("generic-3x3s1-cin24-t64", G, "gaps", 3, 5, 6, 24, 64, 3, 1, 1, tile=64, tiles=2),

    # ---- capnet_conv2d_fwd_kmajor: staging modes PRE x MASK on every tile
    # 3x3 s1, fold + ReLU, negative scales (PRE | MASK), M = 3 x 49 = 147
    row("kmajor-3x3s1-fold-t0", K, "dense", 3, 7, 7, 32, 128, 3, 1, 1, tile=0, pre=1, relu=1, tiles=3),
    row("kmajor-3x3s1-fold-t64", K, "dense", 3, 7, 7, 32, 128, 3, 1, 1, tile=64, pre=1, relu=1, tiles=3),
    row("kmajor-3x3s1-fold-t128", K, "dense", 3, 7, 7, 32, 128, 3, 1, 1, tile=128, pre=1, relu=1, tiles=2),
    row("kmajor-3x3s1-fold-t12864", K, "dense", 3, 7, 7, 32, 128, 3, 1, 1, tile=12864, pre=1, relu=1, tiles=2),
    row("kmajor-3x3s1-fold-t0", K, "gaps", 3, 7, 7, 32, 128, 3, 1, 1, tile=0, pre=1, relu=1, tiles=3),
    row("kmajor-3x3s1-fold-t64", K, "gaps", 3, 7, 7, 32, 128, 3, 1, 1, tile=64, pre=1, relu=1, tiles=3),
    row("kmajor-3x3s1-fold-t128", K, "gaps", 3, 7, 7, 32, 128, 3, 1, 1, tile=128, pre=1, relu=1, tiles=2),
    row("kmajor-3x3s1-fold-t12864", K, "gaps", 3, 7, 7, 32, 128, 3, 1, 1, tile=12864, pre=1, relu=1, tiles=2),
    # 3x3 s2, no fold (MASK alone), odd rectangular map, M = 3 x 5 x 6 = 90
    row("kmajor-3x3s2-t0", K, "dense", 3, 9, 11, 16, 128, 3, 2, 1, tile=0, tiles=2),
    row("kmajor-3x3s2-t64", K, "dense", 3, 9, 11, 16, 128, 3, 2, 1, tile=64, tiles=2),
    row("kmajor-3x3s2-t128", K, "dense", 3, 9, 11, 16, 128, 3, 2, 1, tile=128, tiles=1),
    row("kmajor-3x3s2-t12864", K, "dense", 3, 9, 11, 16, 128, 3, 2, 1, tile=12864, tiles=1),
    row("kmajor-3x3s2-t0", K, "gaps", 3, 9, 11, 16, 128, 3, 2, 1, tile=0, tiles=2),
    row("kmajor-3x3s2-t64", K, "gaps", 3, 9, 11, 16, 128, 3, 2, 1, tile=64, tiles=2),
    row("kmajor-3x3s2-t128", K, "gaps", 3, 9, 11, 16, 128, 3, 2, 1, tile=128, tiles=1),
    row("kmajor-3x3s2-t12864", K, "gaps", 3, 9, 11, 16, 128, 3, 2, 1, tile=12864, tiles=1),
    # 1x1 s1, no fold, whole tiles (neither PRE nor MASK), M = 4 x 64 = 256
    row("kmajor-1x1s1-t0", K, "dense", 4, 8, 8, 64, 128, tile=0, tiles=4),
    row("kmajor-1x1s1-t64", K, "dense", 4, 8, 8, 64, 128, tile=64, tiles=4),
    row("kmajor-1x1s1-t128", K, "dense", 4, 8, 8, 64, 128, tile=128, tiles=2),
    row("kmajor-1x1s1-t12864", K, "dense", 4, 8, 8, 64, 128, tile=12864, tiles=2),
    row("kmajor-1x1s1-t0", K, "gaps", 4, 8, 8, 64, 128, tile=0, tiles=4),
    row("kmajor-1x1s1-t64", K, "gaps", 4, 8, 8, 64, 128, tile=64, tiles=4),
    row("kmajor-1x1s1-t128", K, "gaps", 4, 8, 8, 64, 128, tile=128, tiles=2),
    row("kmajor-1x1s1-t12864", K, "gaps", 4, 8, 8, 64, 128, tile=12864, tiles=2),
    # 1x1 s2, fold without ReLU, whole tiles (PRE alone), M = 4 x 8 x 8 = 256
    row("kmajor-1x1s2-fold-t0", K, "dense", 4, 16, 16, 32, 128, 1, 2, 0, tile=0, pre=1, tiles=4),
    row("kmajor-1x1s2-fold-t64", K, "dense", 4, 16, 16, 32, 128, 1, 2, 0, tile=64, pre=1, tiles=4),
    row("kmajor-1x1s2-fold-t128", K, "dense", 4, 16, 16, 32, 128, 1, 2, 0, tile=128, pre=1, tiles=2),
    row("kmajor-1x1s2-fold-t12864", K, "dense", 4, 16, 16, 32, 128, 1, 2, 0, tile=12864, pre=1, tiles=2),
    row("kmajor-1x1s2-fold-t0", K, "gaps", 4, 16, 16, 32, 128, 1, 2, 0, tile=0, pre=1, tiles=4),
    row("kmajor-1x1s2-fold-t64", K, "gaps", 4, 16, 16, 32, 128, 1, 2, 0, tile=64, pre=1, tiles=4),
    row("kmajor-1x1s2-fold-t128", K, "gaps", 4, 16, 16, 32, 128, 1, 2, 0, tile=128, pre=1, tiles=2),
    row("kmajor-1x1s2-fold-t12864", K, "gaps", 4, 16, 16, 32, 128, 1, 2, 0, tile=12864, pre=1, tiles=2),
    # 1x1 s1, fold + ReLU, ragged last tile; Cout = 64: a requested 128 x 128 tile falls back to 128 x 64
    row("kmajor-1x1s1-fold-ragged-t64", K, "dense", 3, 7, 7, 64, 64, tile=64, pre=1, relu=1, tiles=3),
    row("kmajor-1x1s1-fold-ragged-t64", K, "gaps", 3, 7, 7, 64, 64, tile=64, pre=1, relu=1, tiles=3),
    row("kmajor-1x1s1-fold-ragged-t128", K, "dense", 3, 7, 7, 64, 64, tile=128, pre=1, relu=1, tiles=2),
    row("kmajor-1x1s1-fold-ragged-t128", K, "gaps", 3, 7, 7, 64, 64, tile=128, pre=1, relu=1, tiles=2),
    # 23 x 14 x 14 x 64 -> 256 (4508 rows, 71 x 4 = 284 tiles of 64 x 64): one full round of 256 and 28 more. The planner
    # slices a tail only from two full rounds on, so this shape is NOT sliced: no slab float may be touched
    row("kmajor-tail-unsliced", K, "dense", 23, 14, 14, 64, 256, 3, 1, 1, tile=0, pre=1, relu=1, tiles=71, slab=0),
    # 23 x 14 x 14 x 128 -> 512: 71 x 8 = 568 tiles = 512 + 56; the 56 tail tiles are cut into 4 K-slices of 18 k-tiles
    # (of 72): 56 x 4 slabs of 64 x 64 floats
    row("kmajor-tail-sliced", K, "dense", 23, 14, 14, 128, 512, 3, 1, 1, tile=0, pre=1, relu=1, tiles=71, slab=917504),
    row("kmajor-tail-sliced", K, "gaps", 23, 14, 14, 128, 512, 3, 1, 1, tile=0, pre=1, relu=1, tiles=71, slab=917504),

    # ---- capnet_conv1x1_fwd_dma: tile width 64 / 128, k-tile 16 (32 from 512 tiles on: the last row)
    row("dma-s1-stats", D, "dense", 3, 7, 7, 128, 128, tiles=2),
    row("dma-s1-stats", D, "gaps", 3, 7, 7, 128, 128, tiles=2),
    row("dma-s2-stats", D, "dense", 3, 6, 10, 96, 192, 1, 2, 0, tiles=1),
    row("dma-s2-stats", D, "gaps", 3, 6, 10, 96, 192, 1, 2, 0, tiles=1),
    row("dma-s1-cin16-stats", D, "dense", 3, 5, 5, 16, 64, tiles=1),
    row("dma-s1-cin16-stats", D, "gaps", 3, 5, 5, 16, 64, tiles=1),
    row("dma-s1-epi-res", D, "dense", 3, 7, 7, 64, 128, stats=0, epi=1),
    row("dma-s1-epi-res", D, "gaps", 3, 7, 7, 64, 128, stats=0, epi=1),
    row("dma-s2-epi", D, "dense", 3, 8, 8, 32, 64, 1, 2, 0, stats=0, epi=2),
    row("dma-s2-epi", D, "gaps", 3, 8, 8, 32, 64, 1, 2, 0, stats=0, epi=2),
    row("dma-s1-nostats", D, "dense", 3, 7, 7, 128, 128, stats=0),
    row("dma-s2-nostats", D, "gaps", 3, 6, 10, 96, 192, 1, 2, 0, stats=0),
    row("dma-bk32-520tiles", D, "dense", 5, 25, 40, 512, 832, tiles=40),               # 40 x 13 tiles of 128 x 64
    row("dma-bk32-520tiles", D, "gaps", 5, 25, 40, 512, 832, tiles=40),

    # ---- capnet_conv1x1_fwd_f16x3: <bn, PRE, 1 tap>
    row("h3-1x1-bn128-s1", H3_1X1, "dense", 3, 7, 7, 64, 128, bn=128, tiles=2),
    row("h3-1x1-bn128-s1", H3_1X1, "gaps", 3, 7, 7, 64, 128, bn=128, tiles=2),
    row("h3-1x1-bn64-s2", H3_1X1, "dense", 3, 9, 11, 64, 64, 1, 2, 0, bn=64, tiles=1),
    row("h3-1x1-bn64-s2", H3_1X1, "gaps", 3, 9, 11, 64, 64, 1, 2, 0, bn=64, tiles=1),
    row("h3-1x1-bn128-fold-s2", H3_1X1, "dense", 3, 9, 11, 128, 256, 1, 2, 0, bn=128, pre=1, relu=1, tiles=1),
    row("h3-1x1-bn128-fold-s2", H3_1X1, "gaps", 3, 9, 11, 128, 256, 1, 2, 0, bn=128, pre=1, relu=1, tiles=1),
    row("h3-1x1-bn64-fold-s1", H3_1X1, "dense", 3, 7, 7, 128, 128, bn=64, pre=1, relu=1, tiles=2),
    row("h3-1x1-bn64-fold-s1", H3_1X1, "gaps", 3, 7, 7, 128, 128, bn=64, pre=1, relu=1, tiles=2),
    row("h3-1x1-bn128-epi-res", H3_1X1, "dense", 3, 7, 7, 64, 128, bn=128, stats=0, epi=1),
    row("h3-1x1-bn128-epi-res", H3_1X1, "gaps", 3, 7, 7, 64, 128, bn=128, stats=0, epi=1),
    row("h3-1x1-bn64-fold-epi", H3_1X1, "dense", 3, 7, 7, 64, 64, bn=64, pre=1, stats=0, epi=2),
    row("h3-1x1-bn64-fold-epi", H3_1X1, "gaps", 3, 7, 7, 64, 64, bn=64, pre=1, stats=0, epi=2),
    row("h3-1x1-bn64-fold-cin512", H3_1X1, "dense", 3, 5, 5, 512, 64, bn=64, pre=1, relu=1, tiles=1),   # kFoldMaxH

    # ---- capnet_conv2d_fwd_f16x3, k = 3: <bn, PRE, 9 taps>; without a fold the padding is the 0 / 1 factor
    row("h3-3x3-bn128-fold-s1-7x7", H3, "dense", 3, 7, 7, 64, 128, 3, 1, 1, bn=128, pre=1, relu=1, tiles=2),
    row("h3-3x3-bn128-fold-s1-7x7", H3, "gaps", 3, 7, 7, 64, 128, 3, 1, 1, bn=128, pre=1, relu=1, tiles=2),
    row("h3-3x3-bn64-fold-s2-9x11", H3, "dense", 3, 9, 11, 64, 64, 3, 2, 1, bn=64, pre=1, relu=1, tiles=1),
    row("h3-3x3-bn64-fold-s2-9x11", H3, "gaps", 3, 9, 11, 64, 64, 3, 2, 1, bn=64, pre=1, relu=1, tiles=1),
    row("h3-3x3-bn128-s2-9x11", H3, "dense", 3, 9, 11, 64, 128, 3, 2, 1, bn=128, tiles=1),
    row("h3-3x3-bn128-s2-9x11", H3, "gaps", 3, 9, 11, 64, 128, 3, 2, 1, bn=128, tiles=1),
    row("h3-3x3-bn64-s1-7x7", H3, "dense", 3, 7, 7, 64, 64, 3, 1, 1, bn=64, tiles=2),
    row("h3-3x3-bn64-s1-7x7", H3, "gaps", 3, 7, 7, 64, 64, 3, 1, 1, bn=64, tiles=2),
    row("h3-3x3-bn128-s1-9x11", H3, "dense", 3, 9, 11, 64, 128, 3, 1, 1, bn=128, tiles=3),
    row("h3-3x3-bn128-epi-res", H3, "dense", 3, 7, 7, 64, 128, 3, 1, 1, bn=128, stats=0, epi=1),
    row("h3-3x3-bn128-epi-res", H3, "gaps", 3, 7, 7, 64, 128, 3, 1, 1, bn=128, stats=0, epi=1),
    row("h3-3x3-bn64-fold-epi-9x11", H3, "dense", 3, 9, 11, 64, 64, 3, 1, 1, bn=64, pre=1, relu=1, stats=0, epi=2),
    row("h3-3x3-bn64-fold-epi-9x11", H3, "gaps", 3, 9, 11, 64, 64, 3, 1, 1, bn=64, pre=1, relu=1, stats=0, epi=2),
    # ... through capnet_conv2d_fwd_f16x3 with k = 1
    row("h3-k1-bn128-fold-s2", H3, "dense", 3, 9, 11, 64, 128, 1, 2, 0, bn=128, pre=1, tiles=1),
    row("h3-k1-bn128-fold-s2", H3, "gaps", 3, 9, 11, 64, 128, 1, 2, 0, bn=128, pre=1, tiles=1),
    # ---- capnet_conv2d_fwd_f16x3_scaled: in_exp != 0 (the operand is generated 2^-in_exp times the usual size)
    row("h3-scaled-3x3-bn128-e5", H3_SCALED, "dense", 3, 7, 7, 64, 128, 3, 1, 1, bn=128, in_exp=5, tiles=2),
    row("h3-scaled-3x3-bn128-e5", H3_SCALED, "gaps", 3, 7, 7, 64, 128, 3, 1, 1, bn=128, in_exp=5, tiles=2),
    row("h3-scaled-1x1-bn64-fold-e-3", H3_SCALED, "dense", 3, 7, 7, 64, 64, bn=64, pre=1, relu=1, in_exp=-3, tiles=2),
    row("h3-scaled-1x1-bn64-fold-e-3", H3_SCALED, "gaps", 3, 7, 7, 64, 64, bn=64, pre=1, relu=1, in_exp=-3, tiles=2),

    # ---- capnet_conv3x3_fwd_patch: <bn 64 / 128, K split or not> by shared_chip, <256>; dense only
    row("patch-5x3x3-bn64-shared0", PATCH, "dense", 5, 3, 3, 32, 64, 3, 1, 1, bn=64, shared=0, tiles=1),    # a tile of 5 images
    row("patch-5x3x3-bn64-shared1", PATCH, "dense", 5, 3, 3, 32, 64, 3, 1, 1, bn=64, shared=1, tiles=1),
    row("patch-5x3x3-bn256-fold-shared1", PATCH, "dense", 5, 3, 3, 32, 256, 3, 1, 1, bn=256, pre=1, relu=1, shared=1, tiles=1),
    row("patch-2x9x11-bn128-fold-shared0", PATCH, "dense", 2, 9, 11, 64, 128, 3, 1, 1, bn=128, pre=1, relu=1, shared=0, tiles=2),
    row("patch-2x9x11-bn128-fold-shared1", PATCH, "dense", 2, 9, 11, 64, 128, 3, 1, 1, bn=128, pre=1, relu=1, shared=1, tiles=2),
    row("patch-3x9x11-bn128-shared0", PATCH, "dense", 3, 9, 11, 64, 128, 3, 1, 1, bn=128, shared=0, tiles=3),
    row("patch-3x9x11-bn128-shared1", PATCH, "dense", 3, 9, 11, 64, 128, 3, 1, 1, bn=128, shared=1, tiles=3),
    row("patch-3x9x11-bn64-fold-shared0", PATCH, "dense", 3, 9, 11, 64, 64, 3, 1, 1, bn=64, pre=1, relu=1, shared=0, tiles=3),
    row("patch-3x9x11-bn256-shared0", PATCH, "dense", 3, 9, 11, 64, 256, 3, 1, 1, bn=256, shared=0, tiles=3),
    row("patch-3x9x11-nostats-bn128", PATCH, "dense", 3, 9, 11, 64, 128, 3, 1, 1, bn=128, pre=1, relu=1, stats=0),
    row("patch-1x3x59-bn64-fold-shared0", PATCH, "dense", 1, 3, 59, 32, 64, 3, 1, 1, bn=64, pre=1, relu=1, shared=0, tiles=2),   # W = 59
    row("patch-3x3x59-bn128-shared1", PATCH, "dense", 3, 3, 59, 32, 128, 3, 1, 1, bn=128, shared=1, tiles=5),
    row("patch-3x4x59-bn256-fold-shared0", PATCH, "dense", 3, 4, 59, 32, 256, 3, 1, 1, bn=256, pre=1, relu=1, shared=0, tiles=6),

    # ---- capnet_conv1x1_fwd_areg: <Cin / 32 = 2 / 4 / 8, PRE>; M = 1, 129, 300
    row("areg-m1-cin64-bn64", AREG, "dense", 1, 1, 1, 64, 64, bn=64, tiles=1),
    row("areg-m129-cin128-bn128-fold-relu", AREG, "dense", 129, 1, 1, 128, 128, bn=128, pre=1, relu=1, tiles=2),
    row("areg-m300-cin256-bn64-fold-relu", AREG, "dense", 300, 1, 1, 256, 128, bn=64, pre=1, relu=1, tiles=3),
    row("areg-m300-cin64-bn128-fold", AREG, "dense", 300, 1, 1, 64, 128, bn=128, pre=1, tiles=3),
    row("areg-m129-cin256-bn128-relu", AREG, "dense", 129, 1, 1, 256, 256, bn=128, relu=1, tiles=2),
    row("areg-m300-cin128-bn64", AREG, "dense", 300, 1, 1, 128, 64, bn=64, tiles=3),
    row("areg-m1-cin256-bn128-fold-relu", AREG, "dense", 1, 1, 1, 256, 128, bn=128, pre=1, relu=1, tiles=1),
    row("areg-m300-cin64-bn64-relu-nostats-e4", AREG, "dense", 300, 1, 1, 64, 64, bn=64, relu=1, stats=0, in_exp=4),

    # ---- capnet_conv1x1_fwd_tail: <bn 64 / 128 / 256>; Cin / 32 = 1, 2, 8, 16; M = 1, 129, 300
    row("tail-m1-cin32-bn64", TAIL, "dense", 1, 1, 1, 32, 64, bn=64, tiles=1),
    row("tail-m129-cin64-bn128-ds", TAIL, "dense", 129, 1, 1, 64, 128, bn=128, ds=1, tiles=2),
    row("tail-m300-cin256-bn256", TAIL, "dense", 300, 1, 1, 256, 256, bn=256, tiles=3),
    row("tail-m300-cin512-bn128-ds", TAIL, "dense", 300, 1, 1, 512, 256, bn=128, ds=1, tiles=3),
    row("tail-m129-cin512-bn256-ds", TAIL, "dense", 129, 1, 1, 512, 256, bn=256, ds=1, tiles=2),
    row("tail-m300-cin32-bn64-ds", TAIL, "dense", 300, 1, 1, 32, 64, bn=64, ds=1, tiles=3),
    row("tail-m1-cin256-bn128", TAIL, "dense", 1, 1, 1, 256, 128, bn=128, tiles=1),
    row("tail-m300-cin64-bn128-nostats", TAIL, "dense", 300, 1, 1, 64, 128, bn=128, stats=0),

    # ---- capnet_conv_stem_fwd_f16x3: rows = one per workgroup = B x OH x segments
    row("stem-7x8", STEM, "dense", 3, 7, 8, 3, 64, 7, 2, 3, tiles=12, nchw=1),             # the smallest eligible map
    row("stem-7x8", STEM, "gaps", 3, 7, 8, 3, 64, 7, 2, 3, tiles=12, nchw=1),
    row("stem-7x8-nostats", STEM, "dense", 3, 7, 8, 3, 64, 7, 2, 3, stats=0, nchw=1),
    row("stem-40x264", STEM, "dense", 1, 40, 264, 3, 64, 7, 2, 3, tiles=40, nchw=1),      # OW = 132: two segments, the second ragged
    row("stem-40x264", STEM, "gaps", 1, 40, 264, 3, 64, 7, 2, 3, tiles=40, nchw=1),
    row("stem-40x264-nostats", STEM, "gaps", 1, 40, 264, 3, 64, 7, 2, 3, stats=0, nchw=1),
    row("stem-9x520", STEM, "dense", 3, 9, 520, 3, 64, 7, 2, 3, tiles=45, nchw=1),         # OW = 260: three segments
    row("stem-9x520", STEM, "gaps", 3, 9, 520, 3, 64, 7, 2, 3, tiles=45, nchw=1),
]
del G, K, D

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "row names are unique"


def of(kernel):
    return [c for c in CASES if c.kernel == kernel]


def arm(c):
    """The instantiation a row exercises, as the issue lists them (what tests/test_conv_routes_cpu.py counts)."""
    if c.kernel == GENERIC:
        return (GENERIC, "nchw" if c.nchw else "nhwc", c.tile)
    if c.kernel == KMAJOR:
        return (KMAJOR, c.k, c.stride, bool(c.pre), c.tile)
    if c.kernel == DMA:
        return (DMA, c.stride, bool(c.stats))
    if c.kernel in (H3_1X1, H3):
        return (c.kernel, c.k, c.bn, bool(c.pre), c.stride)
    if c.kernel == PATCH:
        return (PATCH, c.shared, c.bn)
    if c.kernel == AREG:
        return (AREG, c.Cin, bool(c.pre))
    if c.kernel == TAIL:
        return (TAIL, c.bn, bool(c.ds))
    return (c.kernel,)


# ---- operands, float64 reference and magnitude (CPU) ----------------------------------------------------------------

def _key(c):
    """Rows that differ only in view form, tile, tile width, statistics or wave arrangement share their operands."""
    return c._replace(name="", view="", tile=0, bn=0, stats=0, shared=0, tiles=0, slab=0)


def reference(c):
    return _reference(_key(c))


@functools.lru_cache(maxsize=8)
def _reference(c):
    """The row's logical operands (fp32: x in the operand's own layout, w OIHW, fold / epilogue vectors, residual) and, in
    float64, ref = conv(relu?(x s + t), w) with mag = conv(|x| |s| + |t|, |w|) as [M][Cout]; with an output epilogue also
    ref_out / mag_out = mag |sc| + |sh| + |res|. For the tail kernel x is y3, the fold is
    relu(y3 s1 + t1 + res (s2 + t2)) and |res| (|s2|) + (|t2|) joins the magnitude."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in c.kernel) * 7919 + c.B * 131 + c.H * 17 + c.W * 29 + c.Cin * 3 +
                                      c.Cout * 5 + c.k + 11 * c.stride + 2 * c.pre + c.relu + 13 * c.epi + c.ds + 101 * c.in_exp)
    B, Cin, H, W, Cout, k = c.B, c.Cin, c.H, c.W, c.Cout, c.k
    # values spread over several binades, as activations and weights are
    x = torch.randn(B, Cin, H, W, generator=g) * torch.exp(0.5 * torch.randn(B, Cin, H, W, generator=g))
    x = x * 2.0 ** -c.in_exp
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05 * torch.exp(0.5 * torch.randn(Cout, Cin, k, k, generator=g))
    out = {"w": w}
    xd, a = x.double(), x.double().abs()
    if c.kernel == TAIL:
        res = torch.randn(B, Cin, H, W, generator=g)
        s1, t1 = torch.rand(Cin, generator=g) - 0.3, torch.randn(Cin, generator=g)
        v = lambda t: t.double().view(1, -1, 1, 1)
        xd, a = xd * v(s1) + v(t1), a * v(s1).abs() + v(t1).abs()
        if c.ds:
            s2, t2 = torch.rand(Cin, generator=g) - 0.3, torch.randn(Cin, generator=g)
            xd, a = xd + res.double() * v(s2) + v(t2), a + res.double().abs() * v(s2).abs() + v(t2).abs()
            out.update(s2=s2, t2=t2)
        else:
            xd, a = xd + res.double(), a + res.double().abs()
        xd = xd.clamp_min(0)
        out.update(res_in=res.permute(0, 2, 3, 1).reshape(B, Cin).contiguous(), scale=s1, shift=t1)
    elif c.pre:
        scale = torch.rand(Cin, generator=g) - 0.3                                # some negative scales
        shift = torch.randn(Cin, generator=g) * 2.0 ** -c.in_exp                  # (the prescale multiplies x s + t)
        v = lambda t: t.double().view(1, -1, 1, 1)
        xd, a = xd * v(scale) + v(shift), a * v(scale).abs() + v(shift).abs()
        out.update(scale=scale, shift=shift)
    if c.relu and c.kernel != TAIL:
        xd = xd.clamp_min(0)
    M = rows_m(c)

    def conv(t, wt):            # [M][Cout] in float64: the patches of every output pixel times the weight matrix
        cols = F.unfold(t, k, padding=c.pad, stride=c.stride)                       # [B][Cin k k][OH OW]
        return cols.transpose(1, 2).reshape(M, Cin * k * k) @ wt.reshape(Cout, Cin * k * k).t()
    ref, mag = conv(xd, w.double()), conv(a, w.double().abs())
    out.update(x=x if c.nchw else x.permute(0, 2, 3, 1).contiguous(), ref=ref, mag=mag, ref_out=ref, mag_out=mag)
    if c.epi:
        sc, sh = torch.rand(Cout, generator=g) - 0.3, torch.randn(Cout, generator=g)
        ro, mo = ref * sc.double() + sh.double(), mag * sc.double().abs() + sh.double().abs()
        if c.epi == 1:
            res = torch.randn(M, Cout, generator=g)
            ro, mo = (ro + res.double()).clamp_min(0), mo + res.double().abs()
            out.update(res=res)
        out.update(sc=sc, sh=sh, ref_out=ro, mag_out=mo)
    return out
