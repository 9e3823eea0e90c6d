"""Every row of tests/conv_cases.py on the device: the convolution family on fenced views, against float64.

Inputs (the activations, the weight image, the fold and epilogue vectors, the residual) sit in buffers whose every float
outside the operand's window is NaN: a fence in front and behind of at least one map row plus one pixel, and, in the `gaps`
form, the gap behind every pixel, row and image. Outputs (y, tail_out), statistics partials and slabs sit in buffers filled
with a sentinel bit pattern: at least 128 rows behind y, 4 rows behind the statistics, 64 floats behind the slabs. Per row:

  1. status 0;  2. every input buffer bit-identical to its copy from before the call;
  3. per element |y - ref| <= BOUND mag_out, and the window finite;
  4. per channel |sum_tiles psum - sum_rows ref| <= BOUND sum_rows mag;
  5. per channel |sum_tiles psq - sum_rows ref^2| <= 3 BOUND sum_rows mag^2 (2 |y| d + d^2 <= 2 BOUND mag^2 + BOUND^2 mag^2
     for the squares, one more BOUND for the positive sum);
  6. the first `tiles` statistics rows finite;  7. nothing outside an output window, past the used statistics rows or
  past the used slab floats changed;  8. a `gaps` row bit-identical to the same row run `dense`;
  9. the tail kernel's tail_out bit-identical to capnet_bn_add_relu.

ref = conv(relu?(x s + t), w) and mag = conv(|x| |s| + |t|, |w|) in float64 (conv_cases.reference). BOUND is the 2e-6
tests/test_gemm_views_gpu.py holds the f32 GEMM family to; it is not tuned to these kernels.

Isolation: every row of at least three images runs again with one middle image all NaN, then all Inf (the [M][Cin]
kernels: a block of rows; the tail kernel: y3 and the identity separately), without statistics. The other images' outputs
must be bit-identical to the clean run: an image's output depends on that image alone.

Worst error / bound per kernel on the MI355X (output, column sums, column sums of squares):
  capnet_conv2d_fwd 0.167 / 0.009 / 0.001        capnet_conv2d_fwd_kmajor 0.176 / 0.016 / 0.002
  capnet_conv1x1_fwd_dma 0.279 / 0.016 / 0.006   capnet_conv1x1_fwd_f16x3 0.081 / 0.018 / 0.002
  capnet_conv2d_fwd_f16x3 0.103 / 0.014 / 0.003  capnet_conv2d_fwd_f16x3_scaled 0.080 / 0.014 / 0.002
  capnet_conv3x3_fwd_patch 0.114 / 0.012 / 0.001 capnet_conv1x1_fwd_areg 0.069 / 0.030 / 0.008
  capnet_conv1x1_fwd_tail 0.044 / 0.020 / 0.002  capnet_conv_stem_fwd_f16x3 0.110 / 0.006 / 0.001
No kernel needed more than BOUND, so the fp32-oracle rule (max(2e-6, 2 x the fp32 CPU convolution's own ratio)) is unused."""
import pytest
import torch

import conv_cases as CC
from capnet._lib import current_stream, lib
from helpers import SENTINEL, Window, up4

pytestmark = pytest.mark.gpu

BOUND = 2e-6
Y_REAR_ROWS, STAT_REAR_ROWS, SLAB_TAIL = 128, 4, 64
WORST = {}                             # (kernel, what) -> worst error / bound seen so far
DENSE = {}                             # dense row name -> its outputs on the CPU (what the `gaps` rows must reproduce)


def note(kernel, what, ratio):
    WORST[(kernel, what)] = max(WORST.get((kernel, what), 0.0), ratio)


def report(kernel):
    print("worst error / bound on %-13s y %.3f  sum %.3f  sq %.3f" % (
        kernel, WORST.get((kernel, "y"), 0.0), WORST.get((kernel, "sum"), 0.0), WORST.get((kernel, "sq"), 0.0)))


def vec(t, dev):
    """A fold / epilogue vector in its own fenced buffer (None stays None)."""
    return None if t is None else Window(t, (1,), dev)


def p(w):
    return None if w is None else w.ptr


class Operands:
    """The device side of one row: every operand in a fenced buffer, packed weights included."""

    def __init__(self, c, dev, x=None, res_in=None):
        L, s = lib(), current_stream()
        r = CC.reference(c)
        self.c, self.M = c, CC.rows_m(c)
        sxb, sxh, sxw, sxc = CC.strides(c)
        x = r["x"] if x is None else x
        if c.kernel in (CC.AREG, CC.TAIL):
            fence = 2 * c.Cin
            self.x = Window(x.reshape(self.M, c.Cin), (c.Cin, 1), dev, pre=fence, post=fence)
        else:
            fence = up4(sxh + sxw)                      # one map row plus one pixel
            self.x = Window(x, (sxb, sxc, sxh, 1) if c.nchw else (sxb, sxh, sxw, 1), dev, pre=fence, post=fence)
        self.scale, self.shift = vec(r.get("scale"), dev), vec(r.get("shift"), dev)
        self.s2, self.t2 = vec(r.get("s2"), dev), vec(r.get("t2"), dev)
        self.sc, self.sh = vec(r.get("sc"), dev), vec(r.get("sh"), dev)
        self.res = None if r.get("res") is None else Window(r["res"], (c.Cout, 1), dev, pre=c.Cout + 4, post=c.Cout + 4)
        self.res_in = None
        if c.kernel == CC.TAIL:
            self.res_in = Window(r["res_in"] if res_in is None else res_in, (c.Cin, 1), dev, pre=2 * c.Cin, post=2 * c.Cin)
        # the weight image, packed by the library into the window of a fenced buffer
        wd = r["w"].to(dev)
        if c.kernel == CC.GENERIC:
            words = c.Cout * CC.k_rows(c)
        elif c.kernel == CC.KMAJOR:
            words = CC.k_rows(c) * c.Cout
        elif c.kernel == CC.DMA:
            words = c.Cout * c.Cin
        elif c.kernel == CC.STEM:
            words = L.capnet_conv_stem_f16x3_weight_words()
        else:
            words = L.capnet_conv_f16x3_weight_words(c.Cin, c.Cout, c.k)
        self.w = Window(torch.zeros(words), (1,), dev, pre=64, post=64)
        if c.kernel == CC.GENERIC:
            rc = L.capnet_pack_conv_weight(wd.data_ptr(), self.w.ptr, c.Cout, c.Cin, c.k, c.k, CC.k_rows(c), s)
        elif c.kernel == CC.KMAJOR:
            rc = L.capnet_pack_conv_weight_kmajor(wd.data_ptr(), self.w.ptr, c.Cout, c.Cin, c.k, c.k, CC.k_rows(c), s)
        elif c.kernel == CC.DMA:
            self.w = Window(r["w"].reshape(c.Cout, c.Cin), (c.Cin, 1), dev, pre=64, post=64)
            rc = 0
        elif c.kernel == CC.STEM:
            rc = L.capnet_conv_stem_f16x3_pack(wd.data_ptr(), self.w.ptr, s)
        else:
            rc = L.capnet_conv_f16x3_pack(wd.data_ptr(), self.w.ptr, c.Cout, c.Cin, c.k, c.bn, s)
        assert rc == 0, L.capnet_last_error()
        torch.cuda.synchronize()
        assert self.w.outside_unchanged(), "the weight pack wrote outside its image"
        self.w.snapshot()
        self.inputs = [("x", self.x), ("weights", self.w), ("in_scale", self.scale), ("in_shift", self.shift), ("s2", self.s2),
                       ("t2", self.t2), ("out_scale", self.sc), ("out_shift", self.sh), ("residual", self.res),
                       ("identity", self.res_in)]


def launch(c, ops, dev, stats):
    """One call of the row's entry on the row's views into freshly fenced outputs. Returns (status, outputs)."""
    L, s, M = lib(), current_stream(), ops.M
    nan = lambda rows, cols: torch.full((rows, cols), float("nan"))
    y = Window(nan(M, c.Cout), (c.Cout, 1), dev, pre=4 * c.Cout, post=Y_REAR_ROWS * c.Cout, fill_bits=SENTINEL)
    ps = pq = tail = slab = None
    if stats:
        ps = Window(nan(c.tiles, c.Cout), (c.Cout, 1), dev, pre=c.Cout, post=STAT_REAR_ROWS * c.Cout, fill_bits=SENTINEL)
        pq = Window(nan(c.tiles, c.Cout), (c.Cout, 1), dev, pre=c.Cout, post=STAT_REAR_ROWS * c.Cout, fill_bits=SENTINEL)
    sxb, sxh, sxw, sxc = CC.strides(c)
    x, w, k = ops.x.ptr, ops.w.ptr, c.kernel
    dims = (c.B, c.H, c.W, c.Cin, c.Cout)
    relu_out = 1 if c.epi == 1 else 0
    if k == CC.GENERIC:
        rc = L.capnet_conv2d_fwd(x, sxb, sxh, sxw, sxc, w, CC.k_rows(c), y.ptr, p(ops.scale), p(ops.shift), c.relu, p(ps), p(pq),
                                 *dims, c.k, c.k, c.stride, c.pad, c.tile, s)
    elif k == CC.KMAJOR:
        slab = torch.full((c.slab + SLAB_TAIL,), SENTINEL, dtype=torch.int32, device=dev)
        rc = L.capnet_conv2d_fwd_kmajor(x, sxb, sxh, sxw, w, CC.k_rows(c), y.ptr, p(ops.scale), p(ops.shift), c.relu, p(ps), p(pq),
                                        *dims, c.k, c.k, c.stride, c.pad, c.tile, slab.data_ptr(), s)
    elif k == CC.DMA:
        rc = L.capnet_conv1x1_fwd_dma(x, sxb, sxh, sxw, w, y.ptr, p(ps), p(pq), *dims, c.stride, p(ops.sc), p(ops.sh), p(ops.res),
                                      relu_out, s)
    elif k == CC.H3_1X1:
        rc = L.capnet_conv1x1_fwd_f16x3(x, sxb, sxh, sxw, w, c.bn, y.ptr, p(ops.scale), p(ops.shift), c.relu, p(ps), p(pq), *dims,
                                        c.stride, p(ops.sc), p(ops.sh), p(ops.res), relu_out, s)
    elif k == CC.H3:
        rc = L.capnet_conv2d_fwd_f16x3(x, sxb, sxh, sxw, w, c.bn, y.ptr, p(ops.scale), p(ops.shift), c.relu, p(ps), p(pq), *dims,
                                       c.k, c.stride, c.pad, p(ops.sc), p(ops.sh), p(ops.res), relu_out, s)
    elif k == CC.H3_SCALED:
        rc = L.capnet_conv2d_fwd_f16x3_scaled(x, sxb, sxh, sxw, w, c.bn, y.ptr, p(ops.scale), p(ops.shift), c.relu, p(ps), p(pq),
                                              *dims, c.k, c.stride, c.pad, c.in_exp, s)
    elif k == CC.PATCH:
        rc = L.capnet_conv3x3_fwd_patch(x, w, c.bn, y.ptr, p(ops.scale), p(ops.shift), c.relu, p(ps), p(pq), *dims, c.shared, s)
    elif k == CC.AREG:
        rc = L.capnet_conv1x1_fwd_areg(x, w, c.bn, y.ptr, p(ops.scale), p(ops.shift), c.relu, p(ps), p(pq), M, c.Cin, c.Cout,
                                       c.in_exp, s)
    elif k == CC.TAIL:
        tail = Window(nan(M, c.Cin), (c.Cin, 1), dev, pre=4 * c.Cin, post=Y_REAR_ROWS * c.Cin, fill_bits=SENTINEL)
        rc = L.capnet_conv1x1_fwd_tail(x, p(ops.scale), p(ops.shift), ops.res_in.ptr, p(ops.s2), p(ops.t2), tail.ptr, w, c.bn,
                                       y.ptr, p(ps), p(pq), M, c.Cin, c.Cout, s)
    else:
        rc = L.capnet_conv_stem_fwd_f16x3(x, sxb, sxc, sxh, w, y.ptr, p(ps), p(pq), c.B, c.H, c.W, s)
    torch.cuda.synchronize()
    return rc, {"y": y, "psum": ps, "psq": pq, "tail": tail, "slab": slab}


def bits(t):
    return t.contiguous().view(torch.int32)


def run_row(c, dev):
    """The row on its own view: assertions 1 to 7 and 9. Returns (failures, outputs on the CPU or None)."""
    L = lib()
    ops = Operands(c, dev)
    rc, out = launch(c, ops, dev, bool(c.stats))
    if rc != 0:
        return ["status %d: %s" % (rc, L.capnet_last_error())], None
    bad = []
    for name, win in ops.inputs:
        if win is not None and not win.unchanged():
            bad.append("input %s changed" % name)
    r = CC.reference(c)
    got = {"y": out["y"].inside().cpu()}
    for name in ("y", "psum", "psq", "tail"):
        if out[name] is not None and not out[name].outside_unchanged():
            bad.append("%s changed outside its window" % name)
    if out["slab"] is not None and not bool((out["slab"][c.slab:] == SENTINEL).all()):
        bad.append("slabs written past their %d used floats" % c.slab)
    y = got["y"]
    if not bool(torch.isfinite(y).all()):
        bad.append("non-finite output (%d elements)" % int((~torch.isfinite(y)).sum()))
    else:
        ratio = float(((y.double() - r["ref_out"]).abs() / (BOUND * r["mag_out"]).clamp_min(1e-300)).max())
        print("%-44s y %.3f" % (c.name, ratio), end="")
        note(c.kernel, "y", ratio)
        if ratio > 1.0:
            bad.append("output error %.3f of the bound" % ratio)
    if c.stats:
        ps, pq = out["psum"].inside().cpu(), out["psq"].inside().cpu()
        got.update(psum=ps, psq=pq)
        if not bool(torch.isfinite(ps).all() and torch.isfinite(pq).all()):
            bad.append("a statistics row among the first %d is not finite" % c.tiles)
        else:
            rs = float(((ps.double().sum(0) - r["ref"].sum(0)).abs() / (BOUND * r["mag"].sum(0))).max())
            rq = float(((pq.double().sum(0) - (r["ref"] ** 2).sum(0)).abs() / (3 * BOUND * (r["mag"] ** 2).sum(0))).max())
            print("  sum %.3f  sq %.3f" % (rs, rq), end="")
            note(c.kernel, "sum", rs)
            note(c.kernel, "sq", rq)
            if rs > 1.0:
                bad.append("column sums: error %.3f of the bound" % rs)
            if rq > 1.0:
                bad.append("column sums of squares: error %.3f of the bound" % rq)
    print()
    if c.kernel == CC.TAIL:
        want = torch.full((ops.M, c.Cin), float("nan"), device=dev)
        rc = L.capnet_bn_add_relu(ops.x.ptr, p(ops.scale), p(ops.shift), ops.res_in.ptr, p(ops.s2), p(ops.t2), want.data_ptr(),
                                  ops.M, c.Cin, current_stream())
        assert rc == 0, L.capnet_last_error()
        torch.cuda.synchronize()
        got["tail"] = out["tail"].inside().cpu()
        if not torch.equal(bits(got["tail"]), bits(want.cpu())):
            bad.append("tail_out differs from capnet_bn_add_relu (%d elements)" % int((got["tail"] != want.cpu()).sum()))
    return bad, got


def check_row(c, dev):
    bad, got = run_row(c, dev)
    if got is None:
        return bad
    if c.view == "dense":
        DENSE[c.name] = got
        return bad
    d = CC.dense(c)                                    # assertion 8: the same bits as on the dense view
    if d.name not in DENSE:
        bad_d, got_d = run_row(d, dev)
        if got_d is None:
            return bad + ["dense call failed: %s" % bad_d]
        DENSE[d.name] = got_d
    for name, t in got.items():
        if not torch.equal(bits(t), bits(DENSE[d.name][name])):
            bad.append("%s differs from the dense call (%d elements)" % (name, int((t != DENSE[d.name][name]).sum())))
    return bad


@pytest.mark.parametrize("kernel", CC.KERNELS)
def test_every_row_on_fenced_views(dev, kernel):
    rows = CC.of(kernel)
    assert rows
    failures = {}
    for c in rows:
        bad = check_row(c, dev)
        if bad:
            failures[c.name] = bad
    report(kernel)
    assert not failures, (len(failures), list(failures.items())[:8])


def test_every_row_of_the_table_belongs_to_a_kernel_that_runs():
    assert sum(len(CC.of(k)) for k in CC.KERNELS) == len(CC.CASES)


# ---- isolation: an image's output depends on that image alone ----

def poisoned_rows(c):
    """(first, one past last) row of the operand that is poisoned, as (image or matrix row) indices."""
    if c.kernel in (CC.AREG, CC.TAIL):
        return (60, 70) if c.B < 200 else (120, 135)           # inside a tile / across the boundary of two tiles
    return c.B // 2, c.B // 2 + 1


def isolation_rows(kernel):
    return [c for c in CC.of(kernel) if c.B >= 3]


def check_isolation(c, dev):
    L = lib()
    r = CC.reference(c)
    lo, hi = poisoned_rows(c)
    oh, ow = CC.out_hw(c)
    per = oh * ow                                      # output rows of one image (1 for the [M][Cin] kernels)
    keep = torch.ones(CC.rows_m(c), dtype=torch.bool)
    keep[lo * per:hi * per] = False
    clean_rc, clean = launch(c, Operands(c, dev), dev, False)
    if clean_rc != 0:
        return ["clean run: status %d: %s" % (clean_rc, L.capnet_last_error())]
    clean_y = clean["y"].inside().cpu()
    clean_tail = clean["tail"].inside().cpu() if clean["tail"] is not None else None
    bad = []
    if not bool(torch.isfinite(clean_y).all()):
        bad.append("clean run not finite")
    operands = ["x", "identity"] if c.kernel == CC.TAIL else ["x"]
    for which in operands:
        for value in (float("nan"), float("inf")):
            x, res_in = r["x"].clone(), None
            if which == "x":
                x[lo:hi] = value
            else:
                res_in = r["res_in"].clone()
                res_in[lo:hi] = value
            rc, out = launch(c, Operands(c, dev, x=x, res_in=res_in), dev, False)
            if rc != 0:
                bad.append("%s = %s: status %d: %s" % (which, value, rc, L.capnet_last_error()))
                continue
            y = out["y"].inside().cpu()
            if not torch.equal(bits(y[keep]), bits(clean_y[keep])):
                n = int((bits(y[keep]) != bits(clean_y[keep])).any(1).sum())
                bad.append("%s[%d:%d] = %s changed %d rows of other images" % (which, lo, hi, value, n))
            if not out["y"].outside_unchanged():
                bad.append("%s = %s: y changed outside its window" % (which, value))
            if clean_tail is not None and not torch.equal(bits(out["tail"].inside().cpu()[keep]), bits(clean_tail[keep])):
                bad.append("%s[%d:%d] = %s changed tail_out rows of other images" % (which, lo, hi, value))
    return bad


@pytest.mark.parametrize("kernel", CC.KERNELS)
def test_an_images_output_depends_on_that_image_alone(dev, kernel):
    rows = isolation_rows(kernel)
    assert rows, kernel
    failures = {}
    for c in rows:
        bad = check_isolation(c, dev)
        if bad:
            failures[c.name] = bad
    assert not failures, (len(failures), list(failures.items())[:8])
