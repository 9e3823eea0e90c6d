"""Every row of tests/pointwise_cases.py on the device: the loss, Adam, BatchNorm and pooling kernels on fenced views,
against float64.

Inputs sit in buffers whose every float outside the operand's window is NaN (helpers.Window), outputs and in-place
operands in buffers filled with a sentinel bit pattern; the windows start 0 or 1 float behind a 16-B boundary (0 or 4 for
the float4 kernels, which assume 16-B operands). The three large rows past a grid cap (pointwise_cases names them) use
contiguous buffers with a NaN / sentinel tail instead. The device error word is a private int32 between two sentinels.
Per row:

  1. status 0;  2. every input buffer bit-identical to its copy from before the call (in-place entries: the operands that
  are not updated);  3. every output window finite where the reference is and |got - ref| <= BOUND mag per element (the
  entries pointwise_cases.EXACT, and everything the table calls exact, to the bit);  4. nothing outside an output window
  changed;  5. the error word is what the row expects: 0 on every clean row.

ref and mag are pointwise_cases.reference's, in float64 from the float32 inputs as given. BOUND is the 2e-6 of
tests/test_gemm_views_gpu.py and tests/test_conv_views_gpu.py; it is not tuned to these kernels. dlogits alone has an
absolute allowance of 2^-126 beside it (pointwise_cases.ABS_FLOOR: float32 expf underflows where float64 does not).

clamp_adam runs its rounds on the device's own state: each round is measured against the float64 update of the float32
state the round started from. Its NaN row and the bad-target rows of xent run beside the same call without the bad
elements, and every other element is bit-identical.

Isolation (bn_add_relu row blocks, bn_relu_maxpool and global_avgpool images): a middle block all NaN, then all Inf,
leaves the other blocks' outputs bit-identical.

Error-word accumulation: a call with one bad index on a word preset to p leaves p | bit, for every raiser an exported
entry reaches (the raisers used atomicExch / atomicMax and erased or mangled p).

Worst error / bound per entry on the MI355X (topk, pack_tensors, clamp and adaptive_pool_replicate are exact):
  xent         lse 0.030  row_loss 0.037  loss 0.034  dlogits 0.071
  att_loss     colsum 0.113  out 0.016  dalphas 0.060
  clamp_adam   m 0.052  v 0.058  p 0.299
  bn1d         y 0.084  save_mean 0.030  save_invstd 0.046  rmean 0.054  rvar 0.059  dx 0.069  dgamma 0.078  dbeta 0.069
  bn_finalize  scale 0.050  shift 0.081  rmean 0.048  rvar 0.055
  bn_add_relu 0.059   bn_relu_maxpool 0.030   global_avgpool 0.071
No entry needed more than BOUND, so the fp32-oracle rule (max(2e-6, 2 x the CPU float32 ratio of the same row, which
tests/test_pointwise_cases_cpu.py prints)) is unused. The whole module takes about six seconds; the three rows past the
8192-workgroup caps are the issue's own examples and take about a second each, most of it their float64 reference."""
import ctypes

import pytest
import torch

import pointwise_cases as PC
from capnet._lib import current_stream, lib
from helpers import SENTINEL, Window

pytestmark = pytest.mark.gpu

BOUND = 2e-6
WORST = {}                             # (entry, output) -> worst error / bound seen so far
NAN = float("nan")


def note(entry, what, ratio):
    WORST[(entry, what)] = max(WORST.get((entry, what), 0.0), ratio)


def report(entry):
    print("worst error / bound on %-24s %s" % (entry, "  ".join(
        "%s %.3f" % (w, v) for (e, w), v in sorted(WORST.items()) if e == entry)))


def dense(shape):
    st, n = [], 1
    for d in reversed(shape):
        st.append(n)
        n *= d
    return tuple(reversed(st))


class Plain:
    """A contiguous buffer that starts at its allocation, with a tail of 1024 floats behind it: NaN (an input) or the
    sentinel (an output). The interface of Window that the checks use."""

    def __init__(self, dev, values=None, shape=None, tail=1024):
        self.shape = tuple(values.shape) if values is not None else tuple(shape)
        self.n = 1
        for d in self.shape:
            self.n *= d
        if values is not None:
            self.buf = torch.full((self.n + tail,), NAN, device=dev)
            self.buf[:self.n] = values.reshape(-1).to(dev)
        else:
            self.buf = torch.full((self.n + tail,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        self.before = self.buf.clone() if values is not None else None
        self.ptr = self.buf.data_ptr()

    def inside(self):
        return self.buf[:self.n].view(self.shape)

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))

    def outside_unchanged(self):
        return bool((self.buf[self.n:].view(torch.int32) == SENTINEL).all())


def win_in(t, dev, off=0, strides=None, plain=False):
    """An input in a NaN-fenced buffer (None stays None)."""
    if t is None:
        return None
    if plain:
        return Plain(dev, values=t)
    t = t.reshape(1) if t.dim() == 0 else t
    return Window(t, strides or dense(t.shape), dev, off=off, pre=8, post=8)


def win_out(shape, dev, off=0, strides=None, values=None, plain=False):
    """An output (NaN inside) or an in-place operand (`values` inside) in a sentinel-fenced buffer."""
    if plain:
        return Plain(dev, shape=shape)
    v = torch.full(tuple(shape), NAN) if values is None else values
    return Window(v, strides or dense(v.shape), dev, off=off, pre=16, post=64, fill_bits=SENTINEL)


def P(w):
    return None if w is None else w.ptr


class Word:
    """A private device error word between two sentinels."""

    def __init__(self, dev, preset=0):
        self.t = torch.tensor([SENTINEL, preset, SENTINEL], dtype=torch.int32, device=dev)
        self.ptr = self.t.data_ptr() + 4

    def value(self):
        a, v, b = self.t.cpu().tolist()
        assert a == SENTINEL and b == SENTINEL, "the word's neighbours changed"
        return v


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def bounded(bad, c, what, win, ref, mag, tag=""):
    """Assertion 3 for one output; returns what the window holds (CPU)."""
    got = win.inside().cpu().reshape(ref.shape)
    ok = torch.isfinite(ref)
    if not bool(torch.isfinite(got[ok]).all()):
        bad.append("%s%s: %d non-finite elements where the reference is finite" % (tag, what, int((~torch.isfinite(got[ok])).sum())))
        return got
    if bool(ok.any()):
        floor = PC.ABS_FLOOR.get(what, 0.0)
        ratio = float(((got.double() - ref).abs()[ok] / (BOUND * mag[ok] + floor).clamp_min(1e-300)).max())
        note(c.entry, what, ratio)
        if ratio > 1.0:
            bad.append("%s%s: error %.3f of the bound" % (tag, what, ratio))
    return got


def inputs_unchanged(bad, wins):
    for name, w in wins:
        if w is not None and not w.unchanged():
            bad.append("input %s changed" % name)


def outputs_fenced(bad, wins):
    for name, w in wins:
        if w is not None and not w.outside_unchanged():
            bad.append("%s changed outside its window" % name)


def status(bad, rc, what=""):
    if rc != 0:
        bad.append("%s status %d: %s" % (what, rc, lib().capnet_last_error()))
    return rc == 0


# ---- cross entropy ----

def xent_fwd(c, r, dev, targets):
    x = win_in(r["x"], dev, c.off, (c.ld, 1))
    t = targets.to(dev)
    outs = {"lse": win_out((c.N,), dev, c.off), "row_loss": win_out((c.N,), dev, 1 - c.off), "loss": win_out((1,), dev, c.off)}
    w = Word(dev)
    rc = lib().capnet_xent_fwd(x.ptr, c.ld, c.N, c.V, t.data_ptr(), outs["lse"].ptr, outs["row_loss"].ptr, outs["loss"].ptr, w.ptr,
                               current_stream())
    torch.cuda.synchronize()
    return rc, x, t, outs, w


def run_xent(c, dev):
    r, bad = PC.reference(c), []
    rc, x, t, outs, w = xent_fwd(c, r, dev, r["t"])
    if not status(bad, rc, "xent_fwd"):
        return bad
    inputs_unchanged(bad, [("logits", x)])
    if not torch.equal(t.cpu(), r["t"]):
        bad.append("targets changed")
    clean = {k: bounded(bad, c, k, outs[k], *r["out"][k]) for k in ("lse", "row_loss", "loss")}
    outputs_fenced(bad, outs.items())
    if w.value() != 0:
        bad.append("error word %d on a clean call" % w.value())
    if c.bad:
        rc, x, t, outs, w = xent_fwd(c, r, dev, r["t_bad"])
        if not status(bad, rc, "xent_fwd, bad targets"):
            return bad
        got = {k: bounded(bad, c, k, outs[k], *r["out_bad"][k], tag="bad targets: ") for k in ("lse", "row_loss", "loss")}
        outputs_fenced(bad, outs.items())
        if w.value() != 2:
            bad.append("bad targets: error word %d, expected 2" % w.value())
        if not same_bits(got["row_loss"][[0, 2]], torch.zeros(2)):
            bad.append("bad targets: row_loss of the bad rows is %s, expected 0" % got["row_loss"][[0, 2]].tolist())
        if not (same_bits(got["lse"], clean["lse"]) and same_bits(got["row_loss"][1], clean["row_loss"][1])):
            bad.append("bad targets: the other rows differ from the clean call")
        return bad
    # the backward call, handed float32(the reference's lse)
    lse = win_in(r["lse32"], dev, 1 - c.off)
    gout = win_in(r["gout"], dev, c.off)
    d = win_out((c.N, c.V), dev, c.off, (c.V + 5, 1))
    rc = lib().capnet_xent_bwd(x.ptr, c.ld, c.N, c.V, t.data_ptr(), lse.ptr, gout.ptr, d.ptr, c.V + 5, current_stream())
    torch.cuda.synchronize()
    if status(bad, rc, "xent_bwd"):
        inputs_unchanged(bad, [("logits", x), ("lse", lse), ("gout", gout)])
        bounded(bad, c, "dlogits", d, *r["out"]["dlogits"])
        outputs_fenced(bad, [("dlogits", d)])
    return bad


# ---- top-k accuracy ----

def run_topk(c, dev):
    r, bad = PC.reference(c), []
    x = win_in(r["x"], dev, c.off, (c.ld, 1))
    t = r["t"].to(dev)
    count = Word(dev, SENTINEL)
    w = Word(dev)
    rc = lib().capnet_topk_correct(x.ptr, c.ld, c.N, c.V, t.data_ptr(), c.k, count.ptr, w.ptr, current_stream())
    torch.cuda.synchronize()
    if not status(bad, rc):
        return bad
    inputs_unchanged(bad, [("logits", x)])
    if not torch.equal(t.cpu(), r["t"]):
        bad.append("targets changed")
    if count.value() != r["exact"]["count"]:
        bad.append("count %d, expected %d" % (count.value(), r["exact"]["count"]))
    if w.value() != (2 if c.bad else 0):
        bad.append("error word %d" % w.value())
    return bad


# ---- attention loss ----

def run_att(c, dev):
    r, bad = PC.reference(c), []
    L, s = lib(), current_stream()
    nll, al = win_in(r["nll"], dev, c.off), win_in(r["alphas"], dev, c.off)
    col, out = win_out((c.B, c.P), dev, c.off), win_out((1,), dev, 1 - c.off)
    rc = L.capnet_att_loss_fwd(nll.ptr, al.ptr, c.B, c.steps, c.P, c.alpha_c, col.ptr, out.ptr, s)
    torch.cuda.synchronize()
    if not status(bad, rc, "att_loss_fwd"):
        return bad
    inputs_unchanged(bad, [("nll", nll), ("alphas", al)])
    bounded(bad, c, "colsum", col, *r["out"]["colsum"])
    bounded(bad, c, "out", out, *r["out"]["out"])
    outputs_fenced(bad, [("colsum", col), ("out", out)])
    gout, col32 = win_in(r["gout"], dev, 1 - c.off), win_in(r["colsum32"], dev, c.off)
    dal = win_out((c.B, c.steps, c.P), dev, c.off)
    rc = L.capnet_att_loss_bwd(gout.ptr, col32.ptr, c.B, c.steps, c.P, c.alpha_c, dal.ptr, s)
    torch.cuda.synchronize()
    if status(bad, rc, "att_loss_bwd"):
        inputs_unchanged(bad, [("gout", gout), ("colsum", col32)])
        bounded(bad, c, "dalphas", dal, *r["out"]["dalphas"])
        outputs_fenced(bad, [("dalphas", dal)])
    return bad


# ---- clamp + Adam, pack ----

def ptrs(wins):
    return (ctypes.c_void_p * len(wins))(*[P(w) for w in wins])


def longs(vals):
    return (ctypes.c_long * len(vals))(*vals)


def state_windows(tensors, dev, shift):
    """Each tensor in a sentinel-fenced window of its own, at off 0 and 1 in turn; an empty tensor is a null pointer."""
    return [None if t.numel() == 0 else win_out(None, dev, (i + shift) % 2, values=t) for i, t in enumerate(tensors)]


def adam_call(c, dev, r, grads0, skip):
    """The row's rounds on fresh windows. Returns (failures, the windows, the last round's (g, m, v, p) on the CPU)."""
    bad = []
    W = {"p": state_windows(r["p"], dev, 0), "g": state_windows(grads0, dev, 1), "m": state_windows(r["m"], dev, 1),
         "v": state_windows(r["v"], dev, 0)}
    live = [i for i in range(c.count) if c.numel[i]]
    last = {}
    for k in range(c.rounds):
        if k:
            for i in live:
                W["g"][i].buf[W["g"][i].idx] = r["g"][k][i].to(dev)
        cur = {n: {i: W[n][i].inside().cpu() for i in live} for n in ("p", "g", "m", "v")}
        steps = (ctypes.c_int * c.count)(*[s + k for s in r["step"]])
        rc = lib().capnet_clamp_adam(c.count, ptrs(W["p"]), ptrs(W["g"]), ptrs(W["m"]), ptrs(W["v"]), longs(c.numel), steps,
                                     PC.LR, PC.B1, PC.B2, PC.EPS, c.clip, c.write_grad, P(skip), current_stream())
        torch.cuda.synchronize()
        if not status(bad, rc, "round %d:" % k):
            return bad, W, last
        if skip is not None and skip.value() != 0:
            for n in W:
                inputs_unchanged(bad, [("%s[%d] under a set skip word" % (n, i), W[n][i]) for i in live])
            continue
        for i in live:
            gc, ref = PC.adam_reference(cur["p"][i], cur["g"][i], cur["m"][i], cur["v"][i], r["step"][i] + k, c.clip)
            got_g = W["g"][i].inside().cpu()
            if not same_bits(got_g, gc if c.write_grad else cur["g"][i]):
                bad.append("round %d: g[%d] is not %s to the bit" % (k, i, "clamp(g)" if c.write_grad and c.clip > 0 else "unchanged"))
            last[i] = {"g": got_g}
            for n in ("m", "v", "p"):
                last[i][n] = bounded(bad, c, n, W[n][i], *ref[n], tag="round %d, tensor %d: " % (k, i))
                nan = torch.isnan(ref[n][0])
                if bool(nan.any()) and not bool(torch.isnan(last[i][n][nan]).all()):
                    bad.append("round %d: %s[%d] is finite where the gradient is NaN" % (k, n, i))
    for n in W:
        outputs_fenced(bad, [("%s[%d]" % (n, i), W[n][i]) for i in live])
    return bad, W, last


def run_adam(c, dev):
    r = PC.reference(c)
    skip = {"null": None, "zero": Word(dev, 0), "set": Word(dev, 4)}[c.skip]
    bad, _, got = adam_call(c, dev, r, r["g"][0], skip)
    if skip is not None and skip.value() != (4 if c.skip == "set" else 0):
        bad.append("the skip word changed")
    if not c.poison or bad:
        return bad
    # NaN in means NaN out; +-Inf behaves as +-clip; every other element as in the call without them
    bad_c, _, clean = adam_call(c, dev, r, r["g_clean"], skip)
    bad += ["clean call: " + b for b in bad_c]
    for i in got:
        keep = torch.ones(c.numel[i], dtype=torch.bool)
        keep[list(r["poisoned"].get(i, ()))] = False
        for n in ("g", "m", "v", "p"):
            if not same_bits(got[i][n][keep], clean[i][n][keep]):
                bad.append("%s[%d]: elements beside the NaN / Inf gradient differ from the call without them" % (n, i))
    (at_nan, at_inf), (at_ninf,) = r["poisoned"][2], r["poisoned"][44]
    if not all(bool(torch.isnan(got[2][n][at_nan])) for n in ("g", "m", "v", "p")):
        bad.append("the NaN gradient left %s" % {n: float(got[2][n][at_nan]) for n in ("g", "m", "v", "p")})
    if float(got[2]["g"][at_inf]) != c.clip or float(got[44]["g"][at_ninf]) != -c.clip:
        bad.append("+-Inf gradients were not clamped to +-clip")
    return bad


def run_pack(c, dev):
    r, bad = PC.reference(c), []
    live = [i for i in range(c.count) if c.numel[i]]
    total = sum(c.numel)
    if c.dir == 0:
        ts = [None if t.numel() == 0 else win_in(t, dev, i % 2) for i, t in enumerate(r["tensors"])]
        flat = win_out((total,), dev, 1)
    else:
        ts = [None if t.numel() == 0 else win_out((t.numel(),), dev, i % 2) for i, t in enumerate(r["tensors"])]
        flat = win_in(r["flat"], dev, 1)
    rc = lib().capnet_pack_tensors(c.count, ptrs(ts), longs(c.numel), flat.ptr, c.dir, c.scale, current_stream())
    torch.cuda.synchronize()
    if not status(bad, rc):
        return bad
    if c.dir == 0:
        inputs_unchanged(bad, [("tensor %d" % i, ts[i]) for i in live])
        if not same_bits(flat.inside().cpu(), r["exact"]["flat"]):
            bad.append("flat is not the concatenation to the bit")
        outputs_fenced(bad, [("flat", flat)])
    else:
        inputs_unchanged(bad, [("flat", flat)])
        for i in live:
            if not same_bits(ts[i].inside().cpu(), r["exact"]["tensors"][i]):
                bad.append("tensor %d is not flat x scale to the bit" % i)
        outputs_fenced(bad, [("tensor %d" % i, ts[i]) for i in live])
    return bad


def run_clamp(c, dev):
    r, bad = PC.reference(c), []
    x = win_out(None, dev, c.off, values=r["x"])
    rc = lib().capnet_clamp(x.ptr, c.n, c.lo, c.hi, current_stream())
    torch.cuda.synchronize()
    if not status(bad, rc):
        return bad
    if not same_bits(x.inside().cpu(), r["exact"]["x"]):
        bad.append("not torch.clamp to the bit (%d elements)" % int((bits(x.inside().cpu()) != bits(r["exact"]["x"])).sum()))
    outputs_fenced(bad, [("x", x)])
    return bad


# ---- BatchNorm1d, bn_finalize ----

def run_bn1d(c, dev):
    r, bad = PC.reference(c), []
    L, s, B, C, o = lib(), current_stream(), c.B, c.C, c.off
    train = c.mode != "eval"
    x, gamma, beta = win_in(r["x"], dev, o), win_in(r["gamma"], dev, 1 - o), win_in(r["beta"], dev, o)
    rm = rv = sm = si = None
    if c.mode != "train-norun":
        rm, rv = win_out(None, dev, o, values=r["rmean"]), win_out(None, dev, 1 - o, values=r["rvar"])
    if c.mode != "train-nosave":
        sm, si = win_out((C,), dev, 1 - o), win_out((C,), dev, o)
    y = win_out((B, C), dev, o)
    rc = L.capnet_bn1d_fwd(x.ptr, B, C, gamma.ptr, beta.ptr, P(rm), P(rv), int(train), r["momentum"], PC.BN_EPS, y.ptr, P(sm), P(si), s)
    torch.cuda.synchronize()
    if not status(bad, rc, "bn1d_fwd"):
        return bad
    inputs_unchanged(bad, [("x", x), ("gamma", gamma), ("beta", beta)] + ([] if train else [("running_mean", rm), ("running_var", rv)]))
    outs = {"y": y, "save_mean": sm, "save_invstd": si}
    if train:
        outs.update(rmean=rm, rvar=rv)
    got = {k: bounded(bad, c, k, w, *r["out"][k]) for k, w in outs.items() if w is not None}
    outputs_fenced(bad, list(outs.items()) + [("running_mean", rm), ("running_var", rv)])
    if train and (C >= 3 or B == 1):                   # the constant channel: beta to the bit
        col = 1 if C >= 3 else 0
        if not same_bits(got["y"][:, col], r["beta"][col].expand(B)):
            bad.append("y of the constant channel is not beta to the bit")
    if "dx" not in r["out"]:
        return bad
    dy, m32, i32 = win_in(r["dy"], dev, 1 - o), win_in(r["save_mean32"], dev, o), win_in(r["save_invstd32"], dev, 1 - o)
    dx, dg, db = win_out((B, C), dev, 1 - o), win_out((C,), dev, o), win_out((C,), dev, 1 - o)
    rc = L.capnet_bn1d_bwd(dy.ptr, x.ptr, B, C, gamma.ptr, m32.ptr, i32.ptr, dx.ptr, dg.ptr, db.ptr, s)
    torch.cuda.synchronize()
    if status(bad, rc, "bn1d_bwd"):
        inputs_unchanged(bad, [("dy", dy), ("x", x), ("gamma", gamma), ("save_mean", m32), ("save_invstd", i32)])
        for k, w in (("dx", dx), ("dgamma", dg), ("dbeta", db)):
            bounded(bad, c, k, w, *r["out"][k])
        outputs_fenced(bad, [("dx", dx), ("dgamma", dg), ("dbeta", db)])
    return bad


def run_finalize(c, dev):
    r, bad = PC.reference(c), []
    o = c.off
    ps, pq = win_in(r["psum"], dev, o), win_in(r["psq"], dev, 1 - o)
    gamma, beta = win_in(r["gamma"], dev, o), win_in(r["beta"], dev, 1 - o)
    rm = rv = None
    if c.running:
        rm, rv = win_out(None, dev, o, values=r["rmean"]), win_out(None, dev, 1 - o, values=r["rvar"])
    scale, shift = win_out((c.C,), dev, 1 - o), win_out((c.C,), dev, o)
    rc = lib().capnet_bn_finalize(ps.ptr, pq.ptr, c.tiles, c.C, c.count, P(gamma), P(beta), P(rm), P(rv), r["momentum"], PC.BN_EPS,
                                  scale.ptr, shift.ptr, current_stream())
    torch.cuda.synchronize()
    if not status(bad, rc):
        return bad
    inputs_unchanged(bad, [("part_sum", ps), ("part_sq", pq), ("gamma", gamma), ("beta", beta)])
    outs = {"scale": scale, "shift": shift, "rmean": rm, "rvar": rv}
    for k, w in outs.items():
        if w is not None:
            bounded(bad, c, k, w, *r["out"][k])
    outputs_fenced(bad, outs.items())
    return bad


# ---- the float4 kernels ----

def launch_add_relu(c, dev, r, y=None, res=None):
    o, pl = c.off, c.plain
    ins = {"y": win_in(r["y"] if y is None else y, dev, o, plain=pl), "s1": win_in(r["s1"], dev, o), "t1": win_in(r["t1"], dev, 4 - o),
           "res": win_in(r["res"] if res is None else res, dev, 4 - o, plain=pl), "s2": win_in(r["s2"], dev, o),
           "t2": win_in(r["t2"], dev, 4 - o)}
    out = win_out((c.rows, c.C), dev, o, plain=pl)
    rc = lib().capnet_bn_add_relu(ins["y"].ptr, ins["s1"].ptr, ins["t1"].ptr, P(ins["res"]), P(ins["s2"]), P(ins["t2"]), out.ptr,
                                  c.rows, c.C, current_stream())
    torch.cuda.synchronize()
    return rc, ins, out


def launch_maxpool(c, dev, r, y=None):
    o, pl = c.off, c.plain
    ins = {"y": win_in(r["y"] if y is None else y, dev, o, plain=pl), "scale": win_in(r["s"], dev, 4 - o), "shift": win_in(r["t"], dev, o)}
    out = win_out(((c.B, (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1, c.C)), dev, 4 - o, plain=pl)
    rc = lib().capnet_bn_relu_maxpool(ins["y"].ptr, ins["scale"].ptr, ins["shift"].ptr, out.ptr, c.B, c.H, c.W, c.C, current_stream())
    torch.cuda.synchronize()
    return rc, ins, out


def launch_avgpool(c, dev, r, x=None):
    ins = {"x": win_in(r["x"] if x is None else x, dev, c.off)}
    out = win_out((c.B, c.C), dev, 4 - c.off)
    rc = lib().capnet_global_avgpool(ins["x"].ptr, out.ptr, c.B, c.HW, c.C, current_stream())
    torch.cuda.synchronize()
    return rc, ins, out


def launch_upsample(c, dev, r, x=None):
    ins = {"x": win_in(r["x"], dev, c.off, plain=c.plain)}
    out = win_out((c.B, c.OUT, c.OUT, c.C), dev, 4 - c.off, plain=c.plain)
    rc = lib().capnet_adaptive_pool_replicate(ins["x"].ptr, out.ptr, c.B, c.S, c.OUT, c.C, current_stream())
    torch.cuda.synchronize()
    return rc, ins, out


LAUNCH4 = {PC.ADD_RELU: launch_add_relu, PC.MAXPOOL: launch_maxpool, PC.AVGPOOL: launch_avgpool, PC.UPSAMPLE: launch_upsample}


def run_float4(c, dev):
    r, bad = PC.reference(c), []
    rc, ins, out = LAUNCH4[c.entry](c, dev, r)
    if not status(bad, rc):
        return bad
    for w in list(ins.values()) + [out]:
        assert w is None or w.ptr % 16 == 0
    inputs_unchanged(bad, ins.items())
    if c.entry == PC.UPSAMPLE:
        if not same_bits(out.inside().cpu(), r["exact"]["out"]):
            bad.append("not the replicated map to the bit")
    else:
        got = bounded(bad, c, "out", out, *r["out"]["out"])
        if c.entry == PC.ADD_RELU and not same_bits(got[PC.negative_rows(c)], torch.zeros(len(PC.negative_rows(c)), c.C)):
            bad.append("the all-negative rows are not exactly 0")
    outputs_fenced(bad, [("out", out)])
    return bad


RUN = {PC.XENT: run_xent, PC.TOPK: run_topk, PC.ATT: run_att, PC.ADAM: run_adam, PC.PACK: run_pack, PC.CLAMP: run_clamp,
       PC.BN1D: run_bn1d, PC.FINALIZE: run_finalize, PC.ADD_RELU: run_float4, PC.MAXPOOL: run_float4, PC.AVGPOOL: run_float4,
       PC.UPSAMPLE: run_float4}


@pytest.mark.parametrize("entry", PC.ENTRIES)
def test_every_row_on_fenced_views(dev, entry):
    rows = PC.of(entry)
    assert rows
    failures = {}
    for c in rows:
        bad = RUN[entry](c, dev)
        if bad:
            failures[c.name] = bad
    report(entry)
    assert not failures, (len(failures), list(failures.items())[:8])


def test_every_row_of_the_table_belongs_to_an_entry_that_runs():
    assert sum(len(PC.of(e)) for e in RUN) == len(PC.CASES) and set(RUN) == set(PC.ENTRIES)


# ---- isolation: a block's output depends on that block alone ----

def isolation_rows(entry):
    if entry == PC.ADD_RELU:
        return [c for c in PC.of(entry) if c.rows >= 65 and not c.plain]
    return [c for c in PC.of(entry) if c.B >= 3 and not c.plain]


def check_isolation(c, dev):
    r, bad = PC.reference(c), []
    if c.entry == PC.ADD_RELU:
        lo, hi = c.rows // 3, c.rows // 3 + 7          # a block of rows (in the middle of the 256-thread groups)
        operands = [("y", r["y"])] + ([("res", r["res"])] if r["res"] is not None else [])
    else:
        lo, hi = c.B // 2, c.B // 2 + 1                # the middle image
        operands = [("y", r["y"])] if c.entry == PC.MAXPOOL else [("x", r["x"])]
    rc, _, out = LAUNCH4[c.entry](c, dev, r)
    if not status(bad, rc, "clean call:"):
        return bad
    clean = out.inside().cpu()
    keep = torch.ones(clean.shape[0], dtype=torch.bool)
    keep[lo:hi] = False
    if not bool(torch.isfinite(clean).all()):
        bad.append("clean call not finite")
    for name, t in operands:
        for value in (NAN, float("inf")):
            poisoned = t.clone()
            poisoned[lo:hi] = value
            rc, _, out = LAUNCH4[c.entry](c, dev, r, **{name: poisoned})
            if not status(bad, rc, "%s = %s:" % (name, value)):
                continue
            if not same_bits(out.inside().cpu()[keep], clean[keep]):
                bad.append("%s[%d:%d] = %s changed the output of other blocks" % (name, lo, hi, value))
            outputs_fenced(bad, [("%s = %s: out" % (name, value), out)])
    return bad


@pytest.mark.parametrize("entry", [PC.ADD_RELU, PC.MAXPOOL, PC.AVGPOOL])
def test_a_blocks_output_depends_on_that_block_alone(dev, entry):
    rows = isolation_rows(entry)
    assert rows, entry
    failures = {}
    for c in rows:
        bad = check_isolation(c, dev)
        if bad:
            failures[c.name] = bad
    assert not failures, (len(failures), list(failures.items())[:8])


# ---- the error word accumulates: preset | bit ----

def raise_target_xent(dev, w):
    x, t = torch.randn(3, 5, device=dev), torch.tensor([1, 7, 2], device=dev)
    o = torch.empty(7, device=dev)
    return lib().capnet_xent_fwd(x.data_ptr(), 5, 3, 5, t.data_ptr(), o.data_ptr(), o.data_ptr() + 12, o.data_ptr() + 24, w.ptr,
                                 current_stream())


def raise_target_topk(dev, w):
    x, t = torch.randn(3, 5, device=dev), torch.tensor([1, -1, 2], device=dev)
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    return lib().capnet_topk_correct(x.data_ptr(), 5, 3, 5, t.data_ptr(), 2, n.data_ptr(), w.ptr, current_stream())


def raise_target_policy(dev, w):
    x, t = torch.randn(3, 5, device=dev), torch.tensor([1, 2, 5], device=dev)      # two captions, steps of 2 and 1 rows
    adv, o = torch.ones(2, device=dev), torch.empty(9, device=dev)
    a = o.data_ptr()
    return lib().capnet_policy_xent_fwd(x.data_ptr(), 5, 3, 5, t.data_ptr(), adv.data_ptr(), 2, (ctypes.c_int * 2)(2, 1), 2,
                                        a, a + 12, a + 24, a + 32, w.ptr, current_stream())


def raise_token_embedding(dev, w):
    idx, emb = torch.tensor([0, 9, 3], device=dev), torch.randn(5, 8, device=dev)
    out = torch.empty(3, 8, device=dev)
    return lib().capnet_embedding_fwd(idx.data_ptr(), 3, emb.data_ptr(), 8, 5, out.data_ptr(), w.ptr, current_stream())


RAISERS = {"capnet_xent_fwd": (raise_target_xent, 2), "capnet_topk_correct": (raise_target_topk, 2),
           "capnet_policy_xent_fwd": (raise_target_policy, 2), "capnet_embedding_fwd": (raise_token_embedding, 1)}


@pytest.mark.parametrize("entry", sorted(RAISERS))
def test_a_raiser_adds_its_bit_to_the_error_word(dev, entry):
    call, bit = RAISERS[entry]
    wrong = {}
    for preset in (0, 4, 8, 32, 3 - bit):              # ... and the other kind's bit: 1 for the target raisers, 2 for the token raisers
        w = Word(dev, preset)
        rc = call(dev, w)
        torch.cuda.synchronize()
        assert rc == 0, lib().capnet_last_error()
        if w.value() != preset | bit:
            wrong[preset] = w.value()
    assert not wrong, "preset -> word, expected preset | %d: %s" % (bit, wrong)
