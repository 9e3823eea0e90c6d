"""The case table of the loss, optimiser, BatchNorm and pooling kernels (csrc/loss_optim.hip and the elementwise / pooling
half of csrc/bn_pool.hip): one named row per call, grouped by entry point, at the smallest shapes that still reach every
branch -- below, at and above the 256-thread stride, the 40-tensor table rollover, the three bn_finalize widths, the capped
grids. tests/test_pointwise_cases_cpu.py checks the table itself (no GPU); tests/test_pointwise_views_gpu.py runs every row
on fenced views against float64.

reference(row) gives the row's float32 inputs and, in float64 computed FROM those float32 inputs, every expected output
with a magnitude tensor of the same shape (`out`: name -> (ref, mag)); outputs that are compared to the bit are in `exact`.
A kernel is tested as a function of its inputs: a backward call is handed float32(the forward's reference) and its
reference starts from that same value. oracle32(row, r) is a plain float32 torch computation of the same operation, the
proof that BOUND x magnitude can be met. Where the issue's magnitude meets a non-finite input (-inf logits), that element
counts as 0: exp(-inf) adds nothing to any output.

off: the windows start `off` floats behind a 16-B boundary: 0 / 1 for the scalar kernels, 0 / 4 for the float4 kernels
(bn_add_relu, maxpool, avgpool, upsample assume 16-B operands). `plain`: the row lies past a grid cap and is large; it
runs on contiguous buffers with a sentinel tail instead of Window, whose index tensors would dominate its time. Those
rows are add_relu-16385x1024-past-cap, maxpool-11x113x113x256-past-cap and upsample-22x7to14x2048-past-cap (the two
attention-loss rows past their caps are small enough for Window)."""
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

XENT, TOPK, ATT, ADAM, PACK, CLAMP, BN1D, FINALIZE, ADD_RELU, MAXPOOL, AVGPOOL, UPSAMPLE = (
    "xent", "topk", "att_loss", "clamp_adam", "pack_tensors", "clamp", "bn1d", "bn_finalize", "bn_add_relu",
    "bn_relu_maxpool", "global_avgpool", "adaptive_pool_replicate")
ENTRIES = (XENT, TOPK, ATT, ADAM, PACK, CLAMP, BN1D, FINALIZE, ADD_RELU, MAXPOOL, AVGPOOL, UPSAMPLE)
ENTRY = {XENT: ("capnet_xent_fwd", "capnet_xent_bwd"), TOPK: ("capnet_topk_correct",),
         ATT: ("capnet_att_loss_fwd", "capnet_att_loss_bwd"), ADAM: ("capnet_clamp_adam",), PACK: ("capnet_pack_tensors",),
         CLAMP: ("capnet_clamp",), BN1D: ("capnet_bn1d_fwd", "capnet_bn1d_bwd"), FINALIZE: ("capnet_bn_finalize",),
         ADD_RELU: ("capnet_bn_add_relu",), MAXPOOL: ("capnet_bn_relu_maxpool",), AVGPOOL: ("capnet_global_avgpool",),
         UPSAMPLE: ("capnet_adaptive_pool_replicate",)}
FLOAT4 = (ADD_RELU, MAXPOOL, AVGPOOL, UPSAMPLE)
EXACT = (TOPK, PACK, CLAMP, UPSAMPLE)                 # entries whose every output is compared to the bit
NUMELS = (1, 255, 256, 257, 2047, 2048, 2049, 4097)   # around the 256 threads and the 2048-element chunk of a workgroup
STEPS = (1, 2, 1000, 100000)
LR, B1, B2, EPS = (float(np.float32(v)) for v in (2e-4, 0.9, 0.999, 1e-8))       # the float32 values the ABI receives
BN_EPS = float(np.float32(1e-5))
# An absolute allowance beside BOUND x magnitude, by output name: float32 expf underflows to 0 from x - lse < -87.3 on (a
# softmax below 2^-126), where the float64 reference still holds a value; the error there is the whole of that value.
ABS_FLOOR = {"dlogits": 2.0 ** -126}


class Row:
    def __init__(self, name, entry, **kw):
        self.__dict__.update(kw)
        self.name, self.entry = name, entry
        self.off = kw.get("off", 0)
        self.plain = kw.get("plain", False)
        assert self.off in ((0, 4) if entry in FLOAT4 else (0, 1)) and not (self.plain and self.off)

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return self.name == other.name

    def __repr__(self):
        return "Row(%s)" % self.name


def _xent_rows():
    kinds = ("s1", "s80", "off1e4", "neginf")
    rows, i = [], 0
    for V in (1, 5, 255, 256, 257, 1031):
        for N in (1, 3, 37):
            # ld = V or V + 3 (rows padded with NaN), windows at off 0 / 1; the four kinds rotate, three to a V
            rows.append(Row("xent-n%d-v%d-%s-ld%d-off%d" % (N, V, kinds[i % 4], V + 3 * (i % 2), (i // 2) % 2), XENT, N=N, V=V,
                            kind=kinds[i % 4], ld=V + 3 * (i % 2), off=(i // 2) % 2, first=i % 3 == 0, bad=False))
            i += 1
    for V, ld, off in ((5, 5, 0), (257, 260, 1)):          # targets -1 and V in one row each of a 3-row call
        rows.append(Row("xent-n3-v%d-bad-targets-ld%d-off%d" % (V, ld, off), XENT, N=3, V=V, kind="s1", ld=ld, off=off, first=True,
                        bad=True))
    return rows


def _topk_rows():
    rows = [Row("topk-n%d-v%d-k%d" % (N, V, k), TOPK, N=N, V=V, k=min(k, V), ld=V, off=o, bad=False)
            for (N, V, k), o in zip(((7, 37, 5), (1037, 8192, 5), (64, 7411, 1), (3, 4, 5)), (0, 0, 1, 1))]       # tests/test_eval_gpu.py's
    rows += [Row("topk-n5-v%d-k3-ld%d" % (V, V + 3), TOPK, N=5, V=V, k=3, ld=V + 3, off=o, bad=False)
             for V, o in ((255, 1), (256, 0), (257, 1))]
    rows.append(Row("topk-n0-writes-0", TOPK, N=0, V=37, k=5, ld=37, off=0, bad=False))
    rows.append(Row("topk-n7-v37-bad-targets", TOPK, N=7, V=37, k=5, ld=40, off=1, bad=True))
    return rows


def _att_rows():
    shapes = ((1, 1, 1), (3, 5, 196), (2, 7, 49), (5, 1, 257),
              (7, 2, 18727),           # B P = 131 089 > 131 072: the colsum kernel's 512 workgroups make a second trip
              (7, 13, 2897))           # B steps P = 263 627 > 262 144: the backward's 1024 workgroups make a second trip
    rows = []
    for i, (B, steps, P) in enumerate(shapes):
        for j, ac in enumerate((0.0, 1.0, 0.5)):
            if i >= 4 and j != i - 4 + 1:
                continue                                   # the two large rows once each: alpha_c 1 and 0.5
            rows.append(Row("att-%dx%dx%d-ac%g-off%d" % (B, steps, P, ac, (i + j) % 2), ATT, B=B, steps=steps, P=P, alpha_c=ac,
                            off=(i + j) % 2))
    return rows


def _numels(count, zeros):
    return [0 if i in zeros else NUMELS[(3 * i + count) % 8] for i in range(count)]


def _adam_rows():
    def r(name, count, zeros=(), clip=0.5, write_grad=1, skip="null", rounds=3, poison=False):
        return Row("adam-" + name, ADAM, count=count, numel=_numels(count, zeros), clip=clip, write_grad=write_grad, skip=skip,
                   rounds=rounds, poison=poison)
    return [
        r("1", 1, skip="zero"),
        r("40-full-table", 40),                                         # exactly one full table
        r("41-rollover", 41, skip="zero"),                              # a second launch for one tensor
        r("41-zeros-first-last", 41, zeros=(0, 40), clip=0.0),          # clip 0: g untouched
        r("41-no-write-grad", 41, write_grad=0),
        r("83-three-launches", 83),                                     # 40 + 40 + 3
        r("83-zeros-astride-40", 83, zeros=(0, 40, 41, 82), skip="zero"),   # ... and nothing but an empty tensor after a full table
        r("83-clip0-no-write", 83, zeros=(0, 82), clip=0.0, write_grad=0),
        r("41-skip-set", 41, skip="set", rounds=1),                     # a non-zero skip word: nothing moves
        r("83-skip-set", 83, zeros=(41,), skip="set", rounds=1),
        # one NaN and one +Inf gradient in the middle of tensor 2, one -Inf in the middle of tensor 44; one round, run
        # beside the same call without them
        r("83-nan-inf-grad", 83, rounds=1, poison=True),
    ]


def _pack_rows():
    return [Row("pack-%d%s-dir%d" % (count, "z" if zeros else "", d), PACK, count=count, numel=_numels(count, zeros), dir=d,
                scale=float(np.float32(0.37)))
            for count, zeros in ((1, ()), (40, ()), (41, ()), (41, (0, 40)), (83, ()), (83, (0, 40, 41, 82))) for d in (0, 1)]


def _clamp_rows():
    rows = [Row("clamp-n%d-off%d" % (n, o), CLAMP, n=n, lo=-0.5, hi=0.5, off=o)
            for n, o in ((0, 0), (1, 1), (255, 0), (257, 1), (1048576 + 257, 0))]         # the last: past the 4096 workgroups
    rows.append(Row("clamp-n257-lo-equals-hi", CLAMP, n=257, lo=0.25, hi=0.25, off=1))
    return rows


def _bn1d_rows():
    rows, i = [], 0
    for B in (1, 2, 12, 96):
        for C in (1, 63, 64, 65, 300):
            rows.append(Row("bn1d-b%d-c%d-train-off%d" % (B, C, i % 2), BN1D, B=B, C=C, mode="train", off=i % 2))
            i += 1
    for B, C in ((1, 65), (12, 300)):
        rows.append(Row("bn1d-b%d-c%d-train-no-running" % (B, C), BN1D, B=B, C=C, mode="train-norun", off=1))
        rows.append(Row("bn1d-b%d-c%d-train-no-save" % (B, C), BN1D, B=B, C=C, mode="train-nosave", off=0))
    for B, C in ((1, 1), (2, 64), (12, 65), (96, 300)):
        rows.append(Row("bn1d-b%d-c%d-eval" % (B, C), BN1D, B=B, C=C, mode="eval", off=B % 2))
    return rows


def _finalize_rows():
    rows = []
    Cs = (1, 16, 17, 50, 96)
    for i, tiles in enumerate((1, 16, 17, 127, 128, 129, 256, 257, 512, 513, 1025)):
        for j in range(2):                                 # every tile count at two widths, both counts, the four pointer forms
            C, k = Cs[(i + 3 * j) % 5], 2 * i + j
            rows.append(Row("finalize-t%d-c%d-n%s-%s%s" % (tiles, C, "1" if k % 2 else "7t", "affine" if k % 4 < 2 else "plain",
                                                           "-running" if (k // 2) % 3 else ""), FINALIZE, tiles=tiles, C=C,
                            count=1 if k % 2 else 7 * tiles, affine=k % 4 < 2, running=bool((k // 2) % 3), off=k % 2))
    return rows


def _add_relu_rows():
    rows, i = [], 0
    for n in (1, 3, 65, 1000):
        for C in (4, 64, 68, 256):
            rows.append(Row("add_relu-%dx%d-%s-off%d" % (n, C, ("plain", "res", "res-ds")[i % 3], 4 * (i % 2)), ADD_RELU, rows=n, C=C,
                            form=i % 3, off=4 * (i % 2)))
            i += 1
    # 16 385 x 256 quads > 2 x 8192 x 256: the loop's second trip
    rows.append(Row("add_relu-16385x1024-past-cap", ADD_RELU, rows=16385, C=1024, form=2, plain=True))
    return rows


def _maxpool_rows():
    rows, i = [], 0
    for H, W in ((1, 1), (2, 3), (7, 8), (12, 12), (13, 9)):
        for C in (4, 64, 68):
            rows.append(Row("maxpool-%dx%dx%dx%d-off%d" % (1 + 2 * (i % 2), H, W, C, 4 * ((i // 2) % 2)), MAXPOOL, B=1 + 2 * (i % 2),
                            H=H, W=W, C=C, off=4 * ((i // 2) % 2)))
            i += 1
    # 11 x 57 x 57 x 64 = 2 287 296 output quads > 8192 x 256
    rows.append(Row("maxpool-11x113x113x256-past-cap", MAXPOOL, B=11, H=113, W=113, C=256, plain=True))
    return rows


def _avgpool_rows():
    rows, i = [], 0
    for HW in (1, 3, 4, 5, 31, 32, 33, 49, 196):
        for C in (4, 252, 256, 260, 2048):
            rows.append(Row("avgpool-%dx%dx%d-off%d" % (1 + 2 * (i % 2), HW, C, 4 * ((i // 2) % 2)), AVGPOOL, B=1 + 2 * (i % 2), HW=HW,
                            C=C, off=4 * ((i // 2) % 2)))
            i += 1
    return rows


def _upsample_rows():
    rows, i = [], 0
    for S, OUT in ((1, 1), (1, 4), (7, 14), (3, 9)):
        for C in (4, 32, 36):
            rows.append(Row("upsample-%dx%dto%dx%d-off%d" % (1 + 2 * (i % 2), S, OUT, C, 4 * ((i // 2) % 2)), UPSAMPLE,
                            B=1 + 2 * (i % 2), S=S, OUT=OUT, C=C, off=4 * ((i // 2) % 2)))
            i += 1
    # 22 x 14 x 14 x 512 = 2 207 744 quads > 8192 x 256
    rows.append(Row("upsample-22x7to14x2048-past-cap", UPSAMPLE, B=22, S=7, OUT=14, C=2048, plain=True))
    return rows


CASES = (_xent_rows() + _topk_rows() + _att_rows() + _adam_rows() + _pack_rows() + _clamp_rows() + _bn1d_rows() +
         _finalize_rows() + _add_relu_rows() + _maxpool_rows() + _avgpool_rows() + _upsample_rows())
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "row names are unique"


def of(entry):
    return [c for c in CASES if c.entry == entry]


# ---- inputs, float64 references and magnitudes (CPU) -----------------------------------------------------------------

def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()))


@functools.lru_cache(maxsize=4)
def reference(c):
    return _REF[c.entry](c, _gen(c))


def _signed(n, g):
    """Scales away from zero, about a third of them negative."""
    return (0.2 + 0.8 * torch.rand(n, generator=g)) * torch.where(torch.rand(n, generator=g) < 0.35, -1.0, 1.0)


def _spread(shape, g):
    """Values spread over several binades, as activations are."""
    return torch.randn(shape, generator=g) * torch.exp(0.5 * torch.randn(shape, generator=g))


def _xent(c, g):
    N, V = c.N, c.V
    x = torch.randn(N, V, generator=g)
    t = torch.randint(0, V, (N,), generator=g)
    t[0], t[-1] = 0, V - 1                                 # the first column and the last
    if N == 1:
        t[0] = 0 if c.first else V - 1
    ar = torch.arange(N)
    if c.kind == "s80":
        x = x * 80                                         # expf overflows without the max subtraction
    elif c.kind == "off1e4":
        x = x + 1e4
    elif c.kind == "neginf":
        keep = x[ar, t].clone()
        x[torch.rand(N, V, generator=g) < 0.3] = float("-inf")
        x[ar, t] = keep                                    # ... never the target
    gout = torch.rand(1, generator=g) + 0.5
    out = {"x": x, "t": t, "gout": gout}
    xd = x.double()
    a = torch.where(torch.isfinite(xd), xd.abs(), torch.zeros_like(xd))
    lse = torch.logsumexp(xd, 1)
    row, mag = lse - xd[ar, t], a.max(1).values + math.log(V) + a[ar, t] + 1
    if c.bad:
        tb = t.clone()
        tb[0], tb[2] = -1, V
        row_b = row.clone()
        row_b[0] = row_b[2] = 0.0
        out.update(t_bad=tb, out_bad={"lse": (lse, mag), "row_loss": (row_b, mag), "loss": (row_b.mean().view(1), mag.mean().view(1))})
    lse32 = lse.float()
    sm = torch.exp(xd - lse32.double()[:, None])
    hot = F.one_hot(t, V).double()
    gn = gout.double() / N
    out.update(lse32=lse32, out={
        "lse": (lse, mag), "row_loss": (row, mag), "loss": (row.mean().view(1), mag.mean().view(1)),
        "dlogits": ((sm - hot) * gn, gn.abs() * (sm * (a + lse32.double().abs()[:, None] + 1) + hot))})
    return out


def _xent32(c, r):
    x, t, N = r["x"], r["t"], c.N
    lse = torch.logsumexp(x, 1)
    row = lse - x[torch.arange(N), t]
    d = (torch.exp(x - r["lse32"][:, None]) - F.one_hot(t, c.V).float()) * (r["gout"] * (torch.ones(1) / N))
    return {"lse": lse, "row_loss": row, "loss": row.mean().view(1), "dlogits": d}


def topk_count(x, t, k):
    """The kernel's stated rule: the target's rank is the number of entries that are larger, or equal with a lower index."""
    ok = (t >= 0) & (t < x.shape[1])
    tc = t.clamp(0, x.shape[1] - 1)
    tv = x[torch.arange(x.shape[0]), tc][:, None]
    beat = ((x > tv) | ((x == tv) & (torch.arange(x.shape[1])[None, :] < tc[:, None]))).sum(1)
    return int(((beat < k) & ok).sum())


def _topk(c, g):
    N = max(c.N, 1)
    x = torch.randint(-3, 4, (N, c.V), generator=g).float()            # integer values: ties everywhere
    t = torch.randint(0, c.V, (N,), generator=g)
    if c.bad:
        t[1], t[4] = -1, c.V
    return {"x": x, "t": t, "exact": {"count": topk_count(x, t, c.k) if c.N else 0}}


def _att(c, g):
    B, steps, P, ac = c.B, c.steps, c.P, float(np.float32(c.alpha_c))
    al = torch.rand(B, steps, P, generator=g) * 0.3
    nll, gout = torch.rand(1, generator=g) + 2.0, torch.rand(1, generator=g) + 0.5
    col = al.double().sum(1)
    mcol = al.double().abs().sum(1)
    col32 = col.float()
    k = gout.double() * ac * 2.0 / (B * P)
    dal = (k * (col32.double() - 1.0))[:, None, :].expand(B, steps, P)
    mdal = (k.abs() * (mcol + 1.0))[:, None, :].expand(B, steps, P)
    return {"alphas": al, "nll": nll, "gout": gout, "colsum32": col32, "out": {
        "colsum": (col, mcol),
        "out": (nll.double() + ac * ((1.0 - col) ** 2).mean(), nll.double().abs() + ac * ((1.0 + mcol) ** 2).mean()),
        "dalphas": (dal, mdal)}}


def _att32(c, r):
    al, ac = r["alphas"], torch.tensor(c.alpha_c)
    col = al.sum(1)
    k = r["gout"] * ac * 2.0 / torch.tensor(float(c.B * c.P))
    return {"colsum": col, "out": r["nll"] + ac * ((1.0 - col) ** 2).mean(),
            "dalphas": (k * (r["colsum32"] - 1.0))[:, None, :].expand(c.B, c.steps, c.P)}


def adam_scalars(step):
    """step_size and sqrt_bc2 as the launcher forms them: float64 pow, rounded to float32."""
    return (float(np.float32(LR / (1.0 - math.pow(B1, step)))), float(np.float32(math.sqrt(1.0 - math.pow(B2, step)))))


def adam_reference(p, g, m, v, step, clip):
    """One update of one tensor from its float32 state, by the kernel's own formula in float64. Returns the clamped
    gradient (float32, exact: torch.clamp keeps a NaN) and name -> (ref, mag) for m, v, p."""
    ss, sb = adam_scalars(step)
    gc = torch.clamp(g, -clip, clip) if clip > 0 else g
    gd, m0, v0, p0 = gc.double(), m.double(), v.double(), p.double()
    w1, w2 = 1.0 - B1, 1.0 - B2
    mn = m0 + w1 * (gd - m0)
    vn = v0 * B2 + w2 * gd * gd
    denom = vn.sqrt() / sb + EPS
    return gc, {"m": (mn, m0.abs() + w1 * (gd - m0).abs()), "v": (vn, B2 * v0.abs() + w2 * gd * gd),
                "p": (p0 - ss * (mn / denom), p0.abs() + ss * mn.abs() / denom)}


def adam32(p, g, m, v, step, clip):
    ss, sb = (torch.tensor(s) for s in adam_scalars(step))
    b1, b2 = torch.tensor(B1), torch.tensor(B2)
    gc = torch.clamp(g, -clip, clip) if clip > 0 else g
    mn = m + (1 - b1) * (gc - m)
    vn = v * b2 + (1 - b2) * gc * gc
    return {"m": mn, "v": vn, "p": p - ss * (mn / (vn.sqrt() / sb + torch.tensor(EPS)))}


def _tensors(numel, g, scale=1.0):
    return [torch.randn(n, generator=g) * scale for n in numel]


def _adam(c, g):
    out = {"p": _tensors(c.numel, g, 0.1), "m": _tensors(c.numel, g, 0.05),
           "v": [t.abs() * 0.01 + 1e-4 for t in _tensors(c.numel, g)],
           "g": [_tensors(c.numel, g) for _ in range(c.rounds)],        # |g| beyond the clip of 0.5 in a good third of the elements
           "step": [STEPS[i % 4] for i in range(c.count)]}
    if c.poison:
        out["g_clean"] = [t.clone() for t in out["g"][0]]
        mid = [n // 2 for n in c.numel]
        out["g"][0][2][mid[2]], out["g"][0][2][mid[2] + 1], out["g"][0][44][mid[44]] = float("nan"), float("inf"), float("-inf")
        out["poisoned"] = {2: (mid[2], mid[2] + 1), 44: (mid[44],)}
        assert c.numel[2] > 4 and c.numel[44] > 4
    return out


def _pack(c, g):
    ts = _tensors(c.numel, g)
    flat = torch.randn(sum(c.numel), generator=g)
    parts = torch.split(flat, c.numel)
    return {"tensors": ts, "flat": flat, "exact": {"flat": torch.cat(ts), "tensors": [q * torch.tensor(c.scale) for q in parts]}}


def _clamp(c, g):
    x = torch.randn(max(c.n, 1), generator=g)
    if c.n >= 255:
        x[7], x[100], x[101], x[254], x[c.n // 2] = float("nan"), float("inf"), float("-inf"), -0.0, float("nan")
    return {"x": x, "exact": {"x": torch.clamp(x, c.lo, c.hi) if c.n else x}}


def _bn1d(c, g):
    B, C = c.B, c.C
    x = torch.randn(B, C, generator=g)
    if C >= 3:
        x[:, 0] = 1e3 + 1e-2 * torch.randn(B, generator=g)             # mean 1e3, standard deviation 1e-2
        x[:, 1] = 0.37                                                 # constant: y is beta to the bit
    gamma, beta = _signed(C, g) + 0.0, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    dy = torch.randn(B, C, generator=g)
    mom = float(np.float32(0.01))
    out = {"x": x, "gamma": gamma, "beta": beta, "rmean": rm, "rvar": rv, "dy": dy, "momentum": mom}
    xd, gd, bd = x.double(), gamma.double(), beta.double()
    res = {}
    if c.mode == "eval":
        mean, invstd = rm.double(), 1.0 / (rv.double() + BN_EPS).sqrt()
    else:
        mean = xd.mean(0)
        q = ((xd - mean) ** 2).sum(0)
        var = q / B
        invstd = 1.0 / (var + BN_EPS).sqrt()
        unb = q / (B - 1) if B > 1 else var                            # running_var: unbiased, and biased at B = 1
        if c.mode != "train-norun":
            res["rmean"] = ((1 - mom) * rm.double() + mom * mean, (1 - mom) * rm.double().abs() + mom * mean.abs())
            res["rvar"] = ((1 - mom) * rv.double() + mom * unb, (1 - mom) * rv.double().abs() + mom * unb)
    res["y"] = ((xd - mean) * invstd * gd + bd, (xd.abs() + mean.abs()) * invstd * gd.abs() + bd.abs())
    if c.mode != "train-nosave":
        # both are a float64 value rounded once: mean |x| (not |mean|, which may cancel) and invstd are their sizes
        res["save_mean"] = (mean, xd.abs().mean(0) if c.mode != "eval" else mean.abs())
        res["save_invstd"] = (invstd, invstd)
    if c.mode in ("train", "train-norun"):                             # the backward call, from the float32 saves
        sm, si = mean.float(), invstd.float()
        xh = (xd - sm.double()) * si.double()
        dd = dy.double()
        s1, s2 = dd.sum(0), (dd * xh).sum(0)
        a1, a2 = dd.abs().sum(0), (dd * xh).abs().sum(0)
        k = gd * si.double() / B
        res["dx"] = (k * (B * dd - s1 - xh * s2), k.abs() * (B * dd.abs() + a1 + xh.abs() * a2))
        res["dgamma"], res["dbeta"] = (s2, a2), (s1, a1)
        out.update(save_mean32=sm, save_invstd32=si)
    out["out"] = res
    return out


def _bn1d32(c, r):
    x, gm, bt, B, mom = r["x"], r["gamma"], r["beta"], c.B, torch.tensor(r["momentum"])
    eps = torch.tensor(BN_EPS)
    o = {}
    if c.mode == "eval":
        mean, invstd = r["rmean"], 1.0 / (r["rvar"] + eps).sqrt()
    else:
        # the statistics in two passes with a double accumulator, as torch's own float32 batch norm has on the CPU (two
        # float32 passes lose save_invstd on the mean-1e3 channel); everything behind them in float32
        md = x.double().mean(0)
        mean, q = md.float(), ((x.double() - md) ** 2).sum(0).float()
        var = q / B
        invstd = 1.0 / (var + eps).sqrt()
        o["rmean"] = (1 - mom) * r["rmean"] + mom * mean
        o["rvar"] = (1 - mom) * r["rvar"] + mom * (q / (B - 1) if B > 1 else var)
    o.update(y=(x - mean) * invstd * gm + bt, save_mean=mean, save_invstd=invstd)
    if "save_mean32" in r:
        sm, si, dy = r["save_mean32"], r["save_invstd32"], r["dy"]
        xh = (x - sm) * si
        s1, s2 = dy.sum(0), (dy * xh).sum(0)
        o.update(dx=gm * si / B * (B * dy - s1 - xh * s2), dgamma=s2, dbeta=s1)
    return o


def _finalize(c, g):
    tiles, C, n = c.tiles, c.C, c.count
    mu, sd = 2 * torch.rand(C, generator=g) - 1, 0.5 + 1.5 * torch.rand(C, generator=g)
    if C >= 16:
        mu[1], sd[1] = 1e3, 0.25       # mean 1e3, variance 6e-8 of mean^2: gone in a float32 E[x^2] - E[x]^2, kept in float64
    xx = mu.double() + sd.double() * torch.randn(tiles, 7, C, generator=g, dtype=torch.float64)
    ps, pq = xx.sum(1).float(), (xx * xx).sum(1).float()               # [tiles][C]: 7 values per tile and channel
    if C >= 16:
        ps[:, 0], pq[:, 0] = 21.0, float(np.nextafter(np.float32(63.0), np.float32(0.0)))     # 7 x 3 and just under 7 x 9: q / n - mean^2 < 0
    gamma, beta = (_signed(C, g) + 0.0, torch.randn(C, generator=g)) if c.affine else (None, None)
    rm, rv = (torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5) if c.running else (None, None)
    mom = float(np.float32(0.1))
    out = {"psum": ps, "psq": pq, "gamma": gamma, "beta": beta, "rmean": rm, "rvar": rv, "momentum": mom}
    S, Q = ps.double().sum(0), pq.double().sum(0)
    mean = S / n
    raw = Q / n - mean * mean
    var = raw.clamp_min(0.0)
    invstd = 1.0 / (var + BN_EPS).sqrt()
    gd = gamma.double() if c.affine else torch.ones(C, dtype=torch.float64)
    bd = beta.double() if c.affine else torch.zeros(C, dtype=torch.float64)
    scale = gd * invstd
    res = {"scale": (scale, gd.abs() * invstd), "shift": (bd - mean * scale, bd.abs() + mean.abs() * scale.abs())}
    if c.running:
        unb = var * (n / (n - 1.0) if n > 1 else 1.0)
        res["rmean"] = ((1 - mom) * rm.double() + mom * mean, (1 - mom) * rm.double().abs() + mom * mean.abs())
        res["rvar"] = ((1 - mom) * rv.double() + mom * unb, (1 - mom) * rv.double().abs() + mom * unb)
    out.update(out=res, raw_var=raw)
    return out


def _finalize32(c, r):
    """The operation sums its partials in double by definition (as torch's own float32 batch norm does on the CPU); what is
    float32 here is everything behind the sums."""
    n = c.count
    S, Q = r["psum"].double().sum(0), r["psq"].double().sum(0)
    mean = S / n
    var = (Q / n - mean * mean).clamp_min(0.0)
    invstd, mean32 = (1.0 / (var + BN_EPS).sqrt()).float(), mean.float()
    scale = r["gamma"] * invstd if c.affine else invstd
    o = {"scale": scale, "shift": (r["beta"] if c.affine else 0.0) - mean32 * scale}
    if c.running:
        mom = torch.tensor(r["momentum"])
        o["rmean"] = (1 - mom) * r["rmean"] + mom * mean32
        o["rvar"] = (1 - mom) * r["rvar"] + mom * (var * (n / (n - 1.0) if n > 1 else 1.0)).float()
    return o


def negative_rows(c):
    """The rows of a bn_add_relu call whose every pre-ReLU value is negative: their output is exactly 0."""
    return [c.rows // 2, c.rows - 1] if c.rows >= 3 else []


def _add_relu(c, g):
    n, C = c.rows, c.C
    y = _spread((n, C), g)
    s1, t1 = _signed(C, g), torch.randn(C, generator=g)
    res = torch.randn(n, C, generator=g) if c.form else None
    s2, t2 = (_signed(C, g), torch.randn(C, generator=g)) if c.form == 2 else (None, None)
    for k in negative_rows(c):
        y[k] = -50.0 * torch.sign(s1)                                  # -50 |s1| <= -10, beyond any t1 + t2
        if res is not None:
            res[k] = 0.0
    ref = y.double() * s1.double() + t1.double()
    mag = y.double().abs_().mul_(s1.double().abs()).add_(t1.double().abs())
    if res is not None:
        rd = res.double()
        if s2 is not None:
            ref += rd * s2.double() + t2.double()
            mag += rd.abs() * s2.double().abs() + t2.double().abs()
        else:
            ref += rd
            mag += rd.abs()
    return {"y": y, "s1": s1, "t1": t1, "res": res, "s2": s2, "t2": t2, "pre_relu": ref, "out": {"out": (ref.clamp_min(0.0), mag)}}


def _add_relu32(c, r):
    v = r["y"] * r["s1"] + r["t1"]
    if r["res"] is not None:
        v = v + (r["res"] * r["s2"] + r["t2"] if r["s2"] is not None else r["res"])
    return {"out": torch.relu(v)}


def _maxpool(c, g):
    y = _spread((c.B, c.H, c.W, c.C), g)                               # NHWC
    s, t = _signed(c.C, g), torch.randn(c.C, generator=g)
    yd = y.double().permute(0, 3, 1, 2)
    v = lambda u: u.double().view(1, -1, 1, 1)
    ref = F.max_pool2d((yd * v(s) + v(t)).clamp_min_(0.0), 3, 2, 1)
    mag = F.max_pool2d(yd.abs() * v(s).abs() + v(t).abs(), 3, 2, 1)    # the window maximum of |a| |s| + |t|
    nhwc = lambda u: u.permute(0, 2, 3, 1).contiguous()
    return {"y": y, "s": s, "t": t, "out": {"out": (nhwc(ref), nhwc(mag))}}


def _maxpool32(c, r):
    v = lambda u: u.view(1, -1, 1, 1)
    a = torch.relu(r["y"].permute(0, 3, 1, 2) * v(r["s"]) + v(r["t"]))
    return {"out": F.max_pool2d(a, 3, 2, 1).permute(0, 2, 3, 1).contiguous()}


def _avgpool(c, g):
    x = _spread((c.B, c.HW, c.C), g)
    return {"x": x, "out": {"out": (x.double().mean(1), x.double().abs().mean(1))}}


def _upsample(c, g):
    x = torch.randn(c.B, c.S, c.S, c.C, generator=g)
    f = c.OUT // c.S
    return {"x": x, "exact": {"out": x.repeat_interleave(f, 1).repeat_interleave(f, 2).contiguous()}}


_REF = {XENT: _xent, TOPK: _topk, ATT: _att, ADAM: _adam, PACK: _pack, CLAMP: _clamp, BN1D: _bn1d, FINALIZE: _finalize,
        ADD_RELU: _add_relu, MAXPOOL: _maxpool, AVGPOOL: _avgpool, UPSAMPLE: _upsample}
_F32 = {XENT: _xent32, ATT: _att32, BN1D: _bn1d32, FINALIZE: _finalize32, ADD_RELU: _add_relu32, MAXPOOL: _maxpool32,
        AVGPOOL: lambda c, r: {"out": r["x"].mean(1)}}


def oracle32(c, r):
    """name -> float32 tensor for every bounded output of the row (clamp_adam: adam32, round by round)."""
    return _F32[c.entry](c, r)
