"""The case table of the recurrent step kernels (csrc/lstm_step.hip, lstm_decode_step.hip, lstm_upper_step.hip and the gate
kernels of seq_kernels.hip): one hand-written row per call, each named after the template arm it is there for, at the
smallest shapes that reach the arm. tests/test_step_cases_cpu.py checks the table itself (no GPU: coverage of every route
value through capnet_lstm_step_fused_route / capnet_stacked_decode_route, the refusals, the bounds against a float32
restatement, five deliberately wrong references); tests/test_step_views_gpu.py runs every row on fenced buffers.

Families (row.entry):
  FUSED   capnet_lstm_pack_wfrag + capnet_lstm_step_fused        lstm_step_fused_kernel<NGW, MT>, one or two row halves,
                                                                 XCD-major or plain workgroup map
  DECODE  capnet_stacked_decode_step / _cell / _gather / _groups / _tables
                                                                 lstm_decode_step_kernel<NJ, TM, TANH_OUT, GATHER>
  WIDE    capnet_att_decode_step[_groups]                        lstm_decode_step_wide_kernel<NJ, TANH_OUT, GATHER>
  UPPER   capnet_lstm_upper_step                                 lstm_upper_step_kernel<NJ, CELL>
  PW_FWD / PW_BWD  capnet_lstm_pointwise_fwd / _bwd              the gate kernels (no slabs: the slab-summing arms of the two
          kernels exist only below the C ABI, where the sequence drivers choose them; reaching them needs new product code,
          so they stay with the decoder tests)

inputs(row) gives the row's float32 operands from a generator seeded by the row's name (weights 0.06 U(-1, 1), |h| <= 0.3,
|c| <= 1); reference(row, inp) evaluates the operation in float64 FROM those float32 operands, restated here and not
imported from capnet, and returns name -> (ref, bound), both float64 and of the output's shape.

The bounds, written once (BOUND = 2e-6, the project's rule of 2e-6 x magnitude per element):
  pre-activation   pre = a + sum_k x_k w_k (a: the bias or the incoming gate value)
                   m = |a| + sum_k |x_k| |w_k|                      d_pre = BOUND m + sum_k |w_k| d_x_k
                   (d_x: the bound of an input that is itself a computed h -- an upper layer of the same call; else 0)
  activated gates  d_s = d_pre / 4 + BOUND |s| (sigmoid, |s'| <= 1/4)   d_g = d_pre + BOUND |g| (tanh, |tanh'| <= 1)
                   the second term is the gate's own float32 evaluation, 2e-6 of its own magnitude
  c = f c' + i g   d_c = |c'| d_f + |g| d_i + |i| d_g + BOUND (|f c'| + |i g|)        (|g|, |i| <= 1: at most the
                   issue's |c'| d_f + d_i + d_g + BOUND (...))
  h = o c          d_h = |c| d_o + |o| d_c + BOUND |o c|
  h = o tanh(c)    d_h = |tanh c| d_o + |o| (d_c + BOUND |tanh c|) + BOUND |o tanh c|
  pointwise_bwd    BOUND x the value of the same expression with every operand replaced by its magnitude and every
                   difference by a sum (1 - s -> 1 + s, 1 - g^2 -> 1 + g^2, dc_in + ... -> |dc_in| + ...): its inputs are
                   exact and each output is a product chain of at most six float32 roundings.
No absolute floor turned out to be needed: with the gate's own-magnitude term the float32 restatement (oracle32) stays below
0.2 of every bound (tests/test_step_cases_cpu.py prints the worst ratio per family).

`wrong` selects one of five deliberately wrong references (WRONG): they must land at least 10 bounds away on every row
they apply to (applies(row, wrong)), or the row could not see that class of error."""
import functools
import zlib

import torch

BOUND = 2e-6
FUSED, DECODE, WIDE, UPPER, PW_FWD, PW_BWD = "step_fused", "decode", "att_wide", "upper", "pointwise_fwd", "pointwise_bwd"
FAMILIES = (FUSED, DECODE, WIDE, UPPER, PW_FWD, PW_BWD)
WRONG = ("kgroup",      # one 16-wide k group dropped from the product
         "parent",      # parent[r] replaced by r
         "group",       # group g's weights used for group g + 1
         "swap",        # gate blocks o and c~ swapped
         "slot")        # layer l reading the state of slots 2l + 2, 2l + 3
VOCAB = 17              # table rows of the DECODE / WIDE rows that gather by token id (the attention step wants k <= V)
ATT_P, ATT_A, ATT_C = 3, 4, 2048
DROP_P = float(torch.tensor(0.3, dtype=torch.float32))


class Row:
    def __init__(self, name, entry, **kw):
        self.__dict__.update(kw)
        self.name, self.entry = name, entry

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return self.name == other.name

    def __repr__(self):
        return "Row(%s)" % self.name


def round16(v):
    return (v + 15) // 16 * 16


# ---- (a) capnet_lstm_step_fused: (H, b, gap floats between gate rows), each for both cells ----------------------------
# NGW = H padded to 64 / 128 / 256 / 512; MT 1 (b <= 16) / 2; halves 2 (b > 32); XCD-major map where H % 32 == 0
_FUSED = (
    (16, 1, 0), (48, 17, 12), (16, 33, 0),          # NGW 1, plain map:  MT 1 | MT 2 | two halves, second of 1 row
    (64, 15, 12), (64, 32, 0), (64, 49, 12),        # NGW 1 exact, XCD map
    (112, 16, 0), (112, 31, 12), (112, 63, 0),      # NGW 2 padded, plain map
    (96, 1, 12), (96, 17, 0), (96, 48, 12),         # NGW 2 padded, XCD map; second half of exactly 16 rows
    (144, 15, 0), (144, 32, 12), (144, 64, 0),      # NGW 4 padded, plain map
    (256, 16, 12), (256, 31, 0), (256, 33, 12),     # NGW 4 exact, XCD map
    (272, 1, 0), (272, 17, 12), (272, 49, 0),       # NGW 8 padded, plain map
    (320, 16, 12), (512, 32, 0), (512, 64, 12),     # NGW 8 padded / exact, XCD map (b = 64, H = 512: the shipped shape)
    (320, 63, 0),
)
FUSED_ROWS = [Row("fused-h%d-b%d-gap%d-cell%d" % (H, b, gap, cell), FUSED, H=H, b=b, gap=gap, cell=cell)
              for H, b, gap in _FUSED for cell in (0, 1)]


# ---- (b) the decode step: lstm_decode_step_kernel -------------------------------------------------------------------
# (name, C entry, cell, layers, E, H, groups, rows per group, layer-0 source, parents, x base offset in floats)
#   source "tok": token ids into a table [VOCAB][E]; "rows": input rows [rows][E]; "tables": one table per group
#   parents None / "id" / "perm" / "repeat" (inside the row's own group); xoff 1: the x base 4 bytes off 16-B alignment
# NJ by K = round16(E) + H: 2 (K <= 256), 4 (<= 512), 6 (<= 768), 8 (<= 1024), 12 (<= 1536), 16 (<= 2048, TM 1); an upper
# layer has K = 2H: NJ 2 / 2 / 4 / 8 / 16 at H = 64 / 128 / 256 / 512 / 1024
_DECODE = (
    ("nj2-e12-h64-one-row", "step", 0, 1, 12, 64, 1, 1, "tok", None, 0),            # K = 80: three waves own no k group
    ("nj2-e1-h64-scalar-x", "cell", 1, 1, 1, 64, 1, 15, "rows", None, 0),           # E % 4 != 0
    ("nj2-e12-h64-x-off-4-bytes", "gather", 0, 2, 12, 64, 1, 17, "rows", "perm", 1),  # E % 4 == 0, base misaligned; K = 128 above
    ("nj2-e12-h64-three-layers", "gather", 1, 3, 12, 64, 1, 33, "tok", "repeat", 0),
    ("nj4-e200-h128", "step", 0, 1, 200, 128, 1, 16, "tok", None, 0),               # K = 336
    ("nj4-e200-h128-lstm", "cell", 1, 2, 200, 128, 1, 31, "rows", None, 0),
    ("nj6-e300-h256-nj4-above", "step", 0, 2, 300, 256, 1, 32, "tok", None, 0),     # K = 560, then K = 512
    ("nj6-e300-h256-nj4-above-lstm", "cell", 1, 2, 300, 256, 1, 49, "rows", None, 0),
    ("nj6-e300-h256-nj4-above-gather", "gather", 0, 2, 300, 256, 1, 48, "tok", "perm", 0),
    ("nj6-e300-h256-nj4-above-lstm-gather", "gather", 1, 2, 300, 256, 1, 17, "rows", "repeat", 0),
    ("nj8-e300-h512", "step", 0, 1, 300, 512, 1, 17, "tok", None, 0),               # K = 816
    ("nj8-e300-h512-lstm", "cell", 1, 1, 300, 512, 1, 16, "rows", None, 0),
    ("nj8-e300-h512-gather-id", "gather", 0, 2, 300, 512, 1, 33, "rows", "id", 0),    # K = 1024 above
    ("nj8-e300-h512-lstm-gather", "gather", 1, 1, 300, 512, 1, 15, "tok", "perm", 0),
    ("nj12-e100-h1024-nj16-above", "step", 0, 2, 100, 1024, 1, 17, "tok", None, 0),  # K = 1136, then K = 2048 (TM 1)
    ("nj12-e100-h1024-nj16-above-lstm", "cell", 1, 2, 100, 1024, 1, 5, "rows", None, 0),
    ("nj12-e100-h1024-nj16-above-gather", "gather", 0, 2, 100, 1024, 1, 33, "tok", "repeat", 0),
    ("nj12-e100-h1024-nj16-above-lstm-gather", "gather", 1, 2, 100, 1024, 1, 16, "rows", "perm", 0),
    ("nj16-e1000-h1024-tm1", "cell", 0, 1, 1000, 1024, 1, 49, "tok", None, 0),      # K = 2032: four passes of 16 rows
    ("nj16-e1000-h1024-tm1-lstm-gather", "gather", 1, 1, 1000, 1024, 1, 17, "rows", "perm", 0),
    ("groups-2x17-e12-h64", "groups", 0, 2, 12, 64, 2, 17, "tok", "perm", 0),       # a tile ends inside the launch's rows
    ("groups-3x16-e200-h128-lstm", "groups", 1, 1, 200, 128, 3, 16, "rows", "repeat", 0),
    ("groups-8x5-e300-h256-no-parents", "groups", 0, 1, 300, 256, 8, 5, "tok", None, 0),
    ("groups-8x1-e12-h64-lstm", "groups", 1, 2, 12, 64, 8, 1, "rows", "perm", 0),
    ("groups-1x33-e300-h512", "groups", 0, 1, 300, 512, 1, 33, "tok", "repeat", 0),
    ("tables-2x5-e12-h64-lstm", "tables", 1, 2, 12, 64, 2, 5, "tables", "perm", 0),
    ("tables-3x16-e200-h128", "tables", 0, 1, 200, 128, 3, 16, "tables", None, 0),
    ("tables-8x1-e300-h256-lstm", "tables", 1, 1, 300, 256, 8, 1, "tables", "repeat", 0),
    ("tables-1x17-e1-h64-scalar-x", "tables", 1, 1, 1, 64, 1, 17, "tables", "id", 0),
)
DECODE_ROWS = [Row("decode-" + n, DECODE, centry=ce, cell=c, L=L, E=E, H=H, groups=G, rpg=rpg, src=src, parents=par, xoff=xo)
               for n, ce, c, L, E, H, G, rpg, src, par, xo in _DECODE]

# ---- (c) the wide kernel through capnet_att_decode_step[_groups]: P = 3, A = 4, C = 2048 ------------------------------
# (name, cell, layers, E, H, groups, images, beams, parents): a group's rows n k in {1, 16, 17, 33, 49}; `tiles` is 1 at
# 1 and 16 rows, 2 at 17, (2, 1) at 33, (2, 2) at 49
_WIDE = (
    ("w12-k2128-h64-49-rows", 0, 2, 12, 64, 1, 7, 7, "perm"),          # wide <12> at its lower edge; an upper layer behind it
    ("w12-k2128-h64-2x17-lstm", 1, 1, 12, 64, 2, 17, 1, None),
    ("w12-k2128-h64-2x16", 0, 1, 12, 64, 2, 1, 16, "repeat"),
    ("w12-k3072-h512-33-rows-lstm", 1, 1, 512, 512, 1, 11, 3, "perm"),  # 24 groups per wave: both halves full
    ("w12-k3072-h512-one-row", 0, 1, 512, 512, 1, 1, 1, None),
    ("w12-k3072-h512-2x16-lstm", 1, 1, 512, 512, 2, 2, 8, "repeat"),
    ("w16-k3088-h1024-17-rows", 0, 1, 16, 1024, 1, 17, 1, "perm"),     # wide <16> at its lower edge: ng 24 / 25
    ("w16-k3088-h1024-16-rows-lstm", 1, 1, 16, 1024, 1, 1, 16, None),
    ("w16-k4096-h1024-49-rows-lstm", 1, 1, 1024, 1024, 1, 7, 7, "repeat"),   # every wave at ng = 2 NJ
    ("w16-k4096-h1024-33-rows", 0, 1, 1024, 1024, 1, 11, 3, None),
)
WIDE_ROWS = [Row("wide-" + nm, WIDE, cell=c, L=L, E=E, H=H, groups=G, n=n, k=k, rpg=n * k, parents=par, src="xa", xoff=0)
             for nm, c, L, E, H, G, n, k, par in _WIDE]

# ---- (d) capnet_lstm_upper_step: (H, b, cell, dropout) -----------------------------------------------------------------
_UPPER = (
    (64, 1, 0, 0), (64, 16, 1, 0), (128, 5, 1, 0), (128, 15, 0, 0), (256, 15, 1, 0), (256, 16, 0, 0), (512, 1, 1, 0),
    (512, 5, 0, 0), (1024, 16, 1, 0), (1024, 15, 0, 0),               # NJ 1 / 2 / 4 / 8 / 16 for both cells, dropout off
    (64, 5, 0, 1), (256, 16, 1, 1), (1024, 15, 0, 1), (128, 1, 1, 1),  # p = 0.3
)
UPPER_ROWS = [Row("upper-h%d-b%d-cell%d%s" % (H, b, c, "-dropout" if d else ""), UPPER, H=H, b=b, cell=c, dropout=d)
              for H, b, c, d in _UPPER]

# ---- (e) the gate kernels: b H below, at and above one 256-thread workgroup, and not a multiple of it ------------------
_PW = ((1, 16), (3, 28), (16, 16), (5, 100), (64, 512))
PW_FWD_ROWS = [Row("pwfwd-b%d-h%d-cell%d-%s" % (b, H, c, "cprev" if cp else "null"), PW_FWD, b=b, H=H, cell=c, cprev=cp)
               for b, H in _PW for c in (0, 1) for cp in (True, False)]
PW_BWD_ROWS = [Row("pwbwd-b%d-h%d-cell%d-%s" % (b, H, c, "cprev" if cp else "null"), PW_BWD, b=b, H=H, cell=c, cprev=cp)
               for b, H in _PW for c in (0, 1) for cp in (True, False)]

ROWS = FUSED_ROWS + DECODE_ROWS + WIDE_ROWS + UPPER_ROWS + PW_FWD_ROWS + PW_BWD_ROWS
BY_NAME = {r.name: r for r in ROWS}


def rows_of(entry):
    return [r for r in ROWS if r.entry == entry]


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _uni(g, shape, scale):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


@functools.lru_cache(maxsize=1)
def weight_pool():
    """4096 x 4096 weights, 0.06 U(-1, 1), built once: every large weight matrix of the table is a slice of it."""
    return _uni(torch.Generator().manual_seed(20240607), (4096 * 4096,), 0.06)


class _Take:
    def __init__(self):
        self.at = 0

    def __call__(self, *shape):
        n = 1
        for d in shape:
            n *= d
        assert self.at + n <= 4096 * 4096
        w = weight_pool()[self.at:self.at + n].view(shape)
        self.at += n
        return w


def roles(row):
    """The gate block (of the 4H columns as the entry stores them) of each role i, f, o, c~."""
    stored_ifgo = row.entry in (FUSED, UPPER, PW_FWD, PW_BWD) and row.cell == 1
    return (0, 1, 3, 2) if stored_ifgo else (0, 1, 2, 3)


def parents_of(row, g):
    G, rpg = row.groups, row.rpg
    if row.parents is None:
        return None
    out = []
    for q in range(G):
        if row.parents == "id":
            p = torch.arange(rpg)
        elif row.parents == "perm":
            p = torch.randperm(rpg, generator=g)
            if rpg > 1 and bool((p == torch.arange(rpg)).all()):
                p = p.roll(1)
        else:
            p = torch.randint(0, max(1, rpg // 2), (rpg,), generator=g)       # the lower half, each about twice
        out.append(p + q * rpg)
    return torch.cat(out).long()


def inputs(row):
    g = _gen(row.name)
    e = row.entry
    if e == FUSED:
        H, b = row.H, row.b
        return dict(w=_uni(g, (4 * H, H), 0.06), gates=torch.randn(b, 4 * H, generator=g), h_prev=_uni(g, (b, H), 0.3),
                    c_prev=_uni(g, (b, H), 1.0))
    if e in (DECODE, WIDE):
        H, L, G, R = row.H, row.L, row.groups, row.groups * row.rpg
        take = _Take()
        xn0 = row.E + (ATT_C if e == WIDE else 0)
        inp = dict(wcat=[], beff=[], xn0=xn0)
        for l in range(L):
            xn = xn0 if l == 0 else H
            w = take(G, 4 * H, round16(xn) + H)
            if round16(xn) != xn:
                w = w.clone()
                w[:, :, xn:round16(xn)] = 0.0                   # the zero columns the entry's contract puts there
            inp["wcat"].append(w)
            inp["beff"].append(_uni(g, (G, 4 * H), 0.1))
        st = _uni(g, (R, 2 * L, H), 1.0)
        st[:, 0::2] *= 0.3
        inp["state_in"] = st
        inp["parents"] = parents_of(row, g)
        ntab = G if row.src == "tables" else 1
        if row.src == "rows":
            inp["x"] = _uni(g, (R, row.E), 0.5)
        else:
            inp["tables"] = [_uni(g, (VOCAB, row.E), 0.5) for _ in range(ntab)]
            inp["tokens"] = torch.randint(0, VOCAB, (R,), generator=g).long()
        if e == WIDE:
            n = row.n
            inp.update(att1=_uni(g, (G * n, ATT_P, ATT_A), 0.5), feat=_uni(g, (n, ATT_P, ATT_C), 0.5),
                       wz=_uni(g, (G, ATT_A + ATT_C, H), 0.06), bz=_uni(g, (G, ATT_A + ATT_C), 0.1),
                       w_full=_uni(g, (G, ATT_A), 0.5), b_full=_uni(g, (G,), 0.1))
        return inp
    if e == UPPER:
        H, b = row.H, row.b
        take = _Take()
        return dict(xin=_uni(g, (b, H), 0.3), h_prev=_uni(g, (b, H), 0.3), c_prev=_uni(g, (b, H), 1.0), w_eff=take(4 * H, H),
                    w_rec=take(4 * H, H), b_eff=_uni(g, (4 * H,), 0.1), seed=zlib.crc32(row.name.encode()) * 977 + 5, r0=3, layer=1)
    b, H = row.b, row.H
    pre = torch.randn(b, 4 * H, generator=g) * 1.5
    cp = _uni(g, (b, H), 1.0) if row.cprev else None
    if e == PW_FWD:
        return dict(pre=pre, c_prev=cp)
    # the backward is a function of its inputs: float32(the forward's float64 result on a fresh pre)
    f = _cell(_blocks(pre.double(), roles(row), H), None, None if cp is None else cp.double(), row.cell == 1, torch.float64)
    gates = _unblocks([f[k][0] for k in "ifog"], roles(row)).float()
    return dict(gates=gates, c=f["c"][0].float(), c_prev=cp, dh=torch.randn(b, H, generator=g), dc=torch.randn(b, H, generator=g))


# ---- the cell, in any float type ------------------------------------------------------------------------------------------
def _blocks(pre, role_blocks, H):
    """[R][4H] -> the four roles (i, f, o, c~), each [R][H]."""
    return [pre[:, k * H:(k + 1) * H] for k in role_blocks]


def _unblocks(vals, role_blocks):
    """The roles' values back into the entry's block order, [R][4H]."""
    order = sorted(range(4), key=lambda r: role_blocks[r])
    return torch.cat([vals[r] for r in order], 1)


def _cell(pre, dpre, cp, tanh_out, dt):
    """pre: the four roles' pre-activations (i, f, o, c~), dpre their bounds (None: no bounds wanted), cp the previous c or
    None. name -> (value, bound) for i, f, o, g, c, h by the module's formulas."""
    pi, pf, po, pg = pre
    i, f, o, g = torch.sigmoid(pi), torch.sigmoid(pf), torch.sigmoid(po), torch.tanh(pg)
    cp = torch.zeros_like(i) if cp is None else cp
    c = f * cp + i * g
    tc = torch.tanh(c)
    h = o * tc if tanh_out else o * c
    if dpre is None:
        return {k: (v, None) for k, v in zip("ifogch", (i, f, o, g, c, h))}
    di, df, do = (d / 4 + BOUND * s.abs() for d, s in zip(dpre[:3], (i, f, o)))
    dg = dpre[3] + BOUND * g.abs()
    dc = cp.abs() * df + g.abs() * di + i.abs() * dg + BOUND * ((f * cp).abs() + (i * g).abs())
    if tanh_out:
        dh = tc.abs() * do + o.abs() * (dc + BOUND * tc.abs()) + BOUND * (o * tc).abs()
    else:
        dh = c.abs() * do + o.abs() * dc + BOUND * (o * c).abs()
    return dict(i=(i, di), f=(f, df), o=(o, do), g=(g, dg), c=(c, dc), h=(h, dh))


def _product(x, dx, w, add, dt, drop_group=None):
    """pre = add + x w^T with its bound (dt float64) or alone (dx None). drop_group: a 16-wide k group left out."""
    x, w, add = x.to(dt), w.to(dt), add.to(dt)
    if drop_group is not None:
        x = x.clone()
        x[:, 16 * drop_group:16 * drop_group + 16] = 0
    pre = add + x @ w.t()
    if dx is None:
        return pre, None
    mag = add.abs() + x.abs() @ w.abs().t()
    return pre, BOUND * mag + dx @ w.abs().t()


def att_xa(row, inp, dt=torch.float64):
    """xa [rows][E + C] = [emb[token] | sigmoid(gate) * context] of capnet_att_decode_step: the plain attention front, for the
    checks that have no device (the GPU tests read xa from the call's workspace)."""
    G, n, k, H = row.groups, row.n, row.k, row.H
    gk = n * k
    st = inp["state_in"].to(dt)
    par = inp["parents"] if inp["parents"] is not None else torch.arange(G * gk)
    out = []
    for q in range(G):
        rows = slice(q * gk, (q + 1) * gk)
        z = st[rows, 0] @ inp["wz"][q].to(dt).t() + inp["bz"][q].to(dt)
        out.append(z)
    z = torch.cat(out)[par]
    img = torch.arange(G * gk) // k                                   # beam group of a row
    a1 = inp["att1"].to(dt)[img]                                      # [rows][P][A]
    wf = inp["w_full"].to(dt)[img // n]
    sc = (torch.relu(a1 + z[:, None, :ATT_A]) * wf[:, None, :]).sum(2) + inp["b_full"].to(dt)[img // n][:, None]
    alpha = torch.softmax(sc, 1)
    ctx = (alpha[:, :, None] * inp["feat"].to(dt)[img % n]).sum(1)
    return torch.cat([inp["tables"][0].to(dt)[inp["tokens"]], torch.sigmoid(z[:, ATT_A:]) * ctx], 1)


def _decode(row, inp, xa, dt, wrong):
    H, L, G, rpg = row.H, row.L, row.groups, row.rpg
    R, tanh_out = G * rpg, row.cell == 1
    bounds = dt == torch.float64
    st = inp["state_in"].to(dt)
    par = torch.arange(R) if inp["parents"] is None or wrong == "parent" else inp["parents"]
    if row.entry == WIDE:
        x = (att_xa(row, inp, dt) if xa is None else xa).to(dt)
    elif row.src == "rows":
        x = inp["x"].to(dt)
    else:
        tabs = inp["tables"]
        x = torch.cat([tabs[q if len(tabs) > 1 else 0].to(dt)[inp["tokens"][q * rpg:(q + 1) * rpg]] for q in range(G)])
    dx = torch.zeros_like(x) if bounds else None
    ref, bnd = torch.zeros(R, 2 * L, H, dtype=dt), torch.zeros(R, 2 * L, H, dtype=dt)
    for l in range(L):
        s = 2 * l + (2 if wrong == "slot" and l < L - 1 else 0)
        hp, cp = st[par, s], st[par, s + 1]
        xn, kin = x.shape[1], round16(x.shape[1])
        pad = torch.zeros(R, kin - xn, dtype=dt)
        xc = torch.cat([x, pad, hp], 1)
        dxc = torch.cat([dx, pad, torch.zeros_like(hp)], 1) if bounds else None
        hs, dhs = [], []
        for q in range(G):
            rows = slice(q * rpg, (q + 1) * rpg)
            qw = (q + 1) % G if wrong == "group" else q
            pre, dpre = _product(xc[rows], dxc[rows] if bounds else None, inp["wcat"][l][qw], inp["beff"][l][qw], dt,
                                 (kin + H) // 16 - 1 if wrong == "kgroup" else None)
            rb = (0, 1, 3, 2) if wrong == "swap" else (0, 1, 2, 3)
            o = _cell(_blocks(pre, rb, H), _blocks(dpre, rb, H) if bounds else None, cp[rows], tanh_out, dt)
            ref[rows, 2 * l], ref[rows, 2 * l + 1] = o["h"][0], o["c"][0]
            if bounds:
                bnd[rows, 2 * l], bnd[rows, 2 * l + 1] = o["h"][1], o["c"][1]
            hs.append(o["h"][0])
            dhs.append(o["h"][1])
        x, dx = torch.cat(hs), torch.cat(dhs) if bounds else None
    return dict(state_out=(ref, bnd), h_top=(ref[:, 2 * L - 2].clone(), bnd[:, 2 * L - 2].clone()))


def _pw_bwd(row, inp, dt, wrong):
    H, rb = row.H, roles(row)
    if wrong == "swap":
        rb = (rb[0], rb[1], rb[3], rb[2])
    i, f, o, g = _blocks(inp["gates"].to(dt), rb, H)
    ct, dh, dcin = inp["c"].to(dt), inp["dh"].to(dt), inp["dc"].to(dt)
    cp = torch.zeros_like(ct) if inp["c_prev"] is None else inp["c_prev"].to(dt)
    if row.cell == 1:
        tc = torch.tanh(ct)
        d_o, dc = dh * tc, dcin + dh * o * (1 - tc * tc)
        m_o, m_c = (dh * tc).abs(), dcin.abs() + (dh * o).abs() * (1 + tc * tc)
    else:
        d_o, dc = dh * ct, dcin + dh * o
        m_o, m_c = (dh * ct).abs(), dcin.abs() + (dh * o).abs()
    vals = [dc * g * i * (1 - i), dc * cp * f * (1 - f), d_o * o * (1 - o), dc * i * (1 - g * g)]
    mags = [m_c * g.abs() * i * (1 + i), m_c * cp.abs() * f * (1 + f), m_o * o * (1 + o), m_c * i * (1 + g * g)]
    return dict(dpre=(_unblocks(vals, rb), BOUND * _unblocks(mags, rb)), dc_out=(dc * f, BOUND * m_c * f))


def applies(row, wrong):
    e = row.entry
    if wrong == "kgroup":
        return e in (FUSED, DECODE, WIDE, UPPER)
    if wrong == "parent":
        return e in (DECODE, WIDE) and row.parents in ("perm", "repeat") and row.rpg > 1
    if wrong == "group":
        return e in (DECODE, WIDE) and row.groups > 1
    if wrong == "slot":
        return e in (DECODE, WIDE) and row.L > 1
    return True


def reference(row, inp, xa=None, x_out=None, dt=torch.float64, wrong=None):
    """name -> (ref, bound) of every output of the row. xa (WIDE): layer 0's input as the call left it in its workspace;
    x_out (UPPER with dropout): the dropped-out input row as the call stored it. dt float32: the plain float32 restatement
    (bounds None). wrong: one of WRONG."""
    assert wrong is None or applies(row, wrong)
    e, bounds = row.entry, dt == torch.float64
    if e in (DECODE, WIDE):
        return _decode(row, inp, xa, dt, wrong)
    if e == PW_BWD:
        return _pw_bwd(row, inp, dt, wrong)
    H, rb = row.H, roles(row)
    if wrong == "swap":
        rb = (rb[0], rb[1], rb[3], rb[2])
    tanh_out = row.cell == 1
    if e == PW_FWD:
        pre = inp["pre"].to(dt)
        dpre = BOUND * pre.abs() if bounds else None
        cp = inp["c_prev"]
    elif e == FUSED:
        x = inp["h_prev"].to(dt)
        pre, dpre = _product(x, torch.zeros_like(x) if bounds else None, inp["w"], inp["gates"], dt,
                             H // 16 - 1 if wrong == "kgroup" else None)
        cp = inp["c_prev"]
    else:
        xin = (inp["xin"] if x_out is None else x_out).to(dt)
        x = torch.cat([xin, inp["h_prev"].to(dt)], 1)
        pre, dpre = _product(x, torch.zeros_like(x) if bounds else None, torch.cat([inp["w_eff"], inp["w_rec"]], 1), inp["b_eff"],
                             dt, 2 * H // 16 - 1 if wrong == "kgroup" else None)
        cp = inp["c_prev"]
    o = _cell(_blocks(pre, rb, H), _blocks(dpre, rb, H) if bounds else None, None if cp is None else cp.to(dt), tanh_out, dt)
    gates = _unblocks([o[k][0] for k in "ifog"], rb)
    dgates = _unblocks([o[k][1] for k in "ifog"], rb) if bounds else None
    return dict(gates=(gates, dgates), c_out=o["c"], h_out=o["h"])


def oracle32(row, inp, xa=None, x_out=None):
    """The same operation in plain float32 torch on the CPU: what BOUND x magnitude has to leave room for."""
    return {k: v[0] for k, v in reference(row, inp, xa=xa, x_out=x_out, dt=torch.float32).items()}
