"""Every row of tests/step_cases.py on the device, one launch sequence per row: the recurrent step kernels on fenced
buffers, against float64.

Inputs sit in buffers whose every float outside the operand is NaN (helpers.Window; the weight matrices, up to 4096 x
4096, in the contiguous Fenced below, whose NaN fences need no index tensor): the gap between gate rows (ldg = 4H + 12),
the floats behind the last x row (columns [xn, kin) of the last row lie there), the rows beyond `rows`, the tables beyond
V, the attention step's workspace before the call. The state is [rows][2 L][H] at the stride the entry derives from
nlayers, so it has no slots of absent layers to poison; what stands in for them is the fence behind the last row.
Outputs sit in sentinel-filled buffers with guard floats in front and behind; the device error word is a private int32
between two sentinels. Per row:

  1. status 0;  2. every read-only input keeps its bits (state_in, weights, biases, x, tables, tokens, parents; xin and
  the previous state of the upper step; c_prev of pointwise_fwd; gates, c, c_prev, dh of pointwise_bwd);  3. every output
  element is finite and within its bound (step_cases.reference: float64 from the float32 inputs, per-element bounds; the
  fused step's in-place gates against the reference's activated gates);  4. nothing outside an output changed;  5. the
  error word stays 0.

The header's bit-for-bit promises: _gather = _cell on state_in.index_select(0, parents); group g of _groups / _tables =
_gather on that group alone; groups = 1 = _gather; capnet_stacked_decode_step = _cell with cell 0.
Isolation: one row's previous state, or one group's weights, all NaN leaves every other row or group bit-identical.
Error word: on a word preset to 4 | 8, one bad token / one bad parent leaves 4 | 8 | 1 (then 1 on a word of 0), the bad
row is the row of token 0 / of its own state and every other row keeps its bits -- the narrow kernel's two raisers, the
wide kernel's and the attention beam kernels' parent raisers (one call reaches both) and the beam kernels' token raiser.
The wide kernel's own token raiser has no caller: above K = 2048 layer 0 always reads the dense xa rows.

The upper step with dropout (p = 0.3): x_out is 0 or float32(x * float32(1 / (1 - p))) to the bit and both occur, the
same seed gives the same bits, and gates, c, h are held against float64 evaluated on x_out as read back.

Worst error / bound per entry point on the MI355X:
  capnet_lstm_step_fused              gates 0.052  c_out 0.028  h_out 0.020
  capnet_stacked_decode_step*         state_out 0.031  h_top 0.020
  capnet_att_decode_step[_groups]     state_out 0.026  h_top 0.023      (the layers behind xa as read back)
  capnet_lstm_upper_step              gates 0.046  c_out 0.024  h_out 0.017
  capnet_lstm_pointwise_fwd           gates 0.060  c_out 0.037  h_out 0.025
  capnet_lstm_pointwise_bwd           dpre 0.104  dc_out 0.085
The plain float32 restatement on the CPU lands at 0.02 to 0.10 of the same bounds (tests/test_step_cases_cpu.py prints it).
The 222 tests of the module take about five seconds together, the slowest (the first, which loads the library) 0.4 s."""
import ctypes as C
import functools

import pytest
import torch

import step_cases as SC
from capnet import ops
from capnet._lib import current_stream, lib
from helpers import SENTINEL, Window

pytestmark = pytest.mark.gpu

NAN = float("nan")
WORST = {}


def note(entry, what, ratio):
    WORST[(entry, what)] = max(WORST.get((entry, what), 0.0), ratio)
    print("worst error / bound so far on %-14s %s" % (entry, "  ".join(
        "%s %.3f" % (w, v) for (e, w), v in sorted(WORST.items()) if e == entry)))


def dense(shape):
    st, n = [], 1
    for d in reversed(shape):
        st.append(n)
        n *= d
    return tuple(reversed(st))


class Fenced:
    """A contiguous operand between two NaN fences of 64 floats (16-B aligned start): Window's interface for the large
    weight matrices, without its index tensor."""

    def __init__(self, values, dev):
        n = values.numel()
        self.buf = torch.full((n + 128,), NAN, device=dev)
        self.buf[64:64 + n] = values.reshape(-1).to(dev)
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 256
        assert self.ptr % 16 == 0

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))


def win_in(t, dev, off=0, strides=None):
    if t is None:
        return None
    if t.numel() > 1 << 18:
        return Fenced(t, dev)
    return Window(t, strides or dense(t.shape), dev, off=off, pre=8, post=64)


def win_out(shape, dev, values=None, strides=None):
    v = torch.full(tuple(shape), NAN) if values is None else values
    return Window(v, strides or dense(v.shape), dev, pre=16, post=64, fill_bits=SENTINEL)


class Ints:
    """int64 ids between two sentinel words."""

    def __init__(self, t, dev):
        self.buf = torch.cat([torch.tensor([-99]), t.long(), torch.tensor([-99])]).to(dev)
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 8

    def unchanged(self):
        return torch.equal(self.buf, self.before)


class ErrWord:
    def __init__(self, dev, preset=0):
        self.buf = torch.tensor([SENTINEL, preset, SENTINEL], dtype=torch.int32, device=dev)
        self.ptr = self.buf.data_ptr() + 4

    def value(self):
        b = self.buf.cpu()
        assert int(b[0]) == SENTINEL and int(b[2]) == SENTINEL
        return int(b[1])


def P(w):
    return None if w is None else w.ptr


def ptrs(ws):
    return (C.c_void_p * len(ws))(*[w.ptr for w in ws])


def ratio(got, ref, bnd):
    got = got.double().cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    assert bool((err[bnd == 0] == 0).all())
    return float((err / bnd.clamp_min(1e-300)).max())


def check_outputs(row, outs, ref, what=None):
    for k, (r, bnd) in ref.items():
        q = ratio(outs[k].inside(), r, bnd)
        note(what or row.entry, k, q)
        assert q <= 1.0, (row.name, k, q)
        assert outs[k].outside_unchanged(), (row.name, k)


def check_inputs(row, ins):
    for k, w in ins.items():
        for u in (w if isinstance(w, list) else [w]):
            assert u is None or u.unchanged(), (row.name, k)


def bits(w):
    return w.inside().cpu().view(torch.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    row = SC.BY_NAME[name]
    return row, SC.inputs(row)


def ids(rows):
    return [r.name for r in rows]


# ---- (a) capnet_lstm_pack_wfrag + capnet_lstm_step_fused ------------------------------------------------------------------
def run_fused(row, inp, dev):
    L, H, b = lib(), row.H, row.b
    ldg = 4 * H + row.gap
    ins = dict(w=win_in(inp["w"], dev), h_prev=win_in(inp["h_prev"], dev), c_prev=win_in(inp["c_prev"], dev))
    wfrag = win_out((L.capnet_lstm_wfrag_floats(H),), dev)
    assert L.capnet_lstm_pack_wfrag(P(ins["w"]), P(wfrag), H, row.cell, current_stream()) == 0
    torch.cuda.synchronize()
    assert wfrag.outside_unchanged() and bool(torch.isfinite(wfrag.inside()).all())
    wfrag.snapshot()
    outs = dict(gates=win_out(None, dev, values=inp["gates"], strides=(ldg, 1)), c_out=win_out((b, H), dev),
                h_out=win_out((b, H), dev))
    rc = L.capnet_lstm_step_fused(P(ins["h_prev"]), P(wfrag), P(outs["gates"]), ldg, P(ins["c_prev"]), P(outs["c_out"]),
                                  P(outs["h_out"]), b, H, row.cell, current_stream())
    torch.cuda.synchronize()
    assert rc == 0, L.capnet_last_error()
    ins["wfrag"] = wfrag
    return ins, outs


@pytest.mark.parametrize("name", ids(SC.FUSED_ROWS))
def test_step_fused_row(dev, name):
    row, inp = case(name)
    ins, outs = run_fused(row, inp, dev)
    check_inputs(row, ins)
    check_outputs(row, outs, SC.reference(row, inp))


@pytest.mark.parametrize("name", ["fused-h48-b17-gap12-cell0", "fused-h272-b49-gap0-cell1", "fused-h512-b64-gap12-cell0"])
def test_step_fused_rows_are_isolated(dev, name):
    row, inp = case(name)
    _, clean = run_fused(row, inp, dev)
    bad = dict(inp)
    bad["h_prev"] = inp["h_prev"].clone()
    bad["h_prev"][row.b // 2] = NAN
    _, outs = run_fused(row, bad, dev)
    keep = torch.arange(row.b) != row.b // 2
    for k in outs:
        assert torch.equal(bits(outs[k])[keep], bits(clean[k])[keep]), (name, k)
    assert bool(torch.isnan(outs["h_out"].inside()[row.b // 2]).all())


# ---- (b) the decode step --------------------------------------------------------------------------------------------------
def run_decode(dev, centry, cell, L, groups, rpg, E, H, inp, err=None, xoff=0):
    """One call of the C entry `centry` on CPU operands (inp: wcat, beff, state_in, parents, x or tables + tokens)."""
    lb, R = lib(), groups * rpg
    err = err or ErrWord(dev)
    ins = dict(wcat=[win_in(w, dev) for w in inp["wcat"]], beff=[win_in(b, dev) for b in inp["beff"]],
               state_in=win_in(inp["state_in"], dev),
               parents=None if inp.get("parents") is None else Ints(inp["parents"], dev),
               tokens=None if inp.get("tokens") is None else Ints(inp["tokens"], dev),
               x=win_in(inp.get("x"), dev, off=xoff), tables=[win_in(t, dev) for t in inp.get("tables", [])])
    outs = dict(state_out=win_out((R, 2 * L, H), dev), h_top=win_out((R, H), dev))
    x = ins["x"] if ins["x"] is not None else ins["tables"][0]
    tail = (ptrs(ins["wcat"]), ptrs(ins["beff"]), P(ins["state_in"]))
    end = (P(outs["state_out"]), P(outs["h_top"]), err.ptr, current_stream())
    if centry == "step":
        rc = lb.capnet_stacked_decode_step(L, R, E, H, SC.VOCAB, P(ins["tokens"]), P(x), *tail, *end)
    elif centry == "cell":
        rc = lb.capnet_stacked_decode_step_cell(cell, L, R, E, H, SC.VOCAB, P(ins["tokens"]), P(x), *tail, *end)
    elif centry == "gather":
        rc = lb.capnet_stacked_decode_step_gather(cell, L, R, E, H, SC.VOCAB, P(ins["tokens"]), P(x), *tail, P(ins["parents"]), *end)
    elif centry == "groups":
        rc = lb.capnet_stacked_decode_step_groups(cell, L, groups, rpg, E, H, SC.VOCAB, P(ins["tokens"]), P(x), *tail,
                                                  P(ins["parents"]), *end)
    else:
        rc = lb.capnet_stacked_decode_step_tables(cell, L, groups, rpg, E, H, SC.VOCAB, P(ins["tokens"]), ptrs(ins["tables"]), *tail,
                                                  P(ins["parents"]), *end)
    torch.cuda.synchronize()
    assert rc == 0, lb.capnet_last_error()
    return ins, outs, err


def run_decode_row(dev, row, inp, centry=None, err=None):
    return run_decode(dev, centry or row.centry, row.cell, row.L, row.groups, row.rpg, row.E, row.H, inp, err, row.xoff)


@functools.lru_cache(maxsize=None)
def decode_clean(name):
    """The clean run of a DECODE row: (output bits, error word), shared by the promise, isolation and error-word tests."""
    row, inp = case(name)
    _, outs, err = run_decode_row(torch.device("cuda:0"), row, inp)
    return {k: bits(w) for k, w in outs.items()}, err.value()


@pytest.mark.parametrize("name", ids(SC.DECODE_ROWS))
def test_decode_row(dev, name):
    row, inp = case(name)
    ins, outs, err = run_decode_row(dev, row, inp)
    check_inputs(row, ins)
    check_outputs(row, outs, SC.reference(row, inp))
    assert err.value() == 0


def group_slice(row, inp, q):
    """Group q's rows, weights and table as a call of their own."""
    rows = slice(q * row.rpg, (q + 1) * row.rpg)
    sub = dict(wcat=[w[q:q + 1] for w in inp["wcat"]], beff=[b[q:q + 1] for b in inp["beff"]], state_in=inp["state_in"][rows],
               parents=None if inp["parents"] is None else inp["parents"][rows] - q * row.rpg)
    if "x" in inp:
        sub["x"] = inp["x"][rows]
    else:
        sub["tokens"] = inp["tokens"][rows]
        sub["tables"] = [inp["tables"][q if len(inp["tables"]) > 1 else 0]]
    return rows, sub


@pytest.mark.parametrize("name", ids(SC.DECODE_ROWS))
def test_decode_bit_for_bit_promises(dev, name):
    row, inp = case(name)
    clean, _ = decode_clean(name)

    def same(outs, rows=slice(None)):
        for k in clean:
            assert torch.equal(bits(outs[k]), clean[k][rows]), (name, k)

    if row.centry == "step":                              # capnet_stacked_decode_step = _cell with cell 0
        same(run_decode_row(dev, row, inp, "cell")[1])
    elif row.centry == "cell":                            # parent_rows NULL: _gather is exactly _cell
        same(run_decode_row(dev, row, inp, "gather")[1])
    elif row.centry == "gather":                          # _gather = _cell on the gathered state
        alt = dict(inp, state_in=inp["state_in"].index_select(0, inp["parents"]), parents=None)
        same(run_decode_row(dev, row, alt, "cell")[1])
    else:                                                 # group q = _gather on that group alone; groups = 1 = _gather
        for q in range(row.groups):
            rows, sub = group_slice(row, inp, q)
            same(run_decode(dev, "gather", row.cell, row.L, 1, row.rpg, row.E, row.H, sub)[1], rows)


@pytest.mark.parametrize("name", [r.name for r in SC.DECODE_ROWS if r.groups * r.rpg > 1])
def test_decode_rows_and_groups_are_isolated(dev, name):
    row, inp = case(name)
    clean, _ = decode_clean(name)
    R = row.groups * row.rpg
    par = torch.arange(R) if inp["parents"] is None else inp["parents"]
    bad_row = int(par[R // 2])                            # the state the middle row reads
    bad = dict(inp, state_in=inp["state_in"].clone())
    bad["state_in"][bad_row] = NAN
    keep = par != bad_row
    assert bool(keep.any())
    _, outs, _ = run_decode_row(dev, row, bad)
    for k in clean:
        assert torch.equal(bits(outs[k])[keep], clean[k][keep]), (name, k)
    assert bool(torch.isnan(outs["h_top"].inside().cpu()[~keep]).all())
    if row.groups > 1:                                    # the last group's weights of layer 0 all NaN
        bad = dict(inp, wcat=[w.clone() for w in inp["wcat"]])
        bad["wcat"][0][row.groups - 1] = NAN
        _, outs, _ = run_decode_row(dev, row, bad)
        keep = torch.arange(R) < (row.groups - 1) * row.rpg
        for k in clean:
            assert torch.equal(bits(outs[k])[keep], clean[k][keep]), (name, k)
        assert bool(torch.isnan(outs["h_top"].inside().cpu()[~keep]).all())


TOKEN_ROWS = ["decode-nj2-e12-h64-three-layers", "decode-nj6-e300-h256-nj4-above", "decode-tables-2x5-e12-h64-lstm"]
PARENT_ROWS = ["decode-nj2-e12-h64-x-off-4-bytes", "decode-nj12-e100-h1024-nj16-above-gather", "decode-groups-2x17-e12-h64"]


@pytest.mark.parametrize("bad_id", [-1, "past"])
@pytest.mark.parametrize("name", TOKEN_ROWS + PARENT_ROWS)
def test_decode_error_word_accumulates(dev, name, bad_id):
    """One bad id: the word keeps the bits it had (4 | 8 -> 4 | 8 | 1), the bad row reads token 0 / its own state, the rest
    is the clean call's. An out-of-range id is an input the kernels survive: they clamp it before any address is formed."""
    row, inp = case(name)
    R = row.groups * row.rpg
    r = R - 1
    key, limit, good = ("tokens", SC.VOCAB, 0) if name in TOKEN_ROWS else ("parents", R, r)
    bad, twin = dict(inp), dict(inp)
    bad[key], twin[key] = inp[key].clone(), inp[key].clone()
    bad[key][r] = limit if bad_id == "past" else -1
    twin[key][r] = good
    _, want, e0 = run_decode_row(dev, row, twin)
    assert e0.value() == 0
    for preset in (4 | 8, 0):
        _, outs, err = run_decode_row(dev, row, bad, err=ErrWord(dev, preset))
        assert err.value() == preset | 1, (name, preset, err.value())
        for k in outs:
            assert torch.equal(bits(outs[k]), bits(want[k])), (name, k)


# ---- (c) the wide kernel through capnet_att_decode_step[_groups] ------------------------------------------------------------
def run_wide(dev, row, inp, err=None):
    lb, G, n, k, H, L = lib(), row.groups, row.n, row.k, row.H, row.L
    R, E = G * n * k, row.E
    err = err or ErrWord(dev)
    ins = dict(wcat=[win_in(w, dev) for w in inp["wcat"]], beff=[win_in(b, dev) for b in inp["beff"]],
               state_in=win_in(inp["state_in"], dev), parents=None if inp["parents"] is None else Ints(inp["parents"], dev),
               tokens=Ints(inp["tokens"], dev), emb=win_in(inp["tables"][0], dev),
               **{key: win_in(inp[key], dev) for key in ("att1", "feat", "wz", "bz", "w_full", "b_full")})
    outs = dict(state_out=win_out((R, 2 * L, H), dev), h_top=win_out((R, H), dev))
    wsf = lb.capnet_att_decode_step_ws_bytes(G * n, k, SC.ATT_P, SC.ATT_A, SC.ATT_C, E) // 4
    ws = win_out((wsf,), dev)                        # NaN inside: columns [xn, kin) of xa's last row are the scores' NaN
    slab = ops.splitk_slab(dev)
    args = (n, k, SC.ATT_P, SC.ATT_A, SC.ATT_C, E, H, SC.VOCAB, P(ins["att1"]), P(ins["feat"]), P(ins["tokens"]), P(ins["emb"]),
            P(ins["wz"]), P(ins["bz"]), P(ins["w_full"]), P(ins["b_full"]), ptrs(ins["wcat"]), ptrs(ins["beff"]), P(ins["state_in"]),
            P(ins["parents"]), P(outs["state_out"]), P(outs["h_top"]), ws.ptr, slab.data_ptr(), slab.numel(), err.ptr,
            current_stream())
    rc = lb.capnet_att_decode_step(row.cell, L, *args) if G == 1 else lb.capnet_att_decode_step_groups(row.cell, L, G, *args)
    torch.cuda.synchronize()
    assert rc == 0, lb.capnet_last_error()
    assert ws.outside_unchanged()
    z0 = R * (SC.ATT_A + SC.ATT_C)
    xa = ws.inside()[z0:z0 + R * (E + SC.ATT_C)].view(R, E + SC.ATT_C).cpu()
    return ins, outs, err, xa


@pytest.mark.parametrize("name", ids(SC.WIDE_ROWS))
def test_wide_row(dev, name):
    row, inp = case(name)
    ins, outs, err, xa = run_wide(dev, row, inp)
    check_inputs(row, ins)
    # the attention front is pinned elsewhere: here xa only has to be the finite thing the plain front gives, loosely
    front = SC.att_xa(row, inp)
    assert torch.isfinite(xa).all() and float((xa.double() - front).abs().max()) < 1e-4 * float(front.abs().max())
    check_outputs(row, outs, SC.reference(row, inp, xa=xa))
    assert err.value() == 0


@pytest.mark.parametrize("name", ["wide-w12-k2128-h64-49-rows", "wide-w12-k3072-h512-2x16-lstm", "wide-w16-k3088-h1024-17-rows"])
def test_wide_rows_are_isolated(dev, name):
    row, inp = case(name)
    R = row.groups * row.rpg
    _, clean, _, _ = run_wide(dev, row, inp)
    bad = dict(inp, state_in=inp["state_in"].clone())
    bad_row = int(inp["parents"][R // 2])                 # the state the middle row reads
    bad["state_in"][bad_row] = NAN
    keep = inp["parents"] != bad_row
    assert bool(keep.any()) and not bool(keep.all())
    _, outs, _, _ = run_wide(dev, row, bad)
    for k in outs:
        assert torch.equal(bits(outs[k])[keep], bits(clean[k])[keep]), (name, k)
    assert bool(torch.isnan(outs["h_top"].inside().cpu()[~keep]).all())


@pytest.mark.parametrize("key", ["parents", "tokens"])
@pytest.mark.parametrize("name", ["wide-w12-k2128-h64-49-rows", "wide-w16-k3088-h1024-17-rows"])
def test_wide_error_word_accumulates(dev, name, key):
    """parents: the wide kernel's raiser and the beam kernels' (scores and context read z through the same parent);
    tokens: the beam context kernel's, which copies the embedding row into xa."""
    row, inp = case(name)
    R = row.groups * row.rpg
    r = R - 1
    limit, good = (R, r) if key == "parents" else (SC.VOCAB, 0)
    bad, twin = dict(inp), dict(inp)
    bad[key], twin[key] = inp[key].clone(), inp[key].clone()
    bad[key][r], twin[key][r] = limit, good
    _, want, e0, _ = run_wide(dev, row, twin)
    assert e0.value() == 0
    for preset in (4 | 8, 0):
        _, outs, err, _ = run_wide(dev, row, bad, err=ErrWord(dev, preset))
        assert err.value() == preset | 1, (name, key, preset, err.value())
        for k in outs:
            assert torch.equal(bits(outs[k]), bits(want[k])), (name, k)


# ---- (d) capnet_lstm_upper_step ---------------------------------------------------------------------------------------------
def run_upper(dev, row, inp):
    lb, H, b = lib(), row.H, row.b
    ins = {k: win_in(inp[k], dev) for k in ("xin", "h_prev", "c_prev", "w_eff", "w_rec", "b_eff")}
    outs = dict(x_out=win_out((b, H), dev), gates=win_out((b, 4 * H), dev), c_out=win_out((b, H), dev), h_out=win_out((b, H), dev))
    rc = lb.capnet_lstm_upper_step(P(ins["xin"]), P(ins["h_prev"]), P(ins["c_prev"]), P(ins["w_eff"]), P(ins["w_rec"]),
                                   P(ins["b_eff"]), P(outs["x_out"]), P(outs["gates"]), P(outs["c_out"]), P(outs["h_out"]), b, H,
                                   inp["r0"], SC.DROP_P if row.dropout else 0.0, inp["seed"], inp["layer"], row.dropout, row.cell,
                                   current_stream())
    torch.cuda.synchronize()
    assert rc == 0, lb.capnet_last_error()
    return ins, outs


@pytest.mark.parametrize("name", ids(SC.UPPER_ROWS))
def test_upper_step_row(dev, name):
    row, inp = case(name)
    ins, outs = run_upper(dev, row, inp)
    check_inputs(row, ins)
    x_out = outs["x_out"].inside().cpu()
    assert outs["x_out"].outside_unchanged()
    if row.dropout:
        scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(SC.DROP_P))          # float32, as the kernel's
        kept = inp["xin"] * scale
        zero = x_out == 0                                  # a dropped element is x * 0: a zero of either sign
        assert torch.equal(x_out.view(torch.int32)[~zero], kept.view(torch.int32)[~zero])
        frac = float(zero.float().mean())
        assert 0.0 < frac < 1.0 and (row.b * row.H < 2048 or abs(frac - SC.DROP_P) < 0.05), frac
        _, again = run_upper(dev, row, inp)
        for k in outs:
            assert torch.equal(bits(again[k]), bits(outs[k])), (name, k)
        other = dict(inp, seed=inp["seed"] + 1)
        assert not torch.equal(bits(run_upper(dev, row, other)[1]["x_out"]), bits(outs["x_out"]))
    else:
        assert torch.equal(x_out.view(torch.int32), inp["xin"].view(torch.int32))
    ref = SC.reference(row, inp, x_out=x_out if row.dropout else None)
    check_outputs(row, {k: outs[k] for k in ref}, ref)


# ---- (e) the gate kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ids(SC.PW_FWD_ROWS))
def test_pointwise_fwd_row(dev, name):
    row, inp = case(name)
    b, H = row.b, row.H
    ins = dict(c_prev=win_in(inp["c_prev"], dev))
    outs = dict(gates=win_out(None, dev, values=inp["pre"]), c_out=win_out((b, H), dev), h_out=win_out((b, H), dev))
    rc = lib().capnet_lstm_pointwise_fwd(P(outs["gates"]), P(ins["c_prev"]), P(outs["c_out"]), P(outs["h_out"]), b, H, row.cell,
                                         current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    check_inputs(row, ins)
    check_outputs(row, outs, SC.reference(row, inp))


@pytest.mark.parametrize("name", ids(SC.PW_BWD_ROWS))
def test_pointwise_bwd_row(dev, name):
    row, inp = case(name)
    b, H = row.b, row.H
    ins = {k: win_in(inp[k], dev) for k in ("gates", "c", "c_prev", "dh")}
    outs = dict(dc_out=win_out(None, dev, values=inp["dc"]), dpre=win_out((b, 4 * H), dev))
    rc = lib().capnet_lstm_pointwise_bwd(P(ins["gates"]), P(ins["c"]), P(ins["c_prev"]), P(ins["dh"]), P(outs["dc_out"]),
                                         P(outs["dpre"]), b, H, row.cell, current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    check_inputs(row, ins)
    check_outputs(row, outs, SC.reference(row, inp))
