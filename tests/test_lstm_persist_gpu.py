"""The persistent LSTM sequence kernel (csrc/lstm_persist.hip) through the C ABI: one launch runs a
whole run of recurrent steps -- stylenet/model.py:147-153 (h = o*c) and nn.LSTMCell of
nic/model.py:77 (gate order i,f,g,o; h = o*tanh(c)) -- with shrinking batches, mid-sequence restarts
(segments) and every batch size up to 128. Checked against a float64 loop of the same recurrence,
and against the launch-per-step kernel it replaces."""
import ctypes as C

import pytest
import torch

import capnet
from capnet import _lib
from capnet._lib import check, current_stream, int_array

pytestmark = pytest.mark.gpu
H = 512


def _reference(W, pre, bs, cell):
    """float64: gates_t = pre_t + h_{t-1} W^T; returns (hiddens, cells, activated gates), packed."""
    W = W.double()
    off = [0]
    for b in bs:
        off.append(off[-1] + b)
    hs, cs, gs = [], [], []
    h = torch.zeros(bs[0], H, dtype=torch.float64)
    c = torch.zeros(bs[0], H, dtype=torch.float64)
    for t, b in enumerate(bs):
        g = pre[off[t]:off[t + 1]].double() + (h[:b] @ W.t() if t > 0 else 0)
        if cell == 0:
            i, f, o, gg = [g[:, k * H:(k + 1) * H] for k in range(4)]
        else:
            i, f, gg, o = [g[:, k * H:(k + 1) * H] for k in range(4)]
        i, f, o, gg = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(gg)
        c = f * c[:b] + i * gg
        h = o * c if cell == 0 else o * torch.tanh(c)
        act = torch.cat([i, f, o, gg] if cell == 0 else [i, f, gg, o], 1)
        hs.append(h)
        cs.append(c)
        gs.append(act)
    return torch.cat(hs), torch.cat(cs), torch.cat(gs)


def _run(dev, W, pre, bs, cell, segments):
    L = capnet.lib()
    N = sum(bs)
    Wd = W.to(dev)
    img = torch.empty(L.capnet_lstm_persist_w_floats(), device=dev)
    check(L.capnet_lstm_persist_pack(Wd.data_ptr(), img.data_ptr(), cell, current_stream()))
    G = pre.clone().to(dev)
    Cst = torch.full((N, H), float("nan"), device=dev)
    hid = torch.full((N, H), float("nan"), device=dev)
    ctl = torch.zeros(L.capnet_lstm_persist_ctl_ints(), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    off = [0]
    for b in bs:
        off.append(off[-1] + b)
    wf = None
    for k, seg in enumerate(segments):
        t0, t1 = seg[0], seg[1]
        if len(seg) > 2:                 # one step of the launch-per-step kernel (capnet_lstm_step_fused)
            assert t1 == t0 + 1 and t0 > 0 and L.capnet_lstm_step_fused_supported(bs[t0], H)
            if wf is None:
                wf = torch.empty(L.capnet_lstm_wfrag_floats(H), device=dev)
                check(L.capnet_lstm_pack_wfrag(Wd.data_ptr(), wf.data_ptr(), H, cell, current_stream()))
            check(L.capnet_lstm_step_fused(hid[off[t0 - 1]:].data_ptr(), wf.data_ptr(), G[off[t0]:].data_ptr(), 4 * H,
                                           Cst[off[t0 - 1]:].data_ptr(), Cst[off[t0]:].data_ptr(), hid[off[t0]:].data_ptr(),
                                           bs[t0], H, cell, current_stream()), "capnet_lstm_step_fused")
            continue
        check(L.capnet_lstm_persist_run(img.data_ptr(), G.data_ptr(), Cst.data_ptr(), hid.data_ptr(),
                                        int_array(bs), t0, t1, H, cell, k + 1, ctl.data_ptr(), err.data_ptr(),
                                        None, current_stream()), "capnet_lstm_persist_run")
    torch.cuda.synchronize()
    assert int(err.item()) == 0, "a bounded wait expired"
    return hid.cpu(), Cst.cpu(), G.cpu()


def _case(seed, bs):
    g = torch.Generator().manual_seed(seed)
    W = (torch.rand(4 * H, H, generator=g) * 2 - 1) * 0.06
    pre = torch.randn(sum(bs), 4 * H, generator=g)
    return W, pre


def _close(a, b, tol):
    assert torch.isfinite(a).all()
    assert ((a.double() - b).abs().max() / b.abs().max()).item() < tol


def _dist(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


def _close_as_fp32(what, got, f32, ref):
    """got within max(2e-6, 3 e_f) of float64, e_f the distance of the plain fp32 loop on the same case. Prints both."""
    assert torch.isfinite(got).all()
    e_k, e_f = _dist(got, ref), _dist(f32, ref)
    print("%s: kernel %.2e, fp32 loop %.2e of the largest value" % (what, e_k, e_f))
    assert e_k < max(2e-6, 3 * e_f), (what, e_k, e_f)


CASES = {
    "b64_24": [64] * 8 + [60, 57, 50, 44, 41, 33, 32, 30, 25, 17, 16, 9, 8, 7, 2, 1],
    "b96": [96, 96, 90, 75, 66, 65, 64, 40, 13],
    "b128": [128, 128, 127, 100, 97],
    "b8": [8, 8, 8, 5, 3, 1],
    "b3": [3, 3, 2, 2, 1],
    "b33": [33, 33, 32, 31, 17, 16, 15],
    # beyond step 63 the kernel reads its step metadata from a second register (lane l: steps l and l + 64)
    "b16_64": [16] * 60 + [9] * 4,
    "c12_65": [12] * 65,
    "shrink128_100": [128] * 10 + [100] * 20 + [70] * 20 + [40] * 14 + [17] * 16 + [5] * 19 + [1],
    "shrink128_128": [128] * 20 + [96] * 30 + [65] * 13 + [64] + [33] * 10 + [16] * 30 + [3] * 23 + [1],
    "c64_128": [64] * 128,
}
# (case, segments): (t0, t1) is one launch of the persistent kernel, (t, t + 1, "per_step") one step of the launch-per-step
# kernel in between
SEGMENT_CASES = [
    ("shrink128_128", [(0, 63), (63, 64), (64, 65), (65, 127), (127, 128)]),
    ("c64_128", [(0, 64), (64, 65, "per_step"), (65, 127), (127, 128)]),
    ("c64_128", [(0, 62), (62, 63, "per_step"), (63, 64), (64, 100), (100, 101, "per_step"), (101, 128)]),
]


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("cell", [0, 1])
def test_persistent_sequence_matches_float64(dev, name, cell):
    if not capnet.lib().capnet_lstm_persist_supported(64, H):
        pytest.skip("persistent kernel not supported on this device")
    bs = CASES[name]
    W, pre = _case(len(bs) * 7 + cell, bs)
    hid, cst, gates = _run(dev, W, pre, bs, cell, [(0, len(bs))])
    rh, rc, rg = _reference(W, pre, bs, cell)
    if len(bs) <= 24:
        _close(hid, rh, 2e-6)
        _close(cst, rc, 2e-6)
        _close(gates, rg, 2e-6)
        return
    # Long runs: 2e-6 of the largest value was set at <= 24 steps. Held where plain fp32 arithmetic holds it; the kernel
    # may sit no further from float64 than max(2e-6, 3 x the fp32 loop's distance) (the rule of
    # test_split_f16_weights_cover_small_and_large_magnitudes).
    fh, fc = _reference32(W, pre, bs, cell)
    _close_as_fp32("%s cell %d hiddens" % (name, cell), hid, fh, rh)
    _close_as_fp32("%s cell %d cell states" % (name, cell), cst, fc, rc)
    _close(gates, rg, max(2e-6, 3 * _dist(fh, rh)))


def _reference32(W, pre, bs, cell):
    """the same loop in float32 (torch CPU): how far plain fp32 arithmetic sits from float64 on the same case"""
    off = [0]
    for b in bs:
        off.append(off[-1] + b)
    hs, cs = [], []
    h = torch.zeros(bs[0], H)
    c = torch.zeros(bs[0], H)
    for t, b in enumerate(bs):
        g = pre[off[t]:off[t + 1]] + (h[:b] @ W.t() if t > 0 else 0)
        if cell == 0:
            i, f, o, gg = [g[:, k * H:(k + 1) * H] for k in range(4)]
        else:
            i, f, gg, o = [g[:, k * H:(k + 1) * H] for k in range(4)]
        i, f, o, gg = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(gg)
        c = f * c[:b] + i * gg
        h = o * c if cell == 0 else o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
    return torch.cat(hs), torch.cat(cs)


@pytest.mark.parametrize("wscale", [2.0 ** -16, 2.0 ** -6, 30.0, 400.0])
def test_split_f16_weights_cover_small_and_large_magnitudes(dev, wscale):
    """The recurrent weights enter the MFMAs as two f16 pieces scaled by 2^10 (csrc/lstm_persist.hip): weights of
    1e-6 (their residuals still normal f16 numbers), ordinary ones and |w| up to 24 -- the documented domain is |w| < 32,
    far beyond anything a clamped Adam leaves in W_hh. Against float64 the kernel may not sit further away than plain
    fp32 arithmetic does on the same case (with large weights the pre-activations are sums of thousands and no fp32
    method holds 2e-6 of them); h = o c grows with the weights, which exercises the f16 range of h as well."""
    if not capnet.lib().capnet_lstm_persist_supported(64, H):
        pytest.skip("persistent kernel not supported on this device")
    bs = [64, 64, 60, 40, 33, 8]
    W, pre = _case(5, bs)
    W = W * wscale                       # max |w| = 0.06 * wscale
    hid, cst, gates = _run(dev, W, pre, bs, 0, [(0, len(bs))])
    rh, rc, rg = _reference(W, pre, bs, 0)
    fh, fc = _reference32(W, pre, bs, 0)
    assert torch.isfinite(hid).all() and torch.isfinite(cst).all()
    for got, f32, ref in ((hid, fh, rh), (cst, fc, rc)):
        e_k = ((got.double() - ref).abs().max() / ref.abs().max()).item()
        e_f = ((f32.double() - ref).abs().max() / ref.abs().max()).item()
        print("max |w| %.3g: kernel %.2e, fp32 loop %.2e of the largest value" % (0.06 * wscale, e_k, e_f))
        assert e_k < max(2e-6, 3 * e_f)


def test_segments_restart_from_global_state(dev):
    """A forward pass with free-running steps cuts the recurrence into several launches: each one
    picks h and c of the previous step up from the output buffers (same control block, segment
    tags 1, 2, ...), also from a step run by the launch-per-step kernel in between."""
    L = capnet.lib()
    if not L.capnet_lstm_persist_supported(64, H):
        pytest.skip("persistent kernel not supported on this device")
    bs = CASES["b64_24"]
    W, pre = _case(5, bs)
    rh, rc, rg = _reference(W, pre, bs, 0)
    whole = _run(dev, W, pre, bs, 0, [(0, len(bs))])
    parts = _run(dev, W, pre, bs, 0, [(0, 1), (1, 2), (2, 9), (9, 10), (10, 24)])
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)          # same arithmetic whatever the cut
    _close(parts[0], rh, 2e-6)


@pytest.mark.parametrize("k", range(len(SEGMENT_CASES)))
def test_segments_restart_beyond_step_63(dev, k):
    """Restarts at t0 = 63, 64, 65 and 127: the cell state comes from Cst at off[t0 - 1], read through the second
    metadata register from t0 = 65 on. Cuts between launches of the persistent kernel alone change no bit; with a step of
    the launch-per-step kernel in between (another summation order) the result is held to float64 like the whole run."""
    L = capnet.lib()
    if not L.capnet_lstm_persist_supported(64, H):
        pytest.skip("persistent kernel not supported on this device")
    name, segs = SEGMENT_CASES[k]
    bs = CASES[name]
    for cell in (0, 1):
        W, pre = _case(len(bs) * 7 + cell, bs)
        rh, rc, rg = _reference(W, pre, bs, cell)
        fh, fc = _reference32(W, pre, bs, cell)
        parts = _run(dev, W, pre, bs, cell, segs)
        if all(len(s) == 2 for s in segs):
            whole = _run(dev, W, pre, bs, cell, [(0, len(bs))])
            for a, b in zip(whole, parts):
                assert torch.equal(a, b)          # same arithmetic whatever the cut
        _close_as_fp32("%s cut %d cell %d hiddens" % (name, k, cell), parts[0], fh, rh)
        _close_as_fp32("%s cut %d cell %d cell states" % (name, k, cell), parts[1], fc, rc)
        _close(parts[2], rg, max(2e-6, 3 * _dist(fh, rh)))


def test_persistent_equals_launch_per_step_kernel(dev):
    L = capnet.lib()
    if not L.capnet_lstm_persist_supported(64, H):
        pytest.skip("persistent kernel not supported on this device")
    bs = [64] * 6
    W, pre = _case(9, bs)
    hid, cst, gates = _run(dev, W, pre, bs, 0, [(0, len(bs))])
    # launch per step: capnet_lstm_pointwise_fwd for t = 0, capnet_lstm_step_fused afterwards
    Wd = W.to(dev)
    wf = torch.empty(L.capnet_lstm_wfrag_floats(H), device=dev)
    check(L.capnet_lstm_pack_wfrag(Wd.data_ptr(), wf.data_ptr(), H, 0, current_stream()))
    G = pre.clone().to(dev)
    h = torch.zeros(sum(bs), H, device=dev)
    c = torch.zeros(sum(bs), H, device=dev)
    for t in range(len(bs)):
        r0 = 64 * t
        if t == 0:
            check(L.capnet_lstm_pointwise_fwd(G[r0:].data_ptr(), None, c[r0:].data_ptr(), h[r0:].data_ptr(), 64, H, 0,
                                              current_stream()))
        else:
            check(L.capnet_lstm_step_fused(h[r0 - 64:].data_ptr(), wf.data_ptr(), G[r0:].data_ptr(), 4 * H,
                                           c[r0 - 64:].data_ptr(), c[r0:].data_ptr(), h[r0:].data_ptr(), 64, H, 0,
                                           current_stream()))
    torch.cuda.synchronize()
    # different summation orders of the same fp32 products
    assert (hid - h.cpu()).abs().max().item() < 2e-6
    assert (cst - c.cpu()).abs().max().item() < 4e-6


def test_persistent_rejects_bad_arguments(dev):
    L = capnet.lib()
    assert L.capnet_lstm_persist_supported(64, 256) == 0
    assert L.capnet_lstm_persist_supported(129, H) == 0
    if not L.capnet_lstm_persist_supported(64, H):
        pytest.skip("persistent kernel not supported on this device")
    img = torch.zeros(L.capnet_lstm_persist_w_floats(), device=dev)
    buf = torch.zeros(64 * 4 * H, device=dev)
    ctl = torch.zeros(L.capnet_lstm_persist_ctl_ints(), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    args = lambda bs, t0, t1, seg: (img.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), int_array(bs),
                                    t0, t1, H, 0, seg, ctl.data_ptr(), err.data_ptr(), None, current_stream())
    assert L.capnet_lstm_persist_run(*args([4, 8], 0, 2, 1)) != 0        # growing batch
    assert L.capnet_lstm_persist_run(*args([4, 4], 1, 1, 1)) != 0        # empty range
    assert L.capnet_lstm_persist_run(*args([4, 4], 0, 2, 0)) != 0        # segment tags start at 1
    assert b"lstm_persist_run" in L.capnet_last_error()


@pytest.fixture
def persist_mode():
    """Sets capnet_lstm_persist_set_mode for one test and restores the previous mode."""
    L = capnet.lib()
    old = L.capnet_lstm_persist_set_mode(-1)
    yield lambda m: L.capnet_lstm_persist_set_mode(m)
    L.capnet_lstm_persist_set_mode(old)


def test_safe_mode_equals_local_mode(dev, persist_mode):
    """the cross-XCD form of the hand-off (every h byte and flag stored write-through) is chosen at run
    time by placement and never ran in the tests. Forced here (mode bit 1): bit-identical to LOCAL mode, also across
    segment cuts; the control block's diagnostics word says which mode each shard took."""
    L = capnet.lib()
    if not L.capnet_lstm_persist_supported(64, H):
        pytest.skip("persistent kernel not supported on this device")
    bs = CASES["b96"]
    W, pre = _case(11, bs)
    local = _run(dev, W, pre, bs, 1, [(0, len(bs))])
    persist_mode(2)
    safe = _run(dev, W, pre, bs, 1, [(0, 3), (3, len(bs))])
    for a, b in zip(local, safe):
        assert torch.equal(a, b)


def test_abort_path_raises_the_flag_and_every_workgroup_leaves(dev, persist_mode):
    """An expired wait (injected: mode bit 2) must end the launch -- no workgroup may keep spinning --, set bit 2 of
    err_flag, and the optimizer kernel given that word must leave the parameters alone. check_device_errors() names
    the cause and switches the process to the launch-per-step path."""
    from capnet import ops
    L = capnet.lib()
    if not L.capnet_lstm_persist_supported(64, H):
        pytest.skip("persistent kernel not supported on this device")
    bs = [64] * 4
    W, pre = _case(3, bs)
    persist_mode(4)
    img = torch.empty(L.capnet_lstm_persist_w_floats(), device=dev)
    check(L.capnet_lstm_persist_pack(W.to(dev).data_ptr(), img.data_ptr(), 0, current_stream()))
    G = pre.clone().to(dev)
    Cst = torch.zeros(sum(bs), H, device=dev)
    hid = torch.zeros(sum(bs), H, device=dev)
    ctl = torch.zeros(L.capnet_lstm_persist_ctl_ints(), dtype=torch.int32, device=dev)
    err = ops.err_flag(dev)
    err.zero_()
    check(L.capnet_lstm_persist_run(img.data_ptr(), G.data_ptr(), Cst.data_ptr(), hid.data_ptr(), int_array(bs), 0, 4, H, 0,
                                    1, ctl.data_ptr(), err.data_ptr(), None, current_stream()))
    torch.cuda.synchronize()            # returns: every workgroup left
    assert int(err.item()) == 4
    # the guarded update is a no-op while the flag is set
    p = torch.ones(1000, device=dev); g = torch.full((1000,), 0.3, device=dev)
    m = torch.zeros_like(p); v = torch.zeros_like(p)
    ops.clamp_adam([p], [g], [m], [v], [1], 1e-2, 0.9, 0.999, 1e-8, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(p, torch.ones_like(p)) and float(m.abs().max()) == 0.0
    with pytest.raises(capnet.CapnetError, match="persistent LSTM"):
        ops.check_device_errors()
    assert L.capnet_lstm_persist_set_mode(-1) == 1 and not L.capnet_lstm_persist_supported(64, H)
    ops.clamp_adam([p], [g], [m], [v], [1], 1e-2, 0.9, 0.999, 1e-8, 0.5)   # flag cleared: the update runs
    torch.cuda.synchronize()
    assert float((p - 1).abs().max()) > 1e-3
