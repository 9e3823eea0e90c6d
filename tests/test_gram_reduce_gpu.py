"""csrc/fused_block.hip, the statistics launches (fb_gram -> fb_gram_reduce -> fb_quad): the reduction of the Gram
partials, read back from a caller-owned workspace.
 * the partials lie as [pair][m][slice][64], the column-sum partials as [slice][K]; G and mu are their sums over the
   slices in double, in the kernel's order, rounded to float32: recomputed on the host and compared BIT FOR BIT,
   the mirrored lower blocks included;
 * (scale, shift) and the running statistics against float64 with the bounds of test_fused_block_gpu.py;
 * two calls on the same inputs give the same bits."""
import numpy as np
import pytest
import torch

import capnet  # noqa: F401
from capnet import _lib, ops
from capnet._lib import check, current_stream, ptr
from helpers import rel_err

pytestmark = pytest.mark.gpu

SHIPPED = [(200704, 64), (50176, 128), (12544, 256)]
# one slice (and M below a slice's rows); fewer than 8 slices, ragged last slice; slice counts that are no multiple of 8,
# whole and ragged; 65 slices at MID 64 (a second round of 64), ragged; 9 slices at MID 128
RAGGED = [(100, 64), (200, 256), (256, 128), (1297, 128), (2816, 256), (2716, 256), (32805, 64), (2304, 128)]
SHAPES = SHIPPED + RAGGED


def _rows(K):
    return 512 if K == 64 else 256


def _inputs(M, MID, seed):
    g = torch.Generator().manual_seed(seed)
    C = 4 * MID
    y2 = torch.randn(M, MID, generator=g) * torch.exp(0.5 * torch.randn(M, MID, generator=g))
    s2 = torch.rand(MID, generator=g) + 0.5
    t2 = torch.randn(MID, generator=g) * 0.5
    w3 = torch.randn(C, MID, 1, 1, generator=g) * (2.0 / MID) ** 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    return y2, s2, t2, w3, gamma, beta


def _run(dev, y2d, s2d, t2d, img3, gammad, betad):
    """capnet_fused_block_stats on a zeroed caller-owned workspace -> (work, scale, shift) on the host."""
    M, K = y2d.shape
    L = _lib.lib()
    work = torch.zeros(L.capnet_fused_block_stats_floats(M, K), dtype=torch.float32, device=dev)
    scale = torch.empty(4 * K, dtype=torch.float32, device=dev)
    shift = torch.empty_like(scale)
    check(L.capnet_fused_block_stats(ptr(y2d), ptr(s2d), ptr(t2d), ptr(img3), M, K, 0, ptr(gammad), ptr(betad), None, None,
                                     0.1, 1e-5, ptr(scale), ptr(shift), ptr(work), ptr(ops.err_flag(dev)), current_stream()),
          "capnet_fused_block_stats")
    torch.cuda.synchronize()
    return work.cpu().numpy(), scale.cpu().numpy(), shift.cpu().numpy()


def _split(work, M, K):
    """The workspace's parts: partials [pairs][64][slices][64], column-sum partials [slices][K], G [K][K], mu [K]."""
    slices, nb = -(-M // _rows(K)), K // 64
    pairs = nb * (nb + 1) // 2
    o_cs = slices * pairs * 4096
    o_G = o_cs + (slices * K + 3) // 4 * 4
    o_mu = o_G + K * K
    assert o_mu + K + 8 == work.size
    gp = work[:o_cs].reshape(pairs, 64, slices, 64)
    cs = work[o_cs:o_cs + slices * K].reshape(slices, K)
    return gp, cs, work[o_G:o_mu].reshape(K, K), work[o_mu:o_mu + K], slices, nb


def _sum_slices(x, axis):
    """The kernel's order over the slice axis: thread `part` of 8 adds slices part + 8 u + 64 j, u = 0..7 inside round j
    -- its slices in ascending order -- in double, then parts 1..7 are added onto part 0; rounded to float32 once."""
    x = np.moveaxis(x, axis, 0).astype(np.float64)
    parts = []
    for part in range(8):
        s = np.zeros(x.shape[1:], np.float64)
        for sl in range(part, x.shape[0], 8):
            s = s + x[sl]
        parts.append(s)
    s = parts[0]
    for q in range(1, 8):
        s = s + parts[q]
    return s.astype(np.float32)


@pytest.mark.parametrize("M,MID", SHAPES)
def test_gram_and_column_sums_are_the_ordered_double_sums_of_their_partials(dev, M, MID):
    y2, s2, t2, w3, gamma, beta = _inputs(M, MID, 11 * M + MID)
    d = lambda t: t.to(dev)
    img3 = ops.pack_fused_block_weight(d(w3), 0)
    work, _, _ = _run(dev, d(y2), d(s2), d(t2), img3, d(gamma), d(beta))
    gp, cs, G, mu, slices, nb = _split(work, M, MID)
    # the partials are what the layout says: slice sl of pair (bi, bj) is the Gram block of that slice's rows. Split-f16
    # operands carry 2^-22 relative (or 2^-25 absolute) each and the three products of non-negative terms are
    # accumulated in fp32 over at most `rows` rows: rows 2^-24 + 2^-20 of the block's largest entry bounds every entry.
    a2 = torch.relu(y2.double() * s2.double() + t2.double())
    rows = _rows(MID)
    bound = rows * 2.0 ** -24 + 2.0 ** -20
    worst = 0.0
    for sl in sorted({0, slices // 2, slices - 1}):
        a = a2[sl * rows:(sl + 1) * rows]
        ref = (a.t() @ a).numpy()
        p = 0
        for bi in range(nb):
            for bj in range(bi, nb):
                blk = ref[bi * 64:(bi + 1) * 64, bj * 64:(bj + 1) * 64]
                worst = max(worst, np.abs(gp[p, :, sl, :] - blk).max() / np.abs(blk).max())
                p += 1
        csr = a.sum(0).numpy()
        worst = max(worst, np.abs(cs[sl] - csr).max() / np.abs(csr).max())
    print("partials vs float64: %.3e (bound %.3e)" % (worst, bound))
    assert worst < bound
    # G and mu: exactly the ordered sums
    blocks = _sum_slices(gp, 2)                                         # [pairs][64 m][64 n]
    G_ref = np.empty((MID, MID), np.float32)
    p = 0
    for bi in range(nb):
        for bj in range(bi, nb):
            G_ref[bi * 64:(bi + 1) * 64, bj * 64:(bj + 1) * 64] = blocks[p]
            if bi < bj:
                G_ref[bj * 64:(bj + 1) * 64, bi * 64:(bi + 1) * 64] = blocks[p].T
                assert np.array_equal(G[bi * 64:(bi + 1) * 64, bj * 64:(bj + 1) * 64], G[bj * 64:(bj + 1) * 64, bi * 64:(bi + 1) * 64].T)
            p += 1
    assert np.array_equal(G, G_ref), int((G != G_ref).sum())
    assert np.array_equal(mu, _sum_slices(cs, 0))
    ops.check_device_errors()


@pytest.mark.parametrize("M,MID", SHAPES)
def test_statistics_against_float64(dev, M, MID):
    y2, s2, t2, w3, gamma, beta = _inputs(M, MID, 13 * M + MID)
    D = torch.float64
    a2 = torch.relu(y2.to(D) * s2.to(D) + t2.to(D))
    y3 = a2 @ w3.reshape(4 * MID, MID).to(D).t()
    mean, var = y3.mean(0), y3.var(0, unbiased=False)
    del y3
    scale = gamma.to(D) / torch.sqrt(var + 1e-5)
    shift = beta.to(D) - mean * scale
    d = lambda t: t.to(dev)
    img3 = ops.pack_fused_block_weight(d(w3), 0)
    rm, rv = torch.zeros(4 * MID, device=dev), torch.ones(4 * MID, device=dev)
    sc, sh = ops.fused_block_stats(d(y2), d(s2), d(t2), img3, d(gamma), d(beta), rm, rv, momentum=0.1)
    unb = var * (M / max(M - 1, 1))
    e_sc, e_sh = rel_err(sc, scale), (sh.double().cpu() - shift).abs().max().item()
    e_rm, e_rv = rel_err(rm, 0.1 * mean), rel_err(rv, 0.9 + 0.1 * unb)
    print("scale %.3e shift %.3e (of %.3e) running mean %.3e var %.3e" % (e_sc, e_sh, shift.abs().max().item(), e_rm, e_rv))
    # the bounds of test_fused_block_gpu.py
    assert e_sc < 2e-6
    assert e_sh < 4e-6 * max(1.0, shift.abs().max().item())
    assert e_rm < 2e-6
    assert e_rv < 2e-6
    ops.check_device_errors()


@pytest.mark.parametrize("M,MID", [(12544, 256), (50176, 128), (32805, 64)])
def test_two_calls_give_the_same_bits(dev, M, MID):
    y2, s2, t2, w3, gamma, beta = _inputs(M, MID, 17 * M + MID)
    d = lambda t: t.to(dev)
    args = (d(y2), d(s2), d(t2), ops.pack_fused_block_weight(d(w3), 0), d(gamma), d(beta))
    w0, sc0, sh0 = _run(dev, *args)
    w1, sc1, sh1 = _run(dev, *args)
    assert np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
    assert np.array_equal(sc0.view(np.uint32), sc1.view(np.uint32)) and np.array_equal(sh0.view(np.uint32), sh1.view(np.uint32))
    ops.check_device_errors()
