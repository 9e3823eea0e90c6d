"""csrc/fused_block.hip at MID = 64 and 128 (the block boundaries of trunk stages 1 and 2), whose eight-wave instantiations
are sized for two workgroups per CU: one identity register set one chunk ahead, asm loads and stores on a uniform base
with immediate offsets, their own counted waits. Against the same arithmetic in float64, at the smallest shapes that
reach every path: one full 128-row tile, a second tile of two rows (every other row of it a repeat of row M - 1), and
three tiles with a ragged last one; with and without a BatchNorm on the identity branch; with and without prescales.

The bounds are those of tests/test_fused_block_gpu.py. They are literals inside its test functions, so they are named
here and test_the_bounds_are_those_of_the_existing_file pins them to that file's text."""
import inspect

import pytest
import torch

import capnet  # noqa: F401
from capnet import ops
from helpers import rel_err
import test_fused_block_gpu as base

pytestmark = pytest.mark.gpu

SAME = 3e-6        # out, y1 against float64 with the (scale, shift) the kernel was given
PARTIAL = 1e-5     # statistics partials against float64
END_TO_END = 1e-5  # out, y1 against the all-float64 block

TILE = 128


def test_the_bounds_are_those_of_the_existing_file():
    src = inspect.getsource(base.test_statistics_from_the_gram_matrix_and_the_fused_kernel)
    assert "rel_err(out, out_same) < 3e-6" in src and "rel_err(y1, y1_same) < 3e-6" in src
    assert "rel_err(ps.sum(0), y1_same.sum(0)) < 1e-5" in src and "rel_err(pq.sum(0), (y1_same ** 2).sum(0)) < 1e-5" in src
    assert "rel_err(out, out_r) < 1e-5 and rel_err(y1, y1_r) < 1e-5" in src


@pytest.mark.parametrize("e3,e1", [(0, 0), (12, -12)])
@pytest.mark.parametrize("ds", [False, True])
@pytest.mark.parametrize("M", [128, 130, 300])
@pytest.mark.parametrize("MID", [64, 128])
def test_out_y1_and_partials_against_float64(dev, MID, M, ds, e3, e1):
    """A prescale is there to bring an operand into f16's range, so each comes with data at the reciprocal scale (as in
    the existing prescale test): conv3's input at 2^-e3, and the block's output -- BatchNorm3's affine and the identity
    branch -- at 2^-e1. The bounds are relative, so they are the same in both variants."""
    y2, s2, t2, w3, w1, gamma, beta, res, sd, td = base._case(M, MID, ds, 11 * M + MID)
    a_scale, o_scale = 2.0 ** -e3, 2.0 ** -e1
    s2, t2, eps = s2 * a_scale, t2 * a_scale, 1e-5 * a_scale ** 2
    gamma, beta, res = gamma * o_scale, beta * o_scale, res * o_scale
    if ds:
        td = td * o_scale
    _, _, scale, _, out_r, y1_r = base._reference(y2, s2, t2, w3, w1, gamma, beta, res, sd, td, eps=eps)
    d = lambda t: None if t is None else t.to(dev)
    y2d, s2d, t2d, resd = d(y2), d(s2), d(t2), d(res)
    img3, img1 = ops.pack_fused_block_weight(d(w3), 0), ops.pack_fused_block_weight(d(w1), 1)
    sc, sh = ops.fused_block_stats(y2d, s2d, t2d, img3, d(gamma), d(beta), eps=eps, in_exp=e3)
    assert rel_err(sc, scale) < 2e-6
    out, y1, ps, pq = ops.fused_block_forward(y2d, s2d, t2d, img3, sc, sh, resd, img1, d(sd), d(td), e3=e3, e1=e1)
    # with the SAME (scale, shift) the kernel was given
    D = torch.float64
    idn = res.to(D) if sd is None else res.to(D) * sd.to(D) + td.to(D)
    a2 = torch.relu(y2.to(D) * s2.to(D) + t2.to(D))
    y3 = a2 @ w3.reshape(4 * MID, MID).to(D).t()
    out_same = torch.relu(y3 * sc.double().cpu() + sh.double().cpu() + idn)
    y1_same = out.double().cpu() @ w1.reshape(MID, 4 * MID).to(D).t()
    e_out, e_y1 = rel_err(out, out_same), rel_err(y1, y1_same)
    # the partial rows: one per 128-row tile, the rows past M left out
    tiles = (M + TILE - 1) // TILE
    assert tuple(ps.shape) == (tiles, MID) and tuple(pq.shape) == (tiles, MID)
    pad = torch.zeros(tiles * TILE - M, MID, dtype=D)
    rows = torch.cat([y1_same, pad]).reshape(tiles, TILE, MID)
    e_ps, e_pq = rel_err(ps, rows.sum(1)), rel_err(pq, (rows ** 2).sum(1))
    e_out_r, e_y1_r = rel_err(out, out_r), rel_err(y1, y1_r)
    print("MID %d M %d ds %d e (%d, %d): out %.2e y1 %.2e | partial sum %.2e sq %.2e | end to end out %.2e y1 %.2e"
          % (MID, M, ds, e3, e1, e_out, e_y1, e_ps, e_pq, e_out_r, e_y1_r))
    assert e_out < SAME and e_y1 < SAME
    assert e_ps < PARTIAL and e_pq < PARTIAL
    assert rel_err(ps.sum(0), y1_same.sum(0)) < PARTIAL and rel_err(pq.sum(0), (y1_same ** 2).sum(0)) < PARTIAL
    assert e_out_r < END_TO_END and e_y1_r < END_TO_END
    ops.check_device_errors()


@pytest.mark.parametrize("MID,M", [(64, 50176), (128, 50176)])
def test_exact_beside_other_work(dev, MID, M):
    """The form of test_fused_kernel_is_exact_beside_other_work for the two instantiations with waits of their own: the
    same launch alone and beside a stream that keeps the memory system busy, bit for bit. 392 tiles: more than the chip
    has CUs, so that workgroups share a CU."""
    y2, s2, t2, w3, w1, gamma, beta, res, sd, td = base._case(M, MID, False, 77 + MID)
    d = lambda t: None if t is None else t.to(dev)
    y2d, s2d, t2d, resd = d(y2), d(s2), d(t2), d(res)
    img3, img1 = ops.pack_fused_block_weight(d(w3), 0), ops.pack_fused_block_weight(d(w1), 1)
    sc, sh = ops.fused_block_stats(y2d, s2d, t2d, img3, d(gamma), d(beta))
    out0, y10, ps0, pq0 = ops.fused_block_forward(y2d, s2d, t2d, img3, sc, sh, resd, img1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    big = torch.randn(64 * 1024 * 1024, device=dev)
    worst = 0
    for rep in range(6):
        with torch.cuda.stream(side):
            for _ in range(8):
                big = big * 1.0001 + 0.5                      # 512 MB of traffic per launch beside the kernel
        out, y1, ps, pq = ops.fused_block_forward(y2d, s2d, t2d, img3, sc, sh, resd, img1)
        torch.cuda.synchronize()
        worst = max(worst, int((out != out0).sum().item()) + int((y1 != y10).sum().item())
                    + int((ps != ps0).sum().item()) + int((pq != pq0).sum().item()))
    assert worst == 0
    ops.check_device_errors()
