"""The decoders' dropout mask without a GPU: its numpy restatement (oracle/dropout_ref.py) keeps 1 - p of the units
with independent streams, the oracles take masks without changing their mask-free results, and data-parallel ranks
draw different masks. tests/test_dropout_gpu.py holds the kernels to the oracles run with these masks."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import capnet
from capnet.model import DecoderFactoredLSTM, _dropout_seed
from capnet.model_att import DecoderFactoredLSTMAtt
from capnet.nic_model import DecoderRNN
from capnet.stacked import StackedFactoredLSTM
from capnet.stacked_att import StackedFactoredLSTMAtt
from helpers import pin_dropout_seed, rel_err
from oracle import decoders_ref as D
from oracle import dropout_ref as R
from stacked_att_ref import stacked_factored_att_forward

SEED = 0x2C3A5F19D0E7B461        # an arbitrary 62-bit seed


# ---- the restated mask ----------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.22, 0.5])
def test_keep_rate_and_scale(p):
    m = R.embedding_mask(SEED, 64, 24, 300, p)          # configs[1]'s embedding shape
    keep = np.float32(1) / (np.float32(1) - np.float32(p))
    assert m.dtype == np.float32 and set(np.unique(m).tolist()) == {0.0, float(keep)}
    n = m.size
    frac = float((m != 0).mean())
    assert abs(frac - (1 - p)) < 5 * math.sqrt(p * (1 - p) / n), frac
    lm = R.layer_mask(SEED, 64 * 24, 512, p, 1)
    frac = float((lm != 0).mean())
    assert abs(frac - (1 - p)) < 5 * math.sqrt(p * (1 - p) / lm.size), frac


def _corr(a, b):
    a = (a != 0).astype(np.float64).ravel()
    b = (b != 0).astype(np.float64).ravel()
    return float(np.corrcoef(a, b)[0, 1]), a.size


@pytest.mark.parametrize("p", [0.22, 0.5])
def test_streams_are_uncorrelated(p):
    B, T, E = 64, 24, 300
    m = R.embedding_mask(SEED, B, T, E, p)
    pairs = {
        "neighbour samples": (m[:-1], m[1:]),
        "neighbour columns": (m[:, :-1], m[:, 1:]),
        "neighbour units": (m[:, :, :-1], m[:, :, 1:]),
    }
    N, H = B * T, 512
    layers = [R.layer_mask(SEED, N, H, p, l) for l in (1, 2, 3)]
    pairs["layer 1 / layer 2"] = (layers[0], layers[1])
    pairs["layer 2 / layer 3"] = (layers[1], layers[2])
    pairs["neighbour rows of a layer"] = (layers[0][:-1], layers[0][1:])
    # the embedding stream against the layer stream at the same (sample, unit)
    pairs["embedding / layer 1"] = (R.embedding_mask(SEED, N, 1, H, p)[:, 0, :], layers[0])
    # and two seeds one apart (a seed + rank scheme would lean on this)
    pairs["seed / seed + 1"] = (m, R.embedding_mask(SEED + 1, B, T, E, p))
    for name, (a, b) in pairs.items():
        c, n = _corr(a, b)
        assert abs(c) < 5 / math.sqrt(n), (name, c, n)


def test_helpers_state_the_kernel_coordinates():
    p = 0.3
    m = R.embedding_mask(SEED, 5, 7, 11, p)
    lm = R.layer_mask(SEED, 9, 13, p, 2)
    for b, col, e in [(0, 0, 0), (4, 6, 10), (2, 3, 5)]:
        assert m[b, col, e] == R.dropout_scale(SEED, b, col, e, p)
    for r, e in [(0, 0), (8, 12), (3, 7)]:
        assert lm[r, e] == R.dropout_scale(SEED, r, 0x40000000 + 2, e, p)
    assert not np.array_equal(R.layer_mask(SEED, 9, 13, p, 1), lm)


# ---- the oracles with masks -----------------------------------------------------------------------
def _params(dec, seed, lim=0.3):
    g = torch.Generator().manual_seed(seed)
    return {k: ((torch.rand(v.shape, generator=g) * 2 - 1) * (lim if v.dim() > 1 else 0.05)).double()
            for k, v in dec.state_dict().items()}


def _case(B, V, T, seed):
    g = torch.Generator().manual_seed(seed)
    lengths = sorted([int(x) for x in torch.randint(2, T + 1, (B,), generator=g)], reverse=True)
    lengths[0] = T
    return torch.randint(3, V, (B, T), generator=g), lengths


def _oracles():
    """(name, forward(drop_mask, layer_masks), B, T, E, H, N) for every restated decoder."""
    B, T, E, H, F, V, A, Cf, P = 4, 6, 12, 16, 10, 29, 8, 20, 5
    caps, lens = _case(B, V, T, 3)
    N = sum(lens)
    feats = torch.rand(B, E, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    afeats = torch.rand(B, P, Cf, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    tf = [True, True, False, True, False, True]
    pf = _params(DecoderFactoredLSTM(E, H, F, V, 1, dropout=0.0), 4)
    pn = _params(DecoderRNN(E, H, V, 1, dropout=0.0), 5)
    pa = _params(DecoderFactoredLSTMAtt(A, E, H, F, V, 1, feature_size=Cf, dropout=0.0), 6)
    # (larger weights: three small-weight layers would damp the input's effect on the logits below 1e-2)
    ps = _params(StackedFactoredLSTM(E, H, F, V, 3, dropout=0.0), 7, lim=1.0)
    psa = _params(StackedFactoredLSTMAtt(A, E, H, F, V, 2, feature_size=Cf, dropout=0.0), 8, lim=1.0)
    return [
        ("factored", lambda m, lm: D.factored_lstm_forward(pf, caps, lens, feats, tf, drop_mask=m)),
        ("factored_nofeat", lambda m, lm: D.factored_lstm_forward(pf, caps, lens, None, tf, drop_mask=m)),
        ("nic", lambda m, lm: D.lstm_forward(pn, caps, lens, feats, tf, drop_mask=m)),
        ("att", lambda m, lm: D.factored_att_forward(pa, caps, lens, afeats, tf, drop_mask=m)[0]),
        ("stacked", lambda m, lm: D.stacked_factored_lstm_forward(ps, caps, lens, feats, tf, "factual", 3,
                                                                  drop_mask=m, layer_masks=lm)),
        ("stacked_att", lambda m, lm: stacked_factored_att_forward(psa, caps, lens, afeats, tf, "factual", 2,
                                                                   drop_mask=m, layer_masks=lm)[0]),
    ], (B, T, E, H, N)


def test_oracles_take_masks_without_changing_their_defaults():
    cases, (B, T, E, H, N) = _oracles()
    ones = torch.ones(B, T, E, dtype=torch.float64)
    lones = {l: torch.ones(N, H, dtype=torch.float64) for l in (1, 2)}
    mask = torch.from_numpy(R.embedding_mask(SEED, B, T, E, 0.5)).double()
    lmask = {l: torch.from_numpy(R.layer_mask(SEED, N, H, 0.5, l)).double() for l in (1, 2)}
    for name, fwd in cases:
        base = fwd(None, None)
        assert torch.equal(fwd(ones, None), base), name
        assert rel_err(fwd(mask, None), base) > 1e-2, name
        if name.startswith("stacked"):
            assert torch.equal(fwd(None, lones), base), name
            assert rel_err(fwd(None, lmask), base) > 1e-2, name


def test_stacked_restatement_masks_its_packed_rows():
    """layer_masks[l] is indexed by packed row: a mask that is zero on one step's rows and one elsewhere
    changes the logits of that step and later ones only."""
    cases, (B, T, E, H, N) = _oracles()
    fwd = dict(cases)["stacked"]
    base = fwd(None, None)
    bs = D.batch_sizes(_case(B, 29, T, 3)[1])
    off = [sum(bs[:t]) for t in range(len(bs) + 1)]
    m = torch.ones(N, H, dtype=torch.float64)
    m[off[3]:off[4]] = 0.0
    out = fwd(None, {2: m})
    assert torch.equal(out[:off[3]], base[:off[3]])
    assert not torch.equal(out[off[3]:off[4]], base[off[3]:off[4]])


# ---- the seed ------------------------------------------------------------------------------------
def test_seed_without_a_process_group_is_the_plain_draw():
    assert not (dist.is_available() and dist.is_initialized())
    want = pin_dropout_seed(77)
    assert _dropout_seed(True, 0.22) == want
    torch.manual_seed(77)
    assert int(torch.randint(0, 2 ** 62, (1,)).item()) == want           # (the draw itself is unchanged)
    assert _dropout_seed(False, 0.5) == 0 and _dropout_seed(True, 0.0) == 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import capnet  # noqa: F401
    from capnet.model import _dropout_seed
    torch.manual_seed(1234)                        # as every rank of bench.py does
    seeds = [_dropout_seed(True, 0.22) for _ in range(2)]
    after = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.save({"seeds": seeds, "after": after}, "%s.%d" % (out, rank))
    dist.barrier()
    dist.destroy_process_group()


def test_ranks_draw_different_masks(tmp_path):
    out = str(tmp_path / "seeds")
    world = 2
    mp.spawn(_rank_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    got = [torch.load("%s.%d" % (out, r), weights_only=False) for r in range(world)]
    # every rank consumed the same torch draws
    assert len({g["after"] for g in got}) == 1
    for step in range(2):
        seeds = [g["seeds"][step] for g in got]
        assert len(set(seeds)) == world, seeds
        assert all(0 <= s < 2 ** 64 for s in seeds)
        # local row 0 of each rank (global rows 0 and 1 of a length-sorted batch) gets its own mask
        rows = [R.embedding_mask(s, 1, 24, 300, 0.22)[0] for s in seeds]
        assert not np.array_equal(rows[0], rows[1])
        c, n = _corr(rows[0], rows[1])
        assert abs(c) < 5 / math.sqrt(n), c
    # while a single process draws what it always did
    torch.manual_seed(1234)
    plain = [_dropout_seed(True, 0.22) for _ in range(2)]
    torch.manual_seed(1234)
    assert plain == [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2)]
