"""bench.py --dump-outputs: dump_outputs() on CPU tensors -- the byte budget, whole arrays below their share, a fixed
seeded sample of the elements above it, and the same files on every call. No GPU needed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _model(shapes):
    g = torch.Generator().manual_seed(0)
    named = []
    for name, shape in shapes:
        p = torch.nn.Parameter(torch.randn(shape, generator=g))
        p.grad = torch.randn(shape, generator=g)
        named.append((name, p))
    frozen = torch.nn.Parameter(torch.randn(7, generator=g))      # no gradient: not updated by the step, not written
    return named + [("frozen", frozen)]


def _load(d):
    return {f[:-len(".npy")]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_fits_the_budget_and_samples_large_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 200000)
    named = _model([("C.weight", (300, 200)), ("W.weight", (64, 64)), ("W.bias", (64,))])
    loss = torch.tensor(2.5)
    nbytes = bench.dump_outputs(str(tmp_path / "a"), loss, named)
    got = _load(str(tmp_path / "a"))
    assert nbytes == sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert nbytes <= 200000
    assert set(got) == {"loss", "param.C.weight", "grad.C.weight", "param.W.weight", "grad.W.weight",
                        "param.W.bias", "grad.W.bias"}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].shape == (1,) and got["loss"][0] == 2.5
    p = dict(named)
    # below their share: whole, in their own shape
    for name in ("W.weight", "W.bias"):
        assert np.array_equal(got["param." + name], p[name].detach().numpy())
        assert np.array_equal(got["grad." + name], p[name].grad.numpy())
    # above it: flat, the elements at sorted indices of a seeded permutation -- the same ones for parameter and gradient
    a = got["param.C.weight"]
    assert a.ndim == 1 and 0 < a.size < 300 * 200
    idx = torch.randperm(300 * 200, generator=torch.Generator().manual_seed(0))[:a.size].sort().values
    assert np.array_equal(a, p["C.weight"].detach().reshape(-1)[idx].numpy())
    assert np.array_equal(got["grad.C.weight"], p["C.weight"].grad.reshape(-1)[idx].numpy())


def test_dump_is_the_same_on_every_call(tmp_path):
    named = _model([("big", (3000, 3000)), ("mid", (1000, 1000)), ("bias", (1000,))])
    loss = torch.tensor(1.0)
    sizes = [bench.dump_outputs(str(tmp_path / d), loss, named) for d in ("a", "b")]
    assert sizes[0] == sizes[1] <= bench.DUMP_BUDGET_BYTES
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["param.big"].ndim == 1 and a["param.big"].size < 3000 * 3000
