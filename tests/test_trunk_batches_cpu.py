"""The replicated-batch identities that tests/test_trunk_batches_gpu.py takes its expected values from, held in fp64 on
the CPU oracle (oracle/resnet152_ref.py): R copies of a base batch give, in train mode, the base batch's features and
running means, and running variances that differ by the unbiased-count factor alone (tests/trunk_batches_ref.py).
No GPU needed. Measured here in fp64: features 1.0e-11, running means 1.8e-12, running variances 5.7e-12 (bounds 1e-9); the
base batch against the fixture 3.9e-8, the fixture's fp32 storage (bound 1e-6)."""
import pytest
import torch

import capnet  # noqa: F401
from helpers import encoder_state, load_golden, rel_err
from trunk_batches_ref import base_images, expected_running_stats, trunk_oracle

R = 2


@pytest.fixture(scope="module")
def oracles():
    from oracle.resnet152_ref import EncoderCNNRef
    torch.set_num_threads(16)
    state = encoder_state(EncoderCNNRef(300))
    imgs = base_images(3)
    return trunk_oracle(state, imgs, torch.float64), trunk_oracle(state, imgs.repeat(R, 1, 1, 1), torch.float64)


def test_replicas_have_the_base_batch_features(oracles):
    base, big = oracles
    assert base["pooled"].dtype == torch.float64 and tuple(big["pooled"].shape) == (3 * R, 2048)
    for r in range(R):
        e = rel_err(big["pooled"][3 * r:3 * r + 3], base["pooled"])
        print("fp64 oracle, replica %d vs base batch: %.2e" % (r, e))
        assert e < 1e-9
    e = rel_err(base["pooled"], load_golden("trunk_b3.npz")["pooled_train"])
    print("fp64 oracle, base batch vs fixture: %.2e" % e)
    assert e < 1e-6


def test_replicas_have_the_base_batch_running_means(oracles):
    base, big = oracles
    assert len(base["keys"]) == 155 and big["keys"] == base["keys"]
    means, _ = expected_running_stats(base, R)
    errs = [rel_err(big["mean"][k], m) for k, m in zip(base["keys"], means)]
    print("fp64 oracle, running means of %d replicas vs base batch: worst %.2e" % (R, max(errs)))
    for k, e in zip(base["keys"], errs):
        assert e < 1e-9, k
    assert all(torch.equal(m, base["mean"][k]) for k, m in zip(base["keys"], means))
    assert all(big["nbt"][k] == 1 for k in base["keys"])


def test_replicas_running_variances_follow_the_count_factor(oracles):
    base, big = oracles
    _, variances = expected_running_stats(base, R)
    errs = [rel_err(big["var"][k], v) for k, v in zip(base["keys"], variances)]
    print("fp64 oracle, running variances of %d replicas vs count formula: worst %.2e" % (R, max(errs)))
    for k, e in zip(base["keys"], errs):
        assert e < 1e-9, k
    # the factor is not a no-op at the resolution of the check: without it the last stage (147 samples) is 3e-4 off
    k = base["keys"][-1]
    assert base["count"][k] == 3 * 7 * 7 and big["count"][k] == R * 3 * 7 * 7
    assert rel_err(big["var"][k], base["var"][k]) > 1e-6
    # R = 1 is the identity
    _, same = expected_running_stats(base, 1)
    assert all(rel_err(v, base["var"][k]) < 1e-14 for k, v in zip(base["keys"], same))
