"""The ResNet-152 trunk at the batch sizes the project ships -- 12 (the attention path per GPU), 64 (the benchmark)
and 96 -- against the fp64 oracle of a batch of 3 or 4 images, through batches made of replicas.

The launch plan (tile shapes, persistent loops, K-sliced tails, the bn_finalize variant, the fused boundaries' grids)
depends on M = B H W, and the oracle is affordable only at a few images. Train-mode BatchNorm over R copies of a base
batch has the base batch's mean and biased variance in every layer, so every activation is a replica of the base
batch's: features and running means are the base batch's, running variances differ by the unbiased-count factor
(tests/trunk_batches_ref.py; tests/test_trunk_batches_cpu.py holds the oracle to that in fp64). The 155 BatchNorms'
running statistics are per-channel moments of every convolution's output, so they localise a defect to a layer; and
replicas may differ among themselves by summation order only, so a tile that is wrong for some image indices shows in
the replica spread even where pooling averages it below the feature tolerance."""
import contextlib

import pytest
import torch

import capnet  # noqa: F401
from capnet import model_att, ops, synthetic
from capnet._lib import check, current_stream, lib, ptr
from capnet.model import EncoderCNN
from helpers import encoder_state, load_golden, rel_err
from trunk_batches_ref import MOMENTUM, base_images, expected_running_stats, trunk_oracle

pytestmark = pytest.mark.gpu
TOL = 2e-3          # trunk features at a few images per batch against fp64: see tests/test_encoder_gpu.py
SPREAD = 2e-4       # trunk results that differ in summation order only, under given statistics (same file)
STAT_FLOOR = 1e-4   # the stem's running statistics against fp64 (same file)


@pytest.fixture(scope="module")
def golden():
    return load_golden("trunk_b3.npz")


@pytest.fixture(scope="module")
def state():
    return encoder_state(EncoderCNN(300))


@pytest.fixture(scope="module")
def oracle(dev, state, golden):
    """Per base batch size b: the fp64 oracle of one train-mode pass, and the fp32 oracle's own per-layer error in the
    running statistics against it (e_cpu_mean[l], e_cpu_var[l])."""
    torch.set_num_threads(16)
    out = {}
    for b in (3, 4):
        imgs = base_images(b)
        o64 = trunk_oracle(state, imgs, torch.float64, want_map=(b == 3))
        o32 = trunk_oracle(state, imgs, torch.float32)
        o64["e_cpu_mean"] = [rel_err(o32["mean"][k], o64["mean"][k]) for k in o64["keys"]]
        o64["e_cpu_var"] = [rel_err(o32["var"][k], o64["var"][k]) for k in o64["keys"]]
        print("base %d: fp32 oracle vs fp64, features %.2e, running means %.2e .. %.2e, running variances %.2e .. %.2e"
              % (b, rel_err(o32["pooled"], o64["pooled"]), min(o64["e_cpu_mean"]), max(o64["e_cpu_mean"]),
                 min(o64["e_cpu_var"]), max(o64["e_cpu_var"])))
        out[b] = o64
    # the base-3 oracle is the committed fixture (tools/gen_golden.py made it the same way)
    assert rel_err(out[3]["pooled"], golden["pooled_train"]) < 1e-6
    assert rel_err(out[3]["map"][0], golden["att_map_train_b0"]) < 1e-6
    return out


def _spread(x, b):
    """Worst rel_err of a replica (b consecutive images) against replica 0."""
    return max([rel_err(x[r * b:(r + 1) * b], x[:b]) for r in range(1, x.shape[0] // b)] + [0.0])


@pytest.mark.parametrize("B,b,knobs", [
    (12, 3, {}),
    (12, 3, {"defer_stats": True, "graph": True}),
    (64, 4, {}),
    (64, 4, {"defer_stats": True, "balance_tails": False, "slot": 1}),
    (96, 3, {}),
], ids=["12", "12-deferred-graph", "64", "64-deferred-pipelined", "96"])
def test_train_mode_features_and_every_running_statistic(dev, state, golden, oracle, B, b, knobs):
    """One train-mode pass from fresh running statistics over B / b replicas of the base batch: 12 with the defaults
    and as the benchmark runs the trunk below 32 images (deferred statistics, a replayed graph), 64 with the defaults
    and as the pipelined benchmark step runs it (deferred statistics, unbalanced tails, the second workspace), 96.
    Every replica's features within TOL of the base batch's fp64 features; replicas within SPREAD of each other; each
    of the 155 BatchNorms' running statistics within max(1e-4, 2 x the fp32 CPU oracle's own error in that layer) of
    the fp64 expectation; num_batches_tracked advanced by one everywhere.

    The graph row also leaves NaNs in the block the graph's static input buffer will take: the warm-up pass in front
    of the capture used to run on that uninitialised buffer and raised the trunk's non-finite error word.

    Measured on an MI355X (the fp32 CPU oracle is 7.4e-4 / 7.3e-4 from fp64 in the features at base 3 / 4, up to
    1.2e-4 in a running mean and 3.3e-4 in a running variance). Per row: features vs fp64; replica spread; worst
    e_gpu / e_cpu of the running means and of the running variances over all 155 layers, with the layer (mostly a
    layer far below the 1e-4 floor); worst e_gpu / bound for means, variances.
      12                     6.25e-4  0.0  1.66 (resnet.4.1.bn3, 1.3e-7)  1.47 (resnet.4.0.bn1, 9.1e-8)    0.57, 0.61
      12 deferred, graph     the same figures
      64                     6.24e-4  0.0  1.54 (resnet.5.3.bn3, 1.5e-7)  1.76 (resnet.6.27.bn1, 9.98e-5)  0.47, 0.88
      64 deferred, pipelined 6.23e-4  0.0  1.54 (resnet.5.3.bn3, 1.5e-7)  1.76 (resnet.6.27.bn1, 9.99e-5)  0.48, 0.88
      96                     6.95e-4  0.0  2.00 (resnet.5.1.bn1, 1.2e-7)  1.50 (resnet.4.0.bn1, 9.2e-8)    0.58, 0.53
    The replicas agree bit for bit: no kernel's summation order depends on a row's position in the batch."""
    R = B // b
    base = oracle[b]
    want = torch.as_tensor(golden["pooled_train"]).double() if b == 3 else base["pooled"]
    enc = EncoderCNN(300)
    enc.load_state_dict(state)
    enc.to(dev).train()
    imgs = base_images(b).repeat(R, 1, 1, 1).to(dev)
    ctx = contextlib.nullcontext()
    if knobs.get("graph"):
        # a graph is captured on a stream of its own, as capnet.train.TrunkPipeline runs the pass
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        ctx = torch.cuda.stream(side)
    with ctx:
        if knobs.get("graph"):
            # the graph's static input buffer takes the block this frees (the weights are packed first, so that nothing
            # else does): the warm-up pass before the capture must not read what an earlier owner left there (the
            # error word would rise, and capnet.optim.Adam drops steps while it is set)
            runner = enc._trunk()
            runner._pack(runner._plan(B, 224, 224, dev), dev)
            junk = torch.full_like(imgs, float("nan"))
            del junk
        res = enc._trunk().forward(imgs, True, True, False, **knobs)
        if knobs.get("defer_stats"):
            assert len(res) == 3
            sd = enc.state_dict()
            assert all(int(sd[k + ".num_batches_tracked"]) == 0 for k in base["keys"])      # deferred means deferred
            assert float(sd["resnet.1.running_mean"].abs().max()) == 0.0
            res[2]()
        else:
            assert len(res) == 2
    pooled = res[0]
    torch.cuda.synchronize()
    ops.check_device_errors()
    assert tuple(pooled.shape) == (B, 2048)
    feat = max(rel_err(pooled[r * b:(r + 1) * b], want) for r in range(R))
    spread = _spread(pooled, b)
    sd = {k: v.cpu() for k, v in enc.state_dict().items()}
    means, variances = expected_running_stats(base, R, MOMENTUM)
    rows = []
    for l, k in enumerate(base["keys"]):
        rows.append((k, rel_err(sd[k + ".running_mean"], means[l]), base["e_cpu_mean"][l],
                     rel_err(sd[k + ".running_var"], variances[l]), base["e_cpu_var"][l]))
    wm = max(rows, key=lambda r: r[1] / max(r[2], 1e-30))
    wv = max(rows, key=lambda r: r[3] / max(r[4], 1e-30))
    print("B = %d %s: features vs fp64 %.2e, replica spread %.2e; worst e_gpu / e_cpu: running mean %.2f (%s: %.2e vs "
          "%.2e), running variance %.2f (%s: %.2e vs %.2e); worst e_gpu / bound: %.2f, %.2f"
          % (B, knobs, feat, spread, wm[1] / max(wm[2], 1e-30), wm[0], wm[1], wm[2], wv[3] / max(wv[4], 1e-30), wv[0],
             wv[3], wv[4], max(r[1] / max(STAT_FLOOR, 2 * r[2]) for r in rows),
             max(r[3] / max(STAT_FLOOR, 2 * r[4]) for r in rows)))
    assert feat < TOL
    assert spread < SPREAD
    for k, em, cm, ev, cv in rows:
        assert em < max(STAT_FLOOR, 2 * cm), "%s.running_mean: %.3e from fp64, the fp32 oracle %.3e" % (k, em, cm)
        assert ev < max(STAT_FLOOR, 2 * cv), "%s.running_var: %.3e from fp64, the fp32 oracle %.3e" % (k, ev, cv)
    for k in base["keys"]:
        assert int(sd[k + ".num_batches_tracked"]) == 1, k


def test_attention_encoder_at_twelve_per_gpu(dev, state, golden, oracle):
    """model_att.EncoderCNN(14) in train mode on four replicas of the base batch of 3: the bounds the map is held to
    at B = 3 (tests/test_encoder_gpu.py), for every replica, and the replica spread.
    Measured on an MI355X: image 0 against the fixture 1.75e-3 (every image against the fp64 map: the same), the
    checksums 2.8e-6, replica spread 0."""
    b, R = 3, 4
    enc = model_att.EncoderCNN(14)
    enc.load_state_dict({k: v for k, v in state.items() if k.startswith("resnet.") and not k.startswith("resnet.8")})
    enc.to(dev).train()
    fmap = enc(base_images(b).repeat(R, 1, 1, 1).to(dev))
    torch.cuda.synchronize()
    ops.check_device_errors()
    assert tuple(fmap.shape) == (12, 14, 14, 2048)
    cs = golden["att_map_checksum"]
    e0, ecs, eall = [], [], []
    for r in range(R):
        blk = fmap[r * b:(r + 1) * b]
        e0.append(rel_err(blk[0], golden["att_map_train_b0"]))
        ecs.append(max(abs(blk.double().sum().item() - cs[0]) / abs(cs[0]),
                       abs(blk.double().abs().sum().item() - cs[1]) / cs[1]))
        eall.append(max(rel_err(blk[i], oracle[b]["map"][i]) for i in range(b)))
    spread = _spread(fmap, b)
    print("attention map at B = 12: image 0 vs fixture %.2e, checksums %.2e, every image vs fp64 %.2e, replica spread "
          "%.2e" % (max(e0), max(ecs), max(eall), spread))
    assert max(e0) < 2 * TOL
    assert max(ecs) < 1e-3
    assert max(eall) < 2 * TOL      # images 1 and 2 of every replica too, against the live fp64 map
    assert spread < SPREAD
    sd = enc.state_dict()
    assert all(int(sd[k + ".num_batches_tracked"]) == 1 for k in oracle[b]["keys"])


@pytest.fixture(scope="module")
def eval_case(dev, state):
    """Seeded running statistics and the fp32 CPU oracle's inference features of a base of 2 images, as in
    test_folded_bn_inference_trunk_matches_oracle_with_given_statistics (tests/test_encoder_gpu.py)."""
    from oracle.resnet152_ref import EncoderCNNRef
    st = {k: v.clone() for k, v in state.items()}
    g = torch.Generator().manual_seed(99)
    for k in list(st):
        if k.startswith("resnet.") and k.endswith("running_mean"):
            st[k] = torch.randn(st[k].shape, generator=g) * 0.05
        if k.startswith("resnet.") and k.endswith("running_var"):
            st[k] = torch.rand(st[k].shape, generator=g) + 0.5
        if k.startswith("resnet.") and k.endswith("bn3.weight"):
            st[k] = torch.full_like(st[k], 0.3)      # keeps the residual sum bounded over 50 blocks
    ref = EncoderCNNRef(300)
    ref.load_state_dict({k: v.clone() for k, v in st.items()})
    ref.eval()
    imgs = synthetic.make_batch(2, 100, seed=3)[0]
    torch.set_num_threads(16)
    with torch.no_grad():
        want = ref.resnet(imgs).reshape(2, -1)
    return st, imgs, want


@pytest.mark.parametrize("B", [64, 96])
@pytest.mark.parametrize("folded", ["0", "1"])
def test_inference_trunk_at_the_shipped_batches(dev, monkeypatch, eval_case, folded, B):
    """encoder.eval() at 64 and 96 images, both inference plans (CAPNET_EVAL_FOLDED): inference is independent per
    image whatever the batch, so every row of a base of 2 images cycled through the batch is within 2e-4 of the fp32
    CPU oracle's row for that image, equal images agree to 2e-4, and no running statistic moves.
    Measured on an MI355X: rows 7.7e-7 (folded 0) / 8.4e-7 (folded 1) at both batches, spread 0."""
    monkeypatch.setenv("CAPNET_EVAL_FOLDED", folded)
    st, imgs, want = eval_case
    enc = EncoderCNN(300)
    enc.load_state_dict(st)
    enc.to(dev).eval()
    pooled, fmap = enc._trunk().forward(imgs.repeat(B // 2, 1, 1, 1).to(dev), False, True, True)
    torch.cuda.synchronize()
    ops.check_device_errors()
    assert tuple(pooled.shape) == (B, 2048) and tuple(fmap.shape) == (B, 7, 7, 2048)
    e = max(rel_err(pooled[i], want[i % 2]) for i in range(B))
    emap = max(rel_err(fmap[i].mean(dim=(0, 1)), want[i % 2]) for i in range(B))
    spread = max(_spread(pooled, 2), _spread(fmap, 2))
    print("inference trunk, folded = %s, B = %d: rows vs fp32 oracle %.2e (map %.2e), spread over equal images %.2e"
          % (folded, B, e, emap, spread))
    assert e < 2e-4 and emap < 2e-4
    assert spread < SPREAD
    for k, v in enc.state_dict().items():
        if k.startswith("resnet.") and k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked"):
            assert torch.equal(v.cpu(), st[k]), k


@pytest.mark.parametrize("C_", [64, 72])
@pytest.mark.parametrize("tiles", [1, 16, 17, 128, 129, 512, 513, 1568])
def test_bn_finalize_at_the_partial_row_counts_of_the_batches(dev, tiles, C_):
    """capnet_bn_finalize is the one kernel whose variant the batch alone selects: 16 partial rows per workgroup up to
    128 partials, 32 up to 512, 64 beyond (1568: stage 1 at batch 64); 72 channels leave a ragged last group of 16.
    The reference sums THE SAME fp32 partials in fp64 and does the rest in fp64, so only the reduction and the
    kernel's float roundings are under test: double accumulation, one rounding to float and one fma give 2e-6 with
    room. Nothing past channel C is written. Measured on an MI355X: at most 1.1e-7 in any of the four outputs."""
    g = torch.Generator().manual_seed(1000 * C_ + tiles)
    count, pad = tiles * 8, 16
    y = torch.randn(count, C_, generator=g) * 2 + torch.randn(C_, generator=g) * 3
    part = y.view(tiles, 8, C_)
    psum, psq = part.sum(1), (part * part).sum(1)                       # fp32 per-tile partials, as the convolutions leave
    gamma, beta = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
    rm0, rv0 = torch.randn(C_, generator=g), torch.rand(C_, generator=g) + 0.5
    eps = 1e-5
    mom = torch.tensor(MOMENTUM, dtype=torch.float32).double().item()   # the C call takes a float
    s, q = psum.double().sum(0), psq.double().sum(0)
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0)
    want_scale = gamma.double() / torch.sqrt(var + eps)
    want_shift = beta.double() - mean * want_scale
    want_rm = (1 - mom) * rm0.double() + mom * mean
    want_rv = (1 - mom) * rv0.double() + mom * var * (count / (count - 1))

    def padded(x):
        return torch.cat([x, torch.full((pad,), float("nan"))]).to(dev)
    scale, shift = padded(torch.full((C_,), float("nan"))), padded(torch.full((C_,), float("nan")))
    rm, rv = padded(rm0), padded(rv0)
    psum_d, psq_d, gd, bd = psum.to(dev), psq.to(dev), gamma.to(dev), beta.to(dev)
    check(lib().capnet_bn_finalize(ptr(psum_d), ptr(psq_d), tiles, C_, count, ptr(gd), ptr(bd), ptr(rm), ptr(rv),
                                   MOMENTUM, eps, ptr(scale), ptr(shift), current_stream()))
    torch.cuda.synchronize()
    ops.check_device_errors()
    errs = (rel_err(scale[:C_], want_scale), rel_err(shift[:C_], want_shift), rel_err(rm[:C_], want_rm),
            rel_err(rv[:C_], want_rv))
    print("bn_finalize, %d partial rows x %d channels: scale %.1e, shift %.1e, running mean %.1e, running variance %.1e"
          % ((tiles, C_) + errs))
    assert max(errs) < 2e-6, errs
    for name, x in (("scale", scale), ("shift", shift), ("running_mean", rm), ("running_var", rv)):
        assert bool(torch.isfinite(x[:C_]).all()), name
        assert bool(torch.isnan(x[C_:]).all()), name + " written past channel C"
