"""Expected trunk results at large batches from the CPU oracle of a small base batch.

Train-mode BatchNorm normalises with the batch mean and the BIASED batch variance, and a batch of R copies of a base
batch has, in every layer, exactly the base batch's mean and biased variance. By induction every activation of the big
batch is a replica of the base batch's, so features and running means are the base batch's own, and a running variance
differs only by the unbiased-count factor (expected_running_stats). tests/test_trunk_batches_cpu.py holds this module
to that in fp64; tests/test_trunk_batches_gpu.py reads its expected values from here."""
import torch

from capnet import synthetic

MOMENTUM = 0.1          # nn.BatchNorm2d's default, the trunk's


def base_images(b):
    return synthetic.make_batch(b, 100, seed=0)[0]


def trunk_oracle(state, imgs, dtype, want_map=False):
    """One train-mode pass of oracle/resnet152_ref.py in `dtype` from the running statistics in `state`.
    -> {"pooled": [B, 2048], "map": [B, 14, 14, 2048] (want_map), "keys": the 155 BatchNorms' state-dict prefixes in
    module order, "mean" / "var" / "nbt": prefix -> running statistic after the pass, "count": prefix -> samples per
    channel (B H W of that layer)}."""
    from oracle.resnet152_ref import EncoderCNNRef
    ref = EncoderCNNRef(300)
    ref.load_state_dict({k: v.clone() for k, v in state.items()})
    ref.to(dtype).train()
    bns = [(name, m) for name, m in ref.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    count = {}
    hooks = [m.register_forward_hook(lambda mod, inp, out, name=name:
                                     count.__setitem__(name, inp[0].numel() // inp[0].shape[1])) for name, m in bns]
    with torch.no_grad():
        fmap = ref.resnet[:-1](imgs.to(dtype))
        pooled = ref.resnet[-1](fmap).reshape(imgs.shape[0], -1)
    for h in hooks:
        h.remove()
    out = {"pooled": pooled, "keys": [name for name, _ in bns], "count": count,
           "mean": {name: m.running_mean.clone() for name, m in bns},
           "var": {name: m.running_var.clone() for name, m in bns},
           "nbt": {name: int(m.num_batches_tracked) for name, m in bns}}
    if want_map:
        out["map"] = torch.nn.functional.adaptive_avg_pool2d(fmap, 14).permute(0, 2, 3, 1).contiguous()
    return out


def expected_running_stats(base, R, momentum=MOMENTUM):
    """Running statistics after ONE pass from fresh ones (mean 0, variance 1) over R replicas of the base batch, from the
    base batch's oracle `base` (trunk_oracle's result), in fp64: the running means are the base batch's; with n_b
    samples per channel in the base batch and n_B = R n_b in the big one, the unbiased variance is
    unbiased_b (n_b - 1) / n_b  n_B / (n_B - 1). -> (means, variances), two lists over base["keys"]."""
    means, variances = [], []
    for k in base["keys"]:
        n_b = base["count"][k]
        n_B = R * n_b
        unbiased_b = (base["var"][k].double() - (1.0 - momentum)) / momentum
        unbiased_B = unbiased_b * ((n_b - 1) / n_b) * (n_B / (n_B - 1))
        means.append(base["mean"][k].double())
        variances.append((1.0 - momentum) + momentum * unbiased_B)
    return means, variances
