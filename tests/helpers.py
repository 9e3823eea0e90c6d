import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def encoder_state(enc):
    """The seeded state of an EncoderCNN (product or oracle) that the trunk tests and tests/golden/trunk_b3.npz share:
    kaiming-normal convolutions, BatchNorm2d weight 1 / bias 0 with fresh running statistics, a xavier head."""
    from capnet import synthetic
    return synthetic.encoder_state(enc.state_dict(), seed=1234)


def golden_params(z):
    return {k[len("param."):]: t(z[k]) for k in z.files if k.startswith("param.")}


def golden_case(z, cname):
    pre = "case.%s." % cname
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def pin_dropout_seed(k):
    """torch.manual_seed(k) and the dropout seed the next decoder forward (training, p > 0, no process group) will
    draw: capnet.model._dropout_seed's one torch.randint(0, 2**62, (1,)), the first torch draw of a forward. The
    generator is left re-seeded with k, so call the decoder right after this."""
    torch.manual_seed(k)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(k)
    return seed
