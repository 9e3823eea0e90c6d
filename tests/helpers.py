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


SENTINEL = 0x7FC0BEEF                  # a NaN with a payload: int32 bits that no kernel writes


def up4(x):
    return (x + 3) // 4 * 4


class Window:
    """An N-d tensor of floats placed at given strides (in floats) inside a flat device buffer with a fence in front of
    it and behind it: element [i0][i1]... lives at buf[pre + off + i0 * strides[0] + i1 * strides[1] + ...]. Every float
    outside the window -- the fences, the `off` floats, every gap the strides leave -- is NaN (an input: a read outside
    the operand shows in the result) or the bit pattern `fill_bits` (an output or workspace: a write outside it shows).
    `ptr` is the address of element [0][0]..., which is 16-B aligned when off % 4 == 0 and never the start of the
    allocation. pre is rounded up to a multiple of 4 floats."""

    def __init__(self, values, strides, dev, off=0, pre=4, post=4, fill_bits=None):
        assert len(strides) == values.dim() and pre > 0 and post > 0
        pre = up4(pre)
        span = off + sum((n - 1) * s for n, s in zip(values.shape, strides)) + 1
        idx = torch.zeros(values.shape, dtype=torch.long)
        for d, (n, s) in enumerate(zip(values.shape, strides)):
            shape = [1] * values.dim()
            shape[d] = n
            idx = idx + (torch.arange(n) * s).view(shape)
        idx = idx.reshape(-1)
        self.idx = (pre + off + idx).to(dev)
        if fill_bits is None:
            buf = torch.full((pre + span + post,), float("nan"), device=dev)
        else:
            buf = torch.full((pre + span + post,), fill_bits, dtype=torch.int32, device=dev).view(torch.float32)
        buf[self.idx] = values.reshape(-1).to(device=dev, dtype=torch.float32)
        self.buf, self.before, self.shape = buf, buf.clone(), values.shape
        self.ptr = buf.data_ptr() + 4 * (pre + off)
        assert (buf.data_ptr() + 4 * pre) % 16 == 0

    def inside(self):
        return self.buf[self.idx].view(self.shape)

    def snapshot(self):
        """Take the buffer as it is now (after a pack kernel filled the window) as the state to compare against."""
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))

    def outside_unchanged(self):
        now = self.buf.clone()
        now[self.idx] = self.before[self.idx]
        return torch.equal(now.view(torch.int32), self.before.view(torch.int32))


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
