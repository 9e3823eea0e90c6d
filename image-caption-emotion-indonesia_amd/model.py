"""StyleNet models on the MI355X kernels: EncoderCNN and DecoderFactoredLSTM.

Mirrors the class surface of the reference's stylenet/model.py (constructor signatures,
attribute names, state_dict keys, forward()/forward_step() semantics); all arithmetic runs in
libcapnet_hip.so through capnet.ops. Differences from the reference are listed in DESIGN.md.
"""
import ctypes as C
import math
import os
import random
import sys

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import CapnetError, check, current_stream, ptr, ptr_array
from .decode import beam_decode, check_styles, fold_factored, fused_decode_step, plain_stack, plain_styles, sample_random, score_captions, zero_state

random.seed(0)  # stylenet/model.py:7
device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')  # stylenet/model.py:8


# ---------------------------------------------------------------------------------------
# parameter containers (same state_dict keys as torch.nn / torchvision modules; their
# forward() goes through the HIP operators, never through a torch kernel)
# ---------------------------------------------------------------------------------------
class Linear(nn.Module):

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        bound = 1.0 / math.sqrt(in_features)
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        shape = x.shape
        y = ops.linear(x.reshape(-1, shape[-1]), self.weight, self.bias)
        return y.reshape(*shape[:-1], self.out_features)


class Embedding(nn.Module):

    def __init__(self, num_embeddings, embedding_dim):
        super().__init__()
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim).normal_())

    def forward(self, idx):
        return ops.embedding(idx, self.weight)


class Dropout(nn.Module):
    """Holds p; the mask itself is generated inside the decoder kernels."""

    def __init__(self, p):
        super().__init__()
        self.p = p


class _Conv(nn.Module):
    """Conv2d parameter container (weight [Cout, Cin, k, k], no bias)."""

    def __init__(self, cin, cout, k, stride, pad):
        super().__init__()
        self.stride, self.pad = stride, pad
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        nn.init.kaiming_normal_(self.weight, mode='fan_out', nonlinearity='relu')


class _BN2d(nn.Module):
    """BatchNorm2d parameter/buffer container."""

    def __init__(self, c, momentum=0.1, eps=1e-5):
        super().__init__()
        self.momentum, self.eps = momentum, eps
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer('running_mean', torch.zeros(c))
        self.register_buffer('running_var', torch.ones(c))
        self.register_buffer('num_batches_tracked', torch.tensor(0, dtype=torch.long))


class _Marker(nn.Module):
    """Parameter-less position holder (ReLU / MaxPool / AvgPool slots of the nn.Sequential)."""


class _Bottleneck(nn.Module):

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = _Conv(inplanes, planes, 1, 1, 0)
        self.bn1 = _BN2d(planes)
        self.conv2 = _Conv(planes, planes, 3, stride, 1)
        self.bn2 = _BN2d(planes)
        self.conv3 = _Conv(planes, planes * 4, 1, 1, 0)
        self.bn3 = _BN2d(planes * 4)
        self.relu = _Marker()
        if downsample:
            self.downsample = nn.Sequential(_Conv(inplanes, planes * 4, 1, stride, 0),
                                            _BN2d(planes * 4))
        else:
            self.downsample = None


def _resnet152_children(with_avgpool):
    """torchvision resnet152 children[:-1] / [:-2] as parameter containers (same key names)."""
    mods = [_Conv(3, 64, 7, 2, 3), _BN2d(64), _Marker(), _Marker()]
    inplanes = 64
    for li, (planes, blocks) in enumerate(zip((64, 128, 256, 512), (3, 8, 36, 3))):
        layer = []
        for b in range(blocks):
            stride = 2 if (b == 0 and li > 0) else 1
            layer.append(_Bottleneck(inplanes, planes, stride, downsample=(b == 0)))
            inplanes = planes * 4
        mods.append(nn.Sequential(*layer))
    if with_avgpool:
        mods.append(_Marker())
    return nn.Sequential(*mods)


class _TrunkRunner:
    """Owns the C-side plan, workspace and packed weights of one ResNet-152 trunk."""

    def __init__(self, resnet):
        self.resnet = resnet
        self.convs, self.bns = [], []
        seq = list(resnet.children())
        self.convs.append(seq[0]); self.bns.append(seq[1])
        for layer in seq[4:8]:
            for blk in layer.children():
                self.convs += [blk.conv1, blk.conv2, blk.conv3]
                self.bns += [blk.bn1, blk.bn2, blk.bn3]
                if blk.downsample is not None:
                    self.convs.append(blk.downsample[0]); self.bns.append(blk.downsample[1])
        self.plans = {}
        self.timing = False
        self.timing_every, self._graph_timing, self._timed_passes = 1, False, 0
        self.packed = None
        self.packed_key = None
        self._exp_epoch = 0

    def invalidate_exponents(self):
        """Forget the cached per-layer prescale exponents (see _input_exponents): call after writing BatchNorm
        parameters of the trunk through anything that does not bump torch's version counters."""
        self._exp_epoch += 1

    def _plan(self, b, h, w, dev):
        key = (b, h, w, str(dev))
        p = self.plans.get(key)
        if p is None:
            L = _lib.lib()
            handle = C.c_void_p()
            check(L.capnet_trunk_create(b, h, w, C.byref(handle)), "capnet_trunk_create")
            n = L.capnet_trunk_num_convs(handle)
            if n != len(self.convs):
                raise CapnetError("trunk plan has %d convolutions, module has %d" % (n, len(self.convs)))
            nbytes = L.capnet_trunk_workspace_bytes(handle)
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            p = {"handle": handle, "ws": ws, "slots": {0: ws}, "nbytes": nbytes,
                 "side": L.capnet_trunk_final_side(handle), "flops": L.capnet_trunk_flops(handle)}
            self.plans[key] = p
        return p

    def _workspace(self, plan, slot, dev):
        """One workspace per pipeline slot (passes in flight on different streams)."""
        ws = plan["slots"].get(slot)
        if ws is None:
            ws = torch.empty(plan["nbytes"] // 4, dtype=torch.float32, device=dev)
            plan["slots"][slot] = ws
        return ws

    def _pack(self, plan, dev):
        key = (str(dev),) + tuple((c.weight.data_ptr(), c.weight._version) for c in self.convs)
        if self.packed_key != key:
            L = _lib.lib()
            packed = []
            vals = [C.c_int() for _ in range(5)]
            for i, c in enumerate(self.convs):
                check(L.capnet_trunk_conv_shape(plan["handle"], i, *[C.byref(v) for v in vals]))
                cout, cin, k, stride, kw = [v.value for v in vals]
                if tuple(c.weight.shape) != (cout, cin, k, k) or c.stride != stride:
                    raise CapnetError("conv %d: module shape %s does not match the plan" %
                                      (i, tuple(c.weight.shape)))
                # 0 rows, 1 K-major (the f32-MFMA kernels), 5 split f16, 6 the stem's split f16, 7 / 8 fused_block.hip
                kind = L.capnet_trunk_conv_kmajor(plan["handle"], i)
                if kind in (7, 8):    # a block boundary on fused_block.hip: 7 = its conv3, 8 = the next block's conv1
                    packed.append(ops.pack_fused_block_weight(c.weight.detach(), kind - 7))
                elif kind == 6:
                    packed.append(ops.pack_conv_weight_stem_f16x3(c.weight.detach()))
                elif kind == 5:
                    packed.append(ops.pack_conv_weight_f16x3(c.weight.detach(), L.capnet_trunk_conv_tile_n(plan["handle"], i)))
                else:
                    packed.append(ops.pack_conv_weight(c.weight.detach(), kw, kmajor=kind == 1))
            self.packed, self.packed_key = packed, key
            # the images were written on THIS stream; passes on other streams (TrunkPipeline runs
            # one pass per stream) must not read them before these kernels have finished
            self.pack_event = torch.cuda.Event()
            self.pack_event.record()
            self.pack_waited = {torch.cuda.current_stream().cuda_stream}
        elif getattr(self, "pack_event", None) is not None:
            st = torch.cuda.current_stream()
            if st.cuda_stream not in self.pack_waited:
                st.wait_event(self.pack_event)
                self.pack_waited.add(st.cuda_stream)
        return self.packed

    def _input_exponents(self, plan, b, h, w):
        """Per convolution: the power of two its INPUT tensor is multiplied by on its way into the f16 planes of the
        split-f16 kernels (capnet_trunk_forward's input_exponents), chosen so that the tensor's largest possible
        value lands in [2^14, 2^15) -- below f16's 65 504 whatever the scale of the BatchNorm parameters, with the
        typical values far enough above f16's subnormals for their residuals to keep 22 bits.

        The bounds are rigorous in train mode and use nothing but the parameters: a batch-normalised value is at most
        sqrt(M - 1) standard deviations from its mean (M = B OH OW values per channel), so |bn(y)| <= sqrt(M - 1)
        max|gamma| + max|beta|; a block's output is bounded by its two summands' bounds. The exponents are computed
        for 4 096 standard deviations (>= sqrt(M - 1) for every M the kernels take, 2^24): still 2^3 for a typical
        value of one standard deviation, whose low piece is then a normal f16 number.
        Inference (running statistics) has no such bound -- the running statistics need not fit the data --, so it
        only ever scales DOWN (min(e, 0): the range never shrinks below the unscaled 65 504) and relies on the
        error word (bit 3: the launches without statistics look at their own outputs) to say so if an activation
        exceeds it. Images are taken as they come (exponent 0): normalised pixels.
        -> (train exponents, inference exponents) as ctypes int arrays."""
        # every BatchNorm's version and storage (three of 155 missed partial loads). Kernels that write
        # parameters through raw pointers (capnet.optim.Adam on a trunk someone fine-tunes) do not bump `_version`:
        # such a caller invalidates by hand, `runner.invalidate_exponents()`; the reference workflow keeps the trunk
        # under no_grad and only load_state_dict() touches these tensors.
        key = (b, h, w, self._exp_epoch) + tuple(x for bn in self.bns for x in
                                                 (bn.weight._version, bn.bias._version, bn.weight.data_ptr()))
        hit = plan.get("exps")
        if hit is not None and hit[0] == key:
            return hit[1], hit[3]
        with torch.no_grad():
            gb = torch.stack([bn.weight.detach().abs().max() for bn in self.bns] +
                             [bn.bias.detach().abs().max() for bn in self.bns]).cpu().tolist()
        n = len(self.bns)
        g, bt = gb[:n], gb[n:]

        def post(i, m):
            assert m < (1 << 24)
            return 4096.0 * g[i] + bt[i]

        def ea(bound):
            if not (bound > 0.0 and math.isfinite(bound)):
                return 0
            return max(-40, min(40, 15 - math.frexp(bound)[1]))      # bound < 2^e  ->  bound 2^(15 - e) in [2^14, 2^15)

        exps = [0] * n
        oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1                  # stem 7x7 / 2, pad 3
        a_in = post(0, b * oh * ow)                                  # max-pool of relu(bn(stem))
        hh, ww = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1                # max-pool 3x3 / 2, pad 1
        ci = 1
        for li, blocks in enumerate((3, 8, 36, 3)):
            for blk in range(blocks):
                stride = 2 if (blk == 0 and li > 0) else 1
                i1, i2, i3 = ci, ci + 1, ci + 2
                idn = ci + 3 if blk == 0 else -1
                ci += 4 if blk == 0 else 3
                m_in = b * hh * ww
                hh, ww = (hh - 1) // stride + 1, (ww - 1) // stride + 1
                m_out = b * hh * ww
                exps[i1] = ea(a_in)
                exps[i2] = ea(post(i1, m_in))
                exps[i3] = ea(post(i2, m_out))
                if idn >= 0:
                    exps[idn] = ea(a_in)
                    a_in = post(i3, m_out) + post(idn, m_out)
                else:
                    a_in = post(i3, m_out) + a_in
        arr = (C.c_int * n)(*exps)
        arr_eval = (C.c_int * n)(*[min(e, 0) for e in exps])
        plan["exps"] = (key, arr, exps, arr_eval)
        return arr, arr_eval

    def _tables(self, packed):
        """ctypes pointer tables of the C call (packed weights, BN weight / bias / running mean /
        running var), rebuilt only when a tensor moved: building them is ~1 ms of host time per
        pass otherwise."""
        # (module.to() / re-packing replace the tensors; load_state_dict copies in place)
        key = (id(packed), self.bns[0].weight.data_ptr(), self.bns[-1].running_var.data_ptr(),
               self.bns[len(self.bns) // 2].running_mean.data_ptr())
        if getattr(self, "_table_key", None) != key:
            self._table_val = (ptr_array(packed), ptr_array([bn.weight for bn in self.bns]),
                               ptr_array([bn.bias for bn in self.bns]),
                               ptr_array([bn.running_mean for bn in self.bns]),
                               ptr_array([bn.running_var for bn in self.bns]))
            self._table_key = key
        return self._table_val

    def forward(self, images, train, want_pooled, want_map, slot=0, defer_stats=False,
                balance_tails=True, graph=False):
        """defer_stats (train mode only): leave the running statistics alone and return a callable
        that applies this pass's update (capnet_trunk_update_running + num_batches_tracked) on the
        then-current stream; the caller decides when (TrunkPipeline orders passes with events)."""
        ops._need_cuda(images)
        if images.dim() != 4 or images.shape[1] != 3:
            raise CapnetError("images must be [B, 3, H, W]")
        images = images.contiguous()
        b, _, h, w = images.shape
        dev = images.device
        plan = self._plan(b, h, w, dev)
        packed = self._pack(plan, dev)
        side = plan["side"]
        ws = self._workspace(plan, slot, dev)
        if plan.get("balance_tails", True) != bool(balance_tails):
            check(_lib.lib().capnet_trunk_set_tail_balance(plan["handle"], int(bool(balance_tails))),
                  "capnet_trunk_set_tail_balance")
            plan["balance_tails"] = bool(balance_tails)
        bn0 = self.bns[0]
        tables = self._tables(packed)
        exps = self._input_exponents(plan, b, h, w)[0 if train else 1]
        err = ops.err_flag(dev)
        L = _lib.lib()

        def launch(img, pooled, fmap):
            check(L.capnet_trunk_forward(
                plan["handle"], ptr(img), tables[0], tables[1], tables[2], tables[3], tables[4],
                (2 if defer_stats else 1) if train else 0, bn0.momentum, bn0.eps,
                ptr(ws), ptr(pooled), ptr(fmap), exps, ptr(err), current_stream()), "capnet_trunk_forward")

        def new_outputs():
            p = torch.empty((b, 2048), dtype=torch.float32, device=dev) if want_pooled else None
            f = torch.empty((b, side, side, 2048), dtype=torch.float32, device=dev) if want_map else None
            return p, f

        use_graph = graph and train and defer_stats and os.environ.get("CAPNET_NO_GRAPH") != "1"
        if use_graph and self.timing:
            # event records cannot ride in a replayed graph: every N-th pass is launched directly and bracketed
            # (capnet_trunk_time_next_pass), the others replay; the C side's own every-N-th counter stays off, so that
            # the launches under capture are never bracketed
            if not self._graph_timing:
                check(L.capnet_trunk_set_timing(plan["handle"], 0), "capnet_trunk_set_timing")
                self._graph_timing = True
            self._timed_passes += 1
            if (self._timed_passes - 1) % self.timing_every == 0:
                check(L.capnet_trunk_time_next_pass(plan["handle"]), "capnet_trunk_time_next_pass")
                use_graph = False
        if use_graph:
            # The pass is ~330 launches with fixed arguments: captured once per (slot, outputs,
            # tile mode) into a hipGraph and replayed -- one launch call on the host instead of
            # ~3.5 ms of them. Input and outputs are static buffers of the graph.
            gkey = (slot, want_pooled, want_map, bool(balance_tails))
            sig = (id(tables), images.dtype)
            st = plan.setdefault("graphs", {}).get(gkey)
            if st is None or st["sig"] != sig:
                # (a copy of this batch, not uninitialised memory: a NaN left there by an earlier owner would raise
                # the error word in the warm-up below, and capnet.optim.Adam drops steps while it is set)
                static_in = images.clone()
                sp, sf = new_outputs()
                launch(static_in, sp, sf)      # eager warm-up: one-time attribute calls
                g = torch.cuda.CUDAGraph()
                # thread_local: other threads (an RCCL watchdog) may keep calling into HIP meanwhile
                with torch.cuda.graph(g, stream=torch.cuda.current_stream(),
                                      capture_error_mode="thread_local"):
                    launch(static_in, sp, sf)
                st = {"sig": sig, "graph": g, "in": static_in, "pooled": sp, "fmap": sf}
                plan["graphs"][gkey] = st
            st["in"].copy_(images, non_blocking=True)
            st["graph"].replay()
            pooled = st["pooled"].clone() if want_pooled else None
            fmap = st["fmap"].clone() if want_map else None
        else:
            pooled, fmap = new_outputs()
            launch(images, pooled, fmap)
        if train and defer_stats:
            def apply_running_stats():
                check(L.capnet_trunk_update_running(
                    plan["handle"], ptr(ws), tables[3], tables[4], bn0.momentum, current_stream()),
                    "capnet_trunk_update_running")
                torch._foreach_add_([bn.num_batches_tracked for bn in self.bns], 1)
            return pooled, fmap, apply_running_stats
        if train:
            torch._foreach_add_([bn.num_batches_tracked for bn in self.bns], 1)
        return pooled, fmap

    def set_timing(self, plan, on):
        """Per-conv hipEvent timing (bench.py roofline); event records cannot ride in a replayed
        graph, so timed passes are launched directly."""
        self.timing = bool(on)
        self.timing_every = max(int(on), 1)
        self._graph_timing, self._timed_passes = False, 0
        check(_lib.lib().capnet_trunk_set_timing(plan["handle"], int(on)), "capnet_trunk_set_timing")


class _BN1d(nn.Module):
    """nn.BatchNorm1d(embed_size, momentum=0.01) of the encoder head."""

    def __init__(self, c, momentum=0.1, eps=1e-5):
        super().__init__()
        self.momentum, self.eps = momentum, eps
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer('running_mean', torch.zeros(c))
        self.register_buffer('running_var', torch.ones(c))
        self.register_buffer('num_batches_tracked', torch.tensor(0, dtype=torch.long))

    def forward(self, x):
        y = ops.batch_norm1d(x, self.weight, self.bias, self.running_mean, self.running_var,
                             self.training, self.momentum, self.eps)
        if self.training:
            self.num_batches_tracked += 1
        return y


class EncoderCNN(nn.Module):
    """stylenet/model.py:11-27 (identical to nic/model.py:10-26).

    The reference builds torchvision's resnet152(pretrained=True); neither torchvision nor its
    weights exist offline, so the trunk starts from torchvision's own initialisation
    (kaiming-normal fan_out convolutions, BN weight 1 / bias 0) and takes pretrained tensors
    through load_state_dict (same keys: resnet.0.weight, resnet.4.0.conv1.weight, ...).
    """

    def __init__(self, embed_size):
        super(EncoderCNN, self).__init__()
        self.resnet = _resnet152_children(with_avgpool=True)
        self.linear = Linear(2048, embed_size)
        self.bn = _BN1d(embed_size, momentum=0.01)
        self._runner = [None]  # not a submodule
        # optional callable run between the frozen trunk and the trainable head: a data-parallel
        # optimiser uses it to make the compute stream wait for the previous step's update,
        # which it overlapped with this step's trunk forward (capnet.parallel)
        self.pre_head_hook = None

    def _trunk(self):
        if self._runner[0] is None:
            self._runner[0] = _TrunkRunner(self.resnet)
        return self._runner[0]

    def trunk_features(self, images, slot=0, defer_stats=False, balance_tails=True, graph=False):
        """children[:-1] of the ResNet under no_grad (model.py:23-25): pooled [B, 2048].
        slot / defer_stats: see _TrunkRunner.forward (used by capnet.train.TrunkPipeline); with
        defer_stats in train mode the result is (features, apply_running_stats)."""
        with torch.no_grad():
            out = self._trunk().forward(images, self.training, True, False, slot=slot,
                                        defer_stats=defer_stats and self.training,
                                        balance_tails=balance_tails, graph=graph)
        features = out[0].reshape(out[0].size(0), -1)
        if defer_stats:
            return features, (out[2] if len(out) > 2 else None)
        return features

    def zero_grad(self, set_to_none=True):
        """The trunk runs under no_grad and never holds gradients: visit only the head (walking
        the 465 trunk parameters costs more host time per step than the whole decoder launch)."""
        self.linear.zero_grad(set_to_none=set_to_none)
        self.bn.zero_grad(set_to_none=set_to_none)

    def forward(self, images):
        features = self.trunk_features(images)
        if self.pre_head_hook is not None:
            self.pre_head_hook()
        features = self.bn(self.linear(features))
        return features


# ---------------------------------------------------------------------------------------
# decoders
# ---------------------------------------------------------------------------------------
def _draw_tf_mask(n_steps, teacher_forcing_ratio):
    """One random.random() draw per time step, in step order (stylenet/model.py:181)."""
    return [random.random() < teacher_forcing_ratio for _ in range(n_steps)]


def _resolve_tf_mask(tf_mask, n_steps, teacher_forcing_ratio):
    if tf_mask is None:
        return _draw_tf_mask(n_steps, teacher_forcing_ratio)
    if len(tf_mask) < n_steps:
        raise CapnetError("tf_mask has %d entries, %d steps needed" % (len(tf_mask), n_steps))
    return [bool(x) for x in tf_mask[:n_steps]]


def _splitmix64(x):
    """splitmix64 of x: a bijection of the 64-bit integers."""
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def _dropout_seed(training, p):
    """Seed of the decoders' dropout mask (csrc/dropout_mask.h), one torch draw per forward. Under an initialised
    process group of more than one rank the draw is XORed with splitmix64(rank): ranks seed torch alike and key the
    mask by their LOCAL sample index, so without it local row i would get the same mask on every rank. Every rank still
    consumes the same draw, the seeds are pairwise different (XOR with a bijection of the rank), and a process
    without a process group keeps the plain draw."""
    if training and p > 0:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            seed ^= _splitmix64(dist.get_rank())
        return seed
    return 0


def _seq_cfg(dec, batch_sizes, p, tf_mask, teacher_forcing_ratio, **extra):
    """The cfg dict of ops.SeqFn / ops.AttSeqFn for decoder `dec` with dropout p, `extra` being the keys of its class.
    Consumes `random` first (one draw per step unless tf_mask is given), then torch's generator (_dropout_seed)."""
    cfg = {"batch_sizes": batch_sizes,
           "tf_mask": _resolve_tf_mask(tf_mask, len(batch_sizes), teacher_forcing_ratio),
           "hidden_size": dec.hidden_size,
           "dropout": p if dec.training else 0.0,
           "seed": _dropout_seed(dec.training, p),
           "training": dec.training}
    cfg.update(extra)
    return cfg


_MODES = ("factual", "happy", "sad", "angry")
_S_PREFIX = {"factual": "f", "happy": "happy_", "sad": "sad_", "angry": "angry_"}


def _layer_mods(dec, tag, mode):
    """(V, S, U, W) of one factored layer of `dec`, each the four gates' Linears in the order i, f, o, c: V{tag}_g,
    S{tag}_f{g} or S{tag}_{mode}_{g}, U{tag}_g, W{tag}_g. tag: "" for layer 0, the layer's number above it."""
    return tuple([getattr(dec, "%s%s_%s%s" % (name, tag, _S_PREFIX[mode] if name == "S" else "", g)) for g in "ifoc"]
                 for name in "VSUW")


class DecoderFactoredLSTM(nn.Module):
    """stylenet/model.py:30-294. `num_layers` is accepted and ignored, as in the reference."""

    def __init__(self,
                 embed_size,
                 hidden_size,
                 factored_size,
                 vocab_size,
                 num_layers,
                 feature_size=2048,
                 bias=True,
                 dropout=0.22,
                 max_seq_length=40):
        super(DecoderFactoredLSTM, self).__init__()
        if not bias:
            raise CapnetError("DecoderFactoredLSTM: bias=False is not supported by the HIP path")
        self.feature_size = feature_size
        self.hidden_size = hidden_size
        self.factored_size = factored_size
        self.embed_size = embed_size
        self.vocab_size = vocab_size
        self.max_seq_length = max_seq_length

        self.dropout = Dropout(dropout)
        self.B = Embedding(vocab_size, embed_size)

        # registration order follows stylenet/model.py:52-97 (state_dict order)
        for g in "ifoc":
            setattr(self, "U_" + g, Linear(factored_size, hidden_size, bias=bias))
            setattr(self, "S_f" + g, Linear(factored_size, factored_size, bias=bias))
            setattr(self, "V_" + g, Linear(embed_size, factored_size, bias=bias))
            setattr(self, "W_" + g, Linear(hidden_size, hidden_size, bias=bias))
        for emo in ("happy", "sad", "angry"):
            for g in "ifoc":
                setattr(self, "S_%s_%s" % (emo, g), Linear(factored_size, factored_size, bias=bias))
        self.C = Linear(hidden_size, vocab_size, bias=bias)

        self.reset_parameters()
        self.init_weights()

    def reset_parameters(self):
        for p in self.parameters():
            if p.data.ndimension() >= 2:
                nn.init.xavier_uniform_(p.data)
            else:
                nn.init.zeros_(p.data)

    def init_weights(self):
        self.B.weight.data.uniform_(-0.1, 0.1)
        self.C.bias.data.fill_(0)
        self.C.weight.data.uniform_(-0.1, 0.1)

    def _S(self, mode):
        if mode == "factual":
            return [getattr(self, "S_f" + g) for g in "ifoc"]
        if mode in _MODES:
            return [getattr(self, "S_%s_%s" % (mode, g)) for g in "ifoc"]
        # the reference only writes this message and then silently skips S (model.py:144-145);
        # here an unknown mode is an error.
        sys.stderr.write("mode name wrong!")
        raise ValueError("unknown mode %r (expected one of %s)" % (mode, ", ".join(_MODES)))

    def _weights(self, mode):
        V = [getattr(self, "V_" + g) for g in "ifoc"]
        S = self._S(mode)
        U = [getattr(self, "U_" + g) for g in "ifoc"]
        W = [getattr(self, "W_" + g) for g in "ifoc"]
        out = []
        for grp in (V, S, U, W):
            out += [m.weight for m in grp]
            out += [m.bias for m in grp]
        return out

    def forward_step(self, embedded, states, mode):
        h_t, c_t = states
        V = [getattr(self, "V_" + g) for g in "ifoc"]
        S = self._S(mode)
        U = [getattr(self, "U_" + g) for g in "ifoc"]
        W = [getattr(self, "W_" + g) for g in "ifoc"]
        # gate pre-activations [b, 4H]: U_g(S_g(V_g(x))) lands in its column block, W_g(h) is
        # accumulated onto it (no torch.cat / add kernels on the decode path)
        H = self.hidden_size
        with torch.no_grad():
            pre = torch.empty((embedded.shape[0], 4 * H), dtype=torch.float32, device=embedded.device)
            h_c = h_t.contiguous()
            for k in range(4):
                a2 = S[k](V[k](embedded))
                blk = pre[:, k * H:(k + 1) * H]
                ops.sgemm(a2, U[k].weight, transB=True, bias=U[k].bias, out=blk)
                ops.sgemm(h_c, W[k].weight, transB=True, bias=W[k].bias, out=blk, accumulate=True)
        h_t, c_t = ops.lstm_pointwise(pre, c_t, ops.CELL_FACTORED)
        return h_t, (h_t, c_t)

    def forward(self,
                captions,
                lengths,
                features=None,
                teacher_forcing_ratio=0.8,
                mode='factual',
                tf_mask=None):
        """tf_mask (extension): explicit per-step teacher-forcing decisions; by default they
        are drawn from the global `random` module, one per step, as the reference does."""
        batch_sizes = ops.batch_sizes_from_lengths(lengths)
        weights = self._weights(mode)
        cfg = _seq_cfg(self, batch_sizes, self.dropout.p, tf_mask, teacher_forcing_ratio, factored_size=self.factored_size)
        hiddens = ops.SeqFn.apply(cfg, captions, features, self.B.weight, self.C.weight, self.C.bias, *weights)
        outputs = self.C(hiddens)
        return outputs

    def _beam(self, rows, mode, plain=False):
        """(step_fn, the zero state of `rows` beams) of a beam search. plain (one_call=True): the chain folded for the fused
        decode step (capnet.decode.fold_factored, the fold of StackedFactoredLSTM's layer 0) rides on step_fn where that
        step takes the shape (capnet.decode.plain_stack); the steps of step_fn itself stay the composed chain."""
        self._S(mode)   # validates the mode before any launch

        def step_fn(prev_words, state):
            hidden, (h, c) = self.forward_step(self.B(prev_words), state, mode=mode)
            return self.C(hidden), (h, c)
        if plain and fused_decode_step(1, self.embed_size, self.hidden_size):
            plain_stack(step_fn, [fold_factored(*_layer_mods(self, "", mode))], ops.CELL_FACTORED, self.B.weight, self.C)
        return step_fn, zero_state(rows, self.hidden_size, self.B.weight.device)

    def sample(self, features, start_token, end_token, k=5, factual_limit=-1, mode='factual', on_device=False, poll_every=0,
               one_call=False, constraints=None, diversity=None, nbest=False, length_penalty=0.0):
        """Beam search, stylenet/model.py:198-294. As in the reference the image features are NOT
        an input of the decode steps (the first input is B(<start>) and the state starts at zero):
        `features` only fixes the device. Returns LongTensor [1, L].
        on_device / poll_every / one_call: capnet.decode.beam_decode's (the bookkeeping on the device; the whole search
        in one C call, on the folded chain; same sequences).
        constraints: a capnet.beam.Constraints -- no n-gram twice, no <end> before min_words words, no banned word --
        kept inside the search on whichever route runs (capnet.decode.beam_decode); the scores stay the model's own.
        diversity: a capnet.beam.Diversity -- the k beams as groups that pay for the words earlier groups chose at the same
        step, for several different captions of one image (capnet.decode.beam_decode); the scores stay the model's own.
        nbest / length_penalty: capnet.decode.beam_decode's -- every completed hypothesis as a (tokens, score) pair, best
        first, in place of the one caption."""
        return beam_decode(self, *self._beam(k, mode, one_call), None, k, start_token, end_token, on_device, poll_every, one_call,
                           nbest=nbest, length_penalty=length_penalty, constraints=constraints, diversity=diversity)

    def sample_random(self, features, start_token, end_token, samples=1, temperature=1.0, top_k=0, seed=None, mode='factual',
                      top_p=1.0, device=False, greedy=False, exclude=None):
        """`samples` captions per row of `features`, DRAWN from the decoder's distribution softmax(logits / temperature)
        (top_k > 0: renormalised over the top_k best words of every step;
        top_p < 1: over the nucleus) instead of searched for: a list of n lists of
        `samples` (tokens, logprob) pairs, tokens = [start, w_1 .. w_j] cut after the first end_token (none: all
        max_seq_length words), logprob the float sum of the kept words' log-probabilities under the distribution sampled
        from. As in sample(), the image is not an input of the decode steps. seed: an integer makes the call a pure function
        of its arguments; None draws a 63-bit seed from torch's CPU generator (torch.manual_seed). One C call
        (capnet_sample_decode) or the composed loop, the same lists: capnet.decode.sample_random.
        greedy=True: every image's pairs are followed by one more, its greedy caption (the argmax of every step), decoded as
        one more row of the same call; the first `samples` pairs are those of the call without it.
        device=True: (the lists, ids, logp), the decode's raw rows [n samples, max_seq_length] left on the device
        (capnet.decode.sample_random_device).
        exclude (a capnet.beam.Constraints without forced words): what no caption may draw -- a repeated n-gram, <end> within
        min_words, banned words -- excluded words being not pickable and logprob that of the distribution renormalised over
        the allowed words (capnet.decode.sample_random_device); None: the call as it was."""
        n = features.size(0)
        return sample_random(self, *self._beam(n * (int(samples) + bool(greedy)), mode, True), n, samples, start_token, end_token, temperature,
                             top_k, seed, top_p, device, greedy, exclude)

    def score_captions(self, features, captions, mode='factual'):
        """float32 [len(captions)] on the device: the model's log-probability of every caption [start, w_1 .. w_j], summed over
        w_1 .. w_j (<end> too where present), in the caller's order. captions: a flat list of token lists, or the nested
        list sample_random returns (the logprob of a (tokens, logprob) pair is ignored). As in sample(), the image is not an
        input: `features` is not read. Under no_grad, dropout following self.training: capnet.decode.score_captions."""
        return score_captions(self, features, captions, mode)

    def sample_batch(self, features, start_token, end_token, k=5, factual_limit=-1, mode='factual', on_device=False,
                     poll_every=0, one_call=False, constraints=None, diversity=None, nbest=False, length_penalty=0.0):
        """sample() for every row of `features` at once (capnet.beam.beam_search_batched): what the reference's test-set
        evaluator does image by image (stylenet/evaluator.py:76-84). Returns a list of token lists, each equal to
        sample(features[i:i+1], ...)[0].tolist()."""
        n = features.size(0)
        return beam_decode(self, *self._beam(n * k, mode, one_call), n, k, start_token, end_token, on_device, poll_every, one_call,
                           nbest=nbest, length_penalty=length_penalty, constraints=constraints, diversity=diversity)

    def sample_styles(self, features, start_token, end_token, k=5, modes=_MODES, poll_every=0):
        """sample_batch(one_call=True) in every style of `modes` at once -> {mode: [n token lists]}, each list equal to
        sample_batch(features, ..., mode=mode, one_call=True): ONE search over len(modes) x n x k rows on the grouped
        decode step (capnet_beam_decode_groups), every mode's chain folded into its slice of one buffer. As in sample(),
        the image is not an input. modes: a non-empty sequence of distinct mode names (an unknown one as in sample()).
        Where the fused step does not serve (the shape, CAPNET_NO_FUSED_DECODE_STEP=1) the modes are decoded one
        sample_batch(one_call=True) after the other. poll_every: capnet.decode.beam_decode's."""
        modes = check_styles(modes, self._S)
        return plain_styles(self, lambda l, m: _layer_mods(self, "", m), 1, self.B.weight, self.C, features.size(0), k,
                            start_token, end_token, modes, poll_every,
                            lambda m: self.sample_batch(features, start_token, end_token, k=k, mode=m, one_call=True,
                                                        poll_every=poll_every))

    def sample_styles_nbest(self, features, start_token, end_token, k=5, modes=_MODES, poll_every=0, length_penalty=0.0):
        """sample_styles with nbest=True -> {mode: [n lists of (tokens, score)]}, each equal to sample_batch(mode=mode,
        one_call=True, nbest=True, length_penalty=length_penalty): the one grouped search, its completed lists read by
        capnet_beam_nbest. (A method of its own: sample_styles' parameters are pinned.)"""
        modes = check_styles(modes, self._S)
        return plain_styles(self, lambda l, m: _layer_mods(self, "", m), 1, self.B.weight, self.C, features.size(0), k,
                            start_token, end_token, modes, poll_every,
                            lambda m: self.sample_batch(features, start_token, end_token, k=k, mode=m, one_call=True,
                                                        poll_every=poll_every, nbest=True, length_penalty=length_penalty),
                            nbest=True, length_penalty=length_penalty)
