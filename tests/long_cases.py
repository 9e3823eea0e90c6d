"""Inputs of the long-caption and attention-map-size tests, and the host-side arithmetic that says which branch of
which kernel an input reaches. TEST INFRASTRUCTURE, shared by tests/test_long_inputs_cpu.py (which asserts the claims
on the CPU), tests/test_long_sequences_gpu.py and tests/test_attention_shapes_gpu.py (which run the cases).

The formulas restate the kernels' own: att_datt1's steps per LDS chunk and trip count, att_context_fwd_kernel's four
pixel quarters swept 14 at a time, the 14-pixel sweeps of the backward kernels (csrc/att_kernels.hip), the persistent
LSTM kernel's two metadata registers of 64 steps each (csrc/lstm_persist.hip)."""
import random

import torch

from capnet import synthetic
from helpers import pin_dropout_seed
from oracle import decoders_ref as D
from oracle import dropout_ref as R

MAX_STEPS = 128                       # kMaxSteps, csrc/kernels.h


# ---- att_datt1_kernel: steps per LDS chunk -------------------------------------------------------------------------
def t_chunk(A):
    """att_datt1: (60 KiB) / (4 bytes x (A + 14)) steps of a sample's att2 and de rows fit in LDS at a time."""
    return (60 * 1024) // (4 * (A + 14))


def datt1_trips(steps_alive, A, steps_total):
    """Trips of a workgroup through att_datt1_kernel's chunk loop for a sample alive for `steps_alive` steps."""
    tc = min(t_chunk(A), steps_total)
    return max(1, -(-steps_alive // tc))


# ---- pixel sweeps --------------------------------------------------------------------------------------------------
P_LIST = [1, 2, 3, 4, 5, 13, 14, 15, 16, 49, 55, 56, 57, 64, 196, 197, 256, 441, 784]
SWEEP = 14


def context_quarters(P):
    """att_context_fwd_kernel: [pa, pb) of each of the four waves (pb <= pa: the wave has no pixel)."""
    pq = (P + 3) // 4
    return [(w * pq, min(P, w * pq + pq)) for w in range(4)]


def context_classes(P):
    """Which of the kernel's three paths the quarters of a P-pixel map take."""
    out = set()
    for pa, pb in context_quarters(P):
        n = pb - pa
        if n <= 0:
            out.add("empty quarter")
            continue
        if n >= SWEEP:
            out.add("full 14-sweep")
        if n % SWEEP:
            out.add("clamped tail")
    return out


def tail_pixels(P):
    """The pixels the tail code of the attention kernels handles: P - 1, the last pixel of each wave's quarter, the last
    pixel of each 14-pixel sweep (inside a quarter for the forward context, over all of P for the backward kernels and
    att_datt1's 14-pixel workgroups)."""
    px = {P - 1}
    for pa, pb in context_quarters(P):
        if pb > pa:
            px.add(pb - 1)
            px.update(range(pa + SWEEP - 1, pb, SWEEP))
    px.update(range(SWEEP - 1, P, SWEEP))
    return sorted(px)


def tail_only_features(feats):
    """The same map with every pixel but tail_pixels(P) zeroed."""
    keep = torch.zeros(feats.shape[1], dtype=torch.bool)
    keep[tail_pixels(feats.shape[1])] = True
    return feats * keep.view(1, -1, 1).to(feats.dtype)


# ---- the long cases ------------------------------------------------------------------------------------------------
L128 = [128, 120, 100, 70, 64, 3]                   # exactly kMaxSteps steps
L97 = [97, 80, 66, 65, 30, 9]
LATT6 = [100, 59, 58, 30, 29, 5]                    # at A = 512 (29 steps per chunk): 4, 3, 2, 2, 1, 1 trips
LATT20 = [90, 59, 58, 30, 29, 12, 11, 10, 9, 9, 8, 7, 6, 5, 5, 4, 4, 3, 3, 3]
LSTACK = [80, 66, 65, 40, 12, 3]
L127 = [127, 5]

PLAIN = dict(E=300, H=512, F=512, V=1000)
ATT = dict(A=512, E=300, H=512, F=512, V=1000, P=16, Cf=512)
ATT_SMALL_A = dict(ATT, A=24)
STACK = dict(E=64, H=512, F=64, V=200)
STACK_ATT = dict(A=64, E=48, H=512, F=64, V=200, P=9, Cf=512)
TINY_ATT = dict(A=32, E=24, H=64, F=32, V=97, P=9, Cf=512)

# family -> (logits / alphas tolerance, gradient tolerance): the bounds of the family's short tests
# (test_decoder_gpu.py, test_decoder_att_gpu.py, test_stacked_gpu.py, test_stacked_att_gpu.py, test_nic_stacked_gpu.py)
TOL = {
    "factored": (5e-5, 2e-4), "nic": (5e-5, 2e-4),
    "factored_att": (1e-4, 5e-4), "nic_att": (1e-4, 5e-4),
    "stacked": (2e-5, 2e-4), "nic_stacked": (2e-5, 2e-4),
    "stacked_att": (2e-5, 2e-4), "nic_stacked_att": (2e-5, 2e-4),
}

# name -> family, dims, lengths, teacher forcing, layers, dropout, seed, per_step (persistent kernel off: the control)
CASES = {}


def _add(name, family, dims, lengths, tf, layers=1, p=0.0, seed=1, per_step=False, like=None):
    CASES[name] = dict(family=family, dims=dims, lengths=lengths, tf=tf, layers=layers, p=p, seed=seed,
                       per_step=per_step, like=like)


for fam in ("factored", "nic"):
    _add(fam + "_128_all", fam, PLAIN, L128, "all")
    _add(fam + "_128_none", fam, PLAIN, L128, "none")
    _add(fam + "_128_mixed", fam, PLAIN, L128, "mixed")
    _add(fam + "_128_mixed_per_step", fam, PLAIN, L128, "mixed", per_step=True, like=fam + "_128_mixed")
    _add(fam + "_97_mixed", fam, PLAIN, L97, "mixed", seed=2)
    _add(fam + "_97_dropout", fam, PLAIN, L97, "mixed", p=0.5, seed=3)
for fam in ("factored_att", "nic_att"):
    _add(fam + "_b6", fam, ATT, LATT6, "mixed")
    _add(fam + "_b20", fam, ATT, LATT20, "mixed", seed=2)
    _add(fam + "_b6_small_a", fam, ATT_SMALL_A, LATT6, "mixed", seed=3)
    _add(fam + "_b6_dropout", fam, ATT, LATT6, "mixed", p=0.5, seed=4)
for fam, dims in (("stacked", STACK), ("nic_stacked", STACK), ("stacked_att", STACK_ATT), ("nic_stacked_att", STACK_ATT)):
    _add(fam + "_l2", fam, dims, LSTACK, "mixed", layers=2)
    _add(fam + "_l3_dropout", fam, dims, LSTACK, "mixed", layers=3, p=0.5, seed=2)
for fam in ("stacked_att", "nic_stacked_att"):
    _add(fam + "_127_steps", fam, TINY_ATT, L127, "all", layers=2, seed=5)


# Seeds chosen on the CPU so that every fed-back argmax of the fp64 oracle is clear of a tie by more than the logits
# comparison lets through (tests/test_long_inputs_cpu.py asserts it for every case and every fed-back row).
for _name, _seed in (("factored_97_dropout", 6), ("nic_128_mixed", 6), ("factored_att_b20", 6), ("nic_att_b6_small_a", 5),
                     ("nic_stacked_att_l3_dropout", 7)):
    CASES[_name]["seed"] = _seed


def tf_mask(kind, T, seed):
    """all / none / mixed. Mixed: free-running steps at a rate of 0.2, the first step teacher-forced, and free-running
    steps pinned at 20, 66 and T - 3 where the caption is that long, so that runs of teacher-forced steps (one launch
    of the persistent kernel each) start on both sides of step 64."""
    if kind == "all":
        return [True] * T
    if kind == "none":
        return [False] * T
    rng = random.Random(1000 + seed)
    tf = [rng.random() < 0.8 for _ in range(T)]
    tf[0] = True
    for t in (20, 66, T - 3):
        if 0 < t < T:
            tf[t] = False
            if t + 1 < T:
                tf[t + 1] = True
    return tf


def segment_starts(tf):
    """First steps of the runs of teacher-forced steps that follow a free-running one (restarts of the recurrence)."""
    return [t for t in range(1, len(tf)) if tf[t] and not tf[t - 1]]


def _captions(lengths, V, seed):
    g = torch.Generator().manual_seed(seed)
    B, T = len(lengths), max(lengths)
    c = torch.randint(4, V, (B, T), generator=g)
    c[:, 0] = 1
    for i, l in enumerate(lengths):
        c[i, l - 1] = 2 if l > 1 else 1
        c[i, l:] = 0
    return c


def _decoder(family, d, layers, p):
    if family == "factored":
        from capnet.model import DecoderFactoredLSTM
        return DecoderFactoredLSTM(d["E"], d["H"], d["F"], d["V"], 1, dropout=p)
    if family == "nic":
        from capnet.nic_model import DecoderRNN
        return DecoderRNN(d["E"], d["H"], d["V"], 1, dropout=p)
    if family == "factored_att":
        from capnet.model_att import DecoderFactoredLSTMAtt
        return DecoderFactoredLSTMAtt(d["A"], d["E"], d["H"], d["F"], d["V"], 1, feature_size=d["Cf"], dropout=p)
    if family == "nic_att":
        from capnet.nic_model_att import DecoderRNNAtt
        return DecoderRNNAtt(d["A"], d["E"], d["H"], d["V"], 1, feature_size=d["Cf"], dropout=p)
    if family == "stacked":
        from capnet.stacked import StackedFactoredLSTM
        return StackedFactoredLSTM(d["E"], d["H"], d["F"], d["V"], layers, dropout=p)
    if family == "nic_stacked":
        from capnet.nic_stacked import StackedDecoderRNN
        return StackedDecoderRNN(d["E"], d["H"], d["V"], layers, dropout=p)
    if family == "stacked_att":
        from capnet.stacked_att import StackedFactoredLSTMAtt
        return StackedFactoredLSTMAtt(d["A"], d["E"], d["H"], d["F"], d["V"], layers, feature_size=d["Cf"], dropout=p)
    if family == "nic_stacked_att":
        from capnet.nic_stacked import StackedDecoderRNNAtt
        return StackedDecoderRNNAtt(d["A"], d["E"], d["H"], d["V"], layers, feature_size=d["Cf"], dropout=p)
    raise KeyError(family)


def _forward(family):
    if family == "factored":
        return D.factored_lstm_forward
    if family == "nic":
        return D.lstm_forward
    if family == "factored_att":
        return D.factored_att_forward
    if family == "nic_att":
        return D.lstm_att_forward
    if family == "stacked":
        return D.stacked_factored_lstm_forward
    if family == "stacked_att":
        from stacked_att_ref import stacked_factored_att_forward
        return stacked_factored_att_forward
    from nic_stacked_ref import stacked_lstm_att_forward, stacked_lstm_forward
    return stacked_lstm_forward if family == "nic_stacked" else stacked_lstm_att_forward


class LongCase:
    """One case of CASES built on the CPU: the decoder module (not yet on a device), its parameters, the inputs, the
    oracle's forward and the keyword arguments both sides take."""

    def __init__(self, name):
        c = CASES[name]
        if c["like"]:                        # a control: the very inputs of another case
            c = dict(CASES[c["like"]], per_step=c["per_step"])
        self.name, self.family, self.dims = name, c["family"], c["dims"]
        self.lengths, self.layers, self.p, self.per_step = c["lengths"], c["layers"], c["p"], c["per_step"]
        self.att = self.family.endswith("_att")
        d, seed = self.dims, c["seed"]
        self.dec = _decoder(self.family, d, self.layers, self.p)
        self.params = synthetic.decoder_state(self.dec.state_dict(), seed=40 + seed, bias_range=0.05)
        self.dec.load_state_dict(self.params)
        self.captions = _captions(self.lengths, d["V"], 7 + seed)
        g = torch.Generator().manual_seed(90 + seed)
        B = len(self.lengths)
        if self.att:
            self.feats = torch.randn(B, d["P"], d["Cf"], generator=g).abs() * 0.5
        else:
            self.feats = torch.randn(B, d["E"], generator=g)
        self.tf = tf_mask(c["tf"], max(self.lengths), seed)
        self.forward = _forward(self.family)
        self.kw = {"mode": "happy"} if self.family in ("factored", "factored_att", "stacked", "stacked_att") else {}
        self.num_layers = self.layers if "stacked" in self.family else None
        self.seed_k = 20 + seed
        self.tol_logits, self.tol_grad = TOL[self.family]

    @property
    def steps(self):
        return max(self.lengths)

    def masks(self):
        """The oracle's dropout masks for the seed the decoder's forward draws after helpers.pin_dropout_seed(seed_k)."""
        if self.p == 0.0:
            return {}
        seed = pin_dropout_seed(self.seed_k)
        B, T = self.captions.shape
        m = {"drop_mask": torch.from_numpy(R.embedding_mask(seed, B, T, self.dims["E"], self.p)).double()}
        if self.num_layers:
            N = sum(self.lengths)
            m["layer_masks"] = {l: torch.from_numpy(R.layer_mask(seed, N, self.dims["H"], self.p, l)).double()
                                for l in range(1, self.layers)}
        return m

    def oracle_logits(self, dtype=torch.float64):
        """Packed logits of the oracle in `dtype`, no gradients."""
        okw = dict(self.kw, num_layers=self.num_layers) if self.num_layers else self.kw
        masks = self.masks()
        if "drop_mask" in masks:
            masks["drop_mask"] = masks["drop_mask"].to(dtype)
        if "layer_masks" in masks:
            masks["layer_masks"] = {l: v.to(dtype) for l, v in masks["layer_masks"].items()}
        with torch.no_grad():
            res = self.forward({k: v.to(dtype) for k, v in self.params.items()}, self.captions, self.lengths,
                               self.feats.to(dtype), self.tf, **okw, **masks)
        return res[0] if self.att else res


def fed_back_margin(logits, lengths, tf):
    """(smallest top-1 / top-2 margin over the rows whose argmax is fed back into the next step, number of such rows,
    largest |logit|). Row j of step i is fed back when step i + 1 is free-running and sample j is still alive there."""
    bs = D.batch_sizes(lengths)
    margin, rows, r0 = float("inf"), 0, 0
    for i, b in enumerate(bs):
        if i + 1 < len(bs) and not tf[i + 1]:
            top = logits[r0:r0 + bs[i + 1]].double().topk(2, dim=1)[0]
            margin = min(margin, float((top[:, 0] - top[:, 1]).min()))
            rows += bs[i + 1]
        r0 += b
    return margin, rows, float(logits.abs().max())
