"""The cases of the attention-map tests (tests/test_att_alphas_cpu.py, tests/test_att_alphas_gpu.py). TEST INFRASTRUCTURE.

The whole-search cases of tests/att_beam_cases.py are too gentle for a trace: every winner is the first completion, most
winning paths never leave slot 0 and no image ends with nothing completed, so a trace that ignored parents would pass
most of them. Here the six attention families are reused with <end> tokens that make the beams travel, and one family is
added whose map has P = 260 pixels (the kernel's 256-pixel chunk and a ragged tail of 4). The end tokens were found by
scanning every vocabulary entry of a family with tests/att_alpha_ref.fixed_slot_search in fp64:

  family                          end   what the six (k, image) give in fp64
  StackedFactoredLSTMAtt-2-wide    55   winners of 9 - 10 tokens, paths such as [0,1,1,2,4,4,1,0,0]
  StackedFactoredLSTMAtt-2         22   an 11 - 12 token winner on image 0, nothing completed on images 1 and 2
  StackedDecoderRNNAtt-2            3   6 - 9 token winners with slot changes; (k=5, image 2) has margin 3.1e-5: left out
  DecoderRNNAtt                    10   4 - 6 token winners, up to three steps off slot 0; nothing completed at (3, 0)
  DecoderFactoredLSTMAtt           57   4 - 5 token winners, one or two steps off slot 0
  DecoderRNNAtt-wide                8   6 - 7 token winners that stay in slot 0; nothing completed on four of six
  DecoderRNNAtt-wide                2   never produced: nothing completed anywhere
  DecoderFactoredLSTMAtt-P260      34   9 - 11 token winners, two to four steps off slot 0 (seed 6, mode sad)

A case (family, k, image) is admitted only where the fp64 search's beam_margin exceeds MARGIN, the project's rule.

The stored-logits tables drive capnet_beam_advance_traced / capnet_beam_finish_traced against the Python model without a
decoder: n = 4 images, one per script of tests/test_device_beam_gpu.py's _table (restated here), so that one search holds
"several completions in one step", "nothing completed", "the winner is not the first completion" and "all beams complete
before the last step" -- the last leaves a dead image beside three live ones. V = 11 where k <= 11; capnet_beam_advance
takes k <= V only, so k = 16 runs on V = 17."""
import torch

import att_alpha_ref
from att_beam_cases import IMAGES, KS, MARGIN, MAX_LEN, START, _factored_att, families   # noqa: F401
from device_beam_cases import Family

ALPHA_TOL = 3e-5                          # a step's maps: of max|alpha_ref| of the row (test_att_beam_decode_gpu.py's step TOL)
BOUND = (MAX_LEN + 1) * ALPHA_TOL         # a search's maps: the per-step bound accumulated over the steps replayed

ENDS = (("StackedFactoredLSTMAtt-2-wide", 55), ("StackedFactoredLSTMAtt-2", 22), ("StackedDecoderRNNAtt-2", 3),
        ("DecoderRNNAtt", 10), ("DecoderFactoredLSTMAtt", 57), ("DecoderRNNAtt-wide", 8), ("DecoderRNNAtt-wide", 2))
P260 = "DecoderFactoredLSTMAtt-P260"
CLASSES = ("DecoderFactoredLSTMAtt", "StackedFactoredLSTMAtt", "DecoderRNNAtt", "StackedDecoderRNNAtt")


def with_end(family, end):
    """`family` with another <end> token, named name@end."""
    f = Family("%s@%d" % (family.name, end), family.make, family.params, family.V, family.kw, family.features, family.initial)
    f._end = end
    return f


def _p260():
    from capnet.model_att import DecoderFactoredLSTMAtt
    return _factored_att(P260, DecoderFactoredLSTMAtt, 1, "sad", 6, A=16, E=12, H=64, F=32, V=37, Cf=512, P=260)


_cases = None


def alpha_families():
    global _cases
    if _cases is None:
        by_name = {f.name: f for f in families()}
        _cases = [with_end(by_name[name], end) for name, end in ENDS] + [with_end(_p260(), 34)]
    return _cases


def class_of(family):
    return type(family.make()).__name__


_searches, _margins = {}, {}


def search(family, k, image):
    """att_alpha_ref.fixed_slot_search of a case, computed once."""
    key = (family.name, k, image)
    if key not in _searches:
        _searches[key] = att_alpha_ref.fixed_slot_search(family, k, image, START, MAX_LEN)
    return _searches[key]


def margin(family, k, image):
    key = (family.name, k, image)
    if key not in _margins:
        _margins[key] = family.margin(k, image)
    return _margins[key]


def admitted(family):
    """The (k, image) of a family whose fp64 search has the margin."""
    return [(k, i) for k in KS for i in range(IMAGES) if margin(family, k, i) > MARGIN]


def row_error(got, want):
    """max over the rows of max|got - want| / max|want| of the row (0 for no rows)."""
    if not want.shape[0]:
        return 0.0
    return float(((got - want).abs().max(1).values / want.abs().max(1).values).max())


# ---- stored logits ---------------------------------------------------------------------------------------------------
TABLE_N, TABLE_T, TABLE_END, TABLE_START = 4, 8, 2, 1
TABLE_KV = ((3, 11), (5, 11), (16, 17))
TABLE_SEEDS = {3: 5, 5: 0, 16: 0}        # per k: the smallest seed whose search has what test_att_alphas_cpu.py asserts
SITUATIONS = {"several completions in one step", "nothing completed", "all beams complete before the last step",
              "the winner is not the first completion"}


def table(k, V):
    """Logits [T][n k][V]: normal noise of scale 6 (a row's best word is nearly certain, so a long hypothesis can outscore a
    short one), <end> held far down, then image i follows script i:
      0  step 2: <end> is a fair second on slots 0 and 1 (several completions in one step); steps 6 and 7: <end> is
         certain on slot 1 -- a late completion from a slot other than 0, after five re-slottings, with a better score
      1  nothing (the image completes nothing)
      2  step 1: two words far ahead, <end> third and far behind; step 2: <end> wins on slot 0 -- the later completion has
         the better score (the winner is not the first completion)
      3  step 2: <end> wins on every slot (all beams complete before the last step: a dead image from step 3 on)"""
    n, T, E_ = TABLE_N, TABLE_T, TABLE_END
    g = torch.Generator().manual_seed(TABLE_SEEDS[k] + 100 * k + V)
    x = torch.randn(T, n * k, V, generator=g) * 6.0
    x[:, :, E_] = -60.0
    for r in range(min(k, 2)):
        x[1, r, E_] = x[1, r].max() - 2.0
    for t in (5, 6):
        x[t, 1, E_] = x[t, 1].max() + 8.0
    r0 = 2 * k
    x[0, r0, 3], x[0, r0, 4], x[0, r0, E_] = 42.0, 41.5, 36.0        # (apart: no exact tie anywhere)
    x[1, r0, E_] = 60.0
    x[1, 3 * k:4 * k, E_] = 60.0
    return x


def drive_model(k, V, tab=None):
    """The fixed-slot model with paths over table(k, V), its top-k in fp64 -> (TracedBeam, the smallest gap between two
    neighbours among the candidates taken and the first one left out, over all steps and images)."""
    import torch.nn.functional as Fn
    n, T = TABLE_N, TABLE_T
    tab = table(k, V) if tab is None else tab
    beam = att_alpha_ref.TracedBeam(n, k, V, TABLE_START, TABLE_END)
    gap = [float("inf")]
    for step in range(1, T + 1):
        logp = Fn.log_softmax(tab[step - 1].double(), dim=1)

        def topk(i, nrows, kk, logp=logp):
            prev = torch.tensor(beam.scores[i], dtype=torch.float64)
            flat = (prev[:nrows, None] + logp[i * k:i * k + nrows]).reshape(-1)
            s, ix = flat.topk(min(kk + 1, flat.numel()), 0, True, True)
            if s.numel() > 1:          # the slots follow the rank order: every neighbouring pair counts, not only the cut
                gap[0] = min(gap[0], float((s[:-1] - s[1:]).min()))
            return s[:kk].tolist(), ix[:kk].tolist()
        beam.advance(step, topk)
    return beam, gap[0]
