"""What the decoders' inference paths share: the beam-search front end, the attention beam step and its set-up, the
composed factored cell, and the stepper of a stacked decoder. The decoder classes keep what is theirs: which modules a
mode selects, the layout of their beam state, their weight fold.

  * beam_decode: the one caller of capnet.beam's loops. Every class builds (step_fn, initial state) in one private
    `_beam` method; its sample() asks for one group of k beams, its sample_batch() for n groups. one_call=True: the
    whole search of a plain stack in one C call (ops.beam_decode) on the PlainStack a class attaches to its step_fn
    (plain_stack: the fused step's packed weights, the embedding table and the projection).
    The route is chosen in ONE ladder, whatever the keywords: (1) one_call and a PlainStack of a supported shape:
    ops.beam_decode; (2) one_call and an AttStack: ops.att_beam_decode (_one_call_att); (3) on_device, or one_call with
    neither: capnet.beam.beam_search_device; (4) the host loops beam_search / beam_search_batched. nbest and length_penalty
    go to whichever route runs; _beam_result then shapes what it gave (one image: tensors; maps attached) for all four.
    diversity (an active capnet.beam.Diversity): the same ladder -- the one-call entries' _diverse forms, beam_search_device,
    or beam_search_batched for one image too; the loops merge their groups' lists themselves (capnet.beam.merge_groups),
    the one-call searches' raw lists are merged in _beam_result.
    return_alphas: the attention maps that preceded every word of the captions -- recorded by the one-call search
    (ops.att_beam_decode(return_alphas=True): a history of every step's maps, the winners' rows traced through the
    re-slotting, one gather), in chunks of images that keep the history under ALPHA_TRACE_MAX_BYTES; on every other route
    replay_alphas feeds the returned tokens back through the composed step, whose step_fn keeps its last maps in .alpha.
  * sample_random: captions DRAWN from the decoder's distribution (temperature, top-k, top-p) with their log-probabilities, on the
    same (step_fn, state) pair: one C call on the PlainStack / AttStack (ops.sample_decode / ops.att_sample_decode) or the
    composed loop step_fn -> draw_step, the same stream and so the same tokens. CAPNET_NO_FUSED_SAMPLE=1 (read at every
    call) takes the composed loop.
    greedy=True: the image's greedy caption as one more row of the same decode (csrc/sample_key.h: no noise on that row, the
    drawn rows on the noise rows they have without it) -- the self-critical baseline without a second search;
    sample_random_device also returns the raw ids / logp on the device, for a reward computed there (ops.bleu_rows).
  * pack_samples / policy_logits / score_captions: drawn captions back through the teacher-forced forward, whose step-t
    distribution is the one sample_random drew word t from -- what capnet.train.policy_step differentiates and what every
    image decoder's score_captions reports (the model's log-probability of given captions).
  * attend: Attention.forward, the single step outside a beam search.
  * att_beam_start / att_beam_step: an attention decoder's beam search. The set-up (encoder_att once per image, the
    initial state) is written once for one image and once for n; the step (z = [decoder_att; f_beta](h), the embedding
    into xa, ops.attention_step, then the caller's cell, upper layers and vocabulary projection) once.
  * factored_step: U_g(S_g(V_g(x))) + W_g(h) per gate and the pointwise cell, on torch.cat. DecoderFactoredLSTM's own
    forward_step accumulates into column blocks instead and stays where it is.
  * fold_factored: a factored layer's chain folded into the decode step's [Weff | W] and beff.
  * check_styles / fold_styles / plain_styles / att_styles: sample_styles of the factored decoders -- every requested mode
    folded into its slice of one buffer per layer and ONE grouped search (ops.beam_decode / ops.att_beam_decode with
    groups=len(modes)) over modes x images x k rows; a loop of sample_batch(one_call=True) where that does not serve.
  * stack_stepper / cell_stepper / pack_cell / as_state / input_width: one step of a stack over a [rows, 2L, H] state
    (slot 2l = h of layer l, 2l+1 = its c), on capnet_stacked_decode_step or composed. CAPNET_NO_FUSED_DECODE_STEP=1
    (read here, at every stepper built) takes the composed step, which also serves the shapes the kernel does not take.
"""
import os

import torch

from . import ops
from .beam import MIXED, Constraints, Diversity, PerImage, beam_search, beam_search_batched, beam_search_device, by_completion, merge_groups

FUSED_DECODE_OFF = "CAPNET_NO_FUSED_DECODE_STEP"
_GATE_BLOCKS = (0, 1, 3, 2)     # the kernel's gate blocks i, f, o, c~ from torch's i, f, g, o


# ---- beam search ------------------------------------------------------------------------------------
class PlainStack:
    """What ops.beam_decode needs of a decoder whose beam step is a plain stack on the fused decode step, starting at
    zero: the cell kind, the packed weights [(wcat, beff)] per layer, the embedding table, the projection."""

    def __init__(self, cell, packed, emb, Cw, Cb):
        self.cell, self.emb, self.Cw, self.Cb = cell, emb.detach(), Cw.detach(), None if Cb is None else Cb.detach()
        self.wcat, self.beff = [w for w, _ in packed], [b for _, b in packed]


def plain_stack(step_fn, packed, cell, emb, C):
    """step_fn with the PlainStack of `packed` attached -- a stack_stepper's .packed, None unless it runs the fused step
    (the shape is the kernel's and CAPNET_NO_FUSED_DECODE_STEP is not set): beam_decode(one_call=True) then needs no
    step_fn at all."""
    if packed is not None:
        step_fn.plain = PlainStack(cell, packed, emb, C.weight, C.bias)
    return step_fn


class AttStack:
    """What ops.att_beam_decode needs of an attention decoder: the cell kind, the packed or folded weights [(wcat, beff)]
    per layer (layer 0 reading E + C columns), wz / bz = [decoder_att; f_beta] stacked, full_att, the embedding table,
    the projection, the maps feat [n, P, C] and att1 [n, P, A] = encoder_att(feat) PER IMAGE, and the initial state
    [n k, 2L, H] (init_h / init_c of every layer, each image's row k times)."""

    def __init__(self, cell, packed, wz, bz, full_att, emb, Cw, Cb, feat, att1, state):
        self.cell, self.wz, self.bz, self.full_att = cell, wz, bz, full_att
        self.emb, self.Cw, self.Cb = emb.detach(), Cw.detach(), None if Cb is None else Cb.detach()
        self.wcat, self.beff = [w for w, _ in packed], [b for _, b in packed]
        self.feat, self.att1, self.state = feat, att1, state


def att_stack_supported(dec, E, Cdim, P, k, num_layers):
    """Whether an attention decoder of this shape takes ops.att_beam_decode now (CAPNET_NO_FUSED_DECODE_STEP is read here)."""
    return (os.environ.get(FUSED_DECODE_OFF, "")[:1] != "1" and E % 4 == 0 and k <= dec.vocab_size and
            ops.att_decode_supported(E, Cdim, dec.hidden_size, dec.attention_size, P, k, num_layers))


def att_stack(step_fn, dec, cell, pack, attention, embed, project, maps, k, entries):
    """step_fn (att_beam_step's: it carries the stacked wz / bz) with the AttStack of an attention decoder attached where
    the shape is supported: pack() -> [(wcat, beff)]
    per layer is called only then (the fold or the packing costs launches). maps: att_beam_start's (feat, att1) per image;
    entries: the beam state's tensors of every layer in order, [rows, H] or [rows, m, H] each."""
    feat, att1 = maps
    state = torch.cat([t.unsqueeze(1) if t.dim() == 2 else t for t in entries], 1).contiguous()
    if att_stack_supported(dec, embed.weight.shape[1], feat.shape[2], feat.shape[1], k, state.shape[1] // 2):
        step_fn.att = AttStack(cell, pack(), step_fn.wz, step_fn.bz, attention.full_att, embed.weight, project.weight,
                               project.bias, feat, att1, state)
    return step_fn


ALPHA_TRACE_MAX_BYTES = 256 << 20     # the one-call search's map history (steps x rows x P floats): a cap on memory


def replay_alphas(step_fn, state, seqs, n, k, images=None):
    """The attention maps of decoded captions by replay -> a list of float32 [len - 1, P] tensors, row e - 1 the softmax
    over the pixels that preceded word e: the token lists `seqs` (one list, n None; else n lists) are fed back through
    step_fn (att_beam_step's, which keeps the maps of its last step in .alpha) from the initial beam `state` of the search,
    one row per caption -- the first of each image's k. All captions of a batch advance together; a finished one
    repeats its last token and its maps are no longer kept. A caption [<end>] alone (nothing completed) has [0, P].
    images: the image of every caption of `seqs`, for several captions per image (an n-best list); no caption, no maps."""
    with torch.no_grad():
        dev = state[0].device
        lists = [list(seqs)] if n is None and images is None else [list(q) for q in seqs]
        if not lists:
            return []
        first = torch.arange(len(lists), device=dev) * k
        if images is not None:
            first = torch.tensor(images, dtype=torch.long, device=dev) * k
        state = tuple(t.index_select(0, first).contiguous() for t in state)
        steps = [len(q) - 1 for q in lists]
        maps = [[] for _ in lists]
        for e in range(1, max(steps) + 1):
            words = torch.tensor([q[min(e, len(q)) - 1] for q in lists], dtype=torch.long, device=dev)
            _, state = step_fn(words, state)
            for i, m in enumerate(steps):
                if e <= m:
                    maps[i].append(step_fn.alpha[i])
        P = step_fn.alpha.shape[1]     # (no step here: every caption is [<end>], and the search itself ran step_fn)
        return [torch.stack(m) if m else torch.zeros((0, P), dtype=torch.float32, device=dev) for m in maps]


def _one_call_att(dec, att, n_img, k, start_token, end_token, poll_every, return_alphas, nbest=False, length_penalty=0.0,
                  constraints=None, diversity=None):
    """ops.att_beam_decode on an AttStack; with the maps, the images in as few chunks as keep the history [steps, rows, P]
    under ALPHA_TRACE_MAX_BYTES. nbest: every chunk's n-best lists (and maps per hypothesis), image by image as without it."""
    T, P = dec.max_seq_length + 1, att.feat.shape[1]
    con = {} if constraints is None else {"constraints": constraints}
    if diversity is not None:       # (ops.att_beam_decode then returns a list per (image, group): chunks concatenate as ever)
        con["diversity"] = diversity

    def call(a1, ft, st, i0=0, i1=n_img):
        kw = con
        if isinstance(constraints, PerImage) and (i0, i1) != (0, n_img):     # a chunk of images: its own rows of the rule table
            kw = dict(con, constraints=constraints[i0:i1])
        return ops.att_beam_decode(att.cell, a1, ft, att.emb, att.wz, att.bz, att.full_att.weight, att.full_att.bias, att.wcat,
                                   att.beff, att.Cw, att.Cb, st, k, T, start_token, end_token, poll_every,
                                   return_alphas=return_alphas, nbest=nbest, length_penalty=length_penalty, **kw)
    per = max(1, ALPHA_TRACE_MAX_BYTES // (T * k * P * 4)) if return_alphas else n_img
    if per >= n_img:
        return call(att.att1, att.feat, att.state)
    seqs, maps = [], []
    for i0 in range(0, n_img, per):
        i1 = min(n_img, i0 + per)
        q, m = call(att.att1[i0:i1], att.feat[i0:i1], att.state[i0 * k:i1 * k], i0, i1)
        seqs += q
        maps += m
    return seqs, maps


def _nbest_replay(step_fn, state, lists, k):
    """replay_alphas of every hypothesis of the n-best `lists` (per image, (tokens, score) pairs) -> per image, the list of
    its hypotheses' maps."""
    images = [i for i, hyps in enumerate(lists) for _ in hyps]
    flat = iter(replay_alphas(step_fn, state, [q for hyps in lists for q, _ in hyps], None, k, images))
    return [[next(flat) for _ in hyps] for hyps in lists]


def _one_image(lists, dev):
    """An n-best list of token lists as sample() returns it: LongTensor [1, L] per entry (None stays None)."""
    return [None if p is None else (torch.tensor([p[0]], dtype=torch.long, device=dev), p[1]) for p in lists]


def beam_decode(dec, step_fn, state, n, k, start_token, end_token, on_device=False, poll_every=0, one_call=False,
                return_alphas=False, nbest=False, length_penalty=0.0, constraints=None, diversity=None):
    """Beam search over `step_fn` from `state` (a tuple of tensors: k leading rows, or n k with image i's beams at rows
    i k .. i k + k - 1). n None: one group (capnet.beam.beam_search) -> LongTensor [1, L]; else n groups advancing
    together (beam_search_batched) -> a list of n token lists. on_device: the same results from
    capnet.beam.beam_search_device, whose bookkeeping stays on the device (fixed rows, no host read per step; poll_every
    as there). one_call: the same search as ONE C call (ops.beam_decode: the parent rows read by the step itself, no
    Python per step) where step_fn carries a PlainStack and the shape is one ops.beam_decode_supported, or carries an
    AttStack (ops.att_beam_decode; att_stack attaches it only for a supported shape); everywhere else -- an unsupported
    shape, an embedding width that is no multiple of 4, CAPNET_NO_FUSED_DECODE_STEP=1 -- it is on_device=True.
    return_alphas (attention decoders: step_fn is att_beam_step's): the result is followed by the attention maps, float32
    [len - 1, P] per caption on the decoder's device (n None: one tensor), row e - 1 the map that preceded word e. The
    one-call search records them as it goes; every other route decodes as it does without the keyword and gets them from
    replay_alphas. The tokens are those of the call without the keyword.
    nbest: where a call without it returns one token list (one tensor), it returns the list of (tokens, score) pairs of
    every completed hypothesis, best first by score / (len - 1)^length_penalty (len - 1: the generated words, <end>
    included; score: the summed log-probability, a float), ties to the earlier completion; an empty list where nothing
    completed. Entry 0 at length_penalty 0 is the caption the call without the keyword returns. The search is unchanged:
    the host loops rank the completed lists they hold (capnet.beam.rank_completed), the device routes read theirs with
    capnet_beam_nbest. With return_alphas every hypothesis has its own maps, in the same nesting. length_penalty without
    nbest raises CapnetError.
    constraints (a capnet.beam.Constraints): what no hypothesis may contain -- a repeated n-gram, <end> before
    min_words words, a banned word -- excluded inside every step's selection, after the log-softmax, on whichever route runs:
    the host loops build each live row's list (capnet.beam.banned_words) for capnet_beam_topk[_batched]_banned, the device
    routes derive it from the sequences in the beam state (capnet_beam_advance_constrained; the one-call searches'
    _constrained entries). The scores stay the model's own log-probabilities. None, or a Constraints() that excludes
    nothing: every route runs the code it runs without the keyword, unchecked. CapnetError where constraints that exclude
    something could leave a step fewer than k candidates (Constraints.check).
    Constraints(forced=...): words every completed caption must contain, by dynamic beam allocation inside the
    selection, through the same keyword on the same routes -- capnet_beam_topk_batched_forced under the host loops,
    capnet_beam_advance_forced on_device, capnet_beam_decode_forced / capnet_att_beam_decode_forced one_call (the latter
    records the maps itself, as the constrained one-call search does). Not with an active diversity (CapnetError).
    constraints a capnet.beam.PerImage (n images: sample_batch): an entry per image, each a Constraints or None,
    and image i is searched as it would be alone under entries[i]. PerImage.check runs first (an entry per image, every
    active entry's own check), then PerImage.uniform: entries that all say the same are that one Constraints (or no keyword)
    and run the code that ran before; only a mixed set takes the per-image entries, on the same routes --
    capnet_beam_topk_batched_rules under the host loop, capnet_beam_advance_rules on_device, capnet_beam_decode_rules /
    capnet_att_beam_decode_rules one_call (the map chunks each with their slice of the entries). Not for one image (n None)
    and not with an active diversity (CapnetError).
    diversity (a capnet.beam.Diversity): diverse beam search -- the k beams of an image as D groups of k / D
    that select in order at every step, a later group paying `strength` for every candidate an earlier group chose at that
    step with the same word (<end> counted like any word). The penalty shapes the selection only; the scores stay the
    model's own log-probabilities. This is the one place that checks it (Diversity.check: D divides k; CapnetError). None,
    or a Diversity(1, x): every route runs the code it runs without the keyword, unchecked. Routes: the host loop is
    beam_search_batched with its bookkeeping per (image, group) on capnet_beam_topk_batched_diverse (one image: its n = 1
    case); on_device is beam_search_device on capnet_beam_advance_diverse; one_call is capnet_beam_decode_diverse /
    capnet_att_beam_decode_diverse where the plain route would take its one-call entry, else on_device. Results: without nbest the completed hypothesis with the highest score over all groups
    (ties: the lower group, then the earlier completion; [<end>] where no group completed anything); nbest: all groups'
    completed hypotheses, identical token lists once, ranked by rank_completed; Diversity(per_group=True), which needs
    nbest=True: per image D entries in group order, each the group's best (tokens, score) or None. return_alphas: the maps
    per returned hypothesis in the same nesting (None for None): recorded by the one-call attention search, by replay
    elsewhere."""
    length_penalty = ops.check_length_penalty("beam search", nbest, length_penalty)
    dev, n_img, V, T = state[0].device, 1 if n is None else n, dec.vocab_size, dec.max_seq_length
    nb = dict(nbest=True, length_penalty=length_penalty) if nbest else {}
    if isinstance(constraints, PerImage):       # a rule per image: checked, then one rule for all wherever that is what it says
        if n is None:
            raise ops.CapnetError("constraints: a PerImage belongs to sample_batch (sample decodes one image: hand it a Constraints)")
        if diversity is not None and isinstance(diversity, Diversity) and diversity.active:
            raise ops.CapnetError("constraints: a PerImage does not go with an active diversity (DESIGN 7)")
        constraints.check(V, end_token, k, T, n_img)
        one_rule = constraints.uniform()
        if one_rule is MIXED:
            nb["constraints"] = constraints
        constraints = one_rule                  # (a Constraints or None: the call as with that keyword; MIXED: set above)
    if constraints is not None and constraints is not MIXED:
        if not isinstance(constraints, Constraints):
            raise ops.CapnetError("constraints must be a capnet.beam.Constraints, not %r" % (constraints,))
        if constraints.active:                  # (not active: the calls as they were before there was the keyword, unchecked)
            constraints.check(V, end_token, k, T)
            nb["constraints"] = constraints
    if diversity is not None:
        if not isinstance(diversity, Diversity):
            raise ops.CapnetError("diversity must be a capnet.beam.Diversity, not %r" % (diversity,))
        if diversity.active:                    # (not active: the calls as they were before there was the keyword, unchecked)
            diversity.check(k)
            if ops.has_forced(nb.get("constraints")):
                raise ops.CapnetError("constraints: forced words do not go with an active diversity (DESIGN 7)")
            if diversity.per_group and not nbest:
                raise ops.CapnetError("diversity: per_group=True needs nbest=True (one (tokens, score) per group)")
            nb.update(nbest=nbest, length_penalty=length_penalty, diversity=diversity)
    teams = nb.get("diversity")                 # the active Diversity, or None
    plain = getattr(step_fn, "plain", None) if one_call else None
    att = getattr(step_fn, "att", None) if one_call else None
    maps = one = raw = None
    with torch.no_grad():
        if plain is not None and ops.beam_decode_supported(plain.emb.shape[1], plain.Cw.shape[1], k, V, len(plain.wcat)):
            lists = ops.beam_decode(plain.cell, plain.wcat, plain.beff, plain.emb, plain.Cw, plain.Cb, n_img, k, T + 1, start_token,
                                    end_token, poll_every, **nb)
            raw = teams
        elif att is not None:
            lists = _one_call_att(dec, att, n_img, k, start_token, end_token, poll_every, return_alphas, **nb)
            if return_alphas:
                lists, maps = lists
            raw = teams
        elif on_device or one_call:
            lists = beam_search_device(step_fn, state, n_img, V, start_token, end_token, k, T, dev, poll_every, **nb)
        elif n is not None or teams is not None:        # (one image in teams: the batched loop's n = 1 case)
            lists = beam_search_batched(step_fn, state, n_img, V, start_token, end_token, k, T, dev, **nb)
        elif nbest:
            lists = [[(q[0].tolist(), sc) for q, sc in beam_search(step_fn, state, V, start_token, end_token, k, T, dev, **nb)]]
        else:
            one = beam_search(step_fn, state, V, start_token, end_token, k, T, dev, **nb)     # LongTensor [1, L] as it is returned
            lists = [one[0].tolist()] if return_alphas else None
    return _beam_result(step_fn, state, n, k, lists, maps, one, return_alphas, nbest,
                        None if raw is None else (raw, end_token, length_penalty))


def _beam_result(step_fn, state, n, k, lists, maps, one, return_alphas, nbest, raw=None):
    """What beam_decode returns, from what its route gave. lists: per image its token list, or with nbest its list of
    (tokens, score) pairs, an entry None where a group of a per_group search completed nothing (its maps are None too);
    maps: the one-call search's recording in the same nesting, else None: with return_alphas they come from replay_alphas /
    _nbest_replay; one: the host loop's tensor of one image, returned as it is. n None: the one image's entry, the tokens as
    LongTensor [1, L].
    raw = (diversity, end_token, length_penalty), the one-call diverse searches: lists holds per (image, group) its
    capnet_beam_nbest list at penalty 0 (and maps the recorded maps of every hypothesis) -> capnet.beam.merge_groups per
    image, and the recorded maps of what the merge kept, looked up by tokens: the first group that has them."""
    dev = state[0].device
    if raw is not None:
        diversity, end_token, length_penalty = raw
        D, per, per_maps = diversity.groups, lists, maps
        lists = [merge_groups([by_completion(per[i * D + g]) for g in range(D)], end_token, diversity, nbest, length_penalty)
                 for i in range(len(per) // D)]
        if per_maps is not None:
            def recorded(i, tokens):
                for g in range(D):
                    for (q, _), m in zip(per[i * D + g], per_maps[i * D + g]):
                        if q == tokens:
                            return m
                return torch.zeros((0, step_fn.att.feat.shape[1]), dtype=torch.float32, device=dev)   # [<end>]: nothing completed
            maps = [[None if p is None else recorded(i, p[0]) for p in hyps] if nbest else recorded(i, hyps)
                    for i, hyps in enumerate(lists)]
    if return_alphas and maps is None and nbest:     # the hypotheses that are there, image by image; None keeps its place
        got = [iter(m) for m in _nbest_replay(step_fn, state, [[p for p in hyps if p is not None] for hyps in lists], k)]
        maps = [[None if p is None else next(got[i]) for p in hyps] for i, hyps in enumerate(lists)]
    elif return_alphas and maps is None:
        maps = replay_alphas(step_fn, state, lists, len(lists), k)
    if n is None:
        if one is None:
            one = _one_image(lists[0], dev) if nbest else torch.tensor(lists, dtype=torch.long, device=dev)
        lists, maps = one, None if maps is None else maps[0]
    return (lists, maps) if return_alphas else lists


# ---- sampled decoding -------------------------------------------------------------------------------
FUSED_SAMPLE_OFF = "CAPNET_NO_FUSED_SAMPLE"
# the largest measured row count at which the one-call sampler's median beat the composed loop's by more than the spread (the
# larger of the two ranges) at every layer count and top_k measured (tools/time_sample_decode.py,
# profiles/time_sample_decode.jsonl): capnet.seq2seq at 1, 12 and 64 rows -- it wins at 1 and 12 (1.3x to 2.2x) and
# loses at 64 in three cells of four (one workgroup merges all rows); 13 to 63 rows were not measured. Above it sample_random
# takes the composed loop.
FUSED_SAMPLE_MAX_ROWS = 12
# the same for the attention decoders, where the one call also spares the per-row copies of the maps: 12 images at 60, 72 (5
# samples and the greedy row of sample_random(greedy=True)) and 96 physical rows, top_k 0 and 5 -- it wins 2.0x to 3.3x at all
# three; nothing larger was measured
FUSED_ATT_SAMPLE_MAX_ROWS = 96


# the thresholds of the nucleus draw (top_p < 1), from their own measurement by the same rule (tools/time_nucleus.py,
# profiles/time_nucleus.jsonl; capnet.seq2seq at 1, 12 and 64 rows, top_p 0.9):
#   without top_k the one call NEVER beats the composed loop by more than the spread (5.83 against 5.83 ms at 1 layer x 1 row,
#   6.93 against 6.93 at 3 layers x 12 rows): a step is bound by the selection kernel, about 115 us at V 8192, longer than the
#   host needs to issue it, so the launches the one call saves are hidden either way -- 0: the composed loop at every row count
FUSED_NUCLEUS_MAX_ROWS = 0
#   after top_k the draw is vocab_topk + the pick: the one call wins 1.3x to 1.5x at 1 and 12 rows and loses at 64 rows x 3 layers, as
#   FUSED_SAMPLE_MAX_ROWS found without a nucleus
FUSED_NUCLEUS_TOPK_MAX_ROWS = 12
#   the attention decoders, 12 images x 5 samples: 2.2x (top_k 0) and 2.7x (top_k 5); at 72 and 96 rows 1.9x to 2.2x (the cells
#   of FUSED_ATT_SAMPLE_MAX_ROWS at top_p 0.9); nothing larger was measured
FUSED_ATT_NUCLEUS_MAX_ROWS = 96


def fused_sample(rows, att=False, top_p=1.0, top_k=0):
    """Whether a sampled decode of `rows` rows takes the one-call route now (CAPNET_NO_FUSED_SAMPLE is read here, at every
    call; the shape and CAPNET_NO_FUSED_DECODE_STEP are the caller's to check). top_p < 1: the nucleus draw's thresholds."""
    if top_p < 1.0:
        most = FUSED_ATT_NUCLEUS_MAX_ROWS if att else FUSED_NUCLEUS_TOPK_MAX_ROWS if top_k else FUSED_NUCLEUS_MAX_ROWS
    else:
        most = FUSED_ATT_SAMPLE_MAX_ROWS if att else FUSED_SAMPLE_MAX_ROWS
    return os.environ.get(FUSED_SAMPLE_OFF, "")[:1] != "1" and rows <= most


def draw_step(logits, temperature, top_k, seed, step, top_p=1.0, greedy_stride=0, mask=None):
    """The composed route's draw of stream step `step` from logits [rows, V] -> (tokens [rows] int64, logp [rows]): the
    stream and the arithmetic of the one-call route's (ops.sample_rows; top_k > 0: torch.topk's candidates into
    ops.sample_pick), so both routes return the same tokens wherever the best two keys are further apart than the logits'
    last bits. top_p < 1: the nucleus draw (ops.nucleus_rows; top_k > 0: ops.nucleus_pick on the same candidates); top_p ==
    1.0 calls what it called before there was a top_p. greedy_stride: ops.vocab_sample's (0: the calls as they were).
    mask (ops.sample_exclusion_mask's; None: the calls as they were): ops.mask_logits writes -inf over the excluded words of
    `logits` first, which every draw here treats as not pickable."""
    gs = {"greedy_stride": greedy_stride} if greedy_stride else {}
    if mask is not None:
        logits = ops.mask_logits(logits if logits.stride(1) == 1 else logits.contiguous(), mask)
    tail = (temperature, seed, step) if top_p == 1.0 else (temperature, top_p, seed, step)
    if top_k == 0:
        return (ops.sample_rows if top_p == 1.0 else ops.nucleus_rows)(logits, *tail, **gs)
    values, index = torch.topk(logits, top_k, dim=1)
    pick = ops.sample_pick if top_p == 1.0 else ops.nucleus_pick
    return pick(values.contiguous(), index.int().contiguous(), logits.shape[1], *tail, **gs)


def sample_steps(step, steps, tokens, state, temperature, top_k, seed, draw_kw, exclude=None, V=None, end_token=None):
    """The composed sampled decode: per stream step t, step(t, tokens, state) -> (logits [rows, V], state'), then draw_step
    (draw_kw: its top_p / greedy_stride keywords, where set) -> the next tokens. tokens: the rows' start tokens (None where
    step 0 does not read them; the hypotheses are then the words alone). exclude (an active Constraints, with V and end_token): per step
    ops.sample_exclusion_mask on the rows' words so far -- which the kernel reads from one [rows, steps] block -- in front of the draw.
    Returns (ids [rows, steps] int64, logp [rows, steps] float32, the final state)."""
    ids, logp = [], []
    start, so_far, mask = tokens, None, None
    for t in range(steps):
        logits, state = step(t, tokens, state)
        if exclude is not None:
            if so_far is None:       # (sized by the step's rows: there are no start tokens where step 0 runs on given inputs)
                so_far = torch.empty((logits.shape[0], steps), dtype=torch.int64, device=logits.device)
            mask = ops.sample_exclusion_mask(so_far, start, t, V, end_token, exclude, out=mask)
            tokens, lp = draw_step(logits, temperature, top_k, seed, t, **draw_kw, mask=mask)
            so_far[:, t] = tokens
        else:
            tokens, lp = draw_step(logits, temperature, top_k, seed, t, **draw_kw)
        ids.append(tokens)
        logp.append(lp)
    return torch.stack(ids, 1), torch.stack(logp, 1), state


def cut_samples(ids, logp, n, m, start_token, end_token):
    """ids / logp [n m, steps] of a sampled decode -> n lists of m (tokens, logprob): tokens = [start, w_1 .. w_j] cut after
    the first end_token (none: every step), logprob the sum of the kept words' log-probabilities. One copy to the host."""
    ids, logp = ids.cpu().tolist(), logp.double().cpu().tolist()
    out = []
    for i in range(n):
        rows = []
        for r in range(i * m, (i + 1) * m):
            keep = ids[r].index(end_token) + 1 if end_token in ids[r] else len(ids[r])
            rows.append(([int(start_token)] + ids[r][:keep], float(sum(logp[r][:keep]))))
        out.append(rows)
    return out


def sample_random_device(dec, step_fn, state, n, m, start_token, end_token, temperature=1.0, top_k=0, seed=None, top_p=1.0,
                         greedy=False, exclude=None):
    """`m` captions per image DRAWN from the decoder's distribution softmax(logits / temperature) (top_k > 0: renormalised
    over the top_k best words of every step; top_p < 1: over the nucleus, the smallest set of best words -- of the top_k
    where that is set -- whose probability reaches top_p; logprob is that of the distribution drawn from) -> n lists of m
    (tokens, logprob) pairs; row i m + j of the decode is sample j
    of image i. step_fn / state: a class's _beam(...) with m in place of k and one_call=True, so step_fn carries a
    PlainStack or an AttStack where the fused decode step takes the shape. Routes: ONE C call (ops.sample_decode /
    ops.att_sample_decode) where that rides on step_fn, the rows are at most FUSED_SAMPLE_MAX_ROWS (FUSED_ATT_SAMPLE_MAX_ROWS;
    top_p < 1: FUSED_NUCLEUS_MAX_ROWS, FUSED_NUCLEUS_TOPK_MAX_ROWS, FUSED_ATT_NUCLEUS_MAX_ROWS) and CAPNET_NO_FUSED_SAMPLE is not 1; else step_fn ->
    draw_step per step. Both run dec.max_seq_length steps without looking
    at end_token (finished rows cost wasted steps; the host cuts), draw the same stream and so return the same lists.
    seed: an integer makes the call a pure function; None draws one from torch's CPU generator.
    greedy: every image's m pairs are followed by one more, its GREEDY caption -- argmax_v logit_v at every step (ties to
    the lower index), whatever the temperature, top_k or top_p, cut like the others, its logprob under the same distribution
    as theirs. It is one more ROW of the same decode (physical row i (m + 1) + j is sample j of image i, row i (m + 1) + m
    the greedy one; csrc/sample_key.h: the drawn rows keep noise row i m + j, so the first m pairs are those of the call
    without the keyword): step_fn / state are then the class's _beam(...) for m + 1 rows per image, the row limits of the
    routes apply to the n (m + 1) physical rows, and an attention decoder takes m + 1 <= 16.
    exclude (a capnet.beam.Constraints without forced words): what no row may draw -- at stream step t row r is
    the hypothesis [start, its words so far] at step t + 1 of capnet.beam.banned_words, the tokens as drawn whether or not the
    row has emitted <end>. An excluded word is NOT PICKABLE, exactly as a -inf logit: never drawn, never a top_k candidate,
    never in the nucleus, and logprob is that of the distribution renormalised over the allowed words (the beam searches
    renormalise nothing; hence a keyword of its own). The greedy row is the argmax over the allowed words. The routes are the
    same and draw the same tokens: the one call is ops.sample_decode / ops.att_sample_decode with exclude= (the capnet_*_excl
    entries), the composed loop builds ops.sample_exclusion_mask per step for draw_step. None or an inactive Constraints():
    exactly the calls of the decode without the keyword.
    Returns (the lists, ids int64 [rows, steps], logp float32 [rows, steps]): the decode's raw rows stay on the device beside
    the cut lists, for what scores them there (ops.bleu_rows); sample_random returns the lists alone."""
    who = "sample_random"
    m, steps, V = int(m), int(dec.max_seq_length), dec.vocab_size
    per = m + 1 if greedy else m                     # physical rows per image
    gs = {"greedy_stride": per} if greedy else {}    # not greedy: the calls as they were before there was a greedy row
    temperature, top_k, seed, top_p = ops.check_sampling(who, temperature, top_k, seed, V, top_p)
    kw = {} if top_p == 1.0 else {"top_p": top_p}          # top_p == 1.0: the calls as they were before there was a top_p
    if m < 1 or n < 1 or n * per >= ops.SAMPLE_MAX_ROWS or not 1 <= steps <= ops.SAMPLE_MAX_STEPS:
        raise ops.CapnetError("%s: %d images x %d samples, %d steps" % (who, n, m, steps))
    if greedy and is_attention(dec) and per > 16:
        raise ops.CapnetError("%s: %d samples and the greedy row: an attention decoder takes at most 16 rows per image" % (who, m))
    dev = state[0].device
    if exclude is not None:
        if not isinstance(exclude, Constraints):        # (a PerImage too: a draw takes one rule for all rows)
            raise ops.CapnetError("exclude must be a capnet.beam.Constraints, not %r" % (exclude,))
        exclude.check_exclude(V, end_token, top_k, steps)
        if not exclude.active:
            exclude = None
    ex = {} if exclude is None else {"exclude": exclude, "end_token": int(end_token)}
    with torch.no_grad():
        plain, att = getattr(step_fn, "plain", None), getattr(step_fn, "att", None)
        if fused_sample(n * per, False, top_p, top_k) and plain is not None and ops.sample_decode_supported(plain.emb.shape[1], plain.Cw.shape[1], V, top_k):
            tokens = torch.full((n * per,), int(start_token), dtype=torch.int64, device=dev)
            ids, logp, _ = ops.sample_decode(plain.cell, steps, plain.wcat, plain.beff, plain.emb, plain.Cw, plain.Cb,
                                             temperature, top_k, seed, start_tokens=tokens, **kw, **gs, **ex)
        elif fused_sample(n * per, True, top_p, top_k) and att is not None and (top_k == 0 or ops.vocab_topk_supported(att.Cw.shape[1], top_k, V)):
            ids, logp = ops.att_sample_decode(att.cell, att.att1, att.feat, att.emb, att.wz, att.bz, att.full_att.weight,
                                              att.full_att.bias, att.wcat, att.beff, att.Cw, att.Cb, att.state, per, steps,
                                              start_token, temperature, top_k, seed, **kw, **({"greedy": True} if greedy else {}), **ex)
        else:
            words = torch.full((n * per,), int(start_token), dtype=torch.int64, device=dev)
            ids, logp, _ = sample_steps(lambda t, tokens, st: step_fn(tokens, st), steps, words, state, temperature, top_k, seed,
                                        dict(kw, **gs), exclude, V, end_token)
    ops.check_device_errors()
    return cut_samples(ids, logp, n, per, start_token, end_token), ids, logp


def sample_random(dec, step_fn, state, n, m, start_token, end_token, temperature=1.0, top_k=0, seed=None, top_p=1.0, device=False,
                  greedy=False, exclude=None):
    """The lists of sample_random_device; device=True: all it returns (lists, ids, logp)."""
    ex = {} if exclude is None else {"exclude": exclude}      # None: the call as it was before there was an exclude
    out = sample_random_device(dec, step_fn, state, n, m, start_token, end_token, temperature, top_k, seed, top_p, greedy, **ex)
    return out if device else out[0]


# ---- sampled captions back through the teacher-forced forward -----------------------------------------
def flat_captions(captions):
    """captions as score_captions / capnet.train.policy_step take them -> (token lists, image of each): a flat list of token
    lists, caption r belonging to row r of the features, or the nested list sample_random returns (per image a list of
    samples, each a token list or a (tokens, logprob) pair whose logprob is ignored)."""
    tokens, image = [], []
    for i, c in enumerate(captions):
        if len(c) and isinstance(c[0], (list, tuple)):
            for s in c:
                pair = len(s) == 2 and isinstance(s[0], (list, tuple))
                tokens.append([int(w) for w in (s[0] if pair else s)])
                image.append(i)
        else:
            tokens.append([int(w) for w in c])
            image.append(i)
    return tokens, image


def pack_samples(captions):
    """Token lists [start, w_1 .. w_j], j >= 1 -> (inputs, lengths, targets, order) of their teacher-forced batch: order the
    stable sort by descending j (caption order[r] becomes row r), inputs [B, T] int64 with row r = tokens[:-1] padded with 0,
    lengths the j of every row, targets tokens[1:] in pack_padded_sequence order. Host tensors and lists; no GPU."""
    if not len(captions):
        raise ops.CapnetError("pack_samples: no captions")
    caps = [[int(w) for w in c] for c in captions]
    if min(len(c) for c in caps) < 2:
        raise ops.CapnetError("pack_samples: a caption is [start, w_1 .. w_j] with at least one word")
    order = sorted(range(len(caps)), key=lambda r: -len(caps[r]))      # sorted() is stable
    rows = [caps[r] for r in order]
    lengths = [len(c) - 1 for c in rows]
    inputs = torch.zeros((len(rows), lengths[0]), dtype=torch.int64)
    for r, c in enumerate(rows):
        inputs[r, :len(c) - 1] = torch.tensor(c[:-1], dtype=torch.int64)
    targets = torch.tensor([c[t + 1] for t in range(lengths[0]) for c in rows if len(c) - 1 > t], dtype=torch.int64)
    return inputs, lengths, targets, order


def is_attention(dec):
    """Whether the image is an input of `dec`'s decoding (the four attention decoders)."""
    return hasattr(dec, "attention_size")


def policy_logits(dec, inputs, lengths, features, mode=None):
    """Packed logits [sum(lengths), V] of the teacher-forced pass whose step-t distribution is the one sample_random drew word
    t from: inputs / lengths of pack_samples on the device, every step teacher forced (tf_mask given, so the global `random`
    stream is not consumed). The plain decoders run with features=None -- their decode steps start from the embedding of
    <start> at a zero state and ignore the image, as the reference's sample does; the attention decoders take `features`,
    the maps of every row in the batch's sorted order, and their alphas are dropped. mode: None where the class has none."""
    kw = {} if mode is None else {"mode": mode}
    tf_mask = [True] * inputs.shape[1]
    if is_attention(dec):
        return dec(inputs, lengths, features, teacher_forcing_ratio=1.0, tf_mask=tf_mask, **kw)[0]
    return dec(inputs, lengths, None, teacher_forcing_ratio=1.0, tf_mask=tf_mask, **kw)


def policy_batch(dec, features, captions):
    """What policy_logits and ops.policy_loss need of `captions` (flat or nested, flat_captions), on dec's device:
    (inputs, lengths, targets, order, features of every row in sorted order -- each image's maps once per sample of it; None
    for a plain decoder)."""
    tokens, image = flat_captions(captions)
    inputs, lengths, targets, order = pack_samples(tokens)
    dev = next(dec.parameters()).device
    feats = None
    if is_attention(dec):
        if max(image) >= features.size(0):
            raise ops.CapnetError("%d captions' images for %d rows of features" % (max(image) + 1, features.size(0)))
        feats = features.index_select(0, torch.tensor([image[r] for r in order], dtype=torch.int64, device=features.device))
    return inputs.to(dev), lengths, targets.to(dev), order, feats


def score_captions(dec, features, captions, mode=None):
    """float32 [number of captions] on the device: the model's log-probability of every caption, the sum over w_1 .. w_j
    (<end> too where present), in the caller's order. captions: flat_captions'. Under no_grad; dropout follows
    dec.training, as in forward. One teacher-forced pass (policy_logits) and capnet_policy_xent_fwd."""
    with torch.no_grad():
        inputs, lengths, targets, order, feats = policy_batch(dec, features, captions)
        logits = policy_logits(dec, inputs, lengths, feats, mode)
        zeros = torch.zeros(len(order), dtype=torch.float32, device=logits.device)
        _, logp = ops.policy_loss(logits, targets, zeros, ops.batch_sizes_from_lengths(lengths))
        out = torch.empty_like(logp)
        out[torch.tensor(order, dtype=torch.int64, device=logp.device)] = logp
    return out


def zero_state(rows, H, device):
    """(h, c) [rows, H] of a single-layer decoder whose beams start at zero."""
    zeros = torch.zeros(rows, H, dtype=torch.float32, device=device)
    return zeros, zeros.clone()


# ---- attention --------------------------------------------------------------------------------------
@torch.no_grad()
def attend(attention, encoder_out, decoder_hidden):
    """Attention.forward: one step for s rows on their own maps -> (attention-weighted encoding [s, C], alpha [s, P])."""
    s_rows, P, Cdim = encoder_out.shape
    A = attention.encoder_att.weight.shape[0]
    att1 = attention.encoder_att(encoder_out.reshape(s_rows * P, Cdim)).reshape(s_rows, P, A)
    z = torch.zeros((s_rows, A + Cdim), dtype=torch.float32, device=encoder_out.device)
    z[:, :A] = attention.decoder_att(decoder_hidden)
    return ops.attention_step(att1.contiguous(), encoder_out.contiguous(), z, A, attention.full_att.weight,
                              attention.full_att.bias)


def att_beam_start(dec, attention, features, n, k):
    """The set-up of an attention beam search -> (feat, att1_of, feat_of, h0, c0, img, maps). encoder_att(features) is computed
    once per image (the reference recomputes it for every beam and step); att1_of / feat_of (state, rows) give a step the
    map rows of its live beams.
    n None: `features` is the map of ONE image ([1, S, S, C] or [1, P, C]); feat [k, P, C] holds it k times, so
    re-indexing by beam (model_att.py:413) is a slice; h0, c0 [k, H]; img None.
    Else n images ([n, S, S, C] or [n, P, C]): feat [n, P, C]; a beam's rows are gathered by its image index, the LAST
    entry of the beam state; h0, c0 [n k, H]; img [n k].
    maps: (the feature map [n, P, C], att1 [n, P, A]) per image (n None: one image), what att_stack takes."""
    dev = attention.encoder_att.weight.device
    A, Cdim = dec.attention_size, features.size(-1)
    if n is None:
        feat1 = features.reshape(1, -1, Cdim).to(dev).contiguous()
        P = feat1.size(1)
        feat = feat1.expand(k, P, Cdim).contiguous()
        att1_1 = attention.encoder_att(feat1[0]).reshape(1, P, A)
        att1 = att1_1.expand(k, P, A).contiguous()
        h0, c0 = dec.init_hidden_state(feat)
        return feat, lambda st, r: att1[:r], lambda st, r: feat[:r], h0, c0, None, (feat1, att1_1)
    feat = features.reshape(n, -1, Cdim).to(dev).contiguous()
    P = feat.size(1)
    att1 = attention.encoder_att(feat.reshape(n * P, Cdim)).reshape(n, P, A).contiguous()
    h0, c0 = dec.init_hidden_state(feat)
    img = torch.arange(n, device=dev).repeat_interleave(k)
    h0, c0 = h0.index_select(0, img).contiguous(), c0.index_select(0, img).contiguous()
    return (feat, lambda st, r: att1.index_select(0, st[-1]), lambda st, r: feat.index_select(0, st[-1]), h0, c0, img,
            (feat, att1))


def att_beam_step(attention, f_beta, embed, cell, project, att1_of, feat_of, n_att, upper=None):
    """step_fn of an attention beam search over the state (h, c, *rest) of layer 0 and whatever follows it.
    cell(xa, (h, c)) -> (h, c) is layer 0 on xa = [embedding | gated context]; project(top h) -> logits.
    upper() -> step(h, rest) -> (top h, the layers' new entries): the layers above, whose entries lead `rest`; what
    follows them (the image index) is carried over. It is called here, after [decoder_att ; f_beta] is stacked, so a
    stepper that packs weights launches where it always did."""
    E, A, dev = embed.weight.shape[1], attention.decoder_att.weight.shape[0], embed.weight.device
    # [decoder_att ; f_beta] stacked: one product with h per step
    wz = torch.cat([attention.decoder_att.weight, f_beta.weight], 0).contiguous()
    bz = torch.cat([attention.decoder_att.bias, f_beta.bias], 0).contiguous()
    upper_step = upper() if upper is not None else (lambda h, rest: (h, ()))

    def step_fn(prev_words, state):
        h, c, rest = state[0], state[1], tuple(state[2:])
        s_rows = h.shape[0]
        z = ops.linear(h, wz, bz).contiguous()
        if E % 4 == 0:
            xa = torch.empty((s_rows, E + n_att), dtype=torch.float32, device=dev)
            xa[:, :E] = embed(prev_words)
            _, step_fn.alpha = ops.attention_step(att1_of(state, s_rows), feat_of(state, s_rows), z, A, attention.full_att.weight,
                                                  attention.full_att.bias, xa=xa, xa_col=E)
        else:       # the context kernel stores 16-B vectors: behind an embedding width off 4 the context is joined on
            ctx = torch.empty((s_rows, n_att), dtype=torch.float32, device=dev)
            _, step_fn.alpha = ops.attention_step(att1_of(state, s_rows), feat_of(state, s_rows), z, A, attention.full_att.weight,
                                                  attention.full_att.bias, xa=ctx)
            xa = torch.cat([embed(prev_words).reshape(s_rows, E), ctx], 1)
        h, c = cell(xa, (h, c))
        top, new = upper_step(h, rest)
        return project(top), (h, c) + tuple(new) + rest[len(new):]
    step_fn.wz, step_fn.bz, step_fn.alpha = wz, bz, None      # .alpha: the maps [rows, P] of the step taken last
    return step_fn


# ---- cells ------------------------------------------------------------------------------------------
def factored_step(V, S, U, W, x, h, c):
    """One factored-LSTM step at inference -> (h, c): V, S, U, W are the four gates' Linears (i, f, o, c~)."""
    pre = torch.cat([U[k](S[k](V[k](x))) + W[k](h) for k in range(4)], 1)
    return ops.lstm_pointwise(pre, c, ops.CELL_FACTORED)


def input_width(n_in):
    """A layer's input width as capnet_stacked_decode_step reads it: rounded up to 16."""
    return (n_in + 15) // 16 * 16


def pack_cell(cell, kin):
    """(wcat [4H, kin + H] = [weight_ih, zero columns up to kin | weight_hh], beff [4H] = bias_ih + bias_hh), gate
    blocks reordered for capnet_stacked_decode_step_cell."""
    H, n_in = cell.hidden_size, cell.input_size
    dev = cell.weight_ih.device
    wcat = torch.zeros((4 * H, kin + H), dtype=torch.float32, device=dev)
    beff = torch.empty(4 * H, dtype=torch.float32, device=dev)
    with torch.no_grad():
        for dst, src in enumerate(_GATE_BLOCKS):
            rows, srows = slice(dst * H, (dst + 1) * H), slice(src * H, (src + 1) * H)
            wcat[rows, :n_in].copy_(cell.weight_ih[srows])
            wcat[rows, kin:].copy_(cell.weight_hh[srows])
            torch.add(cell.bias_ih[srows], cell.bias_hh[srows], out=beff[rows])
    return wcat, beff


def fold_factored(V, S, U, W, out=None):
    """(wcat, beff) of one factored layer for capnet_stacked_decode_step from its gates' Linears (i, f, o, c~): wcat
    [4H, kin + H] = [U_g S_g V_g, zero columns up to kin | W_g] (kin: the layer's input width rounded up to 16), beff
    [4H] = U_g (S_g bV_g + bS_g) + bU_g + bW_g. Products on the GPU (capnet_sgemm). out: (wcat, beff) to fold into --
    one weight group's slices of fold_styles' buffers, wcat zero where the fold writes nothing."""
    H, n_in, dev = W[0].weight.shape[0], V[0].weight.shape[1], W[0].weight.device
    kin = input_width(n_in)
    if out is not None:
        wcat, beff = out
    else:
        wcat = torch.zeros((4 * H, kin + H), dtype=torch.float32, device=dev)
        beff = torch.empty(4 * H, dtype=torch.float32, device=dev)
    with torch.no_grad():
        for g in range(4):
            blk, bb = wcat[g * H:(g + 1) * H], beff[g * H:(g + 1) * H]
            ops.sgemm(U[g].weight, ops.sgemm(S[g].weight, V[g].weight), out=blk[:, :n_in])       # [H, F][F, F][F, in]
            blk[:, kin:].copy_(W[g].weight)
            sb = ops.sgemm(V[g].bias.view(1, -1), S[g].weight, transB=True, bias=S[g].bias)       # S bV + bS
            ops.sgemm(sb, U[g].weight, transB=True, bias=U[g].bias, out=bb.view(1, H))
            bb += W[g].bias
    return wcat, beff


# ---- every style at once ----------------------------------------------------------------------------
def check_styles(modes, check_mode):
    """`modes` of a sample_styles call as a tuple: a non-empty sequence of distinct mode names. check_mode(name) is the
    class's own check: an unknown name behaves as in its sample()."""
    if isinstance(modes, str):
        modes = (modes,)
    modes = tuple(modes)
    for m in modes:
        check_mode(m)
    if not modes or len(set(modes)) != len(modes):
        raise ValueError("modes must be a non-empty sequence of distinct mode names, not %r" % (modes,))
    return modes


def fold_styles(layer_mods, num_layers, modes):
    """[(wcat [G, 4H, kin_l + H], beff [G, 4H])] per layer for the grouped decode step: fold_factored of layer_mods(l,
    mode) -> (V, S, U, W) for every requested mode, each into its slice of ONE buffer per layer."""
    packed = []
    with torch.no_grad():
        for l in range(num_layers):
            mods = [layer_mods(l, m) for m in modes]
            V, _, _, W = mods[0]
            H, kin, dev = W[0].weight.shape[0], input_width(V[0].weight.shape[1]), W[0].weight.device
            wcat = torch.zeros((len(modes), 4 * H, kin + H), dtype=torch.float32, device=dev)
            beff = torch.empty((len(modes), 4 * H), dtype=torch.float32, device=dev)
            for g, md in enumerate(mods):
                fold_factored(*md, out=(wcat[g], beff[g]))
            packed.append((wcat, beff))
    return packed


def styles_images(n, G, k, width, device):
    """How many of n images one grouped search takes: its G n k rows of `width` floats (the logits, the attention z) must
    fit the split-K slab the single-mode searches use too. 0: take the loop. (No row count above which the loop wins
    was found: at 1280 rows the grouped search still takes 0.63 - 0.71 of the loop's time)"""
    return min(n, ops.splitk_slab(device).numel() // (G * k * width))


def plain_styles(dec, layer_mods, num_layers, emb, C, n, k, start_token, end_token, modes, poll_every, loop, nbest=False,
                 length_penalty=0.0):
    """sample_styles of a plain factored decoder -> {mode: [n token lists]}: every mode's chain folded into one buffer per
    layer (fold_styles) and ONE ops.beam_decode(groups=len(modes)) over modes x images x k rows (the images in as few
    chunks as the slab allows). loop(mode) -> sample_batch(mode=mode, one_call=True): taken mode by mode where the fused
    step does not serve the shape, CAPNET_NO_FUSED_DECODE_STEP=1 is set, or one mode is asked for. nbest / length_penalty:
    beam_decode's, per mode and image (loop(mode) passes them on itself)."""
    G, V, E = len(modes), dec.vocab_size, emb.shape[1]
    length_penalty = ops.check_length_penalty("sample_styles", nbest, length_penalty)
    with torch.no_grad():
        per = styles_images(n, G, k, V, emb.device) if G > 1 else 0
        if per < 1 or not fused_decode_step(num_layers, E, dec.hidden_size) or \
                not ops.beam_decode_supported(E, dec.hidden_size, k, V, num_layers):
            return {m: loop(m) for m in modes}
        packed = fold_styles(layer_mods, num_layers, modes)
        wcat, beff = [w for w, _ in packed], [b for _, b in packed]
        out = {m: [] for m in modes}
        for i0 in range(0, n, per):
            ni = min(per, n - i0)
            seqs = ops.beam_decode(ops.CELL_FACTORED, wcat, beff, emb.detach(), C.weight, C.bias, ni, k, dec.max_seq_length + 1,
                                   start_token, end_token, poll_every, groups=G, nbest=nbest, length_penalty=length_penalty)
            for g, m in enumerate(modes):
                out[m] += seqs[g * ni:(g + 1) * ni]
    return out


def att_styles(dec, layer_mods, num_layers, features, k, start_token, end_token, modes, poll_every, loop, return_alphas=False,
               nbest=False, length_penalty=0.0):
    """sample_styles of an attention decoder -> {mode: [n token lists]}: ONE ops.att_beam_decode(groups=len(modes)) over
    modes x images x k rows. Per mode: its folded chain (fold_styles), its Attention module's encoder_att(feat) (att1
    [G n, P, A]), [decoder_att; f_beta] and full_att; shared: the map feat [n, P, C], the embedding, the projection and
    the initial state (init_h / init_c of every layer), repeated per mode. loop(mode) as plain_styles'.
    return_alphas: -> ({mode: lists}, {mode: [n float32 [len - 1, P] tensors]}), the maps of every mode's own Attention
    module recorded by the grouped search (loop(mode) then returns (lists, tensors)); the images in chunks that also keep
    the map history under ALPHA_TRACE_MAX_BYTES. nbest / length_penalty: beam_decode's, per mode and image, the maps per
    hypothesis (loop(mode) passes them on itself)."""
    length_penalty = ops.check_length_penalty("sample_styles", nbest, length_penalty)
    G, n, Cdim = len(modes), features.size(0), features.size(-1)
    E, A, V = dec.B.weight.shape[1], dec.attention_size, dec.vocab_size
    with torch.no_grad():
        dev = dec.B.weight.device
        feat = features.reshape(n, -1, Cdim).to(dev).contiguous()
        P = feat.size(1)
        per = styles_images(n, G, k, max(V, A + Cdim), dev) if G > 1 else 0
        if per < 1 or not att_stack_supported(dec, E, Cdim, P, k, num_layers):
            res = {m: loop(m) for m in modes}
            return ({m: r[0] for m, r in res.items()}, {m: r[1] for m, r in res.items()}) if return_alphas else res
        if return_alphas:
            per = max(1, min(per, ALPHA_TRACE_MAX_BYTES // ((dec.max_seq_length + 1) * G * k * P * 4)))
        atts = [dec._mode_modules(m)[0] for m in modes]
        packed = fold_styles(layer_mods, num_layers, modes)
        wcat, beff = [w for w, _ in packed], [b for _, b in packed]
        # [decoder_att ; f_beta] per mode (f_beta is shared: replicated), full_att per mode
        wz = torch.stack([torch.cat([a.decoder_att.weight, dec.f_beta.weight], 0) for a in atts]).contiguous()
        bz = torch.stack([torch.cat([a.decoder_att.bias, dec.f_beta.bias], 0) for a in atts]).contiguous()
        wf = torch.stack([a.full_att.weight.reshape(-1) for a in atts]).contiguous()
        bf = torch.cat([a.full_att.bias.reshape(-1) for a in atts]).contiguous()
        out, maps = {m: [] for m in modes}, {m: [] for m in modes}
        for i0 in range(0, n, per):
            fi = feat[i0:i0 + per]
            ni = fi.size(0)
            att1 = torch.cat([a.encoder_att(fi.reshape(ni * P, Cdim)).reshape(ni, P, A) for a in atts], 0).contiguous()
            img = torch.arange(ni, device=dev).repeat_interleave(k)
            h0, c0 = dec.init_hidden_state(fi)
            upper, _ = dec._upper_beam(fi, img, modes[0])          # init_h{l} / init_c{l}: the same for every mode
            entries = (h0.index_select(0, img), c0.index_select(0, img)) + tuple(upper)
            state = torch.cat([t.unsqueeze(1) for t in entries], 1).repeat(G, 1, 1).contiguous()
            seqs = ops.att_beam_decode(ops.CELL_FACTORED, att1, fi, dec.B.weight, wz, bz, wf, bf, wcat, beff, dec.C.weight,
                                       dec.C.bias, state, k, dec.max_seq_length + 1, start_token, end_token, poll_every, groups=G,
                                       return_alphas=return_alphas, nbest=nbest, length_penalty=length_penalty)
            if return_alphas:
                seqs, alphas = seqs
            for g, m in enumerate(modes):
                out[m] += seqs[g * ni:(g + 1) * ni]
                if return_alphas:
                    maps[m] += alphas[g * ni:(g + 1) * ni]
    return (out, maps) if return_alphas else out


def pack_cells(cells, E):
    """[pack_cell] of every layer of a stack of LSTMCells whose first reads E columns."""
    return [pack_cell(c, input_width(E) if l == 0 else c.hidden_size) for l, c in enumerate(cells)]


# ---- stacks -----------------------------------------------------------------------------------------
def as_state(states):
    """A [rows, 2L, H] state from a tensor of that shape or a sequence of L (h, c) pairs."""
    if isinstance(states, torch.Tensor):
        return states
    return torch.stack([t for hc in states for t in hc], 1)


def fused_decode_step(num_layers, E, H):
    """Whether a stack of this shape runs on capnet_stacked_decode_step now (CAPNET_NO_FUSED_DECODE_STEP is read here)."""
    return os.environ.get(FUSED_DECODE_OFF, "")[:1] != "1" and num_layers <= 8 and ops.stacked_decode_supported(E, H)


def stack_stepper(num_layers, E, H, cell, pack, composed):
    """step(x, tokens, state [rows, 2L, H]) -> (top h [rows, H], state') of a stack of `num_layers` cells of kind `cell`,
    the first reading E columns: x is the embedding table when `tokens` is given, else layer 0's inputs. The fused step
    on pack() -> [(wcat, beff)] per layer, called here, once, unless CAPNET_NO_FUSED_DECODE_STEP=1 or the shape is one the
    kernel does not take: then composed(x, state) -> (top h, state'). step.packed: pack()'s result on the fused step,
    else None."""
    if fused_decode_step(num_layers, E, H):
        packed = pack()
        wcat, beff = [w for w, _ in packed], [b for _, b in packed]

        def step(x, tokens, state):
            return ops.stacked_decode_step(state, wcat, beff, x, tokens, cell=cell)
        step.packed = packed
    else:
        def step(x, tokens, state):
            if tokens is not None:
                x = ops.embedding(tokens, x)
            return composed(x, state)
        step.packed = None
    return step


def cell_stepper(cells, E, H):
    """stack_stepper over `cells` (L LSTMCells, the first reading E columns)."""
    def composed(x, state):
        new = torch.empty_like(state)
        for l, c in enumerate(cells):
            h, cc = c(x, (state[:, 2 * l].contiguous(), state[:, 2 * l + 1].contiguous()))
            new[:, 2 * l], new[:, 2 * l + 1] = h, cc
            x = h
        return x, new
    return stack_stepper(len(cells), E, H, ops.CELL_LSTM, lambda: pack_cells(cells, E), composed)
