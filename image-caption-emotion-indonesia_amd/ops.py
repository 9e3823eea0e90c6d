"""Host-side operators over the C ABI: plain wrappers and torch.autograd.Functions.

PyTorch is plumbing here (device memory, streams, autograd bookkeeping). Every arithmetic
step of the hot path is a HIP kernel in libcapnet_hip.so reached through ctypes; nothing in
this file computes on the CPU or through a torch operator. Inputs must be CUDA fp32 tensors.
"""
import ctypes as C

import struct
import sys
import weakref

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import CapnetError, check, current_stream, int_array, ptr, ptr_array

CELL_FACTORED = 0
CELL_LSTM = 1

_err_flags = {}


def _need_cuda(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise CapnetError("capnet operators run on the GPU only (got a %s tensor); there is "
                              "no CPU fallback" % t.device)
        if t.dtype not in (torch.float32, torch.int64, torch.int32):
            raise CapnetError("unsupported dtype %s" % t.dtype)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def err_flag(device):
    """Per-device int32 flag set by kernels on out-of-range token ids / targets."""
    key = torch.device(device).index or 0
    f = _err_flags.get(key)
    if f is None:
        f = torch.zeros(1, dtype=torch.int32, device=device)
        _err_flags[key] = f
    return f


_ERR_BITS = {1: "token id out of range", 2: "target out of range",
             8: "a non-finite value in the ResNet-152 trunk (an activation beyond the range its layer's power-of-two prescale "
                "allows for the split-f16 operands -- possible only in inference, with running statistics far from the data "
                "-- or a genuine fp32 overflow)",
             4: "a bounded wait of the persistent LSTM kernel expired (its 256 workgroups were not co-resident in time); "
                "the process now runs one launch per LSTM step, as CAPNET_NO_PERSISTENT_LSTM=1 does from the start",
             32: "a recurrent LSTM weight beyond |w| < 64, the range the persistent LSTM kernel's f16 weight image covers (the "
                 "step's results are not finite); CAPNET_NO_PERSISTENT_LSTM=1 runs one launch per step on f32 operands",
             16: "another rank of the data-parallel job raised its error word: this rank dropped the same steps so that "
                 "the replicas stay identical (capnet.parallel)"}

_optimizers = weakref.WeakSet()      # capnet.optim.Adam instances: they hold the per-optimizer dropped-step counters


def register_optimizer(opt):
    _optimizers.add(opt)


def skip_counter(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def count_skipped(counter):
    """counter += 1 on the device while the error word is set (one launch per optimizer step)."""
    check(_lib.lib().capnet_count_skipped(ptr(err_flag(counter.device)), ptr(counter), current_stream()),
          "capnet_count_skipped")


def err_word_exchange(slot, direction):
    check(_lib.lib().capnet_err_word_exchange(ptr(err_flag(slot.device)), ptr(slot), int(direction), current_stream()),
          "capnet_err_word_exchange")


def check_device_errors(recover_lstm_timeout=False):
    """Synchronising check of the device-side error flags (call where the loop already syncs).

    While a flag is set capnet.optim.Adam's update kernel leaves parameters and moments alone (capnet_clamp_adam's
    skip_flag), so the steps between the fault and this check were DROPPED, not applied with garbage gradients; every
    registered optimizer takes the dropped steps out of its host-side step counts here (bias correction stays in step
    with the moments on the device), whether or not the error is then raised.
    recover_lstm_timeout: an expired wait of the persistent LSTM kernel ALONE (bit 4: a transient loss of co-residency
    beside the trunk passes) is logged instead of raised -- the process continues on the launch-per-step kernel, as the
    training loops do (capnet.train.train_factual / train_emotion)."""
    for f in _err_flags.values():
        v = int(f.item())
        if not v:
            continue
        f.zero_()
        dropped = [o.forget_dropped_steps() for o in list(_optimizers)]
        if v & 4:
            _lib.lib().capnet_lstm_persist_set_mode(1)
        msg = ("device-side error flag %d: %s. %s optimizer steps since the previous check were skipped."
               % (v, "; ".join(m for b, m in _ERR_BITS.items() if v & b) or "?", sum(dropped) if dropped else "The"))
        if recover_lstm_timeout and v == 4:
            sys.stderr.write("[capnet] " + msg + " Continuing.\n")
            continue
        raise CapnetError(msg)
    for o in list(_optimizers):
        o.forget_dropped_steps(none_dropped=True)


# ---------------------------------------------------------------------------------------
# plain wrappers
# ---------------------------------------------------------------------------------------
def sgemm(A, B, transA=False, transB=False, bias=None, out=None, accumulate=False, force_tile=0):
    """out[M,N] (+)= op(A) @ op(B) + bias, 2-D contiguous operands."""
    _need_cuda(A, B, bias, out)
    A, B = _c(A), _c(B)
    M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
    if transB:
        N, Kb = B.shape
    else:
        Kb, N = B.shape
    if K != Kb:
        raise CapnetError("sgemm: inner dimensions differ (%d vs %d)" % (K, Kb))
    if out is None:
        if accumulate:
            raise CapnetError("sgemm: accumulate needs an output tensor")
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    # `out` may be a column block of a wider row-major matrix (unit column stride)
    if out.dim() != 2 or tuple(out.shape) != (M, N) or out.stride(1) != 1 or out.stride(0) < N:
        raise CapnetError("sgemm: bad output tensor")
    check(_lib.lib().capnet_sgemm(int(transA), int(transB), M, N, K, ptr(A), A.shape[1], ptr(B),
                                  B.shape[1], ptr(out), out.stride(0), ptr(bias), int(accumulate), 1, 0, 0, 0,
                                  0, force_tile, current_stream()), "capnet_sgemm")
    return out


_splitk_ws = {}


def splitk_slab(device):
    """The cached 32 MB slab workspace of sgemm_splitk on `device`."""
    key = torch.device(device).index or 0
    ws = _splitk_ws.get(key)
    if ws is None:
        ws = torch.empty(8 * 1024 * 1024, dtype=torch.float32, device=device)
        _splitk_ws[key] = ws
    return ws


def sgemm_splitk(A, B, transB=False, bias=None):
    """A @ op(B) + bias through capnet_sgemm_splitk: the library cuts K into slabs when the output
    has few tiles (per-step products; dH = dlogits @ C with K = vocab). One cached 32 MB slab
    workspace per device."""
    _need_cuda(A, B, bias)
    A, B = _c(A), _c(B)
    M, K = A.shape
    N = B.shape[0] if transB else B.shape[1]
    if (B.shape[1] if transB else B.shape[0]) != K:
        raise CapnetError("sgemm_splitk: inner dimensions differ")
    ws = splitk_slab(A.device)
    out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    check(_lib.lib().capnet_sgemm_splitk(0, int(transB), M, N, K, ptr(A), A.shape[1], ptr(B), B.shape[1],
                                         ptr(out), N, ptr(bias), 0, ptr(ws), ws.numel(),
                                         current_stream()), "capnet_sgemm_splitk")
    return out


def colsum(x, out=None):
    _need_cuda(x)
    x = _c(x)
    if out is None:
        out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    check(_lib.lib().capnet_colsum(ptr(x), x.shape[1], x.shape[0], x.shape[1], ptr(out), 0,
                                   current_stream()), "capnet_colsum")
    return out


def argmax_rows(x):
    _need_cuda(x)
    x = _c(x)
    out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    check(_lib.lib().capnet_argmax_rows(ptr(x), x.shape[0], x.shape[1], x.shape[1], ptr(out),
                                        current_stream()), "capnet_argmax_rows")
    return out


def _check_bans(who, bans, rows):
    """bans of beam_topk / beam_topk_batched: contiguous int32 [at least `rows`, 1 + cap] on the device -> cap."""
    _need_cuda(bans)
    if bans.dtype != torch.int32 or bans.dim() != 2 or bans.shape[0] < rows or bans.shape[1] < 2 or not bans.is_contiguous():
        raise CapnetError("%s: bans must be a contiguous int32 [rows, 1 + cap] tensor with a row per logits row" % who)
    return bans.shape[1] - 1


def beam_topk(logits, prev_scores, rows, k, bans=None):
    """k best of prev_scores[r] + log_softmax(logits[r]) over the first `rows` rows, flattened.
    Returns (scores [k] float32, flat_index [k] int64) on the device.
    bans (capnet_beam_topk_banned): int32 [rows, 1 + cap], per row its count and that many words that may not be selected;
    they are removed after the rows' log-sum-exp, by -inf written into `logits` (a float32 tensor: it is modified)."""
    _need_cuda(logits)
    logits = _c(logits)
    prev_scores = _c(prev_scores)
    scores = torch.empty(k, dtype=torch.float32, device=logits.device)
    index = torch.empty(k, dtype=torch.int64, device=logits.device)
    if bans is not None:
        cap = _check_bans("beam_topk", bans, rows)
        check(_lib.lib().capnet_beam_topk_banned(ptr(logits), logits.shape[1], rows, logits.shape[1], ptr(prev_scores), k,
                                                 ptr(bans), cap, ptr(scores), ptr(index), current_stream()),
              "capnet_beam_topk_banned")
        return scores, index
    check(_lib.lib().capnet_beam_topk(ptr(logits), logits.shape[1], rows, logits.shape[1],
                                      ptr(prev_scores), k, ptr(scores), ptr(index),
                                      current_stream()), "capnet_beam_topk")
    return scores, index


def beam_topk_batched(logits, prev_scores, meta, bans=None, diversity=None, forced=None):
    """capnet_beam_topk_batched: meta int32 [n, 3] on the device = (first row, competing rows, k) per image.
    Returns (scores [n, 16] float32, flat_index [n, 16] int64) on the device; only the first k entries of a row are set.
    diversity (a capnet.beam.Diversity; capnet_beam_topk_batched_diverse): meta has a row per (image, team), image i's
    teams at rows i D .. i D + D - 1, and one workgroup per image selects for its teams in order under the Hamming penalty
    (include/capnet.h); bans as below or None. `logits` is modified.
    forced = (constraints, met, end_token) (capnet_beam_topk_batched_forced): a capnet.beam.Constraints with forced words,
    met int32 [rows] on the device -- per logits row the mask of the forced ids its hypothesis holds -- and <end>, which the
    kernel excludes on a row whose mask is not full; bans as below or None. The selection is the forced-word allocation
    (include/capnet.h); `logits` is modified. constraints a capnet.beam.PerImage of n entries
    (capnet_beam_topk_batched_rules): every image's forced ids are read from its row of the rule table; met and bans hold
    what each row's own image's entry gives."""
    _need_cuda(logits, prev_scores, meta)
    logits, prev_scores = _c(logits), _c(prev_scores)
    if meta.dtype != torch.int32 or meta.dim() != 2 or meta.shape[1] != 3 or not meta.is_contiguous():
        raise CapnetError("beam_topk_batched: meta must be a contiguous int32 [n, 3] tensor")
    if forced is not None and diversity is not None:
        raise CapnetError("beam_topk_batched: forced words do not go with diversity")
    if (forced is not None or diversity is not None) and (logits.dtype != torch.float32 or prev_scores.dtype != torch.float32):
        raise CapnetError("beam_topk_batched: logits and prev_scores must be float32")
    cap = 0 if bans is None else _check_bans("beam_topk_batched", bans, logits.shape[0])   # a row for every row of the logits
    n = meta.shape[0]
    scores = torch.empty((n, 16), dtype=torch.float32, device=logits.device)
    index = torch.empty((n, 16), dtype=torch.int64, device=logits.device)
    block = (ptr(logits), logits.shape[1], logits.shape[1], ptr(prev_scores), ptr(meta))
    if forced is not None:
        constraints, met, end_token = forced
        _need_cuda(met)
        if met.dtype != torch.int32 or met.dim() != 1 or met.numel() < logits.shape[0] or not met.is_contiguous():
            raise CapnetError("beam_topk_batched: met must be a contiguous int32 tensor with an entry per logits row")
        if is_per_image(constraints):
            name = "capnet_beam_topk_batched_rules"
            args = block + (n, ptr(bans), cap, ptr(met)) + rules_arg("beam_topk_batched", constraints, n, logits.device) \
                + (int(end_token),)
        else:
            name = "capnet_beam_topk_batched_forced"
            args = block + (n, ptr(bans), cap, ptr(met)) + forced_args(constraints, logits.device) + (int(end_token),)
    elif diversity is not None:
        teams = int(diversity.groups)
        if n % teams:
            raise CapnetError("beam_topk_batched: %d rows of meta for teams of %d" % (n, teams))
        name, args = "capnet_beam_topk_batched_diverse", block + (n // teams, teams, float(diversity.strength), ptr(bans), cap)
    elif bans is not None:
        name, args = "capnet_beam_topk_batched_banned", block + (n, ptr(bans), cap)
    else:
        name, args = "capnet_beam_topk_batched", block + (n,)
    check(getattr(_lib.lib(), name)(*args, ptr(scores), ptr(index), current_stream()), name)
    return scores, index


class BeamState:
    """The device-resident state of capnet.beam.beam_search_device (capnet_beam_*): n images x k fixed slots, at most
    `max_steps` advances. live_total [1], live [n] (int32) and scores [n, k] (float32) are views into the state."""

    def __init__(self, n, k, max_steps, device):
        nbytes = _lib.lib().capnet_beam_state_bytes(n, k, max_steps)
        if not nbytes:
            raise CapnetError("beam state: n=%d k=%d max_steps=%d (n, max_steps >= 1; 1 <= k <= 16)" % (n, k, max_steps))
        self.n, self.k, self.max_steps = n, k, max_steps
        self.words = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
        p = [C.c_void_p() for _ in range(3)]
        check(_lib.lib().capnet_beam_live(ptr(self.words), n, k, max_steps, *[C.byref(q) for q in p]), "capnet_beam_live")
        at = [(q.value - self.words.data_ptr()) // 4 for q in p]
        self.live_total = self.words[at[0]:at[0] + 1]
        self.live = self.words[at[1]:at[1] + n]
        self.scores = self.words[at[2]:at[2] + n * k].view(torch.float32).view(n, k)


def beam_init(n, k, max_steps, start_token, prev_words):
    """A fresh BeamState on prev_words' device: every beam live, score 0, sequence [start_token]; prev_words (int64
    [n k], contiguous) is filled with start_token."""
    _need_cuda(prev_words)
    if prev_words.dtype != torch.int64 or prev_words.numel() != n * k or not prev_words.is_contiguous():
        raise CapnetError("beam_init: prev_words must be a contiguous int64 [n k] tensor")
    beam = BeamState(n, k, max_steps, prev_words.device)
    check(_lib.lib().capnet_beam_init(ptr(beam.words), n, k, max_steps, int(start_token), ptr(prev_words), current_stream()),
          "capnet_beam_init")
    return beam


_banned_dev = {}      # (banned, device index) -> the int32 device array of a Constraints' banned words
BANNED_CACHE_MAX = 64   # distinct (ban list, device) pairs kept; one more empties the cache (an array is at most 32 ints)


def _device_ints(values, device):
    """A tuple of ints -> (the pointer of a device int32 array that holds them, their count). The array is made once per
    (tuple, device) and kept, so that a search's steps do not copy it again; the cache holds at most BANNED_CACHE_MAX arrays.
    (An array dropped from it while a launch that reads it is queued stays valid: torch's allocator hands freed memory to
    later work of the same stream only.)"""
    values = tuple(int(w) for w in values)
    key = (values, torch.device(device).index or 0)
    arr = _banned_dev.get(key)
    if arr is None:
        if len(_banned_dev) >= BANNED_CACHE_MAX:
            _banned_dev.clear()
        arr = _banned_dev[key] = torch.tensor(values or (0,), dtype=torch.int32, device=device)
    return ptr(arr), len(values)


def constraint_args(constraints, device):
    """The four trailing arguments of the capnet_*_constrained entries for a capnet.beam.Constraints: (no_repeat_ngram,
    min_words, the banned words as a device int32 array, their count); the array is _device_ints'."""
    return (int(constraints.no_repeat_ngram), int(constraints.min_words)) + _device_ints(constraints.banned, device)


NO_CONSTRAINTS = (0, 0, None, 0)     # the constraint arguments of an entry that takes them, zeros meaning none


def has_forced(constraints):
    """Whether `constraints` (a capnet.beam.Constraints or None) names forced words: the capnet_*_forced entries then."""
    return constraints is not None and bool(getattr(constraints, "forced", ()))


def is_per_image(constraints):
    """Whether `constraints` is a capnet.beam.PerImage (a rule per image): the capnet_*_rules entries then."""
    return hasattr(constraints, "entries") and hasattr(constraints, "table")


RULE_WORDS = 40       # CAPNET_BEAM_RULE_WORDS


def rules_arg(who, per_image, n, device):
    """The `rules` argument of the capnet_*_rules entries for a capnet.beam.PerImage of n entries: the pointer of its table
    on `device` (PerImage.table: int32 [n, RULE_WORDS], uploaded once per device and kept by the object), checked here
    because the C entries cannot read it."""
    if len(per_image) != n:
        raise CapnetError("%s: a PerImage of %d entries for %d images" % (who, len(per_image), n))
    table = per_image.table(device)
    if table.dtype != torch.int32 or tuple(table.shape) != (n, RULE_WORDS) or not table.is_contiguous() or table.data_ptr() % 16:
        raise CapnetError("%s: the rule table must be a contiguous, 16-byte aligned int32 [n, %d] tensor" % (who, RULE_WORDS))
    _need_cuda(table)
    return (ptr(table),)


def forced_args(constraints, device):
    """The two arguments behind constraint_args' four in the capnet_*_forced entries: (the forced ids as a device int32 array,
    their count), the array kept as constraint_args keeps the banned words'."""
    return _device_ints(constraints.forced, device)


def beam_advance(beam, logits, step, end_token, next_words, parent_rows, constraints=None, diversity=None, trace=None,
                 who="beam_advance"):
    """capnet_beam_advance: step `step` (1-based) of every image on logits [n k, V]; fills next_words and parent_rows
    (int64 [n k], contiguous) -- see include/capnet.h. The entry by what is given, not by what it holds:
    diversity (a capnet.beam.Diversity; capnet_beam_advance_diverse): `beam` is the state of n D searches of k / D beams
    (beam_init(n D, k / D, ...)), state-image i D + g being team g of image i; one workgroup per image walks its teams in
    order under the Hamming penalty; constraints may be None.
    Else constraints a capnet.beam.PerImage of n entries (capnet_beam_advance_rules): every image's workgroup takes its rule
    from its own row of the rule table.
    Else constraints with forced words (capnet_beam_advance_forced): their exclusions, then the forced-word allocation.
    Else constraints (a capnet.beam.Constraints; capnet_beam_advance_constrained[_traced]): the selecting workgroup
    excludes what they forbid, from the sequences in the state.
    Else capnet_beam_advance[_traced], the only form that leaves `logits` as it is (the others write -inf over the
    excluded words, the diverse one the penalised logits).
    trace (beam_trace(beam)) or None: the slot every hypothesis occupied at this step is recorded in it.
    who: the name in front of this function's own messages."""
    _need_cuda(logits, next_words, parent_rows)
    n, k = beam.n, beam.k
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[0] != n * k or logits.stride(1) != 1:
        raise CapnetError("%s: logits must be float32 [n k, V] with unit column stride" % who)
    for w in (next_words, parent_rows):
        if w.dtype != torch.int64 or w.numel() != n * k or not w.is_contiguous():
            raise CapnetError("%s: next_words / parent_rows must be contiguous int64 [n k] tensors" % who)
    if trace is not None:
        _check_trace(who, beam, trace)
    state, dev = (ptr(beam.words),), logits.device
    block = (ptr(logits), logits.stride(0) if n * k > 1 else logits.shape[1], logits.shape[1])
    at = (beam.max_steps, int(step), int(end_token))
    if diversity is not None and is_per_image(constraints):
        raise CapnetError("%s: a PerImage does not go with diversity" % who)
    if diversity is not None:
        teams = int(diversity.groups)
        if n % teams:
            raise CapnetError("%s: a state of %d searches for teams of %d" % (who, n, teams))
        name = "capnet_beam_advance_diverse"
        args = state + (ptr(trace),) + block + (n // teams, k * teams, teams, float(diversity.strength)) + at \
            + (NO_CONSTRAINTS if constraints is None else constraint_args(constraints, dev))
    elif is_per_image(constraints):
        name = "capnet_beam_advance_rules"
        args = state + (ptr(trace),) + block + (n, k) + at + rules_arg(who, constraints, n, dev)
    elif has_forced(constraints):
        name = "capnet_beam_advance_forced"
        args = state + (ptr(trace),) + block + (n, k) + at + constraint_args(constraints, dev) + forced_args(constraints, dev)
    else:
        con = () if constraints is None else constraint_args(constraints, dev)
        name = "capnet_beam_advance" + ("_constrained" if con else "") + ("" if trace is None else "_traced")
        args = state + (() if trace is None else (ptr(trace),)) + block + (n, k) + at + con
    check(getattr(_lib.lib(), name)(*args, ptr(next_words), ptr(parent_rows), current_stream()), name)


def beam_advance_topk(beam, values, index, lse, step, end_token, next_words, parent_rows, V=None):
    """capnet_beam_advance_topk: beam_advance on a step's candidates instead of its logits -- values float32 [n k, k] and
    index int32 [n k, k] (per row its k best logits and their vocabulary entries, best first; -1: nothing), lse float32
    [n k] (vocab_topk's outputs). V: the vocabulary size; it only bounds the indices and orders ties by (row, index), so
    None (any bound above every index) selects the same."""
    _need_cuda(values, index, lse, next_words, parent_rows)
    nk, k = beam.n * beam.k, beam.k
    if values.dtype != torch.float32 or tuple(values.shape) != (nk, k) or not values.is_contiguous() \
            or index.dtype != torch.int32 or tuple(index.shape) != (nk, k) or not index.is_contiguous() \
            or lse.dtype != torch.float32 or lse.numel() != nk or not lse.is_contiguous():
        raise CapnetError("beam_advance_topk: values float32 [n k, k], index int32 [n k, k], lse float32 [n k], contiguous")
    for w in (next_words, parent_rows):
        if w.dtype != torch.int64 or w.numel() != nk or not w.is_contiguous():
            raise CapnetError("beam_advance_topk: next_words / parent_rows must be contiguous int64 [n k] tensors")
    check(_lib.lib().capnet_beam_advance_topk(ptr(beam.words), ptr(values), ptr(index), ptr(lse),
                                              0x7fffffff if V is None else int(V), beam.n, k, beam.max_steps, int(step),
                                              int(end_token), ptr(next_words), ptr(parent_rows), current_stream()),
          "capnet_beam_advance_topk")


def beam_exclusion_mask(beam, step, V, end_token, constraints, out=None):
    """What each of the n k rows of `beam` (a BeamState) may not select at step `step` (1-based), from the hypotheses in the
    state (capnet_beam_exclusion_mask; the fused beam step's one extra launch): int32 [n k, ceil(V / 32)], bit v &
    31 of word v >> 5 of row r set where capnet.beam.banned_words(row r's `step` tokens, step, end_token, constraints) holds
    v -- sample_exclusion_mask's layout, for vocab_topk(mask=, select_only=True). constraints: a capnet.beam.Constraints;
    forced words are not the mask's. Rows of dead slots get a mask nobody reads. out: a mask to overwrite."""
    who = "beam_exclusion_mask"
    if has_forced(constraints):
        raise CapnetError("%s: forced words are selected from logits, not through a mask" % who)
    step, V, rows = int(step), int(V), beam.n * beam.k
    if not 1 <= step <= beam.max_steps or not 1 <= V <= SAMPLE_MAX_ROWS:
        raise CapnetError("%s: step %d of %d, V %d" % (who, step, beam.max_steps, V))
    if out is None:
        out = torch.empty((rows, mask_words(V)), dtype=torch.int32, device=beam.words.device)
    _check_mask(who, out, rows, V)
    check(_lib.lib().capnet_beam_exclusion_mask(ptr(beam.words), beam.n, beam.k, beam.max_steps, step, V, int(end_token),
                                                *constraint_args(constraints, beam.words.device), ptr(out), current_stream()),
          "capnet_beam_exclusion_mask")
    return out


def beam_finish(beam, end_token):
    """capnet_beam_finish -> (seqs int64 [n, max_steps + 2], lengths int32 [n], packed): the two are views of the one
    int64 buffer `packed`, so a caller takes both to the host in one copy."""
    n, L = beam.n, beam.max_steps + 2
    packed = torch.empty(n * L + (n + 1) // 2, dtype=torch.int64, device=beam.words.device)
    seqs, lengths = packed[:n * L].view(n, L), packed[n * L:].view(torch.int32)[:n]
    check(_lib.lib().capnet_beam_finish(ptr(beam.words), n, beam.k, beam.max_steps, int(end_token), ptr(seqs), ptr(lengths),
                                        current_stream()), "capnet_beam_finish")
    return seqs, lengths, packed


def beam_trace(beam):
    """The row trace of a BeamState (capnet_beam_trace_bytes): int32 words beside the state, for beam_advance_traced /
    beam_finish_traced. It needs no initialisation."""
    nbytes = _lib.lib().capnet_beam_trace_bytes(beam.n, beam.k, beam.max_steps)
    if not nbytes:
        raise CapnetError("beam trace: n=%d k=%d max_steps=%d" % (beam.n, beam.k, beam.max_steps))
    return torch.empty(nbytes // 4, dtype=torch.int32, device=beam.words.device)


def _check_trace(who, beam, trace):
    _need_cuda(trace)
    if trace is None or trace.dtype != torch.int32 or not trace.is_contiguous() or \
            trace.numel() * 4 < _lib.lib().capnet_beam_trace_bytes(beam.n, beam.k, beam.max_steps):
        raise CapnetError("%s: trace must be beam_trace(beam)" % who)


def beam_advance_traced(beam, trace, logits, step, end_token, next_words, parent_rows, constraints=None):
    """capnet_beam_advance_traced: beam_advance that also records, in `trace` (beam_trace(beam)), the slot every hypothesis
    occupied at this step -- see include/capnet.h. beam_advance(trace=trace), the trace required."""
    if trace is None:
        _check_trace("beam_advance_traced", beam, trace)
    beam_advance(beam, logits, step, end_token, next_words, parent_rows, constraints=constraints, trace=trace,
                 who="beam_advance_traced")


def beam_finish_traced(beam, trace, end_token):
    """capnet_beam_finish_traced -> (seqs int64 [n, max_steps + 2], lengths int32 [n], rows int32 [n, max_steps]): rows[i,
    e - 1] is the decoder-step row (i k + slot) whose step-e attention preceded word e of the winner, -1 past length - 1."""
    _check_trace("beam_finish_traced", beam, trace)
    n, L = beam.n, beam.max_steps + 2
    dev = beam.words.device
    seqs = torch.empty((n, L), dtype=torch.int64, device=dev)
    lengths = torch.empty(n, dtype=torch.int32, device=dev)
    rows = torch.empty((n, beam.max_steps), dtype=torch.int32, device=dev)
    check(_lib.lib().capnet_beam_finish_traced(ptr(beam.words), ptr(trace), n, beam.k, beam.max_steps, int(end_token), ptr(seqs),
                                               ptr(lengths), ptr(rows), current_stream()), "capnet_beam_finish_traced")
    return seqs, lengths, rows


def _nbest_alloc(n, k, L, device, flag=False):
    """The outputs of capnet_beam_nbest as views of ONE int64 buffer, so that a caller takes all of them to the host in one
    copy: seqs int64 [n, k, L] | lengths int32 [n, k] | scores float32 [n, k] | counts int32 [n] | with `flag`, one more
    int32 for the device's error word -> (packed, seqs, lengths, scores, counts, the error word's view or None)."""
    nk = n * k
    packed = torch.empty(nk * L + (2 * nk + n + 2) // 2, dtype=torch.int64, device=device)
    tail = packed[nk * L:].view(torch.int32)
    return (packed, packed[:nk * L].view(n, k, L), tail[:nk].view(n, k), tail[nk:2 * nk].view(torch.float32).view(n, k),
            tail[2 * nk:2 * nk + n], tail[2 * nk + n:2 * nk + n + 1] if flag else None)


def nbest_lists(packed, n, k, L):
    """_nbest_alloc's buffer in one copy to the host -> (per image the list of (tokens, score), best first; the lengths
    [n][k]; the int32 words behind counts, on the host)."""
    host = packed.cpu()
    nk = n * k
    tail = host[nk * L:].view(torch.int32)
    lens = tail[:nk].view(n, k).tolist()
    scores = tail[nk:2 * nk].view(torch.float32).view(n, k).tolist()
    counts = tail[2 * nk:2 * nk + n].tolist()
    rows = host[:nk * L].view(n, k, L).tolist()
    return [[(rows[i][r][:lens[i][r]], scores[i][r]) for r in range(counts[i])] for i in range(n)], lens, tail[2 * nk + n:]


def check_length_penalty(who, nbest, length_penalty):
    length_penalty = float(length_penalty)
    if length_penalty != 0.0 and not nbest:
        raise CapnetError("%s: length_penalty=%r needs nbest=True (the call without it returns the reference's winner)"
                          % (who, length_penalty))
    if length_penalty != length_penalty or length_penalty in (float("inf"), float("-inf")):
        raise CapnetError("%s: length_penalty must be finite" % who)
    return length_penalty


def beam_nbest(beam, end_token, length_penalty=0.0):
    """capnet_beam_nbest -> (seqs int64 [n, k, max_steps + 2], lengths int32 [n, k], scores float32 [n, k], counts int32 [n],
    packed): every completed hypothesis of every image, best first by score / (length - 1)^length_penalty (0: by the score
    itself; entry 0 is then beam_finish's winner), ties to the earlier completion; zeros past counts[i]. The four are views
    of the one int64 buffer `packed`. end_token is beam_finish's argument and fills nothing here: an image that completed
    nothing has count 0. The state is only read."""
    n, L = beam.n, beam.max_steps + 2
    packed, seqs, lengths, scores, counts, _ = _nbest_alloc(n, beam.k, L, beam.words.device)
    check(_lib.lib().capnet_beam_nbest(ptr(beam.words), n, beam.k, beam.max_steps, check_length_penalty("beam_nbest", True, length_penalty),
                                       ptr(seqs), ptr(lengths), ptr(scores), ptr(counts), current_stream()), "capnet_beam_nbest")
    return seqs, lengths, scores, counts, packed


def beam_nbest_traced(beam, trace, end_token, length_penalty=0.0):
    """capnet_beam_nbest_traced -> (seqs, lengths, scores, counts, rows int32 [n, k, max_steps]): beam_nbest, and per
    hypothesis beam_finish_traced's rows."""
    _check_trace("beam_nbest_traced", beam, trace)
    n, L = beam.n, beam.max_steps + 2
    _, seqs, lengths, scores, counts, _ = _nbest_alloc(n, beam.k, L, beam.words.device)
    rows = torch.empty((n, beam.k, beam.max_steps), dtype=torch.int32, device=beam.words.device)
    check(_lib.lib().capnet_beam_nbest_traced(ptr(beam.words), ptr(trace), n, beam.k, beam.max_steps,
                                              check_length_penalty("beam_nbest_traced", True, length_penalty), ptr(seqs), ptr(lengths),
                                              ptr(scores), ptr(counts), ptr(rows), current_stream()), "capnet_beam_nbest_traced")
    return seqs, lengths, scores, counts, rows


def _nbest_of_workspace(ws, beam_offset, n, k, max_steps, length_penalty, flag, maps=None):
    """The n-best of a one-call search out of its workspace (capnet_beam_nbest on ws + beam_offset, a second, tiny call after
    the search returned) -> per image the list of (tokens, score), best first. Sequences, lengths, scores, counts and the
    error word `flag` come to the host in one copy; a set error word raises.
    maps = (trace offset, history offset, P): the search recorded its attention maps -- capnet_beam_nbest_traced and ONE
    capnet_alpha_gather over all n k hypotheses; the result is followed by, per image, its hypotheses' float32 [len - 1, P]
    tensors (on the device)."""
    if not beam_offset or (maps is not None and not (maps[0] and maps[1])):
        raise CapnetError("n-best: no beam state in this workspace (n=%d k=%d max_steps=%d)" % (n, k, max_steps))
    L, T, dev = _lib.lib(), max_steps, ws.device
    packed, seqs, lengths, scores, counts, err = _nbest_alloc(n, k, T + 2, dev, flag=True)
    base = ws.data_ptr()
    beam = C.c_void_p(base + beam_offset)
    alphas = None
    if maps is None:
        check(L.capnet_beam_nbest(beam, n, k, T, length_penalty, ptr(seqs), ptr(lengths), ptr(scores), ptr(counts),
                                  current_stream()), "capnet_beam_nbest")
    else:
        trace_offset, hist_offset, P = maps
        rows = torch.empty((n, k, T), dtype=torch.int32, device=dev)
        check(L.capnet_beam_nbest_traced(beam, C.c_void_p(base + trace_offset), n, k, T, length_penalty, ptr(seqs), ptr(lengths),
                                         ptr(scores), ptr(counts), ptr(rows), current_stream()), "capnet_beam_nbest_traced")
        alphas = torch.empty((n * k, T, P), dtype=torch.float32, device=dev)
        check(L.capnet_alpha_gather(C.c_void_p(base + hist_offset), ptr(rows), n * k, n * k, T, P, ptr(alphas), current_stream()),
              "capnet_alpha_gather")
    err.copy_(flag)
    out, lens, word = nbest_lists(packed, n, k, T + 2)
    if int(word[0]):
        check_device_errors()
    if alphas is None:
        return out
    return out, [[alphas[i * k + r, :lens[i][r] - 1] for r in range(len(out[i]))] for i in range(n)]


def attention_step(att1, feat, z, A, w_full, b_full, xa=None, xa_col=0):
    """One attention step for s rows (no autograd; Attention.forward / sample()).
    att1 [s, P, A] = encoder_att(features); feat [s, P, C]; z [s, A + C] = [decoder_att(h) |
    f_beta(h)] pre-activations (the gate half is overwritten with its sigmoid).
    Returns (awe [s, C] ungated context, alpha [s, P]); if `xa` [s, W] is given, the GATED context
    is written into xa[:, xa_col : xa_col + C]."""
    _need_cuda(att1, feat, z)
    s_rows, P, Adim = att1.shape
    Cdim = feat.shape[2]
    if not (att1.is_contiguous() and feat.is_contiguous() and z.is_contiguous()):
        raise CapnetError("attention_step: inputs must be contiguous")
    if Adim != A or z.shape[1] != A + Cdim or feat.shape[0] != s_rows or feat.shape[1] != P:
        raise CapnetError("attention_step: shape mismatch")
    dev = att1.device
    alpha = torch.empty((s_rows, P), dtype=torch.float32, device=dev)
    alphas_bt = torch.empty((s_rows, 1, P), dtype=torch.float32, device=dev)
    awe = torch.empty((s_rows, Cdim), dtype=torch.float32, device=dev)
    scores_ws = torch.empty((s_rows, P), dtype=torch.float32, device=dev)
    if xa is None:
        xa, xa_col = torch.empty((s_rows, Cdim), dtype=torch.float32, device=dev), 0
    if not xa.is_contiguous() or xa.shape[0] != s_rows or xa_col + Cdim > xa.shape[1] or xa_col % 4:
        raise CapnetError("attention_step: bad xa")
    wf, bf = _c(w_full.detach()).reshape(-1), _c(b_full.detach()).reshape(-1)
    check(_lib.lib().capnet_att_step_fwd(ptr(att1), ptr(feat), ptr(z), C.c_void_p(z.data_ptr() + 4 * A), z.shape[1],
                                         ptr(wf), ptr(bf), s_rows, P, A, Cdim, ptr(alpha),
                                         ptr(alphas_bt), 1, 0, ptr(awe), C.c_void_p(xa.data_ptr() + 4 * xa_col),
                                         xa.shape[1], ptr(scores_ws), current_stream()), "capnet_att_step_fwd")
    return awe, alpha


def embedding(idx, weight):
    """weight[idx] (no autograd: used by forward_step()/sample())."""
    _need_cuda(idx, weight)
    idx, w = _c(idx), _c(weight.detach())
    if idx.dtype != torch.int64:
        raise CapnetError("embedding indices must be int64")
    out = torch.empty(tuple(idx.shape) + (w.shape[1],), dtype=torch.float32, device=w.device)
    check(_lib.lib().capnet_embedding_fwd(ptr(idx), idx.numel(), ptr(w), w.shape[1], w.shape[0],
                                          ptr(out), ptr(err_flag(w.device)), current_stream()),
          "capnet_embedding_fwd")
    return out


def lstm_pointwise(pre, c_prev, cell):
    """(h, c) from gate pre-activations [b, 4H] and the previous cell state (no autograd)."""
    _need_cuda(pre, c_prev)
    pre = pre.detach().clone().contiguous()
    c_prev = _c(c_prev.detach())
    b, h4 = pre.shape
    H = h4 // 4
    c = torch.empty((b, H), dtype=torch.float32, device=pre.device)
    h = torch.empty((b, H), dtype=torch.float32, device=pre.device)
    check(_lib.lib().capnet_lstm_pointwise_fwd(ptr(pre), ptr(c_prev), ptr(c), ptr(h), b, H, cell,
                                               current_stream()), "capnet_lstm_pointwise_fwd")
    return h, c


class LstmCellFn(torch.autograd.Function):
    """(h, c) = cell(pre-activations [b, 4H], c_prev [b, H]) with autograd: capnet_lstm_pointwise_fwd / _bwd.
    cell 0: gates i,f,o,c~ and h = o*c (stylenet/model.py:147-153); cell 1: i,f,g,o and h = o*tanh(c)."""

    @staticmethod
    def forward(ctx, pre, c_prev, cell):
        _need_cuda(pre, c_prev)
        gates = pre.detach().clone().contiguous()          # the kernel leaves the activated gates here
        cp = _c(c_prev.detach())
        b, h4 = gates.shape
        H = h4 // 4
        c = torch.empty((b, H), dtype=torch.float32, device=gates.device)
        h = torch.empty((b, H), dtype=torch.float32, device=gates.device)
        check(_lib.lib().capnet_lstm_pointwise_fwd(ptr(gates), ptr(cp), ptr(c), ptr(h), b, H, cell, current_stream()),
              "capnet_lstm_pointwise_fwd")
        ctx.save_for_backward(gates, c, cp)
        ctx.cell = cell
        ctx.mark_non_differentiable()
        return h, c

    @staticmethod
    def backward(ctx, dh, dc):
        gates, c, cp = ctx.saved_tensors
        b, h4 = gates.shape
        H = h4 // 4
        dh = _c(dh) if dh is not None else torch.zeros_like(c)
        dc_io = dc.clone().contiguous() if dc is not None else torch.zeros_like(c)
        dpre = torch.empty_like(gates)
        check(_lib.lib().capnet_lstm_pointwise_bwd(ptr(gates), ptr(c), ptr(cp), ptr(dh), ptr(dc_io), ptr(dpre), b, H,
                                                   ctx.cell, current_stream()), "capnet_lstm_pointwise_bwd")
        return dpre, dc_io, None


def lstm_cell(pre, c_prev, cell=0):
    return LstmCellFn.apply(pre, c_prev, cell)



DECODE_HIDDEN = (64, 128, 256, 512, 1024)
MAX_GROUPS = 8        # weight groups of the grouped decode step (capnet_*_groups)


def stacked_decode_supported(E, H):
    """The shapes capnet_stacked_decode_step takes (csrc/lstm_decode_step.hip: stacked_decode_supported)."""
    return E >= 1 and H in DECODE_HIDDEN and (E + 15) // 16 * 16 + H <= 2048


def _check_groups(who, groups):
    groups = int(groups)
    if not 1 <= groups <= MAX_GROUPS:
        raise CapnetError("%s: groups %d (1..%d)" % (who, groups, MAX_GROUPS))
    return groups


def _check_layer_weights(who, wcat, beff, groups, H, kin0):
    """wcat[l] [4H, kin_l + H] and beff[l] [4H], with a leading [groups] dimension when groups > 1."""
    lead = () if groups == 1 else (groups,)
    for l, (w, b) in enumerate(zip(wcat, beff)):
        kin = kin0 if l == 0 else H
        if tuple(w.shape) != lead + (4 * H, kin + H) or not w.is_contiguous() or tuple(b.shape) != lead + (4 * H,) \
                or (lead and not b.is_contiguous()):
            raise CapnetError("%s: layer %d weights must be %s[4H, %d] and %s[4H]"
                              % (who, l, "[groups]" if lead else "", kin + H, "[groups]" if lead else ""))


def stacked_decode_step(state, wcat, beff, x, tokens=None, cell=CELL_FACTORED, parent_rows=None, groups=1):
    """One inference step of every layer of a stacked LSTM (capnet_stacked_decode_step, or _cell for the LSTM cell: one
    launch per layer). state [rows, 2L, H] (slot 2l = h of layer l, 2l+1 = c); wcat[l] [4H, kin_l + H] = [folded chain |
    W] (factored) or [weight_ih | weight_hh] (LSTM cell), gate blocks i, f, o, c~; beff[l] [4H]; x: the embedding table
    [V, E] when `tokens` (int64 [rows]) is given, else layer 0's inputs [rows, E]. parent_rows (int64 [rows]): the step on
    state.index_select(0, parent_rows) without that copy (capnet_stacked_decode_step_gather).
    groups > 1 (capnet_stacked_decode_step_groups): the rows are `groups` equal blocks, group-major, and block g runs on
    wcat[l][g] / beff[l][g] -- wcat[l] [groups, 4H, kin_l + H], beff[l] [groups, 4H] -- in the same launches; each block's
    rows equal the step of that block alone on its weights, bit for bit.
    Returns (top-layer h [rows, H], the new state [rows, 2L, H])."""
    if cell not in (CELL_FACTORED, CELL_LSTM):
        raise CapnetError("stacked_decode_step: unknown cell %r" % (cell,))
    groups = _check_groups("stacked_decode_step", groups)
    _need_cuda(state, x, tokens, *wcat, *beff)
    rows, L2, H = state.shape
    if rows % groups:
        raise CapnetError("stacked_decode_step: %d rows in %d groups" % (rows, groups))
    nl = L2 // 2
    if L2 != 2 * nl or len(wcat) != nl or len(beff) != nl:
        raise CapnetError("stacked_decode_step: state [rows, 2L, H] and L weight pairs")
    state, x = _c(state), _c(x)
    E = x.shape[1]
    if tokens is not None:
        tokens = _c(tokens)
        if tokens.dtype != torch.int64 or tokens.numel() != rows:
            raise CapnetError("stacked_decode_step: tokens must be int64 [rows]")
    elif x.shape[0] != rows:
        raise CapnetError("stacked_decode_step: inputs must be [rows, E]")
    _check_layer_weights("stacked_decode_step", wcat, beff, groups, H, (E + 15) // 16 * 16)
    out = torch.empty_like(state)
    top = torch.empty((rows, H), dtype=torch.float32, device=state.device)
    if parent_rows is not None:
        _need_cuda(parent_rows)
        parent_rows = _c(parent_rows)
        if parent_rows.dtype != torch.int64 or parent_rows.numel() != rows:
            raise CapnetError("stacked_decode_step: parent_rows must be int64 [rows]")
    if groups > 1:
        check(_lib.lib().capnet_stacked_decode_step_groups(
            cell, nl, groups, rows // groups, E, H, x.shape[0] if tokens is not None else 0, ptr(tokens), ptr(x),
            ptr_array(wcat), ptr_array(beff), ptr(state), ptr(parent_rows), ptr(out), ptr(top), ptr(err_flag(state.device)),
            current_stream()), "capnet_stacked_decode_step_groups")
        return top, out
    if parent_rows is not None:
        check(_lib.lib().capnet_stacked_decode_step_gather(
            cell, nl, rows, E, H, x.shape[0] if tokens is not None else 0, ptr(tokens), ptr(x), ptr_array(wcat),
            ptr_array(beff), ptr(state), ptr(parent_rows), ptr(out), ptr(top), ptr(err_flag(state.device)), current_stream()),
            "capnet_stacked_decode_step_gather")
        return top, out
    args = (nl, rows, E, H, x.shape[0] if tokens is not None else 0, ptr(tokens), ptr(x), ptr_array(wcat), ptr_array(beff),
            ptr(state), ptr(out), ptr(top), ptr(err_flag(state.device)), current_stream())
    if cell == CELL_FACTORED:
        check(_lib.lib().capnet_stacked_decode_step(*args), "capnet_stacked_decode_step")
    else:
        check(_lib.lib().capnet_stacked_decode_step_cell(cell, *args), "capnet_stacked_decode_step_cell")
    return top, out


def _check_tables(who, tables, shape, groups=None):
    """One contiguous fp32 tensor of `shape` per group, used where it lies (a table is never stacked or copied)."""
    tables = list(tables)
    if groups is None:
        groups = _check_groups(who, len(tables))
    if len(tables) != groups:
        raise CapnetError("%s: %d tables for %d groups" % (who, len(tables), groups))
    for t in tables:
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_contiguous():
            raise CapnetError("%s: one contiguous float32 %r tensor per group" % (who, tuple(shape)))
    _need_cuda(*tables)
    return [t.detach() for t in tables]


def _first_shape(tables):
    tables = list(tables)
    return tuple(tables[0].shape) if tables and tables[0] is not None else ()


def _group_biases(who, bs, groups, V):
    """One bias [V] (or None) per group, used where it lies -> the list, or None where `bs` is None."""
    if bs is None:
        return None
    bs = list(bs)
    if len(bs) != groups:
        raise CapnetError("%s: one bias (or None) per group" % who)
    present = [b for b in bs if b is not None]
    _check_tables(who, present, (V,), len(present))
    return [None if b is None else b.detach() for b in bs]


def _grouped_layer_weights(who, wcat, beff, groups, H, kin0):
    """The layers' weights with their leading [groups] dimension, also for one group."""
    for l, (w, b) in enumerate(zip(wcat, beff)):
        kin = kin0 if l == 0 else H
        if tuple(w.shape) != (groups, 4 * H, kin + H) or not w.is_contiguous() or tuple(b.shape) != (groups, 4 * H) \
                or not b.is_contiguous():
            raise CapnetError("%s: layer %d weights must be [groups, 4H, %d] and [groups, 4H]" % (who, l, kin + H))
    return list(wcat), list(beff)


def stacked_decode_step_tables(state, wcat, beff, tables, tokens, cell=CELL_LSTM, parent_rows=None):
    """stacked_decode_step over len(tables) weight groups whose layer 0 reads ITS OWN table (capnet_stacked_decode_step_
    tables): rows group-major, block g on wcat[l][g] / beff[l][g] and on tables[g] [V, E] by tokens (int64 [rows]). Each
    block's rows equal stacked_decode_step of that block alone on its weights and table, bit for bit.
    Returns (top-layer h [rows, H], the new state [rows, 2L, H])."""
    who = "stacked_decode_step"
    if cell not in (CELL_FACTORED, CELL_LSTM):
        raise CapnetError("%s: unknown cell %r" % (who, cell))
    tables = _check_tables(who, tables, _first_shape(tables))
    groups = len(tables)
    _need_cuda(state, tokens, parent_rows, *wcat, *beff)
    rows, L2, H = state.shape
    nl = L2 // 2
    if rows % groups or L2 != 2 * nl or len(wcat) != nl or len(beff) != nl or tables[0].dim() != 2:
        raise CapnetError("%s: state [groups rows, 2L, H], L weight pairs, tables [V, E]" % who)
    V, E = tables[0].shape
    state, tokens = _c(state), _c(tokens)
    if tokens.dtype != torch.int64 or tokens.numel() != rows:
        raise CapnetError("%s: tokens must be int64 [rows]" % who)
    if parent_rows is not None:
        parent_rows = _c(parent_rows)
        if parent_rows.dtype != torch.int64 or parent_rows.numel() != rows:
            raise CapnetError("%s: parent_rows must be int64 [rows]" % who)
    wcat, beff = _grouped_layer_weights(who, wcat, beff, groups, H, (E + 15) // 16 * 16)
    out = torch.empty_like(state)
    top = torch.empty((rows, H), dtype=torch.float32, device=state.device)
    check(_lib.lib().capnet_stacked_decode_step_tables(
        cell, nl, groups, rows // groups, E, H, V, ptr(tokens), ptr_array(tables), ptr_array(wcat), ptr_array(beff),
        ptr(state), ptr(parent_rows), ptr(out), ptr(top), ptr(err_flag(state.device)), current_stream()),
        "capnet_stacked_decode_step_tables")
    return top, out


def vocab_argmax_groups_workspace(groups, rows_per_group, V, device):
    """A zeroed workspace of capnet_vocab_argmax_groups (back-to-back calls on one stream may share it)."""
    n = _lib.lib().capnet_vocab_argmax_groups_ws_bytes(int(groups), int(rows_per_group), int(V))
    return torch.zeros((n + 7) // 8, dtype=torch.int64, device=device)


def vocab_argmax_groups(h, ws, bs=None, workspace=None):
    """vocab_argmax of len(ws) projections in one launch (capnet_vocab_argmax_groups): h [groups rows, H], group-major;
    block g on ws[g] [V, H] / bs[g] [V] (bs or any bs[g] None: no bias), each tensor used where it lies. Every block's
    tokens equal vocab_argmax of that block alone, bit for bit. Returns tokens [groups rows] int64."""
    who = "vocab_argmax"
    ws = _check_tables(who, ws, _first_shape(ws))
    groups = len(ws)
    _need_cuda(h)
    h = _c(h.detach())
    if h.dim() != 2 or ws[0].dim() != 2:
        raise CapnetError("%s: h [groups rows, H], w [V, H] per group" % who)
    rows, H = h.shape
    V = ws[0].shape[0]
    if ws[0].shape[1] != H or H not in DECODE_HIDDEN or rows < groups or rows % groups:
        raise CapnetError("%s: h [groups rows, H], w [V, H] per group with H in %r" % (who, DECODE_HIDDEN))
    bs = _group_biases(who, bs, groups, V)
    rpg = rows // groups
    if workspace is None:
        workspace = vocab_argmax_groups_workspace(groups, rpg, V, h.device)
    if workspace.numel() * workspace.element_size() < _lib.lib().capnet_vocab_argmax_groups_ws_bytes(groups, rpg, V):
        raise CapnetError("%s: workspace too small" % who)
    out = torch.empty(rows, dtype=torch.int64, device=h.device)
    check(_lib.lib().capnet_vocab_argmax_groups(ptr(h), ptr_array(ws), None if bs is None else ptr_array(bs), groups, rpg, H, V,
                                                ptr(workspace), ptr(out), current_stream()), "capnet_vocab_argmax_groups")
    return out


def vocab_argmax_workspace(rows, V, device):
    """A zeroed workspace of capnet_vocab_argmax for `rows` rows (back-to-back calls on one stream may share it)."""
    n = _lib.lib().capnet_vocab_argmax_ws_bytes(int(rows), int(V))
    return torch.zeros((n + 7) // 8, dtype=torch.int64, device=device)


def vocab_argmax(h, w, b=None, workspace=None):
    """tokens [rows] int64 = the first argmax over v of h[r] . w[v] + b[v] (capnet_vocab_argmax: the projection and the
    argmax in one launch, no logits in memory). h [rows, H], w [V, H], b [V]; H in DECODE_HIDDEN."""
    _need_cuda(h, w, b)
    h, w = _c(h.detach()), _c(w.detach())
    b = None if b is None else _c(b.detach())
    rows, H = h.shape
    V = w.shape[0]
    if w.shape[1] != H or H not in DECODE_HIDDEN or rows < 1 or (b is not None and b.numel() != V):
        raise CapnetError("vocab_argmax: h [rows, H], w [V, H], b [V] with H in %r" % (DECODE_HIDDEN,))
    if workspace is None:
        workspace = vocab_argmax_workspace(rows, V, h.device)
    if workspace.numel() * workspace.element_size() < _lib.lib().capnet_vocab_argmax_ws_bytes(rows, V):
        raise CapnetError("vocab_argmax: workspace too small")
    out = torch.empty(rows, dtype=torch.int64, device=h.device)
    check(_lib.lib().capnet_vocab_argmax(ptr(h), ptr(w), ptr(b), rows, H, V, ptr(workspace), ptr(out), current_stream()),
          "capnet_vocab_argmax")
    return out


def lstm_greedy_decode(steps, wcat, beff, emb, Cw, Cb, features=None, start_tokens=None, state=None):
    """`steps` greedy decode steps of a stacked nn.LSTM + nn.Linear in ONE C call (capnet_lstm_greedy_decode): tokens and
    logits never leave the device. wcat / beff: capnet.decode.pack_cell of every layer; emb [V, E]; Cw [V, H], Cb [V].
    The first input is `features` [rows, E] or emb[start_tokens] (int64 [rows]); state: [rows, 2L, H] or None for zeros.
    Returns (ids [rows, steps] int64, the final state [rows, 2L, H])."""
    if (features is None) == (start_tokens is None):
        raise CapnetError("lstm_greedy_decode: either features or start_tokens")
    _need_cuda(emb, Cw, Cb, features, start_tokens, state, *wcat, *beff)
    emb, Cw, Cb = _c(emb.detach()), _c(Cw.detach()), _c(Cb.detach())
    V, E = emb.shape
    H, nl = Cw.shape[1], len(wcat)
    rows = (features if features is not None else start_tokens).shape[0]
    if features is not None:
        features = _c(features.detach())
        if tuple(features.shape) != (rows, E):
            raise CapnetError("lstm_greedy_decode: features must be [rows, embed_size]")
    else:
        start_tokens = _c(start_tokens)
        if start_tokens.dtype != torch.int64 or start_tokens.dim() != 1:
            raise CapnetError("lstm_greedy_decode: start_tokens must be int64 [rows]")
    if not stacked_decode_supported(E, H) or not 1 <= nl <= 8 or len(beff) != nl or tuple(Cw.shape) != (V, H):
        raise CapnetError("lstm_greedy_decode: unsupported shape (E=%d, H=%d, %d layers)" % (E, H, nl))
    _check_layer_weights("lstm_greedy_decode", wcat, beff, 1, H, (E + 15) // 16 * 16)
    dev = emb.device
    if state is not None:
        state = _c(state.detach())
        if tuple(state.shape) != (rows, 2 * nl, H):
            raise CapnetError("lstm_greedy_decode: state must be [rows, 2L, H]")
    L = _lib.lib()
    ws = torch.empty((L.capnet_lstm_greedy_decode_ws_bytes(nl, rows, H, V) + 7) // 8, dtype=torch.int64, device=dev)
    ids = torch.empty((rows, int(steps)), dtype=torch.int64, device=dev)
    out = torch.empty((rows, 2 * nl, H), dtype=torch.float32, device=dev)
    check(L.capnet_lstm_greedy_decode(nl, rows, E, H, V, int(steps), ptr(features), ptr(start_tokens), ptr(emb),
                                      ptr_array(wcat), ptr_array(beff), ptr(Cw), ptr(Cb), ptr(state), ptr(ws), ptr(ids),
                                      ptr(out), ptr(err_flag(dev)), current_stream()), "capnet_lstm_greedy_decode")
    return ids, out


def lstm_greedy_decode_groups(steps, wcat, beff, embs, Cws, Cbs, start_tokens, state=None):
    """lstm_greedy_decode of len(embs) decoders in ONE C call (capnet_lstm_greedy_decode_groups): rows group-major, block
    g on embs[g] [V, E], wcat[l][g] / beff[l][g] and Cws[g] [V, H] / Cbs[g] [V]. The embeddings and projections are used
    where they lie (one pointer per group; nothing is stacked or copied); wcat[l] [groups, 4H, kin_l + H] and beff[l]
    [groups, 4H] are capnet.decode.pack_cell of every decoder's layer l, stacked. The first input is
    embs[g][start_tokens[r]] (int64 [groups rows]); state: [groups rows, 2L, H] or None for zeros.
    Returns (ids [groups rows, steps] int64, the final state [groups rows, 2L, H])."""
    who = "lstm_greedy_decode"
    embs = _check_tables(who, embs, _first_shape(embs))
    groups = len(embs)
    Cws = list(Cws)
    if embs[0].dim() != 2 or not Cws or Cws[0] is None or Cws[0].dim() != 2:
        raise CapnetError("%s: emb [V, E] and Cw [V, H] per group" % who)
    V, E = embs[0].shape
    H, nl = Cws[0].shape[1], len(wcat)
    Cws = _check_tables(who, Cws, (V, H), groups)
    Cbs = _check_tables(who, Cbs, (V,), groups)
    _need_cuda(start_tokens, state, *wcat, *beff)
    if not stacked_decode_supported(E, H) or not 1 <= nl <= 8 or len(beff) != nl:
        raise CapnetError("%s: unsupported shape (E=%d, H=%d, %d layers)" % (who, E, H, nl))
    start_tokens = _c(start_tokens)
    rows = start_tokens.numel()
    if start_tokens.dtype != torch.int64 or start_tokens.dim() != 1 or rows < groups or rows % groups or int(steps) < 1:
        raise CapnetError("%s: start_tokens must be int64 [groups rows], steps >= 1" % who)
    wcat, beff = _grouped_layer_weights(who, wcat, beff, groups, H, (E + 15) // 16 * 16)
    dev = embs[0].device
    if state is not None:
        state = _c(state.detach())
        if tuple(state.shape) != (rows, 2 * nl, H):
            raise CapnetError("%s: state must be [groups rows, 2L, H]" % who)
    L = _lib.lib()
    rpg = rows // groups
    ws = torch.empty((L.capnet_lstm_greedy_decode_groups_ws_bytes(nl, groups, rpg, H, V) + 7) // 8, dtype=torch.int64, device=dev)
    ids = torch.empty((rows, int(steps)), dtype=torch.int64, device=dev)
    out = torch.empty((rows, 2 * nl, H), dtype=torch.float32, device=dev)
    check(L.capnet_lstm_greedy_decode_groups(nl, groups, rpg, E, H, V, int(steps), ptr(start_tokens), ptr_array(embs),
                                             ptr_array(wcat), ptr_array(beff), ptr_array(Cws), ptr_array(Cbs), ptr(state),
                                             ptr(ws), ptr(ids), ptr(out), ptr(err_flag(dev)), current_stream()),
          "capnet_lstm_greedy_decode_groups")
    return ids, out


def vocab_topk_workspace(rows, k, V, device):
    """A zeroed workspace of capnet_vocab_topk for `rows` rows (back-to-back calls on one stream may share it)."""
    n = _lib.lib().capnet_vocab_topk_ws_bytes(int(rows), int(k), int(V))
    if not n:
        raise CapnetError("vocab_topk: rows=%d k=%d V=%d (rows >= 1; 1 <= k <= 16; k <= V)" % (rows, k, V))
    return torch.zeros((n + 7) // 8, dtype=torch.int64, device=device)


def vocab_topk(h, w, b=None, k=5, workspace=None, mask=None, select_only=False):
    """(values [rows, k] float32, index [rows, k] int32, lse [rows] float32) of the rows' logits h[r] . w[v] + b[v]
    (capnet_vocab_topk: the projection, the k best per row -- logit descending, index ascending -- and the row's
    log-sum-exp in one launch, no logits in memory). h [rows, H], w [V, H], b [V]; H in DECODE_HIDDEN; 1 <= k <= 16, k <= V.
    A NaN or -inf logit is never picked; a row with fewer than k pickable entries ends in (-inf, -1).
    mask (sample_exclusion_mask's, int32 [rows, ceil(V / 32)]; capnet_vocab_topk_masked): a word whose bit is set is not
    pickable either -- the k best of the allowed words, lse over the allowed words. None: capnet_vocab_topk.
    select_only (with a mask; capnet_vocab_topk_select, the constrained beam search's meaning): a word whose bit is set only
    leaves the k best -- lse stays the log-sum-exp over every word, capnet_vocab_topk's bit for bit."""
    _need_cuda(h, w, b)
    h, w = _c(h.detach()), _c(w.detach())
    b = None if b is None else _c(b.detach())
    k = int(k)
    if h.dim() != 2 or w.dim() != 2:
        raise CapnetError("vocab_topk: h [rows, H], w [V, H]")
    rows, H = h.shape
    V = w.shape[0]
    if w.shape[1] != H or H not in DECODE_HIDDEN or rows < 1 or (b is not None and b.numel() != V):
        raise CapnetError("vocab_topk: h [rows, H], w [V, H], b [V] with H in %r" % (DECODE_HIDDEN,))
    if not 1 <= k <= 16 or k > V:
        raise CapnetError("vocab_topk: k=%d (1 <= k <= 16, k <= V = %d)" % (k, V))
    if workspace is None:
        workspace = vocab_topk_workspace(rows, k, V, h.device)
    if workspace.numel() * workspace.element_size() < _lib.lib().capnet_vocab_topk_ws_bytes(rows, k, V):
        raise CapnetError("vocab_topk: workspace too small")
    values = torch.empty((rows, k), dtype=torch.float32, device=h.device)
    index = torch.empty((rows, k), dtype=torch.int32, device=h.device)
    lse = torch.empty(rows, dtype=torch.float32, device=h.device)
    if select_only and mask is None:
        raise CapnetError("vocab_topk: select_only needs a mask")
    if mask is not None:
        mask = _check_mask("vocab_topk", mask, rows, V)
        name = "capnet_vocab_topk_select" if select_only else "capnet_vocab_topk_masked"
        check(getattr(_lib.lib(), name)(ptr(h), ptr(w), ptr(b), rows, H, V, k, ptr(mask), ptr(workspace), ptr(values), ptr(index),
                                        ptr(lse), current_stream()), name)
        return values, index, lse
    check(_lib.lib().capnet_vocab_topk(ptr(h), ptr(w), ptr(b), rows, H, V, k, ptr(workspace), ptr(values), ptr(index), ptr(lse),
                                       current_stream()), "capnet_vocab_topk")
    return values, index, lse


# ---- sampled decoding (csrc/vocab_sample.hip, csrc/sample_rng.h) ----------------------------------------------------------
SAMPLE_MAX_STEPS = 65535          # the stream's step field
SAMPLE_MAX_ROWS = 1 << 24         # the stream's row field (rows below it) and vocabulary field (V up to it)


def sample_uniform(seed, step, row, v):
    """u(seed, step, row, v) of the sampling stream (capnet_sample_uniform, a host function: no GPU): an odd multiple of
    2^-24 strictly inside (0, 1). The kernels draw argmax_v (logit_v / T - log(-log u))."""
    seed, step, row, v = int(seed), int(step), int(row), int(v)
    if not (0 <= seed < 1 << 64 and 0 <= step <= SAMPLE_MAX_STEPS and 0 <= row < SAMPLE_MAX_ROWS and 0 <= v < SAMPLE_MAX_ROWS):
        raise CapnetError("sample_uniform: seed %d step %d row %d v %d (seed < 2^64, step <= 65535, row, v < 2^24)"
                          % (seed, step, row, v))
    return float(_lib.lib().capnet_sample_uniform(seed, step, row, v))


def draw_seed():
    """A 63-bit seed from torch's CPU generator (what seed=None means in every sample_random): torch.manual_seed makes a
    script reproducible."""
    return int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64).item()) * 2 + int(torch.randint(0, 2, (1,)).item())


def check_top_p(who, top_p):
    """top_p of nucleus sampling as the kernels compare it: a number with 0 < top_p <= 1, rounded ONCE to fp32 (a value that
    rounds to 0 or to above 1 is refused; one that rounds to 1.0 is 1.0, "off")."""
    try:
        p32 = struct.unpack("f", struct.pack("f", float(top_p)))[0]
    except (TypeError, ValueError, OverflowError):
        raise CapnetError("%s: top_p %r" % (who, top_p))
    if isinstance(top_p, bool) or not 0.0 < p32 <= 1.0:           # NaN fails
        raise CapnetError("%s: top_p %r (0 < top_p <= 1; 1 = off)" % (who, top_p))
    return p32


def check_sampling(who, temperature, top_k, seed, V=None, top_p=None):
    """(temperature, top_k, seed) checked: temperature finite and > 0; top_k 0 (off) .. 16 and <= V; seed an integer in
    [0, 2^64) or None (draw_seed). With top_p given: (temperature, top_k, seed, top_p), top_p through check_top_p."""
    try:
        temperature = float(temperature)
    except (TypeError, ValueError):
        raise CapnetError("%s: temperature %r" % (who, temperature))
    if not (temperature > 0.0 and temperature <= 3.0e38) or not (float(torch.tensor(temperature, dtype=torch.float32)) > 0.0):
        raise CapnetError("%s: temperature %r (finite, > 0)" % (who, temperature))
    if isinstance(top_k, bool) or int(top_k) != top_k or not 0 <= int(top_k) <= 16 or (V is not None and int(top_k) > V):
        raise CapnetError("%s: top_k=%r (0 = off, 1 .. 16, <= the vocabulary size)" % (who, top_k))
    if seed is None:
        seed = draw_seed()
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise CapnetError("%s: seed %r (an integer in [0, 2^64) or None)" % (who, seed))
    if top_p is not None:
        return temperature, int(top_k), seed, check_top_p(who, top_p)
    return temperature, int(top_k), seed


def _check_stream_pos(who, rows, V, step, row0):
    step, row0 = int(step), int(row0)
    if not (1 <= rows and 0 <= row0 and row0 + rows <= SAMPLE_MAX_ROWS and 1 <= V <= SAMPLE_MAX_ROWS and 0 <= step <= SAMPLE_MAX_STEPS):
        raise CapnetError("%s: rows %d, V %d, step %d, row0 %d (row0 + rows <= 2^24, V <= 2^24, step <= 65535)"
                          % (who, rows, V, step, row0))
    return step, row0


def _check_greedy_stride(who, greedy_stride, rows=None):
    """greedy_stride of the sampling calls: 0 (off), or g >= 1 -- the rows come in groups of g, the last of each the group's
    greedy row (csrc/sample_key.h); the loops need whole groups."""
    if isinstance(greedy_stride, bool) or int(greedy_stride) != greedy_stride or not 0 <= int(greedy_stride) < SAMPLE_MAX_ROWS:
        raise CapnetError("%s: greedy_stride=%r (0 = off, or the rows of a group)" % (who, greedy_stride))
    if greedy_stride and rows is not None and rows % int(greedy_stride):
        raise CapnetError("%s: %d rows in groups of greedy_stride %d" % (who, rows, greedy_stride))
    return int(greedy_stride)


def _call_sampler(name, greedy_stride, *args, excl=None):
    """capnet_<name>(*args, stream); with greedy rows capnet_<name>_greedy(*args, greedy_stride, stream). excl (_exclude_args'
    tuple, the *_excl entries): capnet_<name>(*args, greedy_stride, *excl, stream) -- they take the stride either way."""
    if excl is not None:
        args += (greedy_stride,) + excl
    elif greedy_stride:
        name, args = name + "_greedy", args + (greedy_stride,)
    check(getattr(_lib.lib(), "capnet_" + name)(*(args + (current_stream(),))), "capnet_" + name)


def _call_sampled_loop(who, dims, shape, head, top_k, top_p, seed, outs, greedy_stride, excl, dev, plain_slab=False):
    """The one C call of ops.sample_decode / ops.att_sample_decode (`who`), chosen from (exclusions, top_p < 1, greedy_stride)
    here and in _call_sampler: capnet_<who>_excl, capnet_<who>_nucleus or capnet_<who>, on a workspace of that entry's own
    size query (`dims`: the query's arguments in front of top_k; `shape`: what an error says of them). The entry takes head,
    top_k, top_p (but the plain one), seed, the workspace, the split-K slab (the plain one only with plain_slab), outs."""
    form = "_excl" if excl is not None else "_nucleus" if top_p < 1.0 else ""
    nbytes = getattr(_lib.lib(), "capnet_%s%s_ws_bytes" % (who, form))(*dims, top_k, *((top_p,) if excl is not None else ()))
    if not nbytes:
        raise CapnetError("%s: unsupported shape (%s, top_k=%d)" % (who, shape, top_k))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    args = head + ((top_k, top_p) if form else (top_k,)) + (seed, ptr(ws))
    if form or plain_slab:
        slab = splitk_slab(dev)
        args += (ptr(slab), slab.numel())
    _call_sampler(who + form, greedy_stride, *args, *outs, excl=excl)


# ---- exclusions of a sampled decode (csrc/sample_exclude.hip) ----
def mask_words(V):
    """W of the exclusion mask [rows, W]: one bit per word of the vocabulary, 32 to an int32."""
    return (int(V) + 31) // 32


def _check_mask(who, mask, rows, V):
    _need_cuda(mask)
    if mask.dtype != torch.int32 or tuple(mask.shape) != (rows, mask_words(V)) or not mask.is_contiguous():
        raise CapnetError("%s: mask must be a contiguous int32 [rows, ceil(V / 32)] = [%d, %d] tensor" % (who, rows, mask_words(V)))
    return mask


def sample_exclusion_mask(ids, start_tokens, t, V, end_token, constraints, out=None):
    """The exclusion mask of stream step `t` (0-based) of a sampled decode (capnet_sample_exclusion_mask): int32 [rows, ceil(V
    / 32)], bit v & 31 of word v >> 5 of row r set where capnet.beam.banned_words([start_tokens[r]] + ids[r, :t], t + 1,
    end_token, constraints) holds v. ids int64 [rows, steps] with unit column stride (columns from t on are not read);
    start_tokens int64 [rows] or None (the hypotheses are then the words alone); constraints a capnet.beam.Constraints without
    forced words. out: a mask to overwrite."""
    who = "sample_exclusion_mask"
    _need_cuda(ids, start_tokens)
    if ids.dtype != torch.int64 or ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < 1 or (ids.shape[1] > 1 and ids.stride(1) != 1):
        raise CapnetError("%s: ids must be int64 [rows, steps] with unit column stride" % who)
    rows, steps = ids.shape
    ld = ids.stride(0) if rows > 1 else max(steps, ids.stride(0))
    if start_tokens is not None:
        start_tokens = _c(start_tokens)
        if start_tokens.dtype != torch.int64 or start_tokens.numel() != rows:
            raise CapnetError("%s: start_tokens must be int64 [rows]" % who)
    if has_forced(constraints):
        raise CapnetError("%s: forced words have no meaning for a draw" % who)
    t, V = int(t), int(V)
    if not 0 <= t <= steps or not 1 <= steps <= SAMPLE_MAX_STEPS or not 1 <= V <= SAMPLE_MAX_ROWS or ld < steps:
        raise CapnetError("%s: t %d of %d steps (ld %d), V %d" % (who, t, steps, ld, V))
    if out is None:
        out = torch.empty((rows, mask_words(V)), dtype=torch.int32, device=ids.device)
    _check_mask(who, out, rows, V)
    check(_lib.lib().capnet_sample_exclusion_mask(ptr(ids), ld, steps, ptr(start_tokens), rows, t, V, int(end_token),
                                                  *constraint_args(constraints, ids.device), ptr(out), current_stream()),
          "capnet_sample_exclusion_mask")
    return out


def mask_logits(logits, mask):
    """-inf IN PLACE at the mask's set bits of logits float32 [rows, V] (unit column stride; capnet_mask_logits) -> logits: what
    sample_rows, nucleus_rows and a torch.topk in front of the picks then treat as not pickable."""
    _need_cuda(logits)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[0] < 1 or logits.shape[1] < 1 or logits.stride(1) != 1 \
            or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        raise CapnetError("mask_logits: logits float32 [rows, V] with unit column stride")
    rows, V = logits.shape
    mask = _check_mask("mask_logits", mask, rows, V)
    check(_lib.lib().capnet_mask_logits(ptr(logits), rows, logits.stride(0) if rows > 1 else V, V, ptr(mask), current_stream()),
          "capnet_mask_logits")
    return logits


def _exclude_args(who, exclude, end_token, device):
    """The five trailing arguments of the capnet_*_excl entries in front of the stream: end_token and constraint_args."""
    if has_forced(exclude):
        raise CapnetError("%s: forced words have no meaning for a draw" % who)
    if end_token is None:
        raise CapnetError("%s: exclude needs end_token" % who)
    return (int(end_token),) + constraint_args(exclude, device)


def vocab_sample_workspace(rows, V, device):
    """A zeroed workspace of capnet_vocab_sample for `rows` rows (back-to-back calls on one stream may share it)."""
    n = _lib.lib().capnet_vocab_sample_ws_bytes(int(rows), int(V))
    return torch.zeros((n + 7) // 8, dtype=torch.int64, device=device)


def vocab_sample(h, w, b=None, temperature=1.0, seed=0, step=0, row0=0, workspace=None, greedy_stride=0, mask=None):
    """(tokens [rows] int64, logp [rows] float32): per row a draw from softmax((h[r] . w + b) / temperature) and its
    log-probability (capnet_vocab_sample: projection, Gumbel noise and argmax in one launch, no logits in memory). The noise
    of row r and entry v is a function of (seed, step, row0 + r, v) alone (sample_uniform). h [rows, H], w [V, H], b [V]; H
    in DECODE_HIDDEN. A NaN or -inf logit is never drawn; a row with nothing to draw gives (0, -inf).
    greedy_stride g > 0 (here and in sample_pick, sample_rows, nucleus_rows, nucleus_pick): the physical rows row0 + r come
    in groups of g; the last of a group is its greedy row -- no noise: the argmax, ties to the lower index, logp under the
    same distribution -- and row i g + j before it draws on noise row i (g - 1) + j, as in the call without greedy rows.
    mask (sample_exclusion_mask's; capnet_vocab_sample_masked): a word whose bit is set on the row is never drawn and adds
    nothing to the sum under logp -- the draw from the distribution renormalised over the allowed words; None: the calls as
    they were."""
    temperature, _, seed = check_sampling("vocab_sample", temperature, 0, seed)
    greedy_stride = _check_greedy_stride("vocab_sample", greedy_stride)
    _need_cuda(h, w, b)
    h, w = _c(h.detach()), _c(w.detach())
    b = None if b is None else _c(b.detach())
    if h.dim() != 2 or w.dim() != 2:
        raise CapnetError("vocab_sample: h [rows, H], w [V, H]")
    rows, H = h.shape
    V = w.shape[0]
    if w.shape[1] != H or H not in DECODE_HIDDEN or rows < 1 or (b is not None and b.numel() != V):
        raise CapnetError("vocab_sample: h [rows, H], w [V, H], b [V] with H in %r" % (DECODE_HIDDEN,))
    step, row0 = _check_stream_pos("vocab_sample", rows, V, step, row0)
    if workspace is None:
        workspace = vocab_sample_workspace(rows, V, h.device)
    if workspace.numel() * workspace.element_size() < _lib.lib().capnet_vocab_sample_ws_bytes(rows, V):
        raise CapnetError("vocab_sample: workspace too small")
    tokens = torch.empty(rows, dtype=torch.int64, device=h.device)
    logp = torch.empty(rows, dtype=torch.float32, device=h.device)
    if mask is not None:
        mask = _check_mask("vocab_sample", mask, rows, V)
        check(_lib.lib().capnet_vocab_sample_masked(ptr(h), ptr(w), ptr(b), rows, H, V, temperature, seed, step, row0, ptr(mask),
                                                    ptr(workspace), ptr(tokens), ptr(logp), greedy_stride, current_stream()),
              "capnet_vocab_sample_masked")
        return tokens, logp
    _call_sampler("vocab_sample", greedy_stride, ptr(h), ptr(w), ptr(b), rows, H, V, temperature, seed, step, row0, ptr(workspace),
                  ptr(tokens), ptr(logp))
    return tokens, logp


def _draw_pick(who, values, index, V, temperature, top_p, seed, step, row0, greedy_stride):
    """sample_pick (top_p None: capnet_sample_pick) and nucleus_pick (capnet_nucleus_pick)."""
    temperature, _, seed = check_sampling(who, temperature, 0, seed)
    greedy_stride = _check_greedy_stride(who, greedy_stride)
    _need_cuda(values, index)
    values, index = _c(values.detach()), _c(index)
    if values.dim() != 2 or values.shape != index.shape or values.dtype != torch.float32 or index.dtype != torch.int32 \
            or not 1 <= values.shape[1] <= 16 or values.shape[0] < 1:
        raise CapnetError("%s: values float32 [rows, k], index int32 [rows, k], 1 <= k <= 16" % who)
    rows, k = values.shape
    step, row0 = _check_stream_pos(who, rows, int(V), step, row0)
    tokens = torch.empty(rows, dtype=torch.int64, device=values.device)
    logp = torch.empty(rows, dtype=torch.float32, device=values.device)
    _call_sampler(who, greedy_stride, ptr(values), ptr(index), rows, k, int(V), temperature, *(() if top_p is None else (top_p,)),
                  seed, step, row0, ptr(tokens), ptr(logp))
    return tokens, logp


def _draw_rows(who, logits, temperature, top_p, seed, step, row0, greedy_stride):
    """sample_rows (top_p None: capnet_sample_rows) and nucleus_rows (capnet_nucleus_rows)."""
    temperature, _, seed = check_sampling(who, temperature, 0, seed)
    greedy_stride = _check_greedy_stride(who, greedy_stride)
    _need_cuda(logits)
    logits = logits.detach()
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise CapnetError("%s: logits float32 [rows, V]" % who)
    if logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        logits = logits.contiguous()
    rows, V = logits.shape
    step, row0 = _check_stream_pos(who, rows, V, step, row0)
    tokens = torch.empty(rows, dtype=torch.int64, device=logits.device)
    logp = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _call_sampler(who, greedy_stride, ptr(logits), rows, logits.stride(0), V, temperature, *(() if top_p is None else (top_p,)),
                  seed, step, row0, ptr(tokens), ptr(logp))
    return tokens, logp


def sample_pick(values, index, V, temperature=1.0, seed=0, step=0, row0=0, greedy_stride=0):
    """Top-k sampling on vocab_topk's (values, index) [rows, k], k <= 16 (capnet_sample_pick): (tokens [rows] int64, logp
    [rows] float32), the draw among the k candidates with the noise keyed by their vocabulary index and logp renormalised
    over the candidates. Padding slots (-inf, -1) are never drawn."""
    return _draw_pick("sample_pick", values, index, V, temperature, None, seed, step, row0, greedy_stride)


def sample_rows(logits, temperature=1.0, seed=0, step=0, row0=0, greedy_stride=0):
    """vocab_sample's draw from logits [rows, V] in memory (capnet_sample_rows, one workgroup per row): (tokens [rows] int64,
    logp [rows] float32). Any V up to 2^24."""
    return _draw_rows("sample_rows", logits, temperature, None, seed, step, row0, greedy_stride)


def nucleus_rows(logits, temperature=1.0, top_p=1.0, seed=0, step=0, row0=0, greedy_stride=0):
    """sample_rows' draw among the nucleus of every row (capnet_nucleus_rows): the smallest set of best entries -- scaled
    logit descending, index ascending -- whose probability reaches top_p, found exactly by one workgroup per row; logp is
    renormalised over that set. (tokens [rows] int64, logp [rows] float32). top_p == 1.0 is sample_rows itself."""
    temperature, _, seed, top_p = check_sampling("nucleus_rows", temperature, 0, seed, top_p=top_p)
    if top_p == 1.0:
        return sample_rows(logits, temperature, seed, step, row0, greedy_stride)
    return _draw_rows("nucleus_rows", logits, temperature, top_p, seed, step, row0, greedy_stride)


def nucleus_pick(values, index, V, temperature=1.0, top_p=1.0, seed=0, step=0, row0=0, greedy_stride=0):
    """top_k, then top_p (capnet_nucleus_pick): sample_pick's draw among the nucleus of the k candidates (values, index)
    [rows, k], probabilities renormalised over the k and logp over the kept ones; the order of the list does not matter.
    top_p == 1.0 is sample_pick itself."""
    temperature, _, seed, top_p = check_sampling("nucleus_pick", temperature, 0, seed, top_p=top_p)
    if top_p == 1.0:
        return sample_pick(values, index, V, temperature, seed, step, row0, greedy_stride)
    return _draw_pick("nucleus_pick", values, index, V, temperature, top_p, seed, step, row0, greedy_stride)


def sample_decode_supported(E, H, V, top_k=0):
    """The shapes capnet_sample_decode takes: those of its parts (the decode step; capnet_vocab_topk when top_k > 0)."""
    return stacked_decode_supported(E, H) and 1 <= V <= SAMPLE_MAX_ROWS and (top_k == 0 or vocab_topk_supported(H, top_k, V))


def vocab_topk_supported(H, k, V):
    """The shapes capnet_vocab_topk takes (csrc/vocab_topk.hip: vocab_topk_supported)."""
    return H in DECODE_HIDDEN and 1 <= k <= 16 and k <= V


def sample_decode(cell, steps, wcat, beff, emb, Cw, Cb, temperature, top_k, seed, first_inputs=None, start_tokens=None,
                  state=None, top_p=1.0, greedy_stride=0, exclude=None, end_token=None):
    """`steps` sampled decode steps of a plain stack in ONE C call (capnet_sample_decode): per step one decode-step launch
    per layer and the draw (top_k == 0: capnet_vocab_sample; else capnet_vocab_topk + capnet_sample_pick), tokens and logits
    never leaving the device. wcat / beff: capnet.decode.pack_cell(s) of every layer; emb [V, E]; Cw [V, H], Cb [V] or None.
    The first input is first_inputs [rows, E] or emb[start_tokens] (int64 [rows]); state [rows, 2L, H] or None for zeros.
    Row r draws on stream row r, step t on stream step t. top_p < 1: the nucleus draw (capnet_sample_decode_nucleus: per step
    the projection into a logits block + capnet_nucleus_rows, or capnet_vocab_topk + capnet_nucleus_pick); top_p == 1.0 is
    capnet_sample_decode. greedy_stride g > 0 (vocab_sample's; rows a multiple of g): every g-th row decodes greedily, the
    others draw what they draw in the call of g - 1 rows per group without it (the capnet_*_greedy entries).
    exclude (a capnet.beam.Constraints without forced words, with end_token; needs start_tokens): capnet_sample_decode_excl --
    per step one more launch builds the rows' exclusion mask (sample_exclusion_mask's rule on the ids so far) and the draw
    reads it; None: the calls as they were.
    Returns (ids [rows, steps] int64, logp [rows, steps] float32, the final state [rows, 2L, H])."""
    who = "sample_decode"
    if (first_inputs is None) == (start_tokens is None):
        raise CapnetError("%s: either first_inputs or start_tokens" % who)
    rows, steps = (first_inputs if first_inputs is not None else start_tokens).shape[0], int(steps)
    emb, Cw, Cb, state, (V, E, H, nl) = _plain_stack(who, cell, wcat, beff, emb, Cw, Cb, state, rows)
    temperature, top_k, seed, top_p = check_sampling(who, temperature, top_k, seed, V, top_p)
    greedy_stride = _check_greedy_stride(who, greedy_stride, rows)
    _need_cuda(first_inputs, start_tokens)
    if first_inputs is not None:
        first_inputs = _c(first_inputs.detach())
        if tuple(first_inputs.shape) != (rows, E):
            raise CapnetError("%s: first_inputs must be [rows, embed_size]" % who)
    else:
        start_tokens = _c(start_tokens)
        if start_tokens.dtype != torch.int64 or start_tokens.dim() != 1:
            raise CapnetError("%s: start_tokens must be int64 [rows]" % who)
    if not 1 <= steps <= SAMPLE_MAX_STEPS or not 1 <= rows < SAMPLE_MAX_ROWS:
        raise CapnetError("%s: steps %d (1..65535), rows %d (1..2^24 - 1)" % (who, steps, rows))
    if not sample_decode_supported(E, H, V, top_k):
        raise CapnetError("%s: unsupported shape (E=%d, H=%d, V=%d, %d layers, top_k=%d)" % (who, E, H, V, nl, top_k))
    dev = emb.device
    excl = None
    if exclude is not None:
        if start_tokens is None:
            raise CapnetError("%s: exclude needs start_tokens" % who)
        excl = _exclude_args(who, exclude, end_token, dev)
    ids = torch.empty((rows, steps), dtype=torch.int64, device=dev)
    logp = torch.empty((rows, steps), dtype=torch.float32, device=dev)
    out = torch.empty((rows, 2 * nl, H), dtype=torch.float32, device=dev)
    head = (cell, nl, rows, E, H, V, steps, ptr(first_inputs), ptr(start_tokens), ptr(emb), ptr_array(wcat), ptr_array(beff), ptr(Cw),
            ptr(Cb), ptr(state), temperature)
    _call_sampled_loop(who, (nl, rows, H, V), "rows=%d, V=%d" % (rows, V), head, top_k, top_p, seed,
                       (ptr(ids), ptr(logp), ptr(out), ptr(err_flag(dev))), greedy_stride, excl, dev)
    return ids, logp, out


def vocab_topk_groups_workspace(groups, rows_per_group, k, V, device):
    """A zeroed workspace of capnet_vocab_topk_groups (back-to-back calls on one stream may share it)."""
    n = _lib.lib().capnet_vocab_topk_groups_ws_bytes(int(groups), int(rows_per_group), int(k), int(V))
    if not n:
        raise CapnetError("vocab_topk: groups=%d rows=%d k=%d V=%d (1 <= groups <= 8; rows >= 1; 1 <= k <= 16; k <= V)"
                          % (groups, rows_per_group, k, V))
    return torch.zeros((n + 7) // 8, dtype=torch.int64, device=device)


def vocab_topk_groups(h, ws, bs=None, k=5, workspace=None, mask=None, select_only=False):
    """vocab_topk of len(ws) projections in one launch (capnet_vocab_topk_groups): h [groups rows, H], group-major; block g
    on ws[g] [V, H] / bs[g] [V] (bs or any bs[g] None: no bias), each tensor used where it lies. Every block's values, index
    and lse equal vocab_topk of that block alone, bit for bit. mask / select_only (capnet_vocab_topk_groups_masked): vocab_topk's,
    the mask int32 [groups rows, ceil(V / 32)] in the launch's row order.
    Returns (values [groups rows, k] float32, index [groups rows, k] int32, lse [groups rows] float32)."""
    who = "vocab_topk"
    ws = _check_tables(who, ws, _first_shape(ws))
    groups = len(ws)
    _need_cuda(h)
    h = _c(h.detach())
    k = int(k)
    if h.dim() != 2 or ws[0].dim() != 2:
        raise CapnetError("%s: h [groups rows, H], w [V, H] per group" % who)
    rows, H = h.shape
    V = ws[0].shape[0]
    if ws[0].shape[1] != H or H not in DECODE_HIDDEN or rows < groups or rows % groups:
        raise CapnetError("%s: h [groups rows, H], w [V, H] per group with H in %r" % (who, DECODE_HIDDEN))
    if not 1 <= k <= 16 or k > V:
        raise CapnetError("%s: k=%d (1 <= k <= 16, k <= V = %d)" % (who, k, V))
    bs = _group_biases(who, bs, groups, V)
    rpg = rows // groups
    if workspace is None:
        workspace = vocab_topk_groups_workspace(groups, rpg, k, V, h.device)
    if workspace.numel() * workspace.element_size() < _lib.lib().capnet_vocab_topk_groups_ws_bytes(groups, rpg, k, V):
        raise CapnetError("%s: workspace too small" % who)
    values = torch.empty((rows, k), dtype=torch.float32, device=h.device)
    index = torch.empty((rows, k), dtype=torch.int32, device=h.device)
    lse = torch.empty(rows, dtype=torch.float32, device=h.device)
    if select_only and mask is None:
        raise CapnetError("%s: select_only needs a mask" % who)
    if mask is not None:
        mask = _check_mask(who, mask, rows, V)
        check(_lib.lib().capnet_vocab_topk_groups_masked(
            ptr(h), ptr_array(ws), None if bs is None else ptr_array(bs), groups, rpg, H, V, k, ptr(mask), int(bool(select_only)),
            ptr(workspace), ptr(values), ptr(index), ptr(lse), current_stream()), "capnet_vocab_topk_groups_masked")
        return values, index, lse
    check(_lib.lib().capnet_vocab_topk_groups(ptr(h), ptr_array(ws), None if bs is None else ptr_array(bs), groups, rpg, H, V, k,
                                              ptr(workspace), ptr(values), ptr(index), ptr(lse), current_stream()),
          "capnet_vocab_topk_groups")
    return values, index, lse


# ---- what the one-call searches share: operand check, workspace cache, result buffer, reader, epilogue ----------------------
_search_ws = {}       # (the C size function's name, device index, its dims) -> the int64 workspace of a one-call search


def _search_workspace(size_fn, device, dims, outside, teams=None):
    """The cached workspace of a one-call search: one per size function, device and dims, sized by ONE call of
    capnet_<...>_ws_bytes(*dims) when it is first asked for. A size of 0 raises CapnetError(outside).
    teams = (nq, kt, max_steps, rows_tail), the diverse searches -> (ws, the byte offset of its beam state): those bytes,
    FOLLOWED BY the state of nq searches of kt beams (capnet_beam_state_bytes, rounded up to 16) and, with rows_tail,
    4 nq max_steps bytes for the winners' rows -- the layout include/capnet.h gives for the _diverse entries."""
    key = (size_fn, torch.device(device).index or 0, tuple(dims), teams)
    hit = _search_ws.get(key)
    if hit is None:
        base = nbytes = getattr(_lib.lib(), size_fn)(*dims)
        if teams is not None and base:
            nq, kt, max_steps, rows_tail = teams
            state = _lib.lib().capnet_beam_state_bytes(nq, kt, max_steps)
            nbytes = state and base + (state + 15) // 16 * 16 + ((4 * nq * max_steps + 15) // 16 * 16 if rows_tail else 0)
        if not nbytes:
            raise CapnetError(outside)
        hit = _search_ws[key] = (torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device), base)
    return hit[0] if teams is None else hit


def _teams(who, diversity, k, groups):
    """(teams, strength) of a one-call search's `diversity` (a capnet.beam.Diversity whose groups divide k; one weight group)."""
    teams = int(diversity.groups)
    if groups > 1:
        raise CapnetError("%s: diversity takes one weight group" % who)
    if teams < 1 or k % teams:
        raise CapnetError("%s: diversity: %d groups must divide k=%d" % (who, teams, k))
    return teams, float(diversity.strength)


def _tail_words(n):
    """The int64 words behind the n sequences of a result buffer: n int32 lengths and the int32 error word."""
    return n // 2 + 1


def _result_buffer(n, max_steps, device):
    """A search's results as ONE int64 buffer, so that they reach the host in one copy: seqs int64 [n, max_steps + 2] |
    lengths int32 [n] | the error word -> (packed, the address of seqs, the address of lengths)."""
    SL = max_steps + 2
    packed = torch.empty(n * SL + _tail_words(n), dtype=torch.int64, device=device)
    return packed, ptr(packed), C.c_void_p(packed.data_ptr() + 8 * n * SL)


def split_result(host, n):
    """_result_buffer's buffer on the HOST -> (the n token lists, each cut to its length; the lengths; the error word)."""
    SL = (host.numel() - _tail_words(n)) // n
    tail = host[n * SL:].view(torch.int32)
    lens = tail[:n].tolist()
    rows = host[:n * SL].view(n, SL).tolist()
    return [rows[i][:lens[i]] for i in range(n)], lens, int(tail[n])


def _read_result(packed, flag, n):
    """_result_buffer's buffer with the device's error word `flag` copied in, in one copy to the host -> (token lists,
    lengths); a set error word raises (check_device_errors)."""
    packed[-_tail_words(n):].view(torch.int32)[n:n + 1].copy_(flag)
    out, lens, word = split_result(packed.cpu(), n)
    if word:
        check_device_errors()
    return out, lens


def _search_result(ws, beam_at, packed, flag, n, k, max_steps, steps, return_steps, nbest, length_penalty, alphas=None):
    """What a one-call search returns once its C call is issued. The token lists (_read_result), or with nbest the lists of
    (tokens, score) out of the beam state the search left at capnet_beam_decode_ws_beam_offset(*beam_at) of `ws` -- or at the
    byte offset beam_at, where the caller knows it: the diverse searches, n and k then those of the teams'
    searches (_nbest_of_workspace); with return_steps followed by the steps issued; with alphas = (maps [n, max_steps, P], the dims
    of capnet_att_beam_decode_alphas_ws_*_offset) followed by the maps, cut to len - 1 rows -- per caption, or with nbest
    per hypothesis. One value comes back bare, several as a tuple."""
    L = _lib.lib()
    if nbest:
        where = None
        if alphas is not None:
            maps, dims = alphas
            where = (L.capnet_att_beam_decode_alphas_ws_trace_offset(*dims), L.capnet_att_beam_decode_alphas_ws_hist_offset(*dims),
                     maps.shape[2])
        at = beam_at if isinstance(beam_at, int) else L.capnet_beam_decode_ws_beam_offset(*beam_at)
        res = _nbest_of_workspace(ws, at, n, k, max_steps, length_penalty, flag, where)
        res = res if alphas is not None else (res,)
    else:
        out, lens = _read_result(packed, flag, n)
        res = (out,) if alphas is None else (out, [alphas[0][i, :lens[i] - 1] for i in range(n)])
    if return_steps:
        res = (res[0], steps.value) + res[1:]
    return res if len(res) > 1 else res[0]


def _plain_stack(who, cell, wcat, beff, emb, Cw, Cb, state, rows, groups=1):
    """The checked operands of a plain stack's one-call decode -> (emb, Cw, Cb, state, (V, E, H, layers)): the cell kind;
    emb [V, E]; Cw [V, H]; Cb [V] or None; 1 to 8 layers of weights (_check_layer_weights); state [rows, 2L, H] or None.
    Whether the entry takes E, H and V is its caller's to say."""
    if cell not in (CELL_FACTORED, CELL_LSTM):
        raise CapnetError("%s: unknown cell %r" % (who, cell))
    _need_cuda(emb, Cw, Cb, state, *wcat, *beff)
    if emb.dim() != 2 or Cw.dim() != 2:
        raise CapnetError("%s: emb [V, E], Cw [V, H]" % who)
    emb, Cw = _c(emb.detach()), _c(Cw.detach())
    Cb = None if Cb is None else _c(Cb.detach())
    (V, E), H, nl = emb.shape, Cw.shape[1], len(wcat)
    if not 1 <= nl <= 8 or len(beff) != nl or tuple(Cw.shape) != (V, H):
        raise CapnetError("%s: unsupported shape (E=%d, H=%d, V=%d, %d layers, Cw %r)" % (who, E, H, V, nl, tuple(Cw.shape)))
    if Cb is not None and Cb.numel() != V:
        raise CapnetError("%s: Cb must be [V]" % who)
    _check_layer_weights(who, wcat, beff, groups, H, (E + 15) // 16 * 16)
    if state is not None:
        state = _c(state.detach())
        if tuple(state.shape) != (rows, 2 * nl, H):
            raise CapnetError("%s: state must be [rows, 2L, H] = %r" % (who, (rows, 2 * nl, H)))
    return emb, Cw, Cb, state, (V, E, H, nl)


def beam_decode_supported(E, H, k, V, num_layers):
    """The shapes capnet_beam_decode takes: those of its parts (the decode step, capnet_beam_advance)."""
    return stacked_decode_supported(E, H) and 1 <= k <= 16 and k <= V and 1 <= num_layers <= 8


def beam_decode(cell, wcat, beff, emb, Cw, Cb, n, k, max_steps, start_token, end_token, poll_every=0, state=None,
                return_steps=False, groups=1, nbest=False, length_penalty=0.0, constraints=None, diversity=None):
    """The beam search of a plain stack in ONE C call (capnet_beam_decode): n images x k beams, at most max_steps steps of
    (gathered decode step, vocabulary projection on sgemm_splitk's slab, capnet_beam_advance), then capnet_beam_finish.
    cell / wcat / beff: as stacked_decode_step; emb [V, E]; Cw [V, H], Cb [V] or None; state: [n k, 2L, H] or None for
    zeros; poll_every as capnet.beam.beam_search_device. The workspace is cached per (device, shape). Sequences, lengths
    and the device's error word come to the host in one copy; a set error word raises (check_device_errors).
    groups > 1 (capnet_beam_decode_groups): the searches of `groups` weight groups over the n images in the same launches,
    wcat[l] [groups, 4H, kin_l + H], beff[l] [groups, 4H]; state [groups n k, 2L, H]; groups n token lists come back,
    group-major (list g n + i: group g, image i).
    nbest: instead of its winner, every image gives the list of its completed hypotheses as (tokens, score) pairs, best
    first by score / (len(tokens) - 1)^length_penalty (_nbest_of_workspace: capnet_beam_nbest on the state the search left in
    the workspace); the list is empty where nothing completed. The search itself is the same.
    constraints (a capnet.beam.Constraints; capnet_beam_decode_constrained, one weight group): every step selects with
    capnet_beam_advance_constrained; workspace and results as without. With forced words (Constraints(forced=...)):
    capnet_beam_decode_forced, every step selecting with capnet_beam_advance_forced. A capnet.beam.PerImage of n entries:
    capnet_beam_decode_rules, every step selecting with capnet_beam_advance_rules on the object's rule table.
    diversity (a capnet.beam.Diversity whose groups D divide k; capnet_beam_decode_diverse, one weight group; constraints may
    come with it): the diverse search. The result is then the RAW material of capnet.beam.merge_groups: n D lists, one per
    (image, team) in that order, each capnet_beam_nbest's (tokens, score) pairs at length_penalty 0 -- whatever nbest and
    length_penalty say, which are the merge's to apply.
    Returns the n token lists (each starts with start_token); with return_steps, (lists, the steps issued)."""
    who = "beam_decode"
    length_penalty = check_length_penalty(who, nbest, length_penalty)
    groups = _check_groups(who, groups)
    n_img, k, T = int(n), int(k), int(max_steps)
    n = groups * n_img             # the beam groups
    emb, Cw, Cb, state, (V, E, H, nl) = _plain_stack(who, cell, wcat, beff, emb, Cw, Cb, state, n * k, groups)
    if n_img < 1 or T < 1 or not beam_decode_supported(E, H, k, V, nl):
        raise CapnetError("%s: unsupported shape (E=%d, H=%d, V=%d, k=%d, %d layers, n=%d, max_steps=%d)"
                          % (who, E, H, V, k, nl, n_img, T))
    dev = emb.device
    outside = "%s: n=%d k=%d V=%d max_steps=%d outside the limits" % (who, n, k, V, T)
    if constraints is not None and groups > 1:
        raise CapnetError("%s: constraints take one weight group" % who)
    if diversity is not None and is_per_image(constraints):
        raise CapnetError("%s: a PerImage does not go with diversity" % who)
    nq, kq, beam_at = n, k, (nl, n_img, k, H, V, T, 0, groups)     # the searches whose state the call leaves, and where
    if diversity is not None:
        teams, strength = _teams(who, diversity, k, groups)
        nq, kq = n * teams, k // teams
        ws, beam_at = _search_workspace("capnet_beam_decode_ws_bytes", dev, (nl, n, k, H, V, T), outside, (nq, kq, T, False))
    else:
        ws = _search_workspace("capnet_beam_decode_ws_bytes", dev, (nl, n, k, H, V, T), outside)
    slab = splitk_slab(dev)
    packed, seqs, lengths = _result_buffer(nq, T, dev)
    flag = err_flag(dev)
    steps = C.c_int(0)
    args = (E, H, V, T, int(start_token), int(end_token), ptr(emb), ptr_array(wcat), ptr_array(beff), ptr(Cw), ptr(Cb), ptr(state),
            ptr(ws), ptr(slab), slab.numel(), int(poll_every), seqs, lengths, C.byref(steps), ptr(flag), current_stream())
    if diversity is not None:
        name, args = "capnet_beam_decode_diverse", (n, k, teams, strength) + args \
            + (NO_CONSTRAINTS if constraints is None else constraint_args(constraints, dev))
    elif is_per_image(constraints):
        name, args = "capnet_beam_decode_rules", (n, k) + args + rules_arg(who, constraints, n, dev)
    elif has_forced(constraints):
        name, args = "capnet_beam_decode_forced", (n, k) + args + constraint_args(constraints, dev) + forced_args(constraints, dev)
    elif constraints is not None:
        name, args = "capnet_beam_decode_constrained", (n, k) + args + constraint_args(constraints, dev)
    elif groups > 1:
        name, args = "capnet_beam_decode_groups", (groups, n_img, k) + args
    else:
        name, args = "capnet_beam_decode", (n, k) + args
    check(getattr(_lib.lib(), name)(cell, nl, *args), name)
    if diversity is not None:       # the raw material of the merge: every team's list at penalty 0
        nbest, length_penalty = True, 0.0
    return _search_result(ws, beam_at, packed, flag, nq, kq, T, steps, return_steps, nbest, length_penalty)


def lstm_beam_decode_supported(E, H, k, V, num_layers):
    """The shapes capnet_lstm_beam_decode takes, fused top-k or not: those of its parts (the decode step, capnet_vocab_topk,
    capnet_beam_advance)."""
    return beam_decode_supported(E, H, k, V, num_layers)


def _lstm_constrained(who, entry, constraints, fused, device):
    """(the C entry's name, its trailing constraint arguments) of lstm_beam_decode[_groups]: `entry` and none without
    constraints, entry + "_constrained" with constraint_args + forced_args; forced words are refused on the fused step."""
    if constraints is None:
        return entry, ()
    if fused and has_forced(constraints):
        raise CapnetError("%s: forced words take the unfused step (fused_topk=False)" % who)
    return entry + "_constrained", constraint_args(constraints, device) + forced_args(constraints, device)


def lstm_beam_decode(cell, wcat, beff, emb, Cw, Cb, n, k, max_steps, start_token, end_token, first_inputs=None, state=None,
                     fused_topk=True, poll_every=0, return_steps=False, nbest=False, length_penalty=0.0, constraints=None):
    """The beam search of a stack from a given state in ONE C call (capnet_lstm_beam_decode): n sentences x k beams, at most
    max_steps steps, then capnet_beam_finish. fused_topk: a step is (gathered decode step, capnet_vocab_topk,
    capnet_beam_advance_topk) -- no logits in memory; else beam_decode's step (the projection on sgemm_splitk's slab,
    capnet_beam_advance) in the same call. first_inputs [n k, E]: step 1 feeds these rows to layer 0 instead of
    emb[start_token] (EncoderRNN's feature column). state: [n k, 2L, H] or None for zeros. Everything else as beam_decode:
    the workspace is cached per (device, shape); sequences, lengths and the error word come to the host in one copy.
    nbest / length_penalty: as beam_decode's, on either top-k route.
    constraints (a capnet.beam.Constraints; capnet_lstm_beam_decode_constrained): every step selects under them -- unfused with
    capnet_beam_advance_constrained (forced words: capnet_beam_advance_forced); fused (no forced words) through one more launch
    per step, capnet_beam_exclusion_mask, and capnet_vocab_topk_select in capnet_vocab_topk's place. None: the call as it was.
    Returns the n token lists (each starts with start_token); with return_steps, (lists, the steps issued)."""
    who = "lstm_beam_decode"
    length_penalty = check_length_penalty(who, nbest, length_penalty)
    n, k, T, fused = int(n), int(k), int(max_steps), int(bool(fused_topk))
    emb, Cw, Cb, state, (V, E, H, nl) = _plain_stack(who, cell, wcat, beff, emb, Cw, Cb, state, n * k)
    if n < 1 or T < 1 or not lstm_beam_decode_supported(E, H, k, V, nl):
        raise CapnetError("%s: unsupported shape (E=%d, H=%d, V=%d, k=%d, %d layers, n=%d, max_steps=%d)"
                          % (who, E, H, V, k, nl, n, T))
    if first_inputs is not None:
        _need_cuda(first_inputs)
        first_inputs = _c(first_inputs.detach())
        if tuple(first_inputs.shape) != (n * k, E) or first_inputs.dtype != torch.float32:
            raise CapnetError("%s: first_inputs must be float32 [n k, E]" % who)
    dev = emb.device
    name, con = _lstm_constrained(who, "capnet_lstm_beam_decode", constraints, fused, dev)
    ws = _search_workspace(name + "_ws_bytes", dev, (nl, n, k, H, V, T, fused),
                           "%s: n=%d k=%d V=%d max_steps=%d outside the limits" % (who, n, k, V, T))
    slab = None if fused else splitk_slab(dev)
    packed, seqs, lengths = _result_buffer(n, T, dev)
    flag = err_flag(dev)
    steps = C.c_int(0)
    check(getattr(_lib.lib(), name)(cell, nl, n, k, E, H, V, T, int(start_token), int(end_token), ptr(first_inputs),
                                    ptr(emb), ptr_array(wcat), ptr_array(beff), ptr(Cw), ptr(Cb), ptr(state), ptr(ws),
                                    ptr(slab), 0 if slab is None else slab.numel(), fused, int(poll_every), seqs, lengths,
                                    C.byref(steps), ptr(flag), current_stream(), *con), name)
    return _search_result(ws, (nl, n, k, H, V, T, fused, 1), packed, flag, n, k, T, steps, return_steps, nbest, length_penalty)


def lstm_beam_decode_groups(cell, wcat, beff, embs, Cws, Cbs, n, k, max_steps, start_token, end_token, state=None,
                            fused_topk=True, poll_every=0, return_steps=False, nbest=False, length_penalty=0.0, constraints=None):
    """lstm_beam_decode of len(embs) decoders in ONE C call (capnet_lstm_beam_decode_groups): groups x n sentences x k beams,
    group-major, group g on embs[g] [V, E], wcat[l][g] / beff[l][g] and Cws[g] [V, H] / Cbs[g] [V] (Cbs or any Cbs[g] None:
    no bias). The embeddings and projections are used where they lie (one pointer per group; nothing is stacked or copied);
    wcat[l] [groups, 4H, kin_l + H] and beff[l] [groups, 4H] are capnet.decode.pack_cell of every decoder's layer l, stacked
    as for lstm_greedy_decode_groups. Per step one gathered decode-step launch per layer on a (H / 4, groups) grid, then
    fused_topk: one capnet_vocab_topk_groups launch and one capnet_beam_advance_topk; else one sgemm_splitk per group into
    its row block of the logits and one capnet_beam_advance. There are no first_inputs. state: [groups n k, 2L, H] or None
    for zeros. Everything else as lstm_beam_decode, nbest / length_penalty and constraints
    (capnet_lstm_beam_decode_groups_constrained: the same constraints on every group) included.
    Returns the groups n token lists, group-major (list g n + i: group g, sentence i); with return_steps, (lists, the steps
    issued)."""
    who = "lstm_beam_decode_groups"
    if cell not in (CELL_FACTORED, CELL_LSTM):
        raise CapnetError("%s: unknown cell %r" % (who, cell))
    length_penalty = check_length_penalty(who, nbest, length_penalty)
    embs = _check_tables(who, embs, _first_shape(embs))
    groups = len(embs)
    Cws = list(Cws)
    if embs[0].dim() != 2 or not Cws or Cws[0] is None or Cws[0].dim() != 2:
        raise CapnetError("%s: emb [V, E] and Cw [V, H] per group" % who)
    V, E = embs[0].shape
    H, nl = Cws[0].shape[1], len(wcat)
    Cws = _check_tables(who, Cws, (V, H), groups)
    Cbs = _group_biases(who, Cbs, groups, V)
    _need_cuda(state, *wcat, *beff)
    n, k, T, fused = int(n), int(k), int(max_steps), int(bool(fused_topk))
    if n < 1 or T < 1 or len(beff) != nl or not lstm_beam_decode_supported(E, H, k, V, nl):
        raise CapnetError("%s: unsupported shape (E=%d, H=%d, V=%d, k=%d, %d layers, n=%d, max_steps=%d)"
                          % (who, E, H, V, k, nl, n, T))
    wcat, beff = _grouped_layer_weights(who, wcat, beff, groups, H, (E + 15) // 16 * 16)
    dev = embs[0].device
    nq = groups * n
    if state is not None:
        state = _c(state.detach())
        if tuple(state.shape) != (nq * k, 2 * nl, H):
            raise CapnetError("%s: state must be [groups n k, 2L, H]" % who)
    name, con = _lstm_constrained(who, "capnet_lstm_beam_decode_groups", constraints, fused, dev)
    ws = _search_workspace(name + "_ws_bytes", dev, (nl, groups, n, k, H, V, T, fused),
                           "%s: groups=%d n=%d k=%d V=%d max_steps=%d outside the limits" % (who, groups, n, k, V, T))
    slab = None if fused else splitk_slab(dev)
    packed, seqs, lengths = _result_buffer(nq, T, dev)
    flag = err_flag(dev)
    steps = C.c_int(0)
    check(getattr(_lib.lib(), name)(
        cell, nl, groups, n, k, E, H, V, T, int(start_token), int(end_token), ptr_array(embs), ptr_array(wcat), ptr_array(beff),
        ptr_array(Cws), None if Cbs is None else ptr_array(Cbs), ptr(state), ptr(ws), ptr(slab),
        0 if slab is None else slab.numel(), fused, int(poll_every), seqs, lengths, C.byref(steps), ptr(flag), current_stream(),
        *con), name)
    return _search_result(ws, (nl, n, k, H, V, T, fused, groups), packed, flag, nq, k, T, steps, return_steps, nbest,
                          length_penalty)


def att_decode_supported(E, Cdim, H, A, P, k, num_layers):
    """The shapes capnet_att_decode_step / capnet_att_beam_decode take (capnet_att_decode_supported)."""
    return bool(_lib.lib().capnet_att_decode_supported(int(E), int(Cdim), int(H), int(A), int(P), int(k), int(num_layers)))


def _att_decode_args(who, cell, att1, feat, k, emb, wz, bz, w_full, b_full, wcat, beff, state, groups=1):
    """The checked operands the two attention-decode calls share -> (tensors..., dims n, P, A, Cdim, E, H, V, nl); n counts
    the images. groups > 1: att1 [groups n, P, A], feat [n, P, C], wz [groups, A + C, H], bz [groups, A + C], w_full
    [groups, A], b_full [groups], the layers' weights with a leading [groups], state [groups n k, 2L, H]."""
    if cell not in (CELL_FACTORED, CELL_LSTM):
        raise CapnetError("%s: unknown cell %r" % (who, cell))
    _need_cuda(att1, feat, emb, wz, bz, w_full, b_full, state, *wcat, *beff)
    att1, feat, emb, wz, bz = _c(att1.detach()), _c(feat.detach()), _c(emb.detach()), _c(wz.detach()), _c(bz.detach())
    wf, bf = _c(w_full.detach()).reshape(-1), _c(b_full.detach()).reshape(-1)
    state = _c(state.detach())
    nq, P, A = att1.shape
    n = feat.shape[0]
    Cdim, (V, E), nl, k = feat.shape[2], emb.shape, len(wcat), int(k)
    H = state.shape[2]
    lead = () if groups == 1 else (groups,)
    if nq != groups * n or feat.shape[1] != P or tuple(wz.shape) != lead + (A + Cdim, H) or bz.numel() != groups * (A + Cdim) \
            or wf.numel() != groups * A or bf.numel() != groups:
        raise CapnetError("%s: att1 [n, P, A], feat [n, P, C], wz [A + C, H], bz [A + C], w_full [A]%s"
                          % (who, " (groups: att1 [groups n, P, A], [groups] in front of wz, bz, w_full, b_full)" if lead else ""))
    if len(beff) != nl or k < 1 or tuple(state.shape) != (nq * k, 2 * nl, H) or not att_decode_supported(E, Cdim, H, A, P, k, nl):
        raise CapnetError("%s: unsupported shape (E=%d, C=%d, H=%d, A=%d, P=%d, k=%d, %d layers, state %r)"
                          % (who, E, Cdim, H, A, P, k, nl, tuple(state.shape)))
    _check_layer_weights(who, wcat, beff, groups, H, (E + Cdim + 15) // 16 * 16)
    return att1, feat, emb, wz, bz, wf, bf, state, (n, P, A, Cdim, E, H, V, nl)


def att_decode_step_workspace(n, k, P, A, Cdim, E, device):
    """float32 workspace of capnet_att_decode_step: z [n k, A + C] first, then xa and the raw scores."""
    return torch.empty(_lib.lib().capnet_att_decode_step_ws_bytes(n, k, P, A, Cdim, E) // 4, dtype=torch.float32, device=device)


def att_decode_step(att1, feat, k, tokens, emb, wz, bz, w_full, b_full, wcat, beff, state, cell=CELL_FACTORED, parent_rows=None,
                    workspace=None, groups=1, alphas=None):
    """One beam step of an attention decoder without the projection (capnet_att_decode_step): n images x k fixed slots, row
    r on the maps of image r // k. att1 [n, P, A] = encoder_att(feat), feat [n, P, C]: per image, never per row. wz [A + C,
    H] / bz = [decoder_att; f_beta]; w_full / b_full: full_att; wcat / beff: capnet.decode.pack_cell / fold_factored per
    layer, layer 0 reading E + C columns; state [n k, 2L, H]; tokens int64 [n k]; parent_rows int64 [n k]: the step on
    state.index_select(0, parent_rows) without that copy. workspace: att_decode_step_workspace(...) or None.
    groups > 1 (capnet_att_decode_step_groups): `groups` weight groups on the same n images, operands as _att_decode_args
    says, workspace att_decode_step_workspace(groups n, ...); each group's rows equal the step of that group alone.
    alphas: a contiguous float32 [groups n k, P] tensor that receives every row's attention map
    (capnet_att_decode_step_alphas); the state and the top h are those of the call without it, bit for bit.
    Returns (top-layer h [n k, H], the new state)."""
    groups = _check_groups("att_decode_step", groups)
    att1, feat, emb, wz, bz, wf, bf, state, (n, P, A, Cdim, E, H, V, nl) = _att_decode_args(
        "att_decode_step", cell, att1, feat, k, emb, wz, bz, w_full, b_full, wcat, beff, state, groups)
    rows, dev = groups * n * int(k), state.device
    _need_cuda(tokens, parent_rows, workspace)
    for name, idx in (("tokens", tokens), ("parent_rows", parent_rows)):
        if idx is not None and (idx.dtype != torch.int64 or idx.numel() != rows or not idx.is_contiguous()):
            raise CapnetError("att_decode_step: %s must be contiguous int64 [n k]" % name)
    if tokens is None:
        raise CapnetError("att_decode_step: tokens are required")
    L = _lib.lib()
    if workspace is None:
        workspace = att_decode_step_workspace(groups * n, int(k), P, A, Cdim, E, dev)
    if workspace.dtype != torch.float32 or not workspace.is_contiguous() or \
            workspace.numel() * 4 < L.capnet_att_decode_step_ws_bytes(groups * n, int(k), P, A, Cdim, E):
        raise CapnetError("att_decode_step: workspace too small")
    slab = splitk_slab(dev)
    out = torch.empty_like(state)
    top = torch.empty((rows, H), dtype=torch.float32, device=dev)
    args = (n, int(k), P, A, Cdim, E, H, V, ptr(att1), ptr(feat), ptr(tokens), ptr(emb), ptr(wz), ptr(bz), ptr(wf), ptr(bf),
            ptr_array(wcat), ptr_array(beff), ptr(state), ptr(parent_rows), ptr(out), ptr(top), ptr(workspace), ptr(slab),
            slab.numel(), ptr(err_flag(dev)), current_stream())
    if alphas is not None:
        _need_cuda(alphas)
        if alphas.dtype != torch.float32 or tuple(alphas.shape) != (rows, P) or not alphas.is_contiguous():
            raise CapnetError("att_decode_step: alphas must be a contiguous float32 [n k, P] tensor")
        check(L.capnet_att_decode_step_alphas(cell, nl, groups, *args, ptr(alphas)), "capnet_att_decode_step_alphas")
    elif groups > 1:
        check(L.capnet_att_decode_step_groups(cell, nl, groups, *args), "capnet_att_decode_step_groups")
    else:
        check(L.capnet_att_decode_step(cell, nl, *args), "capnet_att_decode_step")
    return top, out


def att_beam_decode(cell, att1, feat, emb, wz, bz, w_full, b_full, wcat, beff, Cw, Cb, state, k, max_steps, start_token,
                    end_token, poll_every=0, return_steps=False, groups=1, return_alphas=False, nbest=False,
                    length_penalty=0.0, constraints=None, diversity=None):
    """The beam search of an attention decoder in ONE C call (capnet_att_beam_decode): n images x k beams, at most max_steps
    steps of (att_decode_step's step, vocabulary projection on sgemm_splitk's slab, capnet_beam_advance), then
    capnet_beam_finish. Operands as att_decode_step; Cw [V, H], Cb [V] or None; state [n k, 2L, H]: the initial state
    (init_h / init_c per layer and image, each image's row k times). The workspace is cached per (device, shape).
    Sequences, lengths and the device's error word come to the host in one copy; a set error word raises
    (check_device_errors). groups > 1 (capnet_att_beam_decode_groups): the searches of `groups` weight groups over the same n
    images in the same launches, operands as att_decode_step's; groups n token lists come back, group-major.
    return_alphas (capnet_att_beam_decode_alphas): the search also records its attention maps -- every step's maps into a
    history, the winners' rows through the re-slotting, one gather at the end; the maps stay on the device. The token
    lists are those of the call without it.
    nbest / length_penalty: as beam_decode's; with return_alphas every hypothesis has its own maps (capnet_beam_nbest_traced's
    rows, one capnet_alpha_gather over all n k hypotheses): per image a list of float32 [len - 1, P] tensors beside its list
    of (tokens, score) pairs.
    constraints (a capnet.beam.Constraints; capnet_att_beam_decode_constrained / capnet_att_beam_decode_alphas_constrained, one
    weight group): every step selects with capnet_beam_advance_constrained; workspaces and results as without. With forced
    words (Constraints(forced=...)): capnet_att_beam_decode_forced, with or without the maps. A capnet.beam.PerImage with an
    entry per image: capnet_att_beam_decode_rules on the object's rule table, with or without the maps.
    diversity (capnet_att_beam_decode_diverse, one weight group; constraints may come with it): as beam_decode's -- the
    result is n D lists of (tokens, score), one per (image, team), capnet_beam_nbest's at length_penalty 0; with
    return_alphas followed by the maps of every hypothesis in the same nesting.
    Returns the n token lists; with return_steps, (lists, the steps issued); with return_alphas the lists are followed by
    the list of n float32 [len - 1, P] tensors: row e - 1 is the map that preceded word e."""
    groups = _check_groups("att_beam_decode", groups)
    length_penalty = check_length_penalty("att_beam_decode", nbest, length_penalty)
    att1, feat, emb, wz, bz, wf, bf, state, (n, P, A, Cdim, E, H, V, nl) = _att_decode_args(
        "att_beam_decode", cell, att1, feat, k, emb, wz, bz, w_full, b_full, wcat, beff, state, groups)
    _need_cuda(Cw, Cb)
    Cw = _c(Cw.detach())
    Cb = None if Cb is None else _c(Cb.detach())
    k, T = int(k), int(max_steps)
    if T < 1 or k > V or tuple(Cw.shape) != (V, H) or (Cb is not None and Cb.numel() != V):
        raise CapnetError("att_beam_decode: Cw [V, H], Cb [V], k <= V, max_steps >= 1 (V=%d, k=%d, max_steps=%d)" % (V, k, T))
    dev = emb.device
    n_img, n = n, groups * n       # from here on n counts the beam groups
    outside = "att_beam_decode: n=%d k=%d V=%d max_steps=%d outside the limits" % (n, k, V, T)
    if constraints is not None and groups > 1:
        raise CapnetError("att_beam_decode: constraints take one weight group")
    per_image = is_per_image(constraints)
    if diversity is not None and per_image:
        raise CapnetError("att_beam_decode: a PerImage does not go with diversity")
    alpha_dims = (nl, groups, n_img, k, P, A, Cdim, E, H, V, T)
    size = ("capnet_att_beam_decode_alphas_ws_bytes", dev, alpha_dims, outside) if return_alphas else \
        ("capnet_att_beam_decode_ws_bytes", dev, (nl, n, k, P, A, Cdim, E, H, V, T), outside)
    nq, kq, beam_at = n, k, (nl, n, k, H, V, T, 0, 1)     # the searches whose state the call leaves, and where
    if diversity is not None:
        teams, strength = _teams("att_beam_decode", diversity, k, groups)
        nq, kq = n * teams, k // teams
        ws, beam_at = _search_workspace(*size, (nq, kq, T, return_alphas))
    else:
        ws = _search_workspace(*size)
    slab = splitk_slab(dev)
    packed, seqs, lengths = _result_buffer(nq, T, dev)
    flag = err_flag(dev)
    steps = C.c_int(0)
    alphas = (torch.empty((nq, T, P), dtype=torch.float32, device=dev), alpha_dims) if return_alphas else None
    maps = (ptr(alphas[0]) if alphas else None,)
    con = () if constraints is None or per_image else constraint_args(constraints, dev)
    args = (P, A, Cdim, E, H, V, T, int(start_token), int(end_token), ptr(att1), ptr(feat), ptr(emb), ptr(wz), ptr(bz), ptr(wf),
            ptr(bf), ptr_array(wcat), ptr_array(beff), ptr(Cw), ptr(Cb), ptr(state), ptr(ws), ptr(slab), slab.numel(),
            int(poll_every), seqs, lengths, C.byref(steps), ptr(flag), current_stream())
    if diversity is not None:       # one entry, the maps nullable
        name, args = "capnet_att_beam_decode_diverse", (n, k, teams, strength) + args + maps + (con or NO_CONSTRAINTS)
    elif per_image:                 # one entry, the maps nullable
        name, args = "capnet_att_beam_decode_rules", (n_img, k) + args + maps + rules_arg("att_beam_decode", constraints, n_img, dev)
    elif has_forced(constraints):   # one entry, the maps nullable
        name, args = "capnet_att_beam_decode_forced", (n_img, k) + args + maps + con + forced_args(constraints, dev)
    elif return_alphas:
        name, args = ("capnet_att_beam_decode_alphas_constrained", (n_img, k) + args + maps + con) if con else \
            ("capnet_att_beam_decode_alphas", (groups, n_img, k) + args + maps)
    elif con:
        name, args = "capnet_att_beam_decode_constrained", (n_img, k) + args + con
    elif groups > 1:
        name, args = "capnet_att_beam_decode_groups", (groups, n_img, k) + args
    else:
        name, args = "capnet_att_beam_decode", (n_img, k) + args
    check(getattr(_lib.lib(), name)(cell, nl, *args), name)
    if diversity is not None:       # the raw material of the merge: every team's list at penalty 0
        nbest, length_penalty = True, 0.0
    return _search_result(ws, beam_at, packed, flag, nq, kq, T, steps, return_steps, nbest, length_penalty, alphas)


def att_sample_decode(cell, att1, feat, emb, wz, bz, w_full, b_full, wcat, beff, Cw, Cb, state, m, steps, start_token,
                      temperature, top_k, seed, top_p=1.0, greedy=False, exclude=None, end_token=None):
    """`steps` sampled decode steps of an attention decoder in ONE C call (capnet_att_sample_decode; top_p < 1:
    capnet_att_sample_decode_nucleus, the draw as ops.sample_decode's): n images x m samples
    each (row i m + j = sample j of image i), the step att_decode_step's with k = m and every row continuing from itself --
    an image's maps are read once per step for all its samples -- then the draw as ops.sample_decode's. Operands as
    att_beam_decode; state [n m, 2L, H]: the initial state. Returns (ids [n m, steps] int64, logp [n m, steps] float32).
    greedy: the last of an image's m rows decodes greedily (greedy_stride = m, ops.vocab_sample's) and the m - 1 before it draw
    what the call with m - 1 rows per image draws: the greedy caption on the same read of the maps. m <= 16 either way.
    exclude / end_token: ops.sample_decode's (capnet_att_sample_decode_excl); None: the calls as they were."""
    who = "att_sample_decode"
    att1, feat, emb, wz, bz, wf, bf, state, (n, P, A, Cdim, E, H, V, nl) = _att_decode_args(
        who, cell, att1, feat, m, emb, wz, bz, w_full, b_full, wcat, beff, state)
    temperature, top_k, seed, top_p = check_sampling(who, temperature, top_k, seed, V, top_p)
    _need_cuda(Cw, Cb)
    Cw = _c(Cw.detach())
    Cb = None if Cb is None else _c(Cb.detach())
    m, steps = int(m), int(steps)
    if not 1 <= steps <= SAMPLE_MAX_STEPS or tuple(Cw.shape) != (V, H) or (Cb is not None and Cb.numel() != V):
        raise CapnetError("%s: Cw [V, H], Cb [V], 1 <= steps <= 65535 (V=%d, steps=%d)" % (who, V, steps))
    dev, rows = emb.device, n * m
    excl = None if exclude is None else _exclude_args(who, exclude, end_token, dev)
    tokens = torch.full((rows,), int(start_token), dtype=torch.int64, device=dev)
    ids = torch.empty((rows, steps), dtype=torch.int64, device=dev)
    logp = torch.empty((rows, steps), dtype=torch.float32, device=dev)
    head = (cell, nl, n, m, P, A, Cdim, E, H, V, steps, ptr(tokens), ptr(att1), ptr(feat), ptr(emb), ptr(wz), ptr(bz), ptr(wf), ptr(bf),
            ptr_array(wcat), ptr_array(beff), ptr(Cw), ptr(Cb), ptr(state), temperature)
    _call_sampled_loop(who, (nl, n, m, P, A, Cdim, E, H, V), "n=%d, m=%d, V=%d" % (n, m, V), head, top_k, top_p, seed,
                       (ptr(ids), ptr(logp), None, ptr(err_flag(dev))), m if greedy else 0, excl, dev, plain_slab=True)
    return ids, logp


def packed_targets(captions, lengths):
    """pack_padded_sequence(captions, lengths, batch_first=True)[0] for int64 captions."""
    _need_cuda(captions)
    captions = _c(captions)
    bs = batch_sizes_from_lengths(lengths)
    if bs[0] != captions.shape[0] or len(bs) > captions.shape[1]:
        raise CapnetError("packed_targets: lengths do not match captions %s" % (tuple(captions.shape),))
    out = torch.empty(sum(bs), dtype=torch.int64, device=captions.device)
    check(_lib.lib().capnet_packed_targets(ptr(captions), captions.shape[1], len(bs), int_array(bs),
                                           ptr(out), current_stream()), "capnet_packed_targets")
    return out


def pack_tensors(tensors, flat, unpack=False, scale=1.0):
    """Gather `tensors` into `flat` (or scatter back, scaled)."""
    n = len(tensors)
    if n == 0:
        return
    _need_cuda(flat, *tensors)
    numel = (C.c_long * n)(*[t.numel() for t in tensors])
    if sum(t.numel() for t in tensors) > flat.numel():
        raise CapnetError("pack_tensors: flat buffer too small")
    for t in tensors:
        if not t.is_contiguous():
            raise CapnetError("pack_tensors: tensors must be contiguous")
    check(_lib.lib().capnet_pack_tensors(n, ptr_array(tensors), numel, ptr(flat), int(unpack),
                                         float(scale), current_stream()), "capnet_pack_tensors")


def pack_conv_weight(w_oihw, row_stride, kmajor=False):
    """OIHW -> [Cout][row_stride] rows, or (kmajor) the K-major [row_stride][Cout] image."""
    _need_cuda(w_oihw)
    w = _c(w_oihw)
    co, ci, kh, kw = w.shape
    if kmajor:
        out = torch.empty((row_stride, co), dtype=torch.float32, device=w.device)
        check(_lib.lib().capnet_pack_conv_weight_kmajor(ptr(w), ptr(out), co, ci, kh, kw, row_stride,
                                                        current_stream()), "capnet_pack_conv_weight_kmajor")
        return out
    out = torch.empty((co, row_stride), dtype=torch.float32, device=w.device)
    check(_lib.lib().capnet_pack_conv_weight(ptr(w), ptr(out), co, ci, kh, kw, row_stride,
                                             current_stream()), "capnet_pack_conv_weight")
    return out


def pack_conv_weight_f16x3(w_oihw, bn):
    """1x1 or 3x3 OIHW weights -> header + the split-f16 image of capnet_conv2d_fwd_f16x3 for tile width bn
    (two f16 pieces per weight scaled by the per-tensor power of two in the header, laid out as the
    kernel's LDS image, k = (tap, channel))."""
    _need_cuda(w_oihw)
    w = _c(w_oihw)
    co, ci, kh, kw = w.shape
    if (kh, kw) not in ((1, 1), (3, 3)):
        raise CapnetError("pack_conv_weight_f16x3: 1x1 or 3x3 weights only")
    out = torch.empty(_lib.lib().capnet_conv_f16x3_weight_words(ci, co, kh), dtype=torch.int32, device=w.device)
    check(_lib.lib().capnet_conv_f16x3_pack(ptr(w), ptr(out), co, ci, kh, int(bn), current_stream()),
          "capnet_conv_f16x3_pack")
    return out


def pack_fused_block_weight(w_oihw, role):
    """1x1 OIHW weights -> the image of capnet_fused_block_forward: role 0 = conv3 of a bottleneck ([C][MID][1][1]),
    role 1 = the next block's conv1 ([MID][C][1][1])."""
    _need_cuda(w_oihw)
    w = _c(w_oihw)
    co, ci = w.shape[0], w.shape[1]
    cc, mid = (co, ci) if role == 0 else (ci, co)
    if tuple(w.shape[2:]) != (1, 1) or cc != 4 * mid:
        raise CapnetError("pack_fused_block_weight: role %d expects a 1x1 convolution between MID and 4 MID channels" % role)
    out = torch.empty(_lib.lib().capnet_fused_block_weight_words(cc, mid, role), dtype=torch.int32, device=w.device)
    check(_lib.lib().capnet_fused_block_pack(ptr(w), ptr(out), cc, mid, role, current_stream()), "capnet_fused_block_pack")
    return out


def fused_block_stats(y2, s2, t2, w3img, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, in_exp=0):
    """(scale, shift) of bn3 behind conv3(relu(y2 s2 + t2)) without forming conv3's output (capnet_fused_block_stats)."""
    _need_cuda(y2, s2, t2, w3img, gamma, beta, running_mean, running_var)
    M, mid = y2.shape
    work = torch.empty(_lib.lib().capnet_fused_block_stats_floats(M, mid), dtype=torch.float32, device=y2.device)
    scale = torch.empty(4 * mid, dtype=torch.float32, device=y2.device)
    shift = torch.empty_like(scale)
    check(_lib.lib().capnet_fused_block_stats(ptr(y2), ptr(s2), ptr(t2), ptr(w3img), M, mid, in_exp, ptr(gamma), ptr(beta),
                                              ptr(running_mean), ptr(running_var), momentum, eps, ptr(scale), ptr(shift),
                                              ptr(work), ptr(err_flag(y2.device)), current_stream()), "capnet_fused_block_stats")
    return scale, shift


def fused_block_forward(y2, s2, t2, w3img, s3, t3, res, w1img, sd=None, td=None, stats=True, e3=0, e1=0):
    """-> (out [M, 4 MID], y1 [M, MID], part_sum, part_sq) (capnet_fused_block_forward)."""
    _need_cuda(y2, s2, t2, w3img, s3, t3, res, w1img, sd, td)
    M, mid = y2.shape
    dev = y2.device
    out = torch.empty(M, 4 * mid, dtype=torch.float32, device=dev)
    y1 = torch.empty(M, mid, dtype=torch.float32, device=dev)
    tiles = _lib.lib().capnet_fused_block_tiles(M, mid)
    ps = torch.empty(tiles, mid, dtype=torch.float32, device=dev) if stats else None
    pq = torch.empty(tiles, mid, dtype=torch.float32, device=dev) if stats else None
    check(_lib.lib().capnet_fused_block_forward(ptr(y2), ptr(s2), ptr(t2), ptr(w3img), ptr(s3), ptr(t3), ptr(res), ptr(sd),
                                                ptr(td), ptr(out), ptr(w1img), ptr(y1), ptr(ps), ptr(pq), M, mid, e3, e1,
                                                ptr(err_flag(dev)), current_stream()), "capnet_fused_block_forward")
    return out, y1, ps, pq


def pack_conv_weight_stem_f16x3(w_oihw):
    """The stem's OIHW weights [64][3][7][7] -> header + the split-f16 image of capnet_conv_stem_fwd_f16x3."""
    _need_cuda(w_oihw)
    w = _c(w_oihw)
    if tuple(w.shape) != (64, 3, 7, 7):
        raise CapnetError("pack_conv_weight_stem_f16x3: weights must be [64][3][7][7]")
    out = torch.empty(_lib.lib().capnet_conv_stem_f16x3_weight_words(), dtype=torch.int32, device=w.device)
    check(_lib.lib().capnet_conv_stem_f16x3_pack(ptr(w), ptr(out), current_stream()), "capnet_conv_stem_f16x3_pack")
    return out


def clamp_adam(params, grads, exp_avg, exp_avg_sq, steps, lr, beta1, beta2, eps, clip,
               write_grad=True):
    """Fused element-wise clamp + Adam over a list of tensors (in place); a no-op on the device while the
    device's error word is set (check_device_errors)."""
    n = len(params)
    if n == 0:
        return
    _need_cuda(*params, *grads, *exp_avg, *exp_avg_sq)
    for p, g in zip(params, grads):
        if not (p.is_contiguous() and g.is_contiguous()) or p.numel() != g.numel():
            raise CapnetError("clamp_adam: parameters and gradients must be contiguous and equal-sized")
    numel = (C.c_long * n)(*[p.numel() for p in params])
    check(_lib.lib().capnet_clamp_adam(n, ptr_array(params), ptr_array(grads), ptr_array(exp_avg),
                                       ptr_array(exp_avg_sq), numel, int_array(steps), lr, beta1,
                                       beta2, eps, clip if clip else 0.0, int(write_grad),
                                       ptr(err_flag(params[0].device)), current_stream()), "capnet_clamp_adam")


# ---------------------------------------------------------------------------------------
# autograd: nn.Linear
# ---------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    """y = x @ w.T + b   (x [M,K], w [N,K])."""

    @staticmethod
    def forward(ctx, x, w, b):
        _need_cuda(x, w, b)
        x, w = _c(x), _c(w)
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        # (through the K-split entry: the encoder head's 64 x 300 x 2048 is five 64 x 64 tiles walking the whole K on the
        #  plain one -- 94 us; large products go to the same kernels either way)
        return sgemm_splitk(x, w, transB=True, bias=b)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = sgemm_splitk(dy, w)               # [M,N] @ [N,K]; K-split when N (vocab) is long
        if ctx.needs_input_grad[1]:
            dw = sgemm(dy, x, transA=True)         # dy^T [N,M] @ x [M,K]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = colsum(dy)
        return dx, dw, db


def linear(x, w, b=None):
    return LinearFn.apply(x, w, b)


# ---------------------------------------------------------------------------------------
# autograd: nn.CrossEntropyLoss (mean)
# ---------------------------------------------------------------------------------------
class CrossEntropyFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, targets):
        _need_cuda(logits, targets)
        logits, targets = _c(logits), _c(targets)
        if targets.dtype != torch.int64:
            raise CapnetError("targets must be int64")
        n, v = logits.shape
        if targets.numel() != n:
            raise CapnetError("cross entropy: %d logits rows vs %d targets" % (n, targets.numel()))
        lse = torch.empty(n, dtype=torch.float32, device=logits.device)
        row_loss = torch.empty(n, dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        check(_lib.lib().capnet_xent_fwd(ptr(logits), v, n, v, ptr(targets), ptr(lse),
                                         ptr(row_loss), ptr(loss), ptr(err_flag(logits.device)),
                                         current_stream()), "capnet_xent_fwd")
        ctx.save_for_backward(logits, targets, lse)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        logits, targets, lse = ctx.saved_tensors
        n, v = logits.shape
        gout = _c(gout.to(torch.float32)).reshape(1)
        dlogits = torch.empty_like(logits)
        check(_lib.lib().capnet_xent_bwd(ptr(logits), v, n, v, ptr(targets), ptr(lse), ptr(gout),
                                         ptr(dlogits), v, current_stream()), "capnet_xent_bwd")
        return dlogits, None


def cross_entropy(logits, targets):
    return CrossEntropyFn.apply(logits, targets)


class PolicyLossFn(torch.autograd.Function):
    """-(1/N) sum_i advantages[cap(i)] * log p(target_i) over packed rows (capnet_policy_xent_fwd / _bwd): the loss of a
    policy-gradient step on sampled captions. The gradient goes to the logits only."""

    @staticmethod
    def forward(ctx, logits, targets, advantages, batch_sizes):
        _need_cuda(logits, targets, advantages)
        logits, targets, advantages = _c(logits), _c(targets), _c(advantages)
        if targets.dtype != torch.int64 or advantages.dtype != torch.float32:
            raise CapnetError("policy loss: targets must be int64 and advantages float32")
        n, v = logits.shape
        bs = [int(b) for b in batch_sizes]
        if targets.numel() != n or sum(bs) != n or not bs or advantages.numel() != bs[0]:
            raise CapnetError("policy loss: %d logits rows, %d targets, %d advantages, batch_sizes summing to %d from %d"
                              % (n, targets.numel(), advantages.numel(), sum(bs), bs[0] if bs else 0))
        dev = logits.device
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        row_logp = torch.empty(n, dtype=torch.float32, device=dev)
        caption_logp = torch.empty(bs[0], dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        check(_lib.lib().capnet_policy_xent_fwd(ptr(logits), v, n, v, ptr(targets), ptr(advantages), bs[0], int_array(bs),
                                                len(bs), ptr(lse), ptr(row_logp), ptr(caption_logp), ptr(loss),
                                                ptr(err_flag(dev)), current_stream()), "capnet_policy_xent_fwd")
        ctx.save_for_backward(logits, targets, lse, advantages)
        ctx.batch_sizes = bs
        ctx.mark_non_differentiable(caption_logp)
        return loss, caption_logp

    @staticmethod
    @once_differentiable
    def backward(ctx, gout, _):
        logits, targets, lse, advantages = ctx.saved_tensors
        n, v = logits.shape
        bs = ctx.batch_sizes
        gout = _c(gout.to(torch.float32)).reshape(1)
        dlogits = torch.empty_like(logits)
        check(_lib.lib().capnet_policy_xent_bwd(ptr(logits), v, n, v, ptr(targets), ptr(lse), ptr(advantages), bs[0],
                                                int_array(bs), len(bs), ptr(gout), ptr(dlogits), v, current_stream()),
              "capnet_policy_xent_bwd")
        return dlogits, None, None, None


def policy_loss(logits, targets, advantages, batch_sizes):
    """(loss, caption_logp) of a packed batch of sampled captions: loss = -(1/N) sum over packed rows of
    advantages[caption of the row] * log softmax(logits)[target], differentiable in `logits` only; caption_logp [B]
    (detached) the model's log-probability of every caption. advantages [B] float32 on the device, in the batch's
    sorted order; batch_sizes as ops.batch_sizes_from_lengths gives them."""
    return PolicyLossFn.apply(logits, targets, advantages, batch_sizes)


BLEU_MAX_STEPS = 128          # capnet_bleu_rows: a hypothesis is [start] + at most this many decoded words
BLEU_MAX_REFS = 16            # reference slots per image
BLEU_MAX_REF_WORDS = 4096     # reference slots x padded reference length


def bleu_rows(ids, start_token, end_token, per_image, refs, ref_len, weights=(0.25, 0.25, 0.25, 0.25), smooth=0, steps=None):
    """(reward float32 [rows], stats int32 [rows, 10]) on the device: sentence BLEU of every row of a sampled decode against
    the references of its image (capnet_bleu_rows) -- capnet.metrics.sentence_bleu of what decode.cut_samples makes of the
    row. ids int64 [rows, ld] as the samplers leave them, the first `steps` columns read (None: all); row r belongs to image
    r // per_image. refs int32 [images, R, Lr] zero padded and ref_len int32 [images, R] on the device, a length of 0 an
    absent slot (capnet.train.DeviceBleuReward packs them). weights: four floats; smooth: 0, or 1 for add-one on n >= 2.
    stats: num_1..4, den_1..4, the hypothesis length, the closest reference length. No host read."""
    _need_cuda(ids, refs, ref_len)
    if ids.dtype != torch.int64 or refs.dtype != torch.int32 or ref_len.dtype != torch.int32:
        raise CapnetError("bleu_rows: ids must be int64, refs and ref_len int32")
    if ids.dim() != 2 or refs.dim() != 3 or ref_len.dim() != 2 or tuple(ref_len.shape) != tuple(refs.shape[:2]):
        raise CapnetError("bleu_rows: ids [rows, ld], refs [images, R, Lr], ref_len [images, R]; got %s, %s, %s"
                          % (tuple(ids.shape), tuple(refs.shape), tuple(ref_len.shape)))
    if ids.stride(1) != 1 or len(weights) != 4:
        raise CapnetError("bleu_rows: the columns of ids must be adjacent, and there are four weights")
    refs, ref_len = _c(refs), _c(ref_len)
    rows = ids.shape[0]
    steps = ids.shape[1] if steps is None else int(steps)
    if not 1 <= steps <= ids.shape[1]:
        raise CapnetError("bleu_rows: %d steps of %d columns" % (steps, ids.shape[1]))
    images, R, Lr = refs.shape
    reward = torch.empty(rows, dtype=torch.float32, device=ids.device)
    stats = torch.empty((rows, 10), dtype=torch.int32, device=ids.device)
    w = (C.c_double * 4)(*[float(x) for x in weights])
    check(_lib.lib().capnet_bleu_rows(ptr(ids), ids.stride(0), rows, steps, int(start_token), int(end_token), int(per_image),
                                      ptr(refs), ptr(ref_len), images, R, Lr, w, int(smooth), ptr(reward), ptr(stats),
                                      current_stream()), "capnet_bleu_rows")
    return reward, stats


def cider_rows(ids, start_token, end_token, per_image, refs, ref_len, ref_norm, tables, log_n, sigma=6.0, steps=None):
    """(reward float32 [rows], parts float64 [rows, 4], stats int32 [rows, 9]) on the device: CIDEr-D of every row of a
    sampled decode against the references of its image (capnet_cider_rows) -- capnet.metrics.sentence_cider_d / cider_d_parts
    of what decode.cut_samples makes of the row. ids / per_image / refs / ref_len / steps: as bleu_rows. ref_norm float64
    [images, R, 4]: norm_n of every reference slot; tables: four (keys int32 [count_n, n] ascending, idf float64 [count_n])
    pairs on the device, one per order n = 1..4; log_n: ln of the corpus' image count, the idf of an n-gram no table holds
    (capnet.metrics.CiderCorpus.on and capnet.train.DeviceCiderReward make all of these). stats: the hypothesis length, its
    distinct n-grams for n = 1..4, and how many of those the tables hold. No host read; the same input gives the same bits."""
    _need_cuda(ids, refs, ref_len)
    if ids.dtype != torch.int64 or refs.dtype != torch.int32 or ref_len.dtype != torch.int32:
        raise CapnetError("cider_rows: ids must be int64, refs and ref_len int32")
    if ids.dim() != 2 or refs.dim() != 3 or ref_len.dim() != 2 or tuple(ref_len.shape) != tuple(refs.shape[:2]):
        raise CapnetError("cider_rows: ids [rows, ld], refs [images, R, Lr], ref_len [images, R]; got %s, %s, %s"
                          % (tuple(ids.shape), tuple(refs.shape), tuple(ref_len.shape)))
    if ids.stride(1) != 1:
        raise CapnetError("cider_rows: the columns of ids must be adjacent")
    if not ref_norm.is_cuda or ref_norm.dtype != torch.float64 or tuple(ref_norm.shape) != tuple(refs.shape[:2]) + (4,):
        raise CapnetError("cider_rows: ref_norm must be float64 [images, R, 4] on the device")
    if len(tables) != 4:
        raise CapnetError("cider_rows: four (keys, idf) tables, one per order, not %d" % len(tables))
    keys, idfs = [], []
    for n, (k, v) in enumerate(tables, 1):
        if not (k.is_cuda and v.is_cuda and k.dtype == torch.int32 and v.dtype == torch.float64 and k.dim() == 2
                and k.shape[1] == n and tuple(v.shape) == (k.shape[0],)):
            raise CapnetError("cider_rows: order %d needs keys int32 [count, %d] and idf float64 [count] on the device" % (n, n))
        keys.append(_c(k))
        idfs.append(_c(v))
    if not float(sigma) > 0.0:
        raise CapnetError("cider_rows: sigma %r (must be positive)" % (sigma,))
    refs, ref_len, ref_norm = _c(refs), _c(ref_len), _c(ref_norm)
    rows = ids.shape[0]
    steps = ids.shape[1] if steps is None else int(steps)
    if not 1 <= steps <= ids.shape[1]:
        raise CapnetError("cider_rows: %d steps of %d columns" % (steps, ids.shape[1]))
    images, R, Lr = refs.shape
    reward = torch.empty(rows, dtype=torch.float32, device=ids.device)
    parts = torch.empty((rows, 4), dtype=torch.float64, device=ids.device)
    stats = torch.empty((rows, 9), dtype=torch.int32, device=ids.device)
    counts = [k.shape[0] for k in keys]
    kp = (C.c_void_p * 4)(*[k.data_ptr() if c else None for k, c in zip(keys, counts)])
    vp = (C.c_void_p * 4)(*[v.data_ptr() if c else None for v, c in zip(idfs, counts)])
    check(_lib.lib().capnet_cider_rows(ptr(ids), ids.stride(0), rows, steps, int(start_token), int(end_token), int(per_image),
                                       ptr(refs), ptr(ref_len), ptr(ref_norm), images, R, Lr, kp, vp, int_array(counts),
                                       float(log_n), float(sigma), ptr(reward), ptr(parts), ptr(stats), current_stream()),
          "capnet_cider_rows")
    return reward, parts, stats


class AttentionLossFn(torch.autograd.Function):
    """nll + alpha_c * ((1 - alphas.sum(dim=1)) ** 2).mean()  (train_multitask_att.py:409-411)."""

    @staticmethod
    def forward(ctx, nll, alphas, alpha_c):
        _need_cuda(nll, alphas)
        alphas = _c(alphas)
        B, steps, P = alphas.shape
        colsum = torch.empty(B * P, dtype=torch.float32, device=alphas.device)
        out = torch.empty((), dtype=torch.float32, device=alphas.device)
        check(_lib.lib().capnet_att_loss_fwd(ptr(_c(nll.reshape(1))), ptr(alphas), B, steps, P, float(alpha_c),
                                             ptr(colsum), ptr(out), current_stream()), "capnet_att_loss_fwd")
        ctx.dims, ctx.alpha_c = (B, steps, P), float(alpha_c)
        ctx.save_for_backward(colsum)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        (colsum,) = ctx.saved_tensors
        B, steps, P = ctx.dims
        gout = _c(gout.to(torch.float32)).reshape(1)
        dalphas = torch.empty((B, steps, P), dtype=torch.float32, device=colsum.device)
        check(_lib.lib().capnet_att_loss_bwd(ptr(gout), ptr(colsum), B, steps, P, ctx.alpha_c, ptr(dalphas),
                                             current_stream()), "capnet_att_loss_bwd")
        return gout.reshape(()), dalphas, None


def attention_loss(nll, alphas, alpha_c=1.0):
    return AttentionLossFn.apply(nll, alphas, alpha_c)


# ---------------------------------------------------------------------------------------
# autograd: nn.BatchNorm1d (encoder head)
# ---------------------------------------------------------------------------------------
class BatchNorm1dFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, train, momentum, eps):
        _need_cuda(x, gamma, beta, running_mean, running_var)
        x = _c(x)
        b, c = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        invstd = torch.empty(c, dtype=torch.float32, device=x.device)
        check(_lib.lib().capnet_bn1d_fwd(ptr(x), b, c, ptr(gamma), ptr(beta), ptr(running_mean),
                                         ptr(running_var), int(train), momentum, eps, ptr(y),
                                         ptr(mean), ptr(invstd), current_stream()),
              "capnet_bn1d_fwd")
        ctx.train = train
        ctx.save_for_backward(x, gamma, mean, invstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        if not ctx.train:
            raise CapnetError("BatchNorm1d backward is implemented for train mode only")
        x, gamma, mean, invstd = ctx.saved_tensors
        dy = _c(dy)
        b, c = x.shape
        dx = torch.empty_like(x)
        dgamma = torch.empty_like(gamma)
        dbeta = torch.empty_like(gamma)
        check(_lib.lib().capnet_bn1d_bwd(ptr(dy), ptr(x), b, c, ptr(gamma), ptr(mean), ptr(invstd),
                                         ptr(dx), ptr(dgamma), ptr(dbeta), current_stream()),
              "capnet_bn1d_bwd")
        return dx, dgamma, dbeta, None, None, None, None, None


def batch_norm1d(x, gamma, beta, running_mean, running_var, train, momentum, eps):
    return BatchNorm1dFn.apply(x, gamma, beta, running_mean, running_var, train, momentum, eps)


# ---------------------------------------------------------------------------------------
# autograd: whole-sequence decoder recurrence
# ---------------------------------------------------------------------------------------
def batch_sizes_from_lengths(lengths):
    """pack_padded_sequence(..., lengths).batch_sizes for lengths sorted in decreasing order."""
    lengths = [int(l) for l in lengths]
    if not lengths or any(l <= 0 for l in lengths):
        raise CapnetError("lengths must be positive")
    if any(lengths[i] < lengths[i + 1] for i in range(len(lengths) - 1)):
        raise CapnetError("lengths must be sorted in decreasing order (pack_padded_sequence contract)")
    return [sum(1 for l in lengths if l > t) for t in range(lengths[0])]


def _gate_grads(cell, F, H, dV, dbV, dS, dbS, dU, dbUW, dW):
    """The gate-stacked gradients of one layer cut into the per-gate views of its weight table: V w x4, V b x4, S w x4,
    S b x4, U w x4, U b x4, W w x4, W b x4 (b_U and b_W enter the same pre-activation: W b gets a copy of dbUW). The
    LSTM cell: (weight_ih, bias_ih, weight_hh, bias_hh). dW / dbUW may run on past 4H rows (the attention cell's z
    block): only the first 4H are the gates'."""
    if cell != CELL_FACTORED:
        return [dV, dbUW[:4 * H], dW[:4 * H], dbUW[:4 * H].clone()]

    def gates(x, n):
        return [x[g * n:(g + 1) * n] for g in range(4)]
    return (gates(dV, F) + gates(dbV, F) + [dS[g] for g in range(4)] + gates(dbS, F) + [dU[g] for g in range(4)] +
            gates(dbUW, H) + gates(dW, H) + [b.clone() for b in gates(dbUW, H)])


def _seq_args(cfg, captions):
    """-> (cell, num_layers) of cfg (defaults: the factored cell, one layer), with the checks both sequence Functions
    make: the cell, the layer count (either cell stacks 1 to 8), int64 captions, batch_sizes / tf_mask against the
    batch."""
    cell, nl = cfg.get("cell", CELL_FACTORED), cfg.get("num_layers", 1)
    if cell not in (CELL_FACTORED, CELL_LSTM):
        raise CapnetError("unknown cell %r" % (cell,))
    if not 1 <= nl <= 8:
        raise CapnetError("%d layers: a decoder stacks 1 to 8" % nl)
    if captions.dtype != torch.int64:
        raise CapnetError("captions must be int64")
    if "batch_sizes" not in cfg or "tf_mask" not in cfg:
        raise CapnetError("decoder: cfg needs batch_sizes and tf_mask")
    bs, tf = cfg["batch_sizes"], cfg["tf_mask"]
    if len(tf) != len(bs) or bs[0] != captions.shape[0]:
        raise CapnetError("decoder: batch_sizes / tf_mask do not match the batch")
    return cell, nl


def _lstm_slots(ws):
    """The LSTM cell's (weight_ih, bias_ih, weight_hh, bias_hh) of each layer in slots 0 / 4 / 24 / 28 of the factored
    cell's 32 (4 tensors per layer in, 32 out)."""
    out = []
    for l in range(0, len(ws), 4):
        slots = [None] * 32
        slots[0], slots[4], slots[24], slots[28] = ws[l:l + 4]
        out += slots
    return out


def _tf_bytes(tf):
    return (C.c_ubyte * len(tf))(*[1 if x else 0 for x in tf])


def _seq_training(cfg):
    """capnet_seq_forward_stacked's `training` bit set: 1 = training; + 2 (cfg["input_dropout_only"]) = dropout on the
    token embeddings only, none between the layers (torch.nn.LSTM without dropout=, capnet.seq2seq)."""
    return int(bool(cfg["training"])) | (2 if cfg.get("input_dropout_only") else 0)


class SeqFn(torch.autograd.Function):
    """The top layer's hiddens [N, H] (pack_padded_sequence order) of the scheduled-sampling recurrence of 1 to 8 stacked
    layers: ONE C call each way (capnet_seq_forward_stacked / capnet_seq_backward_stacked, csrc/decoder_seq.cpp).
    cfg: batch_sizes, tf_mask, hidden_size, factored_size (factored cell), dropout, seed, training; cell (default
    CELL_FACTORED), num_layers (default 1, at most 8); input_dropout_only (default False: the same p between the layers).
    With cfg["want_final_state"], forward leaves cfg["final_state"] = (h, c), each [num_layers, b_last, H]: the state after
    the last step of the rows alive there (copies without a gradient path).
    weights: the factored cell -> 32 tensors per layer, layer 0 first (V w x4, V b x4, S w x4, S b x4, U w x4, U b x4,
             W w x4, W b x4); the LSTM cell -> 4 per layer, layer 0 first (weight_ih, bias_ih, weight_hh, bias_hh)."""

    @staticmethod
    def forward(ctx, cfg, captions, features, emb, Cw, Cb, *weights):
        _need_cuda(captions, features, emb, Cw, Cb, *weights)
        captions = _c(captions)
        cell, nl = _seq_args(cfg, captions)
        ws = [_c(w) for w in weights]
        if len(ws) != (32 if cell == CELL_FACTORED else 4) * nl:
            raise CapnetError("the factored cell takes 32 weight tensors per layer, the LSTM cell 4")
        if cell != CELL_FACTORED:
            ws = _lstm_slots(ws)
        emb, Cw, Cb = _c(emb), _c(Cw), _c(Cb)
        dev = emb.device
        bs, tf = cfg["batch_sizes"], cfg["tf_mask"]
        B, T = captions.shape
        V, E = emb.shape
        H, F, N = cfg["hidden_size"], cfg.get("factored_size", 0), sum(bs)
        if features is not None:
            features = _c(features)
            if tuple(features.shape) != (B, E):
                raise CapnetError("features must be [batch, embed_size]")
        dims = [[B, T, len(bs), N, E if l == 0 else H, F, H, V, int(features is not None) if l == 0 else 0, cell]
                for l in range(nl)]
        L = _lib.lib()
        cd = [int_array(d) for d in dims]
        saved = [torch.empty(L.capnet_seq_saved_floats(c), dtype=torch.float32, device=dev) for c in cd]
        saved_i = [torch.empty(L.capnet_seq_saved_ints(c), dtype=torch.int32, device=dev) for c in cd]
        scratch = torch.empty(L.capnet_seq_fwd_scratch_floats(cd[0]), dtype=torch.float32, device=dev)
        hid = [torch.empty((N, H), dtype=torch.float32, device=dev) for _ in range(nl)]
        check(L.capnet_seq_forward_stacked(cd[0], nl, int_array(bs), _tf_bytes(tf), ptr(captions), ptr(features),
                                           ptr(emb), ptr_array(ws), ptr(Cw), ptr(Cb), float(cfg["dropout"]),
                                           int(cfg["seed"]), _seq_training(cfg), ptr_array(saved), ptr_array(saved_i),
                                           ptr(scratch), ptr_array(hid), ptr(err_flag(dev)), current_stream()),
              "capnet_seq_forward_stacked")
        if cfg.get("want_final_state"):
            last = N - bs[-1]
            cst = [saved[l][L.capnet_seq_saved_cell_offset(cd[l]):][:N * H].view(N, H) for l in range(nl)]
            cfg["final_state"] = (torch.stack([h[last:] for h in hid]), torch.stack([c[last:] for c in cst]))
        ctx.cfg, ctx.dims, ctx.has_features = cfg, dims, features is not None
        ctx.save_for_backward(*(saved + saved_i + hid))
        return hid[-1]

    @staticmethod
    @once_differentiable
    def backward(ctx, d_hiddens):
        cfg, dims = ctx.cfg, ctx.dims
        nl = len(dims)
        t = ctx.saved_tensors
        saved, saved_i, hid = t[:nl], t[nl:2 * nl], t[2 * nl:]
        B, T, steps, N, E, F, H, V, _, cell = dims[0]
        dev = saved[0].device
        L = _lib.lib()
        cd = [int_array(d) for d in dims]
        scratch = torch.empty(max(L.capnet_seq_bwd_scratch_floats(c) for c in cd), dtype=torch.float32, device=dev)

        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)

        dEmb = new(V, E)
        dFeat = new(B, E) if ctx.has_features else None
        grads, per_layer = [], []
        for l in range(nl):
            El = E if l == 0 else H
            if cell == CELL_FACTORED:
                g = [new(4 * F, El), new(4 * F), new(4, F, F), new(4 * F), new(4, H, F), new(4 * H), new(4 * H, H)]
            else:
                g = [new(4 * H, El), None, None, None, None, new(4 * H), new(4 * H, H)]
            grads += g + [dEmb if l == 0 else None, dFeat if l == 0 else None]
            per_layer.append(g)
        dh_work = [new(N, H) for _ in range(nl - 1)]
        check(L.capnet_seq_backward_stacked(cd[0], nl, int_array(cfg["batch_sizes"]), ptr(_c(d_hiddens)), ptr_array(hid),
                                            ptr_array(saved), ptr_array(saved_i), ptr(scratch),
                                            ptr_array(dh_work) if dh_work else None, ptr_array(grads),
                                            float(cfg["dropout"]), int(cfg["seed"]), _seq_training(cfg), current_stream()),
              "capnet_seq_backward_stacked")
        wg = []
        for g in per_layer:
            wg += _gate_grads(cell, F, H, *g)
        # cfg, captions, features, emb, Cw, Cb, *weights
        return (None, None, dFeat, dEmb, None, None) + tuple(wg)


class AttSeqFn(torch.autograd.Function):
    """(top-layer hiddens [N, H], layer 0's alphas [B, steps, P]) of the attention recurrence of 1 to 8 stacked layers:
    ONE C call each way (capnet_att_seq_forward_stacked / capnet_att_seq_backward_stacked, csrc/decoder_att_seq.cpp).
    cfg: SeqFn's keys and attention_size.
    weights: layer 0's 44 tensors (V w x4, V b x4, S w x4, S b x4, U w x4, U b x4, W w x4, W b x4, init_h w,b, init_c w,b,
    encoder_att w,b, decoder_att w,b, full_att w,b, f_beta w,b) -- the LSTM cell's 16: weight_ih, bias_ih, weight_hh,
    bias_hh, then the same 12 --, then 36 per upper layer: its 32 in the same order, init_h{l} w, b, init_c{l} w, b --
    the LSTM cell's 8: weight_ih, bias_ih, weight_hh, bias_hh, init_h{l} w, b, init_c{l} w, b.
    `features` gets no gradient (frozen trunk)."""

    @staticmethod
    def forward(ctx, cfg, captions, features, emb, Cw, Cb, *weights):
        _need_cuda(captions, features, emb, Cw, Cb, *weights)
        captions = _c(captions)
        cell, nl = _seq_args(cfg, captions)
        ws = [_c(w) for w in weights]
        if len(ws) != (44 + 36 * (nl - 1) if cell == CELL_FACTORED else 16 + 8 * (nl - 1)):
            raise CapnetError("attention decoder: 44 + 36 (num_layers - 1) weight tensors (factored) / "
                              "16 + 8 (num_layers - 1) (LSTMCell)")
        if cell != CELL_FACTORED:
            upper = []
            for l in range(1, nl):
                u = ws[16 + 8 * (l - 1):16 + 8 * l]
                upper += _lstm_slots(u[:4]) + u[4:]
            ws = _lstm_slots(ws[:4]) + ws[4:16] + upper
        emb, Cw, Cb = _c(emb), _c(Cw), _c(Cb)
        dev = emb.device
        bs, tf = cfg["batch_sizes"], cfg["tf_mask"]
        B, T = captions.shape
        V, E = emb.shape
        H, A = cfg["hidden_size"], cfg["attention_size"]
        F = cfg["factored_size"] if cell == CELL_FACTORED else 4
        features = _c(features)
        if features.dim() != 3 or features.shape[0] != B:
            raise CapnetError("features must be [batch, pixels, feature_size]")
        P, Cf = features.shape[1], features.shape[2]
        N = sum(bs)
        dims = [B, T, len(bs), N, E, F, H, V, A, P, Cf, cell]
        cdims = int_array(dims)
        L = _lib.lib()
        saved = [torch.empty(L.capnet_att_stacked_saved_floats(cdims, l), dtype=torch.float32, device=dev) for l in range(nl)]
        saved_i = [torch.empty(L.capnet_att_stacked_saved_ints(cdims, l), dtype=torch.int32, device=dev) for l in range(nl)]
        scratch = torch.empty(L.capnet_att_stacked_fwd_scratch_floats(cdims, nl), dtype=torch.float32, device=dev)
        # upper layers: B leading rows hold the initial state
        hid = [torch.empty((N if l == 0 else B + N, H), dtype=torch.float32, device=dev) for l in range(nl)]
        alphas = torch.empty((B, len(bs), P), dtype=torch.float32, device=dev)
        check(L.capnet_att_seq_forward_stacked(cdims, nl, int_array(bs), _tf_bytes(tf), ptr(captions), ptr(features),
                                               ptr(emb), ptr_array(ws), ptr(Cw), ptr(Cb), float(cfg["dropout"]),
                                               int(cfg["seed"]), int(cfg["training"]), ptr_array(saved), ptr_array(saved_i),
                                               ptr(scratch), ptr_array(hid), ptr(alphas), ptr(err_flag(dev)),
                                               current_stream()), "capnet_att_seq_forward_stacked")
        ctx.cfg, ctx.dims, ctx.nl = cfg, dims, nl
        ctx.save_for_backward(*(saved + saved_i + hid), features, *ws)
        return (hid[0] if nl == 1 else hid[-1][B:]), alphas

    @staticmethod
    @once_differentiable
    def backward(ctx, d_hiddens, d_alphas):
        cfg, dims, nl = ctx.cfg, ctx.dims, ctx.nl
        t = ctx.saved_tensors
        saved, saved_i, hid, features, ws = t[:nl], t[nl:2 * nl], t[2 * nl:3 * nl], t[3 * nl], t[3 * nl + 1:]
        B, T, steps, N, E, F, H, V, A, P, Cf, cell = dims
        dev = features.device
        L = _lib.lib()
        cdims = int_array(dims)
        scratch = torch.empty(L.capnet_att_stacked_bwd_scratch_floats(cdims, nl), dtype=torch.float32, device=dev)

        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)

        d_hiddens = _c(d_hiddens) if d_hiddens is not None else torch.zeros((N, H), dtype=torch.float32, device=dev)
        d_alphas = _c(d_alphas) if d_alphas is not None else None
        XW = E + Cf
        if cell == CELL_FACTORED:
            dV, dbV, dS, dbS, dU = new(4 * F, XW), new(4 * F), new(4, F, F), new(4 * F), new(4, H, F)
        else:
            dV, dbV, dS, dbS, dU = new(4 * H, XW), None, None, None, None
        dWz, dbz = new(4 * H + A + Cf, H), new(4 * H + A + Cf)
        dWe, dbe, dwf, dbf = new(A, Cf), new(A), new(1, A), new(1)
        dWih, dbih, dWic, dbic = new(H, Cf), new(H), new(H, Cf), new(H)
        dEmb = new(V, E)
        grads = [dV, dbV, dS, dbS, dU, dWz, dbz, dWe, dbe, dwf, dbf, dWih, dbih, dWic, dbic, dEmb]
        upper = []
        for _ in range(1, nl):
            if cell == CELL_FACTORED:
                g = [new(4 * F, H), new(4 * F), new(4, F, F), new(4 * F), new(4, H, F), new(4 * H), new(4 * H, H)]
            else:
                g = [new(4 * H, H), None, None, None, None, new(4 * H), new(4 * H, H)]
            g += [new(H, Cf), new(H), new(H, Cf), new(H)]
            grads += g
            upper.append(g)
        dh_work = [new(N, H) for _ in range(nl - 1)]
        check(L.capnet_att_seq_backward_stacked(cdims, nl, int_array(cfg["batch_sizes"]), ptr(d_hiddens), ptr(d_alphas),
                                                ptr_array(hid), ptr(features), ptr_array(ws), ptr_array(saved),
                                                ptr_array(saved_i), ptr(scratch), ptr_array(dh_work) if dh_work else None,
                                                ptr_array(grads), float(cfg["dropout"]), int(cfg["seed"]),
                                                int(cfg["training"]), current_stream()), "capnet_att_seq_backward_stacked")
        wg = _gate_grads(cell, F, H, dV, dbV, dS, dbS, dU, dbz, dWz)
        wg += [dWih, dbih, dWic, dbic, dWe, dbe, dWz[4 * H:4 * H + A], dbz[4 * H:4 * H + A], dwf, dbf,
               dWz[4 * H + A:], dbz[4 * H + A:]]
        for g in upper:
            wg += _gate_grads(cell, F, H, *g[:7]) + g[7:]
        # cfg, captions, features, emb, Cw, Cb, *weights
        return (None, None, None, dEmb, None, None) + tuple(wg)
