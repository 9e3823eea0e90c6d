"""Beam search shared by the decoders' `sample()` methods.

Mirrors the loop of stylenet/model.py:198-294 (identical in nic/model.py and, with the attention
inputs, stylenet/model_att.py:307-426): k live beams, every step expands them by
log-softmax + running score, keeps the k best of the flattened [s*V] scores, retires beams that
produced <end>, and returns the completed sequence with the highest score.

Device work per step: the decoder's own step (C-ABI kernels) and ONE `capnet_beam_topk` launch
(log-softmax + add + top-k fused); the k scores / indices come back in one transfer and the
bookkeeping (sequence lists, which beam survives) is host Python, as in the reference.

beam_search_device is the opt-in third loop: the same search with that bookkeeping done by the selecting workgroup
(capnet_beam_advance), fixed rows per image and nothing read by the host until the end.

Constraints / banned_words: what a search must not emit (no repeated n-gram, a minimum length, banned words),
one rule for all three loops through their `constraints` keyword. The host loops, which hold the sequences, build every
live row's list and hand it to capnet_beam_topk[_batched]_banned; beam_search_device leaves it to the selecting workgroup
(capnet_beam_advance_constrained), which reads the sequences in the beam state. None: the loops as they were.

Diversity / merge_groups: diverse beam search (beam groups that pay for the words earlier groups chose at the same step; DESIGN
4al) through the `diversity` keyword of beam_search_batched and beam_search_device, which then keep their bookkeeping per
(image, group) -- n D searches of k / D beams -- and select with capnet_beam_topk_batched_diverse /
capnet_beam_advance_diverse, one workgroup per image walking its groups in order. None: the loops as they were.

Constraints(forced=...) / forced_allocate / met_mask: words every completed caption must contain (dynamic beam allocation; DESIGN
4am), through the same `constraints` keyword: the host loops hand every row's met mask beside its ban list to
capnet_beam_topk_batched_forced (beam_search with n = 1), beam_search_device's ops.beam_advance selects with
capnet_beam_advance_forced. Without forced words: the loops as they were.

PerImage: a Constraints (or None) per image of a batched search, through the same keyword of
beam_search_batched and beam_search_device: the host loop builds every row's ban list and met mask from its own image's
entry for capnet_beam_topk_batched_rules; beam_search_device's ops.beam_advance selects with capnet_beam_advance_rules, one
workgroup per image on its own row of the rule table.

Deviation from the reference text: `top_k_words / vocab_size` (model.py:249) is an integer
division here. Under the torch 1.1 the reference pins it was one; under current torch the
reference line raises.
"""
import torch

from . import ops


def rank_completed(done, length_penalty=0.0):
    """The n-best list of one image from its completed hypotheses `done`, (score, tokens) pairs in completion order ->
    [(tokens, score)], best first: the key is score / (len(tokens) - 1)^length_penalty (len - 1: the generated words, <end>
    included; penalty 0: the score itself), ties go to the earlier completion -- capnet_beam_nbest's rule. Entry 0 at
    penalty 0 is the first maximum, the searches' winner."""
    def key(q):
        score, tokens = done[q]
        return score if length_penalty == 0 else score / float(len(tokens) - 1) ** length_penalty
    return [(list(done[q][1]), float(done[q][0])) for q in sorted(range(len(done)), key=lambda q: (-key(q), q))]


class Constraints(object):
    """What a beam search must not emit, the same rule on every route. At step s (1-based) a live hypothesis
    is tokens = [start, w_1 .. w_{s-1}]; the candidate (hypothesis, word v) is excluded from that step's selection if
      * v is in `banned` (a tuple of at most 32 distinct word ids, none of them end_token), or
      * v == end_token and s <= min_words (a completed caption has at least min_words words between <start> and <end>), or
      * g = no_repeat_ngram (0 to 4) >= 1, len(tokens) >= g, and appending v would complete a g-gram the hypothesis already
        contains, <start> included (g = 1: no word twice; a context seen several times bans several words).
    Excluded candidates leave AFTER the log-softmax: a survivor's score is the model's own summed log-probability, the number
    score_captions returns; nothing is renormalised. Constraints() excludes nothing and runs the unconstrained code.
    forced (Post & Vilar 2018, dynamic beam allocation): a tuple of at most MAX_FORCED distinct word ids that
    every completed caption must contain. The met count of a candidate (row r, word v) is the number of forced ids among
    w_1 .. w_{s-1} of r or equal to v (<start> does not count). <end> is excluded on a row whose own met count is below
    F = len(forced). The step's pool holds (1) the plain selection's `live` best non-excluded candidates, (2) for every
    competing row every forced id not yet in it and not excluded on it, (3) every competing row's best non-excluded word --
    a flat index once -- and forced_allocate deals the `live` slots out of it: banks by met count, each by score descending
    with ties to the lower flat index, visited F, F - 1 .. 0, F ..; the order of taking is the output order. Scores stay the
    model's own log-probabilities. Without `forced` every route runs exactly the code it runs without the field."""
    MAX_NGRAM, MAX_BANNED, MAX_FORCED = 4, 32, 4

    def __init__(self, no_repeat_ngram=0, min_words=0, banned=(), forced=()):
        for name, v in (("no_repeat_ngram", no_repeat_ngram), ("min_words", min_words)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ops.CapnetError("Constraints: %s must be an int, not %r" % (name, v))
        if not 0 <= no_repeat_ngram <= self.MAX_NGRAM:
            raise ops.CapnetError("Constraints: no_repeat_ngram=%d (0 .. %d)" % (no_repeat_ngram, self.MAX_NGRAM))
        if min_words < 0:
            raise ops.CapnetError("Constraints: min_words=%d (>= 0)" % min_words)
        if isinstance(banned, (str, bytes)) or not hasattr(banned, "__iter__"):
            raise ops.CapnetError("Constraints: banned must be a sequence of word ids, not %r" % (banned,))
        banned = tuple(banned)
        for w in banned:
            if isinstance(w, bool) or not isinstance(w, int) or w < 0:
                raise ops.CapnetError("Constraints: banned holds word ids (ints >= 0), not %r" % (w,))
        if len(banned) > self.MAX_BANNED or len(set(banned)) != len(banned):
            raise ops.CapnetError("Constraints: banned must be at most %d distinct word ids" % self.MAX_BANNED)
        if isinstance(forced, (str, bytes)) or not hasattr(forced, "__iter__"):
            raise ops.CapnetError("Constraints: forced must be a sequence of word ids, not %r" % (forced,))
        forced = tuple(forced)
        for w in forced:
            if isinstance(w, bool) or not isinstance(w, int) or w < 0:
                raise ops.CapnetError("Constraints: forced holds word ids (ints >= 0), not %r" % (w,))
        if len(forced) > self.MAX_FORCED or len(set(forced)) != len(forced):
            raise ops.CapnetError("Constraints: forced must be at most %d distinct word ids" % self.MAX_FORCED)
        if set(forced) & set(banned):
            raise ops.CapnetError("Constraints: forced=%r and banned=%r share a word id" % (forced, banned))
        self.no_repeat_ngram, self.min_words, self.banned, self.forced = no_repeat_ngram, min_words, banned, forced

    @property
    def active(self):
        return bool(self.no_repeat_ngram or self.min_words or self.banned or self.forced)

    def check(self, vocab_size, end_token, k, max_seq_length):
        """The front end's check for one search (CapnetError): no banned id is end_token or outside the vocabulary, and
        every step keeps k finite candidates -- V - len(banned) - 1 - (max_seq_length + 1) >= k (the banned words, <end>
        and one word per token of the longest hypothesis gone from a row) and min_words < max_seq_length."""
        if int(end_token) in self.banned or any(w >= vocab_size for w in self.banned):
            raise ops.CapnetError("constraints: banned=%r must be word ids below %d other than end_token %d"
                                  % (self.banned, vocab_size, int(end_token)))
        if vocab_size - len(self.banned) - 1 - (max_seq_length + 1) < k:
            raise ops.CapnetError("constraints: vocab_size %d - %d banned - 1 - (max_seq_length %d + 1) leaves fewer than k = %d "
                                  "candidates" % (vocab_size, len(self.banned), max_seq_length, k))
        if not self.min_words < max_seq_length:
            raise ops.CapnetError("constraints: min_words=%d must be below max_seq_length %d" % (self.min_words, max_seq_length))
        if int(end_token) in self.forced or any(w >= vocab_size for w in self.forced):
            raise ops.CapnetError("constraints: forced=%r must be word ids below %d other than end_token %d"
                                  % (self.forced, vocab_size, int(end_token)))
        if self.forced and not len(self.forced) < max_seq_length:
            raise ops.CapnetError("constraints: %d forced words must be fewer than max_seq_length %d" % (len(self.forced), max_seq_length))

    def check_exclude(self, vocab_size, end_token, top_k, max_seq_length):
        """The front end's check for one sampled decode under `exclude=` (sample_random; CapnetError): no forced
        words (they have no meaning for a draw), no banned id is end_token or outside the vocabulary, min_words <
        max_seq_length, and every row keeps max(top_k, 1) words to choose among at every step -- check's count: V -
        len(banned) - 1 - (max_seq_length + 1) >= max(top_k, 1)."""
        if self.forced:
            raise ops.CapnetError("exclude: forced=%r has no meaning for a draw" % (self.forced,))
        if int(end_token) in self.banned or any(w >= vocab_size for w in self.banned):
            raise ops.CapnetError("exclude: banned=%r must be word ids below %d other than end_token %d"
                                  % (self.banned, vocab_size, int(end_token)))
        if not self.min_words < max_seq_length:
            raise ops.CapnetError("exclude: min_words=%d must be below max_seq_length %d" % (self.min_words, max_seq_length))
        if vocab_size - len(self.banned) - 1 - (max_seq_length + 1) < max(int(top_k), 1):
            raise ops.CapnetError("exclude: vocab_size %d - %d banned - 1 - (max_seq_length %d + 1) leaves fewer than max(top_k, 1) "
                                  "= %d words" % (vocab_size, len(self.banned), max_seq_length, max(int(top_k), 1)))

    def __repr__(self):
        tail = ", forced=%r" % (self.forced,) if self.forced else ""
        return "Constraints(no_repeat_ngram=%d, min_words=%d, banned=%r%s)" % (self.no_repeat_ngram, self.min_words, self.banned, tail)


MIXED = type("Mixed", (object,), {"__repr__": lambda self: "capnet.beam.MIXED", "__slots__": ()})()   # PerImage.uniform()


class PerImage(object):
    """A rule per image for a batched beam search: `entries`, one per image in batch order, each a Constraints
    or None (no rule). Image i is searched exactly as it would be alone under entries[i]. It is NOT a Constraints: what takes
    only a Constraints refuses it. The device routes read the rules from table() -- int32 [n][RULE_WORDS], row i: word 0
    no_repeat_ngram, 1 min_words, 2 n_banned, 3 n_forced, 4 .. 35 banned, 36 .. 39 forced; a None or inactive entry is a row
    of zeros (include/capnet.h) -- the host loops build every row's ban list and met mask from its own image's entry. len(),
    indexing and slicing work; a slice is a PerImage."""
    RULE_WORDS, BANNED_AT, FORCED_AT = 40, 4, 36

    def __init__(self, entries):
        if isinstance(entries, (str, bytes, Constraints)) or not hasattr(entries, "__iter__"):
            raise ops.CapnetError("PerImage: entries must be a sequence of capnet.beam.Constraints or None, not %r" % (entries,))
        entries = tuple(entries)
        for c in entries:
            if c is not None and not isinstance(c, Constraints):
                raise ops.CapnetError("PerImage: every entry must be a capnet.beam.Constraints or None, not %r" % (c,))
        self.entries = entries
        self._tables = {}

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, i):
        return PerImage(self.entries[i]) if isinstance(i, slice) else self.entries[i]

    def __iter__(self):
        return iter(self.entries)

    @property
    def active(self):
        return any(c is not None and c.active for c in self.entries)

    @staticmethod
    def _fields(c):
        return (0, 0, (), ()) if c is None else (c.no_repeat_ngram, c.min_words, c.banned, c.forced)

    def uniform(self):
        """The one Constraints all entries equal field by field (None where that is no rule: None and an inactive
        Constraints() count as equal), or MIXED. An empty PerImage is None."""
        fields = set(self._fields(c) for c in self.entries)
        if len(fields) > 1:
            return MIXED
        first = self.entries[0] if self.entries else None
        return first if first is not None and first.active else None

    def check(self, vocab_size, end_token, k, max_seq_length, n):
        """The front end's check (CapnetError): an entry per image, and every active entry's own Constraints.check."""
        if len(self.entries) != n:
            raise ops.CapnetError("constraints: a PerImage of %d entries for %d images" % (len(self.entries), n))
        for c in self.entries:
            if c is not None and c.active:
                c.check(vocab_size, end_token, k, max_seq_length)

    def rows(self):
        """The table as n lists of RULE_WORDS ints."""
        out = []
        for c in self.entries:
            g, m, banned, forced = self._fields(c)
            out.append([g, m, len(banned), len(forced)] + list(banned) + [0] * (Constraints.MAX_BANNED - len(banned))
                       + list(forced) + [0] * (Constraints.MAX_FORCED - len(forced)))
        return out

    def table(self, device):
        """The rule table on `device`: contiguous int32 [n, RULE_WORDS], made once per device and kept."""
        key = str(torch.device(device))
        if key not in self._tables:
            self._tables[key] = torch.tensor(self.rows(), dtype=torch.int32, device=device).reshape(len(self.entries), self.RULE_WORDS)
        return self._tables[key]

    def __repr__(self):
        return "PerImage(%r)" % (list(self.entries),)


def entry_of(constraints, image):
    """The rule of image `image`: a PerImage's entry (None -> a Constraints() that excludes nothing), else `constraints`."""
    if isinstance(constraints, PerImage):
        c = constraints[image]
        return Constraints() if c is None else c
    return constraints


class Diversity(object):
    """Diverse beam search (Vijayakumar et al. 2016), the same rule on every route. Image i's k beams form
    `groups` = D groups of k' = k / D; group g holds slots g k' .. g k' + k' - 1 and is a beam search of its own with the
    plain bookkeeping (step 1: its first row alone; <end> retires a beam; it ends when none is live). At each step the
    groups select in order; group g takes its live best candidates (row, word v) by
        key = score - strength * c_g(v),
    score = the running score + the row's log-softmax, c_g(v) = the number of candidates selected at this step by groups
    0 .. g - 1 of the same image whose word is v. <end> is counted like any word: that is the published rule and fairseq's.
    A group with no live beam selects nothing and counts nothing; ties go to the lower flat index within the group. The
    penalty shapes the selection only: a caption's score stays the model's own summed log-probability, the number
    score_captions returns. With constraints, the exclusions apply first, then the penalty.
    per_group (needs nbest=True): the result per image is D entries in group order, each the group's best (tokens, score)
    by rank_completed's key, or None where the group completed nothing -- the "D different captions" call.
    Diversity(1, x) is not active and runs the plain search."""
    MAX_GROUPS = 16

    def __init__(self, groups=2, strength=0.5, per_group=False):
        if isinstance(groups, bool) or not isinstance(groups, int) or not 1 <= groups <= self.MAX_GROUPS:
            raise ops.CapnetError("Diversity: groups must be an int, 1 .. %d, not %r" % (self.MAX_GROUPS, groups))
        if isinstance(strength, bool) or not isinstance(strength, (int, float)):
            raise ops.CapnetError("Diversity: strength must be a float, not %r" % (strength,))
        strength = float(strength)
        if not 0.0 <= strength < float("inf"):      # (NaN fails both comparisons)
            raise ops.CapnetError("Diversity: strength=%r must be finite and >= 0" % strength)
        if not isinstance(per_group, bool):
            raise ops.CapnetError("Diversity: per_group must be a bool, not %r" % (per_group,))
        self.groups, self.strength, self.per_group = groups, strength, per_group

    @property
    def active(self):
        return self.groups > 1

    def check(self, k):
        """The front end's check for one search (CapnetError): groups divides k (transformers' rule)."""
        if isinstance(k, bool) or not isinstance(k, int) or k < self.groups or k % self.groups:
            raise ops.CapnetError("diversity: groups=%d must divide the beam size k=%r" % (self.groups, k))

    def __repr__(self):
        return "Diversity(groups=%d, strength=%r, per_group=%r)" % (self.groups, self.strength, self.per_group)


def dedupe_completed(done):
    """(score, tokens) pairs with every token list once: the first is kept, the order stays."""
    seen, out = set(), []
    for score, tokens in done:
        key = tuple(int(w) for w in tokens)
        if key not in seen:
            seen.add(key)
            out.append((score, tokens))
    return out


def merge_groups(done_groups, end_token, diversity, nbest=False, length_penalty=0.0):
    """What a diverse search returns for ONE image from its groups' completed lists `done_groups` (D lists of (score,
    tokens) in completion order). Without nbest: the token list with the highest score over all groups, ties to the lower
    group, then the earlier completion; [end_token] where nothing completed. nbest: the lists concatenated in group order,
    identical token lists once (two groups that find the same caption differ in the last bit of its score: the first is
    kept), ranked by rank_completed. per_group: D entries, each group's rank_completed winner (tokens, score) or None."""
    if diversity.per_group:
        return [(rank_completed(d, length_penalty)[0] if d else None) for d in done_groups]
    flat = [p for d in done_groups for p in d]
    if nbest:
        return rank_completed(dedupe_completed(flat), length_penalty)
    if not flat:
        return [int(end_token)]
    return rank_completed(flat)[0][0]       # penalty 0: the first maximum in group, then completion order


def by_completion(ranked):
    """A state-image's capnet_beam_nbest list at length_penalty 0 ((tokens, score), score descending, ties to the earlier
    completion) -> (score, tokens) in completion order: hypotheses complete by step, so by length, and those of one step
    all end in <end> and share its count, so their rank at that step is their score order -- a stable sort by length."""
    return [(sc, q) for q, sc in sorted(ranked, key=lambda p: len(p[0]))]


def banned_words(tokens, step, end_token, constraints):
    """Constraints' rule as code: the sorted word ids a hypothesis `tokens` = [start, w_1 .. w_{step-1}] may not take at step
    `step` (1-based)."""
    out = set(constraints.banned)
    if step <= constraints.min_words:
        out.add(int(end_token))
    g, n = constraints.no_repeat_ngram, len(tokens)
    if g >= 1 and n >= g:
        tail = list(tokens[n - (g - 1):]) if g > 1 else []
        for e in range(n - g + 1):
            if list(tokens[e:e + g - 1]) == tail:
                out.add(int(tokens[e + g - 1]))
    if constraints.forced and met_mask(tokens, constraints.forced) != (1 << len(constraints.forced)) - 1:
        out.add(int(end_token))       # forced words: no <end> before the hypothesis holds them all
    return sorted(out)


def met_mask(tokens, forced):
    """Bit f set where forced[f] occurs in `tokens` = [start, w_1 ..] behind <start>."""
    words = set(int(w) for w in tokens[1:])
    return sum(1 << f for f, w in enumerate(forced) if int(w) in words)


def forced_allocate(pool, live, F):
    """The allocation of Constraints' forced words as code. pool: [(score, flat, met)], a flat index once, met the
    candidate's met count 0 .. F -> the entries taken, in taking order: within a bank (a met count) by score descending, ties
    to the lower flat index; the banks are visited F, F - 1 .. 0, F .., a visit takes the bank's best untaken entry if it
    has one, until `live` are taken or the pool is empty. (A flat index listed twice -- a candidate that entered the pool by
    two of its parts -- counts once, its first entry.)"""
    seen, once = set(), []
    for p in pool:
        if p[1] not in seen:
            seen.add(p[1])
            once.append(p)
    pool = once
    banks = [sorted((p for p in pool if p[2] == b), key=lambda p: (-p[0], p[1])) for b in range(F + 1)]
    at, out, b = [0] * (F + 1), [], F
    target = min(live, len(pool))
    while len(out) < target:
        if at[b] < len(banks[b]):
            out.append(banks[b][at[b]])
            at[b] += 1
        b = F if b == 0 else b - 1
    return out


def _met(rows_tokens, constraints, device, images=None):
    """The met masks of a step's logits rows as capnet_beam_topk_batched_forced takes them: int32 [rows] on the device.
    images (with a PerImage): the image of every row, whose own entry's forced ids are the row's (none: 0)."""
    return torch.tensor([met_mask(t, entry_of(constraints, None if images is None else images[r]).forced)
                         for r, t in enumerate(rows_tokens)], dtype=torch.int32, device=device)


def _bans(rows_tokens, step, end_token, constraints, device, images=None):
    """The ban lists of a step's logits rows as capnet_beam_topk[_batched]_banned takes them: int32 [rows, 1 + cap] on the
    device, per row its count and its words. images (with a PerImage): the image of every row, whose own entry is the row's
    rule (None: an empty list)."""
    lists = [banned_words(t, step, end_token, entry_of(constraints, None if images is None else images[r]))
             for r, t in enumerate(rows_tokens)]
    cap = max(1, max(len(b) for b in lists))
    return torch.tensor([[len(b)] + b + [0] * (cap - len(b)) for b in lists], dtype=torch.int32, device=device)


def _select(logits, scores, meta, rows_tokens, step, end_token, constraints, diversity, device, images=None):
    """One step's selection for the host loops, which hold the hypotheses: every logits row's ban list where there are
    constraints (removed after the log-sum-exp), every row's met mask where they force words, then ONE call.
    meta: [(first row, competing rows, k)] per image -- per (image, group) with diversity -- for capnet_beam_topk_batched and
    its _banned / _diverse / _forced forms -> (scores [n, 16], flat [n, 16]). A single such tuple: beam_search's one image ->
    (scores [k], flat [k]) from capnet_beam_topk[_banned], the single-image kernel, or under forced words from
    capnet_beam_topk_batched_forced with n = 1. rows_tokens: the token lists of the logits rows (None without constraints).
    constraints a PerImage (beam_search_batched; images: the image of every logits row): every row's list and mask under its
    own image's entry, and capnet_beam_topk_batched_rules, which reads every image's forced ids from the rule table."""
    if isinstance(constraints, PerImage):
        meta_d = torch.tensor(meta, dtype=torch.int32, device=device)
        bans = _bans(rows_tokens, step, end_token, constraints, device, images)
        met = (constraints, _met(rows_tokens, constraints, device, images), end_token)
        return ops.beam_topk_batched(logits, scores, meta_d, bans=bans, forced=met)
    forced = constraints is not None and bool(constraints.forced) and diversity is None
    if isinstance(meta, tuple) and not forced:
        _, rows, k = meta
        bans = None if constraints is None else _bans(rows_tokens[:rows], step, end_token, constraints, device)
        return ops.beam_topk(logits, scores, rows, k, bans=bans)
    meta_d = torch.tensor([meta] if isinstance(meta, tuple) else meta, dtype=torch.int32, device=device)
    bans = None if constraints is None else _bans(rows_tokens, step, end_token, constraints, device)
    met = (constraints, _met(rows_tokens, constraints, device), end_token) if forced else None
    scores_d, flat_d = ops.beam_topk_batched(logits, scores, meta_d, bans=bans, diversity=diversity, forced=met)
    return (scores_d[0, :meta[2]], flat_d[0, :meta[2]]) if isinstance(meta, tuple) else (scores_d, flat_d)


def beam_search(step_fn, state, vocab_size, start_token, end_token, k, max_seq_length, device, nbest=False, length_penalty=0.0,
                constraints=None):
    """step_fn(prev_words LongTensor[s], state) -> (logits [s, V], state'); `state` is a tuple of
    tensors whose leading dimension is the beam and which are re-indexed here when beams are
    re-ordered or retired. Returns LongTensor [1, L] (starts with start_token); nbest: the list of
    (LongTensor [1, L], score) of every completed sequence, rank_completed's order, empty where
    nothing completed."""
    k_prev_words = torch.full((k,), start_token, dtype=torch.long, device=device)
    seqs = [[int(start_token)] for _ in range(k)]
    top_k_scores = torch.zeros(k, dtype=torch.float32, device=device)
    complete_seqs, complete_seqs_scores = [], []
    step = 1
    while True:
        logits, state = step_fn(k_prev_words, state)
        # first step: all k beams are identical, only row 0 competes (model.py:240-242)
        rows = 1 if step == 1 else logits.shape[0]
        scores_d, flat_d = _select(logits, top_k_scores, (0, rows, k), seqs, step, end_token, constraints, None, device)
        scores = scores_d.tolist()
        flat = flat_d.tolist()
        prev_word_inds = [f // vocab_size for f in flat]
        next_word_inds = [f % vocab_size for f in flat]
        seqs = [seqs[p] + [w] for p, w in zip(prev_word_inds, next_word_inds)]
        incomplete_inds = [i for i, w in enumerate(next_word_inds) if w != end_token]
        complete_inds = [i for i, w in enumerate(next_word_inds) if w == end_token]
        for i in complete_inds:
            complete_seqs.append(seqs[i])
            complete_seqs_scores.append(scores[i])
        k -= len(complete_inds)
        if k == 0:
            break
        seqs = [seqs[i] for i in incomplete_inds]
        keep = torch.tensor([prev_word_inds[i] for i in incomplete_inds], dtype=torch.long,
                            device=device)
        state = tuple(s.index_select(0, keep) for s in state)
        top_k_scores = scores_d[torch.tensor(incomplete_inds, dtype=torch.long, device=device)]
        k_prev_words = torch.tensor([next_word_inds[i] for i in incomplete_inds], dtype=torch.long,
                                    device=device)
        if step > max_seq_length:
            break
        step += 1
    if nbest:
        return [(torch.tensor([q], dtype=torch.long, device=device), sc)
                for q, sc in rank_completed(list(zip(complete_seqs_scores, complete_seqs)), length_penalty)]
    if not complete_seqs_scores:   # "prevent empty sequence", model.py:287-289
        return torch.tensor([[int(end_token)]], dtype=torch.long, device=device)
    best = complete_seqs_scores.index(max(complete_seqs_scores))
    return torch.tensor([complete_seqs[best]], dtype=torch.long, device=device)


def beam_search_device(step_fn, state, n, vocab_size, start_token, end_token, k, max_seq_length, device, poll_every=0,
                       nbest=False, length_penalty=0.0, constraints=None, diversity=None):
    """beam_search_batched with the bookkeeping on the device (capnet_beam_advance): no host read and no host-built
    tensor per step. Image i keeps rows i k .. i k + k - 1 for the whole search -- its live beams in its first slots, in
    the order beam_search_batched keeps them; dead slots still take the decoder step, their logits are never read -- so
    every step runs on n k rows, and `state` is re-indexed by the parent rows the kernel wrote. T = max_seq_length + 1
    steps, all the host loop can run; then capnet_beam_finish picks the winners and ONE copy brings sequences and lengths
    to the host. poll_every = m > 0: after every m-th step the count of live beams is read (one blocking 4-byte copy)
    and the loop stops at zero -- same result, for decoders whose beams end long before T.
    Returns a list of n token lists (each starts with start_token); nbest: per image the list of (tokens, score) of its
    completed hypotheses, best first (capnet_beam_nbest in capnet_beam_finish's place, still one copy).
    diversity (an active Diversity whose groups divide k): the state is that of n D searches of k / D beams, every step
    selects with capnet_beam_advance_diverse, and the result is per image merge_groups of its groups' completed lists
    (read with capnet_beam_nbest, one copy)."""
    if k > 16 or k > vocab_size:
        raise ops.CapnetError("beam_search_device: k <= 16 and k <= vocab_size")
    if isinstance(constraints, PerImage) and (diversity is not None or len(constraints) != n):
        raise ops.CapnetError("beam_search_device: a PerImage takes an entry per image and no diversity")
    T = max_seq_length + 1
    words = [torch.empty(n * k, dtype=torch.long, device=device) for _ in range(2)]
    parent_rows = torch.empty(n * k, dtype=torch.long, device=device)
    D = 1 if diversity is None else diversity.groups
    beam = ops.beam_init(n * D, k // D, T, start_token, words[0])
    prev_words = words[0]
    for step in range(1, T + 1):
        logits, state = step_fn(prev_words, state)
        if logits.shape[1] != vocab_size:
            raise ops.CapnetError("beam_search_device: the step returned %d columns, vocab_size is %d" % (logits.shape[1], vocab_size))
        next_words = words[step & 1]
        # (the sequences stay in the beam state: the selecting workgroup derives the exclusions from them, and with diversity
        # walks the image's groups in order)
        ops.beam_advance(beam, logits, step, end_token, next_words, parent_rows, constraints=constraints, diversity=diversity)
        if poll_every > 0 and step % poll_every == 0 and step < T and not int(beam.live_total.item()):
            break
        state = tuple(s.index_select(0, parent_rows) for s in state)
        prev_words = next_words
    if diversity is not None:
        per = ops.nbest_lists(ops.beam_nbest(beam, end_token, 0.0)[-1], n * D, k // D, T + 2)[0]
        return [merge_groups([by_completion(per[i * D + g]) for g in range(D)], end_token, diversity, nbest, length_penalty)
                for i in range(n)]
    if nbest:
        packed = ops.beam_nbest(beam, end_token, length_penalty)[-1]
        return ops.nbest_lists(packed, n, k, T + 2)[0]
    seqs, lengths, packed = ops.beam_finish(beam, end_token)
    host = packed.cpu()
    L = seqs.shape[1]
    lens = host[n * L:].view(torch.int32)[:n].tolist()
    rows = host[:n * L].view(n, L).tolist()
    return [rows[i][:lens[i]] for i in range(n)]


def beam_search_batched(step_fn, state, n, vocab_size, start_token, end_token, k, max_seq_length, device, nbest=False,
                        length_penalty=0.0, constraints=None, diversity=None):
    """beam_search for n images at once: the evaluator of the reference (stylenet/evaluator.py:63-120) calls sample() per
    test image, k rows per decode step; here the beams of ALL images advance together -- one decoder step over sum(live
    beams) rows and one capnet_beam_topk_batched launch per step -- with per image exactly beam_search's bookkeeping
    (first step: row 0 only; <end> retires a beam; the best completed sequence wins; empty -> [<end>]).
    `state`: tuple of tensors with n * k leading rows (image i's k beams at rows i k .. i k + k - 1).
    Returns a list of n token lists (each starts with start_token); nbest: per image rank_completed of its completed list.
    constraints: a Constraints for all images, or a PerImage of n entries (without diversity): every row under its own image's.
    diversity (an active Diversity whose groups divide k): the bookkeeping below is kept per (image, group) -- n D searches
    of k / D beams, group g of image i at rows (i D + g) k / D .. -- and every step selects with
    capnet_beam_topk_batched_diverse, one workgroup per image walking its groups; the result is merge_groups per image."""
    if k > 16:
        raise ops.CapnetError("beam_search_batched: k <= 16")
    if isinstance(constraints, PerImage) and (diversity is not None or len(constraints) != n):
        raise ops.CapnetError("beam_search_batched: a PerImage takes an entry per image and no diversity")
    D = 1 if diversity is None else diversity.groups
    n_img, n, k = n, n * D, k // D
    live = [k] * n                                           # beams still open per image
    seqs = [[[int(start_token)] for _ in range(k)] for _ in range(n)]
    done = [[] for _ in range(n)]                            # (score, sequence) of completed beams
    prev_words = torch.full((n * k,), start_token, dtype=torch.long, device=device)
    top_scores = torch.zeros(n * k, dtype=torch.float32, device=device)
    step = 1
    while True:
        logits, state = step_fn(prev_words, state)
        row0, meta = 0, []
        for i in range(n):
            meta.append((row0, (1 if step == 1 else live[i]) if live[i] else 0, live[i]))
            row0 += live[i]
        live_seqs = None if constraints is None else [q for i in range(n) for q in seqs[i]]     # image i's live beams in order
        images = [i for i in range(n) for _ in seqs[i]] if isinstance(constraints, PerImage) else None
        scores_d, flat_d = _select(logits, top_scores, meta, live_seqs, step, end_token, constraints, diversity, device, images)
        scores, flat = scores_d.tolist(), flat_d.tolist()
        keep_rows, next_words, next_scores = [], [], []
        for i in range(n):
            if not live[i]:
                continue
            r0 = meta[i][0]
            new_seqs = []
            for j in range(live[i]):
                p, w = flat[i][j] // vocab_size, flat[i][j] % vocab_size
                sq = seqs[i][p] + [w]
                if w == end_token:
                    done[i].append((scores[i][j], sq))
                else:
                    new_seqs.append(sq)
                    keep_rows.append(r0 + p)
                    next_words.append(w)
                    next_scores.append(scores[i][j])
            seqs[i] = new_seqs
            live[i] = len(new_seqs)
        if not keep_rows or step > max_seq_length:
            break
        keep = torch.tensor(keep_rows, dtype=torch.long, device=device)
        state = tuple(s.index_select(0, keep) for s in state)
        prev_words = torch.tensor(next_words, dtype=torch.long, device=device)
        top_scores = torch.tensor(next_scores, dtype=torch.float32, device=device)
        step += 1
    if diversity is not None:
        return [merge_groups(done[i * D:(i + 1) * D], end_token, diversity, nbest, length_penalty) for i in range(n_img)]
    if nbest:
        return [rank_completed(done[i], length_penalty) for i in range(n)]
    out = []
    for i in range(n):
        if not done[i]:
            out.append([int(end_token)])
        else:
            best = max(range(len(done[i])), key=lambda q: (done[i][q][0], -q))       # first maximum, as list.index(max(...))
            out.append(done[i][best][1])
    return out
