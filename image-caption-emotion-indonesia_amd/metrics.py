"""Host-side caption metrics of the validation loop.

corpus_bleu: BLEU-4 as the reference calls it (`nltk.translate.bleu_score.corpus_bleu(references,
hypotheses)` with default weights, stylenet/train_multitask.py:341). nltk is not installable here,
so this is a restatement of the published definition (Papineni et al. 2002: clipped n-gram
precisions pooled over the corpus, uniform weights over n = 1..4, brevity penalty against the
closest reference length). Pinned to nltk only through the worked example of nltk's own docstring
(corpus 0.5920..., sentence 0.5045... / 0.7400...; tests/test_oracle_cpu.py) plus hand-computed
corpora; anything that example does not exercise is parity unpinned. Where nltk's default
smoothing substitutes `sys.float_info.min` for an empty n-gram match count, this returns 0.0.
Token lists are lists of ints; pure Python, runs on the host like the reference's.

sentence_bleu: BLEU of one hypothesis, optionally with Lin & Och's add-one smoothing (no counterpart in the reference; the
oracle of capnet.ops.bleu_rows); sentence_stats: its integers.

CiderCorpus / cider_d_parts / sentence_cider_d / corpus_cider_d: CIDEr-D (Vedantam et al. 2015) as the COCO caption tools'
cider_scorer forms it (no counterpart in the reference, which reports BLEU only; the reward self-critical training was
published with, and the oracle of capnet.ops.cider_rows). The original tool is not available here, so this is a restatement
of the published definition: per order n = 1..4 a tf-idf vector per sentence, idf(g) = ln N - ln max(1, df(g)) with df
counted over the N images of a corpus; per reference the clipped similarity sum_g min(v_h(g), v_r(g)) v_r(g) /
(|v_h| |v_r|) times the Gaussian length penalty exp(-(len h - len r)^2 / (2 sigma^2)), sigma = 6; the mean over the image's
references, then 10 x the mean over n. Pinned by that definition and by worked cases in closed form (a two-image corpus:
2.5 e^(-1/72) (1/sqrt 2 + 1/sqrt 6) and the "-D" clipping's 2.5 e^(-1/72) 2/(3 sqrt 2), a copy's 10.0, a one-image corpus'
0.0; tests/test_cider_cpu.py); parity with the tool beyond what those exercise is unpinned. Tokens are taken as they are.
"""
import math
from collections import Counter


def _ngrams(tokens, n):
    return Counter(tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1))


def distinct_n(list_of_token_lists, n):
    """Distinct n-grams divided by total n-grams over the given token lists (Li et al. 2016's distinct-n, the usual number
    for how different a set of captions is; tokens are taken as they are). 0.0 where there is no n-gram at all."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError("distinct_n: n must be an int >= 1, not %r" % (n,))
    seen, total = set(), 0
    for tokens in list_of_token_lists:
        tokens = [int(w) for w in tokens]
        for i in range(len(tokens) - n + 1):
            seen.add(tuple(tokens[i:i + n]))
            total += 1
    return len(seen) / float(total) if total else 0.0


def _closest_ref_length(refs, hyp_len):
    return min((len(r) for r in refs), key=lambda rl: (abs(rl - hyp_len), rl))


def corpus_bleu(list_of_references, hypotheses, weights=(0.25, 0.25, 0.25, 0.25)):
    assert len(list_of_references) == len(hypotheses), \
        "The number of hypotheses and their reference(s) should be the same"
    num = [0] * len(weights)
    den = [0] * len(weights)
    hyp_lengths, ref_lengths = 0, 0
    for refs, hyp in zip(list_of_references, hypotheses):
        for i in range(len(weights)):
            counts = _ngrams(hyp, i + 1)
            max_counts = Counter()
            for r in refs:
                rc = _ngrams(r, i + 1)
                for g in counts:
                    max_counts[g] = max(max_counts[g], rc[g])
            num[i] += sum(min(c, max_counts[g]) for g, c in counts.items())
            den[i] += max(1, sum(counts.values()))
        hyp_lengths += len(hyp)
        ref_lengths += _closest_ref_length(refs, len(hyp))
    if hyp_lengths == 0 or num[0] == 0:
        return 0.0
    bp = 1.0 if hyp_lengths > ref_lengths else math.exp(1.0 - ref_lengths / hyp_lengths)
    if any(n == 0 for n in num):
        return 0.0
    return bp * math.exp(sum(w * math.log(n / d) for w, n, d in zip(weights, num, den)))


def sentence_stats(references, hypothesis, orders=4):
    """The integers sentence BLEU is made of, as ops.bleu_rows reports them: [num_1 .. num_orders, den_1 .. den_orders, the
    hypothesis length, the closest reference length] -- corpus_bleu's clipped counts, totals and lengths of one sentence."""
    num, den = [], []
    for n in range(1, orders + 1):
        counts = _ngrams(hypothesis, n)
        ref_counts = [_ngrams(r, n) for r in references]
        num.append(sum(min(c, max(rc[g] for rc in ref_counts)) for g, c in counts.items()))
        den.append(max(1, sum(counts.values())))
    return num + den + [len(hypothesis), _closest_ref_length(references, len(hypothesis))]


def sentence_bleu(references, hypothesis, weights=(0.25, 0.25, 0.25, 0.25), smooth=0):
    """BLEU of ONE hypothesis against its references. smooth=0: corpus_bleu([references], [hypothesis], weights) itself, which
    is 0.0 whenever some n-gram order has no match -- nearly every caption early in training. smooth=1: Lin & Och's (2004)
    add-one, (num_n + 1) / (den_n + 1) in place of num_n / den_n for n >= 2; then 0.0 only where no word matches. The
    reward capnet.ops.bleu_rows computes on the device."""
    if smooth not in (0, 1):
        raise ValueError("smooth %r (0: none, 1: add one for n >= 2)" % (smooth,))
    if not smooth:
        return corpus_bleu([references], [hypothesis], weights)
    k = len(weights)
    st = sentence_stats(references, hypothesis, k)
    num, den, hyp_len, ref_len = st[:k], st[k:2 * k], st[2 * k], st[2 * k + 1]
    if hyp_len == 0 or num[0] == 0:
        return 0.0
    bp = 1.0 if hyp_len > ref_len else math.exp(1.0 - ref_len / hyp_len)
    return bp * math.exp(sum(w * math.log((n + (i > 0)) / (d + (i > 0))) for i, (w, n, d) in enumerate(zip(weights, num, den))))


class CiderCorpus(object):
    """The document frequencies CIDEr-D weighs n-grams by. list_of_reference_sets [image][reference][word]: df(g) is the
    number of images with at least one reference that contains the n-gram g (n = 1..4), N the number of images, and
    idf(g) = ln N - ln max(1, df(g)) -- ln N for an n-gram the corpus never saw, and 0 for everything where N is 1. Empty
    references are skipped. Tokens must be non-negative and fit int32 (ValueError otherwise): the device tables hold them so.
    Normally built once from the whole training set and shared by every batch's DeviceCiderReward."""

    ORDERS = 4

    def __init__(self, list_of_reference_sets):
        sets = [[[int(w) for w in r] for r in refs if len(r)] for refs in list_of_reference_sets]
        if not sets:
            raise ValueError("CiderCorpus: no images")
        if any(w < 0 or w > 2 ** 31 - 1 for refs in sets for r in refs for w in r):
            raise ValueError("CiderCorpus: tokens must be non-negative and fit int32")
        self.N = len(sets)
        self.log_n = math.log(float(self.N))
        self.df = [Counter() for _ in range(self.ORDERS)]
        for refs in sets:
            for n in range(1, self.ORDERS + 1):
                self.df[n - 1].update(set(g for r in refs for g in _ngrams(r, n)))
        self._tables, self._on = None, {}

    def idf(self, g):
        """idf of the n-gram g (a tuple of 1 to 4 words)."""
        g = tuple(int(w) for w in g)
        return self.log_n - math.log(float(max(1, self.df[len(g) - 1].get(g, 0))))

    def vectors(self, tokens):
        """The tf-idf vectors of one sentence: ([{g: tf(g) * idf(g)} for n = 1..4], [norm_1 .. norm_4]), each dict in order
        of first occurrence and each norm the square root of the squares summed in that order."""
        vecs, norms = [], []
        for n in range(1, self.ORDERS + 1):
            vec = {g: float(c) * self.idf(g) for g, c in _ngrams(tokens, n).items()}
            vecs.append(vec)
            norms.append(math.sqrt(sum((v * v for v in vec.values()), 0.0)))
        return vecs, norms

    def tables(self):
        """Four (keys, idf) pairs on the host, one per order n: keys int32 [count_n, n] in ascending lexicographic order, idf
        float64 [count_n] = idf(key) as computed here -- the device looks these very values up (capnet.ops.cider_rows)."""
        if self._tables is None:
            import torch
            out = []
            for n in range(1, self.ORDERS + 1):
                keys = sorted(self.df[n - 1])
                out.append((torch.tensor(keys, dtype=torch.int32).reshape(len(keys), n),
                            torch.tensor([self.idf(g) for g in keys], dtype=torch.float64)))
            self._tables = tuple(out)
        return self._tables

    def on(self, device):
        """tables() on `device`, uploaded at the first call for it."""
        import torch
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = tuple((k.to(device), v.to(device)) for k, v in self.tables())
        return self._on[device]


def cider_d_parts(corpus, references, hypothesis, sigma=6.0):
    """[part_1 .. part_4] of one hypothesis against its image's references: part_n the mean over the non-empty references of
    sim_n (the module docstring), summed over the hypothesis' distinct n-grams in order of first occurrence."""
    if not float(sigma) > 0.0:
        raise ValueError("sigma %r (must be positive)" % (sigma,))
    hypothesis = [int(w) for w in hypothesis]
    references = [[int(w) for w in r] for r in references if len(r)]
    vec_h, norm_h = corpus.vectors(hypothesis)
    sums = [0.0] * corpus.ORDERS
    for r in references:
        vec_r, norm_r = corpus.vectors(r)
        d = float(len(hypothesis) - len(r))
        penalty = math.exp(-(d * d) / (2.0 * sigma * sigma))
        for n in range(corpus.ORDERS):
            raw = 0.0
            for g, vh in vec_h[n].items():
                vr = vec_r[n].get(g, 0.0)
                raw += min(vh, vr) * vr
            if norm_h[n] != 0.0 and norm_r[n] != 0.0:
                raw /= norm_h[n] * norm_r[n]
            sums[n] += raw * penalty
    return [s / len(references) if references else 0.0 for s in sums]


def sentence_cider_d(corpus, references, hypothesis, sigma=6.0):
    """CIDEr-D of ONE hypothesis against its image's references, in [0, 10]: 10 x the mean of cider_d_parts. The reward
    capnet.ops.cider_rows computes on the device."""
    p = cider_d_parts(corpus, references, hypothesis, sigma)
    return 2.5 * (p[0] + p[1] + p[2] + p[3])


def corpus_cider_d(list_of_references, hypotheses, corpus=None, sigma=6.0):
    """(mean, [per sentence]) CIDEr-D of hypotheses[i] against list_of_references[i]. corpus=None: the document frequencies
    are those of list_of_references itself, as the COCO scorer takes them on a test split."""
    assert len(list_of_references) == len(hypotheses), \
        "The number of hypotheses and their reference(s) should be the same"
    if corpus is None:
        corpus = CiderCorpus(list_of_references)
    scores = [sentence_cider_d(corpus, refs, hyp, sigma) for refs, hyp in zip(list_of_references, hypotheses)]
    return (sum(scores) / len(scores) if scores else 0.0), scores
