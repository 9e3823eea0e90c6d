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
"""
import math
from collections import Counter


def _ngrams(tokens, n):
    return Counter(tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1))


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
