"""Inputs shared by tests/test_cider_cpu.py and tests/test_cider_gpu.py: corpora, decoded rows and references for CIDEr-D
(capnet.metrics.CiderCorpus / cider_d_parts / sentence_cider_d, ops.cider_rows). TEST INFRASTRUCTURE.

Rows, the hypothesis rule, NAMED and sweep are caption_reward_cases' (imported, not copied). Added here: the two-image corpus
of the worked cases with their closed forms, corpora whose tables have a chosen number of keys per order (lookup edges),
and seeded random corpora."""
import math
import random

from caption_reward_cases import END, NAMED, START, STEPS, hypothesis, sweep  # noqa: F401

# ---- the worked cases: corpus of two images, every hypothesis scored against the listed references -------------------------
A, B = [[1, 3, 4, 2]], [[1, 5, 2]]
WORKED_CORPUS = [A, B]
_E = math.exp(-1.0 / 72.0)
# (hypothesis, references, score, parts or None)
WORKED = [
    # <start> 3 <end> against <start> 3 4 <end>: unigrams 3 (idf ln 2; <start> and <end> are in both images: idf 0), bigram (1, 3)
    ([1, 3, 2], A, 2.5 * _E * (1 / math.sqrt(2) + 1 / math.sqrt(6)), [_E / math.sqrt(2), _E / math.sqrt(6), 0.0, 0.0]),
    # the "-D" clipping: three 3s against one -- min(3 idf, idf) idf, but the hypothesis' norm carries all three
    ([1, 3, 3, 3, 2], A, 2.5 * _E * 2 / (3 * math.sqrt(2)), [_E / (3 * math.sqrt(2)), _E / (3 * math.sqrt(2)), 0.0, 0.0]),
    ([1, 3, 4, 2], A, 10.0, [1.0, 1.0, 1.0, 1.0]),
    ([1, 3, 4, 2], A + [[]], 10.0, [1.0, 1.0, 1.0, 1.0]),                 # an empty reference slot is not a reference
    ([1, 3, 4, 2], [[1, 3, 4, 2], [1, 5, 2]], 5.0, None),
]
WORKED_VALUES = [2.749927773395139, 1.1622562331734, 10.0, 10.0, 5.0]     # the same scores as decimals
WORKED_PARTS = [[0.69735373990, 0.40261736945, 0.0, 0.0], [0.2324512466, 0.2324512466, 0.0, 0.0]]   # and the first two's parts


def row(words, steps=STEPS):
    """The `steps` ids a sampler would leave for the hypothesis [START] + words + [END]."""
    assert len(words) + 1 <= steps
    return [int(w) for w in words] + [END] + [0] * (steps - len(words) - 1)


def random_corpus(images, V, seed, lo=3, hi=12, max_refs=4):
    """`images` reference sets of one to max_refs random references of lo..hi words over V words."""
    rng = random.Random(seed)
    return [[[rng.randrange(V) for _ in range(rng.randint(lo, hi))] for _ in range(rng.randint(1, max_refs))]
            for _ in range(images)]


def oracle_stats(corpus, hyp):
    """ops.cider_rows' nine integers: the length, the distinct n-grams per order, and how many of them the corpus holds."""
    grams = [set(tuple(hyp[i:i + n]) for i in range(len(hyp) - n + 1)) for n in range(1, 5)]
    return [len(hyp)] + [len(g) for g in grams] + [sum(1 for x in g if x in corpus.df[n]) for n, g in enumerate(grams)]


# ---- lookup edges ----------------------------------------------------------------------------------------------------------
EDGE_KEYS = (1, 2, 3, 7, 8, 9)


def edge_corpus(K):
    """A corpus whose table has exactly K keys in EVERY order: one reference that walks a cycle of K words (10, 20, ..) for
    K + 3 steps has K distinct n-grams for n = 1..4; two more images hold pieces of the same walk, so they add no key but
    make the document frequencies, and so the idf values, differ between keys."""
    cyc = [10 * (1 + i % K) for i in range(K + 3)]
    return [[cyc], [cyc[:max(1, (K + 3) // 2)]], [cyc[1:3]]]


def edge_rows(corpus, steps=STEPS):
    """Rows whose n-grams sit at the edges of order n's table, for every n: the first key, the last key, an n-gram below the
    first key and one above the last, and every key's neighbours that equal it in all but the last word (first and last
    key only). `corpus` a capnet.metrics.CiderCorpus."""
    rows = []
    for n in range(1, 5):
        keys = sorted(corpus.df[n - 1])
        rows += [row([3] * n, steps), row([99] * n, steps)]
        for k in ((keys[0], keys[-1]) if keys else ()):
            k = list(k)
            rows += [row(k, steps), row(k[:-1] + [k[-1] + 1], steps), row(k[:-1] + [k[-1] - 1], steps)]
    return rows


def three_word_corpus():
    """No 4-gram anywhere: every reference has three words, so count_4 == 0."""
    return [[[1, 3, 2], [1, 4, 2]], [[1, 5, 2]], [[3, 4, 5]], [[1, 3, 5], [5, 4, 2]]]
