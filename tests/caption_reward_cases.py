"""Inputs shared by tests/test_caption_reward_cpu.py and tests/test_caption_reward_gpu.py: decoded rows and references for
sentence BLEU (capnet.metrics.sentence_bleu, ops.bleu_rows). TEST INFRASTRUCTURE.

A row is what a sampler leaves on the device: `steps` ids; its hypothesis is [START] + the ids through the first END
inclusive, or all of them (hypothesis(), the rule of capnet.decode.cut_samples). NAMED: one row per image, each with its own
references, so the batch also has ragged reference counts (one to four)."""
import random

START, END, STEPS = 1, 2, 8
WEIGHTS = (0.25, 0.25, 0.25, 0.25)

# name -> (ids [STEPS], references)
NAMED = {
    # one word four times against a reference that holds it twice: the unigram count is clipped to 2, the bigram (5, 5) to 1
    "clipped": ([5, 5, 5, 5, END, 0, 0, 0], [[START, 5, 5, 6, END]]),
    # two references with one occurrence each: the MAXIMUM over references (1), not their sum (2)
    "max_not_sum": ([5, 5, END, 0, 0, 0, 0, 0], [[START, 5, 6, END], [START, 7, 5, END]]),
    # [start, end]: two words, no 3-gram and no 4-gram (their totals are max(1, .) = 1, their matches 0)
    "start_end": ([END, 0, 0, 0, 0, 0, 0, 0], [[START, END], [START, 3, END]]),
    # no <end> in the STEPS columns: all of them
    "no_end": ([3, 4, 5, 6, 7, 3, 4, 5], [[START, 3, 4, 5, 6, 7, 3, 4, 5, END], [START, 3, 4, 5, 6, END]]),
    # <end> at column 0, reference words behind it: ignored
    "end_first": ([END, 3, 4, 5, 6, END, 3, 4], [[START, 3, 4, 5, 6, END]]),
    # hypothesis of 6 words, references of 5 and 7: the tie goes to the shorter, so the hypothesis is LONGER than it (bp = 1)
    "length_tie": ([3, 4, 5, 6, END, 0, 0, 0], [[START, 3, 4, 5, END], [START, 3, 4, 5, 6, 7, END]]),
    # the brevity penalty on both sides of its branch: equal lengths (bp = exp(0)), a shorter and a longer hypothesis
    "equal_length": ([3, 4, 5, 6, END, 0, 0, 0], [[START, 3, 4, 5, 7, END]]),
    "shorter": ([3, 4, 5, END, 0, 0, 0, 0], [[START, 3, 4, 5, 6, 7, 8, END]]),
    "longer": ([3, 4, 5, 6, 7, 8, END, 0], [[START, 3, 4, 5, END]]),
    # an exact copy of a reference: 1.0
    "copy": ([3, 4, 5, 6, END, 0, 0, 0], [[START, 3, 4, 5, 6, END]]),
    # four references beside the images with one
    "four_refs": ([3, 4, 5, 6, 7, END, 0, 0], [[START, 3, 4, 9, END], [START, 4, 5, 6, 7, END], [START, 3, END],
                                             [START, 9, 9, 3, 4, 5, 6, 8, 8, END]]),
    # no word in common beyond <start>: no bigram match
    "no_match": ([9, 9, 9, 9, 0, 0, 0, 0], [[START, 3, 4, 5, END]]),
}


def hypothesis(ids, steps=None):
    ids = [int(w) for w in ids[:steps]]
    keep = ids.index(END) + 1 if END in ids else len(ids)
    return [START] + ids[:keep]


def sweep(rows=256, per_image=1, V=6, steps=12, seed=0):
    """(ids [rows][steps], references per image): random rows over V words (START and END among them, so ends fall anywhere)
    and one to four random references of 3 to 12 words per image."""
    rng = random.Random(1000 * per_image + seed)
    ids = [[rng.randrange(V) for _ in range(steps)] for _ in range(rows)]
    images = (rows + per_image - 1) // per_image
    refs = [[[rng.randrange(V) for _ in range(rng.randint(3, 12))] for _ in range(rng.randint(1, 4))] for _ in range(images)]
    return ids, refs
