"""Inputs shared by tests/test_seq2seq_beam_styles_cpu.py (the rule) and tests/test_seq2seq_beam_styles_gpu.py (the runs):
Seq2Seq.sample_beam_styles against the fp64 restatement of sample_beam, mode by mode. TEST INFRASTRUCTURE.

A style case is ONE seed and a list of modes: one seq2seq_beam_cases.Case per mode, all on the same parameters and the
same features (Case draws both from the seed alone), so the emotions start from the same encoder run, as they do in
sample_beam_styles.

THE RULE is seq2seq_beam_cases', per mode: every mode's Case clears it (Case.clears()) with that Case's OWN <end> (the fifth
token of sentence 0's greedy decode in that mode); tests/test_seq2seq_beam_styles_cpu.py asserts that for every case below,
and nothing is skipped on the GPU. sample_beam_styles takes one <end> for all modes, and a mode's margins are not known at
another mode's <end>. So the GPU test calls it once per listed mode m with m's <end>: entry m is compared with the
restatement (StyleCase.reference), and every other entry with sample_beam(mode=...) at the same <end> on the same step,
which is the same arithmetic bit for bit and needs no margin.
The seeds are fixed; search() is how the composed one was found."""
from seq2seq_beam_cases import KS, Case

EMOTIONS = ("happy", "sad", "angry")
ALL_MODES = ("factual",) + EMOTIONS


class StyleCase:
    def __init__(self, name, E, H, V, L, rows, seed, modes, out_scale, lstm_scale, ks=KS):
        self.name, self.E, self.H, self.V, self.L, self.rows, self.seed = name, E, H, V, L, rows, seed
        self.modes, self.ks = tuple(modes), tuple(ks)
        self.cases = {m: Case("%s-%s" % (name, m), E, H, V, L, rows, seed, m, out_scale, lstm_scale, ks) for m in self.modes}

    def __repr__(self):
        return self.name

    @property
    def emotions(self):
        return tuple(m for m in self.modes if m != "factual")

    @property
    def features(self):
        """[rows, E] fp64, the same for every mode."""
        return self.cases[self.modes[0]].features

    def module(self):
        return self.cases[self.modes[0]].module()

    def end(self, mode):
        return self.cases[mode].end

    def reference(self, k, mode):
        """What sample_beam_styles returns under `mode` when it is called with end(mode): the list of every sentence."""
        return [self.cases[mode].reference(k, r) for r in range(self.rows)]

    def clears(self):
        return all(c.clears() for c in self.cases.values())


def search(E, H, V, L, rows, modes, out_scale, lstm_scale, ks=KS, seeds=range(40)):
    """The first seed at which every mode of `modes` clears the rule, or None (seq2seq_beam_cases.search for a list of
    modes)."""
    for seed in seeds:
        if StyleCase("probe", E, H, V, L, rows, seed, modes, out_scale, lstm_scale, ks).clears():
            return seed
    return None


SMALL = dict(E=12, H=64, V=37, L=2, out_scale=24.0, lstm_scale=3.0)

CASES = [
    # 15 rows per group at k = 5: groups start off the 16-row tile; two workgroups, the last ragged
    StyleCase("small-all", rows=3, seed=50, modes=ALL_MODES, **SMALL),
    StyleCase("small-all-b", rows=3, seed=104, modes=ALL_MODES, **SMALL),
    # an embedding width off 4: scalar loads from per-group tables; one layer
    StyleCase("e10-l1", 10, 64, 37, 1, 3, 23, EMOTIONS, 24.0, 3.0),
    StyleCase("l3", 12, 64, 37, 3, 3, 45, EMOTIONS, 24.0, 3.0),
    # 20 rows per group at k = 5: a group spans two row tiles, the merge at 16 lanes per row
    StyleCase("rows4", rows=4, seed=313, modes=EMOTIONS, **SMALL),
    # 35 rows per group: two passes of the row walk
    StyleCase("rows7", rows=7, seed=49, modes=("sad", "angry"), ks=(5,), **SMALL),
    # 36 rows per group, k near its limit
    StyleCase("k12", rows=3, seed=3, modes=("happy", "sad"), ks=(12,), **SMALL),
    # seven workgroups, the last ragged, H = 128
    StyleCase("mid", 30, 128, 211, 1, 3, 220, ("sad", "angry"), 32.0, 3.0),
    # the real shape: 3 x 256 workgroups
    StyleCase("full", 300, 512, 8192, 2, 2, 180, EMOTIONS, 64.0, 2.0, ks=(5,)),
]

# a hidden size the decode step does not take (seq2seq_beam_cases' h16 shape): one search after the other on the composed
# step. search(12, 16, 37, 1, 3, ("factual", m), 24.0, 3.0, seeds=range(200)) gives 27 for happy, 0 for sad, 25 for angry
COMPOSED_MODES, COMPOSED_SEED = ("factual", "sad"), 0
COMPOSED = [StyleCase("h16", 12, 16, 37, 1, 3, COMPOSED_SEED, COMPOSED_MODES, 24.0, 3.0)]


def case(name):
    return [c for c in CASES + COMPOSED if c.name == name][0]
