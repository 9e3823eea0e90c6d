"""What each of the 23 exported sampling entries says when one of its arguments is wrong, byte for byte.

The entries share their argument checks below the C ABI; which function holds a check is free to change, the text a caller
reads is not: the name in front (the _greedy and _masked entries report under the base name, capnet_nucleus_rows /
capnet_nucleus_pick at top_p == 1 forward and report as sample_rows / sample_pick), the rule for top_p (the plain loops have
none, the _nucleus loops admit 0 < top_p < 1, the _excl loops and the stand-alone draws 0 < top_p <= 1), the slab and the
start tokens an entry requires.

Every entry has a base argument set that passes every host check -- dummy aligned pointers, never dereferenced, wcat / beff
real one-element tables of them since the layer check reads them -- and the base set itself is never called: each case breaks
exactly one thing in it, so every call is refused on the host, nothing is launched and no GPU is needed. (Where top_p == 1 is
itself valid, the case pairs it with temperature 0 to read the name the message comes under.) The return is non-zero and
capnet_last_error() equals tests/sample_entries_expected.json. That table was recorded ONCE from a build of the commit before
the entries were merged, by running this file with CAPNET_RECORD_SAMPLE_ENTRIES=<path of the table to write>; no normal
run sets it, and it is never recorded from the code under test. One fault per case: the order of the checks inside an entry
is not pinned here."""
import ctypes as C
import json
import os

import pytest

import capnet

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sample_entries_expected.json")
RECORD = os.environ.get("CAPNET_RECORD_SAMPLE_ENTRIES")
ROWS, E, H, V, STEPS = 2, 16, 64, 37, 12
ATT = dict(n=1, m=2, P=4, A=16, C=512)
NAN = float("nan")


def ptr():
    return C.c_void_p(16)


def off():
    return C.c_void_p(18)            # misaligned for every pointer class (16, 8 and 4 bytes)


def table_of(p):
    return (C.c_void_p * 1)(p)


def _draw(kind, top_p=False, greedy=False, masked=False):
    """The stand-alone draws: (argument, base value) in the order of the C signature."""
    head = {"vocab": [("h", ptr()), ("w", ptr()), ("b", None), ("rows", ROWS), ("H", H), ("V", V)],
            "pick": [("values", ptr()), ("index", ptr()), ("rows", ROWS), ("k", 5), ("V", V)],
            "rows": [("logits", ptr()), ("rows", ROWS), ("ld", V), ("V", V)]}[kind]
    a = head + [("temperature", 1.0)] + ([("top_p", 0.5)] if top_p else []) + [("seed", 0), ("step", 0), ("row0", 0)]
    a += ([("mask", ptr())] if masked else []) + ([("workspace", ptr())] if kind == "vocab" else [])
    a += [("tokens", ptr()), ("logp", ptr())] + ([("greedy_stride", 0)] if greedy or masked else []) + [("stream", None)]
    return a


EXCL = [("end_token", 2), ("no_repeat_ngram", 1), ("min_words", 0), ("banned", None), ("n_banned", 0)]


def _loop(att, top_p=None, greedy=False, excl=False):
    """The one-call loops. Under exclusions the first input is the start tokens; else first_inputs (the plain stacks)."""
    if att:
        a = [("cell", 0), ("nlayers", 1), ("n", ATT["n"]), ("m", ATT["m"]), ("P", ATT["P"]), ("A", ATT["A"]), ("C", ATT["C"]), ("E", E),
             ("H", H), ("V", V), ("steps", STEPS), ("start_tokens", ptr()), ("att1", ptr()), ("feat", ptr()), ("emb", ptr()),
             ("wz", ptr()), ("bz", ptr()), ("w_full", ptr()), ("b_full", ptr())]
    else:
        a = [("cell", 0), ("nlayers", 1), ("rows", ROWS), ("E", E), ("H", H), ("V", V), ("steps", STEPS),
             ("first_inputs", None if excl else ptr()), ("start_tokens", ptr() if excl else None), ("emb", ptr())]
    a += [("wcat", table_of(16)), ("beff", table_of(16)), ("Cw", ptr()), ("Cb", None), ("state0", ptr()), ("temperature", 1.0),
          ("top_k", 0)] + ([("top_p", top_p)] if top_p else []) + [("seed", 0), ("workspace", ptr())]
    a += ([("slab", ptr()), ("slab_floats", 1 << 20)] if att or top_p else [])
    a += [("ids", ptr()), ("logp", ptr()), ("state_out", None), ("err_flag", ptr())]
    return a + ([("greedy_stride", 0)] if greedy or excl else []) + (EXCL if excl else []) + [("stream", None)]


ENTRIES = {
    "capnet_vocab_sample": _draw("vocab"),
    "capnet_vocab_sample_greedy": _draw("vocab", greedy=True),
    "capnet_vocab_sample_masked": _draw("vocab", masked=True),
    "capnet_sample_pick": _draw("pick"),
    "capnet_sample_pick_greedy": _draw("pick", greedy=True),
    "capnet_sample_rows": _draw("rows"),
    "capnet_sample_rows_greedy": _draw("rows", greedy=True),
    "capnet_nucleus_rows": _draw("rows", top_p=True),
    "capnet_nucleus_rows_greedy": _draw("rows", top_p=True, greedy=True),
    "capnet_nucleus_pick": _draw("pick", top_p=True),
    "capnet_nucleus_pick_greedy": _draw("pick", top_p=True, greedy=True),
    "capnet_sample_decode": _loop(False),
    "capnet_sample_decode_greedy": _loop(False, greedy=True),
    "capnet_sample_decode_nucleus": _loop(False, top_p=0.5),
    "capnet_sample_decode_nucleus_greedy": _loop(False, top_p=0.5, greedy=True),
    "capnet_sample_decode_excl": _loop(False, top_p=0.5, excl=True),
    "capnet_att_sample_decode": _loop(True),
    "capnet_att_sample_decode_greedy": _loop(True, greedy=True),
    "capnet_att_sample_decode_nucleus": _loop(True, top_p=0.5),
    "capnet_att_sample_decode_nucleus_greedy": _loop(True, top_p=0.5, greedy=True),
    "capnet_att_sample_decode_excl": _loop(True, top_p=0.5, excl=True),
    "capnet_sample_exclusion_mask": [("ids", ptr()), ("ld", STEPS), ("steps", STEPS), ("start_tokens", ptr()), ("rows", ROWS), ("t", 3),
                                     ("V", V)] + EXCL + [("mask", ptr()), ("stream", None)],
    "capnet_mask_logits": [("logits", ptr()), ("rows", ROWS), ("ld", V), ("V", V), ("mask", ptr()), ("stream", None)],
}

# the pointers an entry refuses when null / when misaligned (the others are optional or unchecked: breaking them would launch)
NEEDED = {"vocab": ("h", "w", "workspace", "tokens", "logp", "mask"), "pick": ("values", "index", "tokens", "logp"),
          "rows": ("logits", "tokens", "logp"),
          "plain": ("emb", "wcat", "beff", "Cw", "workspace", "ids", "logp", "err_flag", "slab"),
          "att": ("start_tokens", "att1", "feat", "emb", "wz", "bz", "w_full", "b_full", "wcat", "beff", "Cw", "state0", "workspace",
                  "slab", "ids", "logp", "err_flag"),
          "capnet_sample_exclusion_mask": ("ids", "mask"), "capnet_mask_logits": ("logits", "mask")}
ALIGNED = {"vocab": ("h", "w", "workspace", "tokens", "logp", "mask"), "pick": ("values", "index", "tokens", "logp"),
           "rows": ("logits", "tokens", "logp"),
           "plain": ("Cw", "state0", "state_out", "workspace", "ids", "logp", "slab"),
           "att": ("start_tokens", "att1", "feat", "emb", "wz", "w_full", "Cw", "state0", "state_out", "workspace", "slab", "ids", "logp"),
           "capnet_sample_exclusion_mask": ("ids", "start_tokens", "mask"), "capnet_mask_logits": ("logits", "mask")}
EXCL_FAULTS = (("ngram_5", dict(no_repeat_ngram=5)), ("ngram_neg", dict(no_repeat_ngram=-1)), ("min_words_neg", dict(min_words=-1)),
               ("n_banned_33", dict(banned=ptr(), n_banned=33)), ("n_banned_neg", dict(banned=ptr(), n_banned=-1)),
               ("banned_null", dict(n_banned=2)), ("banned_misaligned", dict(banned=off(), n_banned=2)))


def family(name):
    if name in NEEDED:
        return name
    if "decode" in name:
        return "att" if "_att_" in name else "plain"
    return "vocab" if "vocab" in name else "pick" if "pick" in name else "rows"


def cases(name):
    """[(case, {argument: broken value})], each breaking one thing of the entry's base set."""
    base, fam = dict(ENTRIES[name]), family(name)
    has = base.__contains__
    loop = fam in ("plain", "att")
    out = []
    if has("top_p"):
        out += [("top_p_%s" % p, dict(top_p=p)) for p in (0.0, 1.5, NAN)]
        if loop and "_excl" not in name:
            out.append(("top_p_1.0", dict(top_p=1.0)))                         # the _nucleus loops leave 1 to the plain entries
        else:
            out.append(("top_p_1.0_temperature_0", dict(top_p=1.0, temperature=0.0)))   # valid: read the name it reports under
    if has("temperature"):
        out.append(("temperature_0", dict(temperature=0.0)))
    if has("steps"):
        out.append(("steps_0", dict(steps=0)))
    if loop:
        out += [("cell_7", dict(cell=7)), ("layers_9", dict(nlayers=9)), ("top_k_17", dict(top_k=17)), ("H_100", dict(H=100)),
                ("wcat0_null", dict(wcat=table_of(None))), ("beff0_null", dict(beff=table_of(None))),
                ("wcat0_misaligned", dict(wcat=table_of(18)))]
    if fam == "vocab":
        out.append(("H_100", dict(H=100)))
    if has("k"):
        out += [("k_17", dict(k=17)), ("k_0", dict(k=0))]
    if has("ld"):
        out.append(("ld_short", dict(ld=STEPS - 1 if has("t") else V - 1)))
    if has("step"):
        out.append(("step_65536", dict(step=65536)))
    if has("t"):
        out += [("t_past_steps", dict(t=STEPS + 1)), ("t_neg", dict(t=-1))]
    if has("first_inputs"):
        if "_excl" in name:
            out += [("both_first_inputs", dict(first_inputs=ptr())), ("start_tokens_missing", dict(start_tokens=None)),
                    ("start_tokens_missing_first_inputs_given", dict(first_inputs=ptr(), start_tokens=None))]
        else:
            out += [("both_first_inputs", dict(start_tokens=ptr())), ("neither_first_input", dict(first_inputs=None))]
    out += [("%s_null" % a, {a: None}) for a in NEEDED[fam] if has(a)]
    out += [("%s_misaligned" % a, {a: off()}) for a in ALIGNED[fam] if has(a)]
    if has("slab_floats"):
        out.append(("slab_floats_0", dict(slab_floats=0)))
    if has("rows"):
        out.append(("rows_0", dict(rows=0)))
    if has("n"):
        out += [("n_0", dict(n=0)), ("m_0", dict(m=0))]
    if has("greedy_stride"):
        out.append(("greedy_stride_2^24", dict(greedy_stride=1 << 24)))
        if loop:
            out.append(("greedy_stride_3", dict(greedy_stride=3)))             # 2 rows are no whole groups of 3
        if fam == "att":
            out.append(("greedy_stride_1_m_2", dict(greedy_stride=1)))         # divides the rows, but is not the rows per image
    if has("n_banned"):
        out += list(EXCL_FAULTS)
    assert len({c for c, _ in out}) == len(out)
    return out


def test_the_entries_are_the_sampling_entries_of_the_abi():
    from capnet import _lib
    want = {n for n in _lib.SIGNATURES if ("sample" in n or "nucleus" in n or n == "capnet_mask_logits")
            and not n.endswith("_bytes") and n != "capnet_sample_uniform"}
    assert set(ENTRIES) == want and len(ENTRIES) == 23
    for name, args in ENTRIES.items():
        assert len(args) == len(_lib.SIGNATURES[name][1]), name


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_one_broken_argument_is_refused_in_the_words_of_the_table(name):
    lib = capnet.lib()
    fn = getattr(lib, name)
    seen = {}
    for case, broken in cases(name):
        args = dict(ENTRIES[name])
        assert set(broken) <= set(args), (name, case)
        args.update(broken)
        rc = fn(*args.values())
        assert rc != 0, (name, case)
        seen["%s/%s" % (name, case)] = lib.capnet_last_error().decode()
    if RECORD:
        table = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        table.update(seen)
        with open(RECORD, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    table = json.load(open(TABLE))
    assert sorted(k for k in table if k.split("/")[0] == name) == sorted(seen)
    for cell, text in seen.items():
        assert text == table[cell], (cell, text, table[cell])
