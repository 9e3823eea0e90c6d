"""Every style in one search on the GPU: the grouped decode step (capnet_stacked_decode_step_groups) and the grouped
attention step (capnet_att_decode_step_groups) against one call of the existing step per group, bit for bit; sample_styles
of the four factored decoder classes against sample_batch(mode=m, one_call=True) and the fp64 beam search of every family
of style_decode_cases; subsets of the modes, poll_every, the fallbacks, the errors; evaluate_styles.

The step comparisons are exact: a group's rows run the arithmetic of that group alone, in the same order. The whole
searches go by the margin rule of style_decode_cases (tests/test_style_decode_cpu.py asserts the margin of every case)."""
import pytest
import torch

import capnet
from capnet import _lib, ops
from capnet._lib import check, ptr, ptr_array
from capnet.model import DecoderFactoredLSTM
from helpers import load_golden, t
from style_decode_cases import IMAGES, KS, MODES, NAMES, START, family

pytestmark = pytest.mark.gpu

H, V = 64, 23


# ---- 1. the grouped step -------------------------------------------------------------------------------------------
def _group_parents(G, rpg):
    """test_beam_decode_gpu's pattern inside each group: a reversal in which every third row shares the first parent."""
    out = []
    for g in range(G):
        rev = [g * rpg + rpg - 1 - r for r in range(rpg)]
        out += [rev[0] if r % 3 == 1 else p for r, p in enumerate(rev)]
    return out


def _step_inputs(dev, G, L, E, rpg, seed):
    g = torch.Generator().manual_seed(seed)
    kin, rows = (E + 15) // 16 * 16, G * rpg

    def u(*shape, a=1.0):
        return ((torch.rand(shape, generator=g) * 2 - 1) * a).to(dev)
    wcat, beff = [], []
    for l in range(L):
        w = u(G, 4 * H, (kin if l == 0 else H) + H, a=0.2)
        if l == 0:
            w[:, :, E:kin] = 0
        wcat.append(w.contiguous())
        beff.append(u(G, 4 * H, a=0.1))
    emb = u(V, E)
    tokens = torch.randint(0, V, (rows,), generator=g).to(dev)
    # every group on the SAME previous state and tokens where there are several: only the weights tell the groups apart
    state = u(rpg, 2 * L, H).repeat(G, 1, 1).contiguous()
    tokens = tokens[:rpg].repeat(G).contiguous()
    return wcat, beff, emb, tokens, state, torch.tensor(_group_parents(G, rpg), dtype=torch.long, device=dev)


def _grouped_entry(cell, G, rpg, E, wcat, beff, x, tokens, state, parent):
    """capnet_stacked_decode_step_groups itself (ops takes the existing entries at one group)."""
    out, top = torch.empty_like(state), torch.empty(state.shape[0], H, device=state.device)
    check(_lib.lib().capnet_stacked_decode_step_groups(
        cell, len(wcat), G, rpg, E, H, V if tokens is not None else 0, ptr(tokens), ptr(x), ptr_array(wcat), ptr_array(beff),
        ptr(state), ptr(parent), ptr(out), ptr(top), ptr(ops.err_flag(state.device)), _lib.current_stream()), "groups")
    return top, out


@pytest.mark.parametrize("rpg", [1, 5, 17, 33])
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("E", [12, 10], ids=["x-f32x4", "x-scalar"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("cell", [ops.CELL_FACTORED, ops.CELL_LSTM], ids=["factored", "lstm"])
def test_grouped_step_equals_the_step_of_every_group(dev, cell, L, E, G, rpg):
    wcat, beff, emb, tokens, state, parent = _step_inputs(dev, G, L, E, rpg, 1000 * G + 100 * L + 10 * E + rpg)
    x = emb.index_select(0, tokens).contiguous()
    for par in (None, parent):
        for xin, tok in ((emb, tokens), (x, None)):
            tops, outs = [], []
            for g in range(G):
                rs = slice(g * rpg, (g + 1) * rpg)
                top, out = ops.stacked_decode_step(
                    state[rs].contiguous(), [w[g] for w in wcat], [b[g] for b in beff], xin if tok is not None else xin[rs].contiguous(),
                    None if tok is None else tok[rs].contiguous(), cell=cell, parent_rows=None if par is None else par[rs] - g * rpg)
                tops.append(top)
                outs.append(out)
            want_top, want = torch.cat(tops), torch.cat(outs)
            top, out = _grouped_entry(cell, G, rpg, E, wcat, beff, xin, tok, state, par)
            assert torch.equal(out, want) and torch.equal(top, want_top), (par is None, tok is None)
            if G > 1:
                top, out = ops.stacked_decode_step(state, wcat, beff, xin, tok, cell=cell, parent_rows=par, groups=G)
                assert torch.equal(out, want) and torch.equal(top, want_top), (par is None, tok is None)
                # same state, same tokens, other weights: the groups' outputs differ
                assert not torch.equal(outs[0], outs[1])
    ops.check_device_errors()


# ---- 2. the grouped attention step (the wide kernel) ---------------------------------------------------------------
A, EA = 16, 24


def _att_inputs(dev, G, L, n, k, P, Cf, seed):
    g = torch.Generator().manual_seed(seed)
    nk, kin = n * k, (EA + Cf + 15) // 16 * 16

    def u(*shape, a=1.0):
        return ((torch.rand(shape, generator=g) * 2 - 1) * a).to(dev).contiguous()
    d = dict(k=k)
    d["att1"], d["feat"] = u(G * n, P, A), torch.rand((n, P, Cf), generator=g).to(dev)
    d["wz"], d["bz"] = u(G, A + Cf, H, a=(3.0 / H) ** 0.5), u(G, A + Cf, a=0.1)
    d["w_full"], d["b_full"] = u(G, A, a=(3.0 / A) ** 0.5 * 4), u(G, a=0.1)
    d["emb"] = u(V, EA)
    wcat, beff = [], []
    for l in range(L):
        w = u(G, 4 * H, (kin if l == 0 else H) + H, a=(3.0 / (EA + Cf / 3 + H if l == 0 else 2 * H)) ** 0.5)
        if l == 0:
            w[:, :, EA + Cf:kin] = 0
        wcat.append(w.contiguous())
        beff.append(u(G, 4 * H, a=0.1))
    d["wcat"], d["beff"] = wcat, beff
    d["state"] = u(nk, 2 * L, H).repeat(G, 1, 1).contiguous()
    d["tokens"] = torch.randint(0, V, (nk,), generator=g).to(dev).repeat(G).contiguous()
    parents = []
    for q in range(G * n):       # within-image reversals with repeats, as tests/test_att_beam_decode_gpu.py
        rev = [q * k + k - 1 - r for r in range(k)]
        parents += [rev[0] if r % 3 == 1 else p for r, p in enumerate(rev)]
    d["parent"] = torch.tensor(parents, dtype=torch.long, device=dev)
    return d


def _xa(ws, rows, Cf):
    """xa [rows, E + C] of a step's workspace: it follows z [rows, A + C]."""
    return ws[rows * (A + Cf):rows * (A + Cf) + rows * (EA + Cf)].view(rows, EA + Cf)


@pytest.mark.parametrize("P", [1, 9])
@pytest.mark.parametrize("Cf", [2048, 3072, 512], ids=["wide-12", "wide-16", "narrow"])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("G", [2, 4])
def test_grouped_attention_step_equals_the_step_of_every_group(dev, G, n, k, Cf, P):
    L, nk = 2, n * k
    d = _att_inputs(dev, G, L, n, k, P, Cf, 1000 * G + 100 * n + 10 * k + P + Cf)
    for par in (None, d["parent"]):
        tops, outs, xas = [], [], []
        for g in range(G):
            rs = slice(g * nk, (g + 1) * nk)
            ws = ops.att_decode_step_workspace(n, k, P, A, Cf, EA, dev)
            top, out = ops.att_decode_step(
                d["att1"][g * n:(g + 1) * n], d["feat"], k, d["tokens"][rs].contiguous(), d["emb"], d["wz"][g], d["bz"][g],
                d["w_full"][g:g + 1], d["b_full"][g:g + 1], [w[g] for w in d["wcat"]], [b[g] for b in d["beff"]],
                d["state"][rs].contiguous(), parent_rows=None if par is None else (par[rs] - g * nk).contiguous(), workspace=ws)
            tops.append(top)
            outs.append(out)
            xas.append(_xa(ws, nk, Cf).clone())
        ws = ops.att_decode_step_workspace(G * n, k, P, A, Cf, EA, dev)
        top, out = ops.att_decode_step(d["att1"], d["feat"], k, d["tokens"], d["emb"], d["wz"], d["bz"], d["w_full"], d["b_full"],
                                       d["wcat"], d["beff"], d["state"], parent_rows=par, workspace=ws, groups=G)
        assert torch.equal(_xa(ws, G * nk, Cf), torch.cat(xas)), par is None
        assert torch.equal(out, torch.cat(outs)) and torch.equal(top, torch.cat(tops)), par is None
        assert not torch.equal(outs[0], outs[1]) and not torch.equal(xas[0], xas[1])
    ops.check_device_errors()


# ---- 3. the whole search -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", NAMES)
def test_sample_styles_equals_every_mode_and_fp64(dev, monkeypatch, name, k):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    fam = family(name)
    dec = fam.make().to(dev).eval()
    feats, end = fam.features().to(dev), fam.end
    calls = []
    real = ops.att_beam_decode if "Att" in name else ops.beam_decode
    monkeypatch.setattr(ops, "att_beam_decode" if "Att" in name else "beam_decode",
                        lambda *a, **kw: (calls.append(kw.get("groups", 1)), real(*a, **kw))[1])
    styled = dec.sample_styles(feats, START, end, k=k)
    assert calls == [4]                                     # one grouped search, not a loop
    assert tuple(styled) == MODES
    for m in MODES:
        want = [fam.reference(m, k, i) for i in range(IMAGES)]
        assert styled[m] == want, (m, k)
        assert dec.sample_batch(feats, START, end, k=k, mode=m, one_call=True) == want, (m, k)
    two = dec.sample_styles(feats, START, end, k=k, modes=("sad", "factual"))
    assert tuple(two) == ("sad", "factual") and two["sad"] == styled["sad"] and two["factual"] == styled["factual"]
    for poll in (1, 3):
        assert dec.sample_styles(feats, START, end, k=k, poll_every=poll) == styled, poll
    ops.check_device_errors()


# ---- 4. fallbacks --------------------------------------------------------------------------------------------------
def _loop(dec, feats, start, end, k, poll=0):
    return {m: dec.sample_batch(feats, start, end, k=k, mode=m, one_call=True, poll_every=poll) for m in MODES}


@pytest.mark.parametrize("name", NAMES)
def test_the_composed_step_switch_takes_the_loop(dev, monkeypatch, name):
    fam = family(name)
    dec = fam.make().to(dev).eval()
    feats = fam.features().to(dev)
    monkeypatch.setenv("CAPNET_NO_FUSED_DECODE_STEP", "1")
    for target in ("beam_decode", "att_beam_decode"):
        monkeypatch.setattr(ops, target, lambda *a, **kw: pytest.fail("the one call ran"))
    assert dec.sample_styles(feats, START, fam.end, k=5) == _loop(dec, feats, START, fam.end, 5)
    ops.check_device_errors()


Z = load_golden("sample_tiny.npz")


def test_an_unsupported_hidden_size_takes_the_loop(dev):
    start, end = [int(v) for v in Z["start_end"]]
    seen = 0
    for name in [str(c) for c in Z["cases"]]:
        pre = "case.%s." % name
        c = {key[len(pre):]: Z[key] for key in Z.files if key.startswith(pre)}
        if str(c["kind"]) != "factored":
            continue
        E, H_, F, V_, k, maxlen = [int(v) for v in c["dims"]][:6]
        dec = DecoderFactoredLSTM(E, H_, F, V_, 1, dropout=0.0, max_seq_length=maxlen)
        dec.load_state_dict({key[len("param."):]: t(v) for key, v in c.items() if key.startswith("param.")})
        dec = dec.to(dev).eval()
        assert dec.hidden_size == 16 and not ops.stacked_decode_supported(dec.embed_size, 16)
        feats = torch.zeros(3, E, device=dev)
        for poll in (0, 3):
            assert dec.sample_styles(feats, start, end, k=k, poll_every=poll) == _loop(dec, feats, start, end, k, poll)
        assert dec.sample_styles(feats, start, end, k=k)[str(c["mode"])][0] == c["seq"].tolist()[0]
        seen += 1
    assert seen >= 1
    ops.check_device_errors()


# ---- 5. errors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["StackedFactoredLSTM-2", "StackedFactoredLSTMAtt-2"])
def test_a_start_token_out_of_range_raises_after_the_call(dev, monkeypatch, name):
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    fam = family(name)
    dec = fam.make().to(dev).eval()
    feats = fam.features().to(dev)
    ops.check_device_errors()
    with pytest.raises(capnet.CapnetError, match="token id out of range"):
        dec.sample_styles(feats, fam.V + 3, fam.end, k=3)
    ops.check_device_errors()                       # (raised and cleared)
    assert dec.sample_styles(feats, START, fam.end, k=3, modes=("happy",))["happy"] == \
        [fam.reference("happy", 3, i) for i in range(IMAGES)]


@pytest.mark.parametrize("bad", ["rows", -1])
@pytest.mark.parametrize("rpg", [5, 17])
def test_a_parent_out_of_range_sets_the_flag_and_reads_the_row_itself(dev, rpg, bad):
    G = 2
    ops.check_device_errors()
    wcat, beff, emb, tokens, state, parent = _step_inputs(dev, G, 2, 12, rpg, 7)
    r = G * rpg - 2                                  # a row of the last group
    mended = parent.clone()
    mended[r] = r
    want_top, want = ops.stacked_decode_step(state, wcat, beff, emb, tokens, parent_rows=mended, groups=G)
    # a parent in ANOTHER group is inside [0, R): it is read, and raises nothing
    across = parent.clone()
    across[r] = 0
    ops.stacked_decode_step(state, wcat, beff, emb, tokens, parent_rows=across, groups=G)
    ops.check_device_errors()
    parent[r] = G * rpg if bad == "rows" else bad
    top, out = ops.stacked_decode_step(state, wcat, beff, emb, tokens, parent_rows=parent, groups=G)
    assert torch.equal(out, want) and torch.equal(top, want_top)
    with pytest.raises(capnet.CapnetError):
        ops.check_device_errors()
    ops.check_device_errors()                       # (the check cleared the flag)


# ---- 6. evaluate_styles --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["StackedFactoredLSTM-2", "StackedFactoredLSTMAtt-2"])
def test_evaluate_styles(dev, monkeypatch, name):
    from capnet.train import evaluate, evaluate_styles
    monkeypatch.delenv("CAPNET_NO_FUSED_DECODE_STEP", raising=False)
    fam = family(name)
    dec = fam.make().to(dev).eval()
    start, end, V_ = START, fam.end, fam.V

    class Vocab:
        word2idx = {"<start>": start, "<end>": end}
        idx2word = {i: ("<end>" if i == end else "<start>" if i == start else "w%d" % i) for i in range(V_)}

    class Enc(torch.nn.Module):
        passes = 0

        def forward(self, images):
            Enc.passes += 1
            return images
    # what goes into BLEU is compared too: the captions here are short, and BLEU-4 of a short corpus is 0 on both sides
    from capnet import train
    rec, real = [], train.corpus_bleu
    monkeypatch.setattr(train, "corpus_bleu", lambda refs, hyps, weights: (rec.append((refs, hyps)), real(refs, hyps, weights=weights))[1])
    # the references are what the decoder says in each mode, one of them cut short
    said = {m: dec.sample_batch(fam.features().to(dev), start, end, k=5, mode=m) for m in MODES}
    per_mode = [{m: [torch.tensor(said[m][i]), torch.tensor(said[m][i][:-2] + [end])] for m in MODES} for i in range(IMAGES)]
    shared = [d["factual"] for d in per_mode]
    for caps in (shared, per_mode):
        batches = [(fam.features(), None, None, caps)]
        Enc.passes = 0
        del rec[:]
        got = evaluate_styles(Enc(), dec, Vocab(), batches, k=5)
        assert Enc.passes == 1 and tuple(got) == MODES and len(rec) == 16
        fed = {m: rec[4 * j] for j, m in enumerate(MODES)}
        for m in MODES:
            mode_caps = [c[m] if isinstance(c, dict) else c for c in caps]
            del rec[:]
            assert got[m] == evaluate(Enc(), dec, Vocab(), [(fam.features(), None, None, mode_caps)], mode=m, k=5, one_call=True), m
            assert fed[m] == rec[0], m                      # the same references and hypotheses
            assert fed[m][1] == [fam.reference(m, 5, i) for i in range(IMAGES)], m
            assert fed[m][0] == [[[int(w) for w in c] for c in cs] for cs in mode_caps], m
    if "Att" not in name:
        assert got["factual"][0] > 0.99                     # six tokens: BLEU is not degenerate there
    assert evaluate_styles(Enc(), dec, Vocab(), batches, modes=("sad",), k=5)["sad"] == got["sad"]
