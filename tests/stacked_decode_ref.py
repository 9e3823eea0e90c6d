"""CPU restatement of capnet.stacked.StackedFactoredLSTM's decoding (forward_step / sample / sample_batch). TEST
INFRASTRUCTURE. PARITY UNPINNED with more than one layer: the reference ignores num_layers (stylenet/model.py:37).

  * one step of the stack is the cell of oracle.decoders_ref.stacked_factored_lstm_forward at inference: layer 0 is
    factored_step on the input, layer l > 0 factored_step on h of layer l-1 at the same step, with the parameters
    V{l}_g, S{l}_{mode}g, U{l}_g, W{l}_g; no dropout;
  * the beam search is oracle.beam_ref._beam with DecoderFactoredLSTM.sample's semantics (stylenet/model.py:198-294):
    every layer's state starts at zero, the first input is B(<start>), only the top layer feeds C;
  * folded_step is the same step with each gate's chain folded into one matrix, Weff_g = U_g S_g V_g (what the fused
    kernel computes with).
"""
import torch
import torch.nn.functional as Fn

from oracle import beam_ref, decoders_ref as D
from stacked_att_ref import layer_params

_SFX = {"factual": "f", "happy": "happy_", "sad": "sad_", "angry": "angry_"}


def _layer(p, l):
    return p if l == 0 else layer_params(p, l)


def stacked_step(p, x, hs, cs, mode, num_layers):
    """One inference step of the stack -> (top h, [h per layer], [c per layer])."""
    hs2, cs2 = [], []
    for l in range(num_layers):
        h, c = D.factored_step(_layer(p, l), x, hs[l], cs[l], mode)
        hs2.append(h)
        cs2.append(c)
        x = h
    return x, hs2, cs2


def fold(p, l, mode):
    """Layer l's [Weff_g | W_g] ([4H, in + H]) and beff ([4H]), gate blocks i, f, o, c~."""
    q = _layer(p, l)
    ws, bs = [], []
    for g in "ifoc":
        Vw, Vb = q["V_%s.weight" % g], q["V_%s.bias" % g]
        Sw, Sb = q["S_%s%s.weight" % (_SFX[mode], g)], q["S_%s%s.bias" % (_SFX[mode], g)]
        Uw, Ub = q["U_%s.weight" % g], q["U_%s.bias" % g]
        Ww, Wb = q["W_%s.weight" % g], q["W_%s.bias" % g]
        ws.append(torch.cat([Uw @ Sw @ Vw, Ww], 1))
        bs.append(Uw @ (Sw @ Vb + Sb) + Ub + Wb)
    return torch.cat(ws, 0), torch.cat(bs, 0)


def folded_step(p, x, hs, cs, mode, num_layers):
    """stacked_step through the folded weights -> (top h, [h per layer], [c per layer])."""
    hs2, cs2 = [], []
    for l in range(num_layers):
        w, b = fold(p, l, mode)
        pre = Fn.linear(torch.cat([x, hs[l]], 1), w, b)
        i, f, o, ct = pre.chunk(4, 1)
        c = torch.sigmoid(f) * cs[l] + torch.sigmoid(i) * torch.tanh(ct)
        h = torch.sigmoid(o) * c
        hs2.append(h)
        cs2.append(c)
        x = h
    return x, hs2, cs2


def _step_fn(p, mode, num_layers):
    def step_fn(prev_words, state):
        L = num_layers
        x = p["B.weight"][prev_words].squeeze(1)
        top, hs, cs = stacked_step(p, x, list(state[:L]), list(state[L:]), mode, L)
        return Fn.linear(top, p["C.weight"], p["C.bias"]), tuple(hs + cs)
    return step_fn


def _zeros(p, k, num_layers):
    H = p["W_i.weight"].shape[0]
    return tuple(torch.zeros(k, H, dtype=p["W_i.weight"].dtype) for _ in range(2 * num_layers))


def sample_stacked(p, num_layers, start_token, end_token, k=5, mode="factual", max_seq_length=40):
    """StackedFactoredLSTM.sample restated: LongTensor [1, L]."""
    V = p["C.weight"].shape[0]
    return beam_ref._beam(_step_fn(p, mode, num_layers), _zeros(p, k, num_layers), V, start_token, end_token, k,
                          max_seq_length)


def beam_margin(p, num_layers, start_token, end_token, k=5, mode="factual", max_seq_length=40):
    """The smallest gap, over the steps of sample_stacked's beam search, between the k-th and the (k+1)-th best
    candidate score (_beam's loop replayed with topk(k + 1)), and between the best and the second-best completed
    sequence. Where it is well above the GPU's rounding, the GPU's beam search must pick the same sequence."""
    V = p["C.weight"].shape[0]
    step_fn = _step_fn(p, mode, num_layers)
    state = _zeros(p, k, num_layers)
    words = torch.LongTensor([[start_token]] * k)
    top = torch.zeros(k, 1, dtype=p["C.weight"].dtype)
    margin, done = float("inf"), []
    step = 1
    while True:
        out, state = step_fn(words, state)
        scores = top.expand_as(out) + Fn.log_softmax(out, dim=1)
        flat = scores[0] if step == 1 else scores.view(-1)
        best, idx = flat.topk(min(k + 1, flat.numel()), 0, True, True)
        if best.numel() > k:
            margin = min(margin, float(best[k - 1] - best[k]))
        best, idx = best[:k], idx[:k]
        prev, nxt = idx // V, idx % V
        keep = [i for i, w in enumerate(nxt.tolist()) if w != end_token]
        done += [float(best[i]) for i in range(k) if i not in keep]
        k = len(keep)
        if k == 0 or step > max_seq_length:
            break
        state = tuple(s[prev[keep]] for s in state)
        top = best[keep].unsqueeze(1)
        words = nxt[keep].unsqueeze(1)
        step += 1
    done.sort(reverse=True)
    if len(done) > 1:                       # the completed sequence with the best score wins
        margin = min(margin, done[0] - done[1])
    return margin


def decode_params(module, seed, emb_scale=1.0, c_scale=8.0):
    """fp64 parameters for `module`'s state_dict: every matrix U(-a, a) with a = sqrt(3 / fan_in) (unit-variance
    products, so the gates stay out of saturation at any size), biases U(-0.05, 0.05), B U(-emb_scale, emb_scale), C
    scaled by c_scale (well-separated beam candidates)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in module.state_dict().items():
        if v.dim() > 1:
            a = 3.0 ** 0.5 / v.shape[1] ** 0.5
            if k == "B.weight":
                a = emb_scale
            elif k == "C.weight":
                a *= c_scale
        else:
            a = 0.05
        out[k] = ((torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1) * a)
    return out


def greedy_path(p, num_layers, start_token, steps, mode="factual"):
    """The first `steps` tokens of the restatement's greedy decode (beam width 1, no end token): tests take their end
    token from it, so that every beam search they run completes."""
    step_fn = _step_fn(p, mode, num_layers)
    state, words, out = _zeros(p, 1, num_layers), torch.LongTensor([[start_token]]), []
    for _ in range(steps):
        logits, state = step_fn(words, state)
        words = logits.argmax(1, keepdim=True)
        out.append(int(words))
    return out
