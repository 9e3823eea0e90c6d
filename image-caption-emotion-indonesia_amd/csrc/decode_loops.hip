// The one-call decodes: the host loops that chain a decode step and a vocabulary kernel per step, their workspace
// layouts, and the gather of the attention maps. No loop reads the device except the beam search's optional poll.
//   token loops: the greedy `sample` of capnet.seq2seq (seq2seq/model.py:100-122, 193-217; capnet_lstm_greedy_decode and
//                its _groups form) and sampled decoding (capnet_sample_decode, capnet_att_sample_decode and their _nucleus
//                and _excl forms)
//   beam loops:  beam_decode, lstm_beam_decode, lstm_beam_decode_groups, att_beam_decode
// The kernels they launch: lstm_decode_step.hip, att_kernels.hip, vocab_argmax.hip, vocab_topk.hip, vocab_sample.hip,
// vocab_nucleus.hip, beam_search.hip (beam_advance), gemm_f32.hip.
#include "common.h"
#include "kernels.h"

namespace capnet {

// ---- the token loops: steps x (the decode step: one launch per layer + the draw: the step's token per row) ----------------
// ws: [state A | state B] ([rows][2L][H] each) | h_top [rows][H] | tok int64 [rows] | top_k > 0 only: values f32 [rows][k] |
// index int32 [rows][k] | lse f32 [rows] | the draw's workspace (vocab_argmax's, vocab_sample's or vocab_topk's: its
// arrival counters first; the nucleus draw without top_k: the step's logits f32 [rows][V], no counter); every part starts
// 16-B aligned
struct TokenDecodeWs {
  size_t state, h_top, tok, tk_values, tk_index, tk_lse, draw;   // byte offsets (state B at state + h_top / 2)
};
static TokenDecodeWs token_decode_layout(int nlayers, int rows, int H, int top_k = 0) {
  const size_t n = (size_t)rows;
  TokenDecodeWs w;
  w.state = 0;
  w.h_top = 2 * align16(n * 2 * nlayers * H * sizeof(float));
  w.tok = w.h_top + align16(n * H * sizeof(float));
  w.tk_values = w.tk_index = w.tk_lse = w.draw = w.tok + align16(n * 8);
  if (top_k > 0) {
    w.tk_index = w.tk_values + align16(n * top_k * sizeof(float));
    w.tk_lse = w.tk_index + align16(n * top_k * sizeof(int));
    w.draw = w.tk_lse + align16(n * sizeof(float));
  }
  return w;
}

// step_fn(t, tokens, state_in, state_out, h_top) is the decode step of step t, draw_fn(t, h_top, tokens) writes the step's
// tokens over its inputs (and into the caller's ids). `counters`: the arrival counters at the head of the draw's workspace,
// 16 bytes each. The loop does not look at an end token: it runs `steps` steps and the host truncates.
template <class Step, class Draw>
static int token_loop(const TokenDecodeWs& w, int nlayers, int rows, int H, int steps, int counters, const long long* start_tokens,
                      const float* state0, void* ws, float* state_out, hipStream_t s, Step&& step_fn, Draw&& draw_fn) {
  const size_t st_bytes = (size_t)rows * 2 * nlayers * H * sizeof(float);
  char* p = reinterpret_cast<char*>(ws);
  float* state[2] = {reinterpret_cast<float*>(p + w.state), reinterpret_cast<float*>(p + w.state + w.h_top / 2)};
  float* h_top = reinterpret_cast<float*>(p + w.h_top);
  long long* tok = reinterpret_cast<long long*>(p + w.tok);
  if (state0) CAPNET_HIP_CHECK(hipMemcpyAsync(state[0], state0, st_bytes, hipMemcpyDeviceToDevice, s));
  else CAPNET_HIP_CHECK(hipMemsetAsync(state[0], 0, st_bytes, s));
  if (start_tokens) CAPNET_HIP_CHECK(hipMemcpyAsync(tok, start_tokens, (size_t)rows * 8, hipMemcpyDeviceToDevice, s));
  if (counters) CAPNET_HIP_CHECK(hipMemsetAsync(p + w.draw, 0, 16 * (size_t)counters, s));
  for (int t = 0; t < steps; ++t) {
    int rc = step_fn(t, tok, state[t & 1], state[(t + 1) & 1], h_top);
    if (rc == kOk) rc = draw_fn(t, h_top, tok);
    if (rc != kOk) return rc;
  }
  if (state_out) CAPNET_HIP_CHECK(hipMemcpyAsync(state_out, state[steps & 1], st_bytes, hipMemcpyDeviceToDevice, s));
  return kOk;
}

// ---- the whole greedy `sample`: the draw is one vocab_argmax launch ----
size_t lstm_greedy_decode_groups_ws_bytes(int nlayers, int groups, int rpg, int H, int V) {
  return token_decode_layout(nlayers, groups * rpg, H).draw + vocab_argmax_groups_ws_bytes(groups, rpg, V);
}

size_t lstm_greedy_decode_ws_bytes(int nlayers, int rows, int H, int V) {
  return lstm_greedy_decode_groups_ws_bytes(nlayers, 1, rows, H, V);
}

int lstm_greedy_decode(int nlayers, int rows, int E, int H, int V, int steps, const float* features,
                       const long long* start_tokens, const float* emb, const float* const* wcat,
                       const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* ws,
                       long long* ids, float* state_out, int* err_flag, hipStream_t s) {
  return lstm_greedy_decode_groups(nlayers, 1, rows, E, H, V, steps, features, start_tokens, &emb, wcat, beff, &Cw, &Cb, state0,
                                   ws, ids, state_out, err_flag, s);
}

// group g's rows [g rpg, (g + 1) rpg) decode on emb[g], wcat[l] + g 4H (kin + H), beff[l] + g 4H, Cw[g], Cb[g]
int lstm_greedy_decode_groups(int nlayers, int groups, int rpg, int E, int H, int V, int steps, const float* features,
                              const long long* start_tokens, const float* const* emb, const float* const* wcat,
                              const float* const* beff, const float* const* Cw, const float* const* Cb, const float* state0,
                              void* ws, long long* ids, float* state_out, int* err_flag, hipStream_t s) {
  const int rows = groups * rpg;
  const TokenDecodeWs w = token_decode_layout(nlayers, rows, H);
  void* va_ws = reinterpret_cast<char*>(ws) + w.draw;
  return token_loop(
      w, nlayers, rows, H, steps, groups, start_tokens, state0, ws, state_out, s,
      [&](int t, const long long* tok, const float* sin, float* sout, float* h_top) {
        const bool feat = t == 0 && features;    // (one group only: capnet_lstm_greedy_decode)
        return stacked_decode_step(kCellLSTM, nlayers, rows, E, H, V, feat ? nullptr : tok, feat ? features : emb[0], wcat, beff,
                                   sin, sout, h_top, err_flag, s, nullptr, groups, feat ? nullptr : emb);
      },
      [&](int t, const float* h_top, long long* tok) {
        return vocab_argmax_groups(h_top, Cw, Cb, groups, rpg, H, V, va_ws, tok, ids + t, steps, s);
      });
}

// ---- the sampling loops: the draw is vocab_sample (top_k == 0) or vocab_topk + sample_pick (top_k > 0); with a nucleus
// (top_p < 1) the projection into the workspace's logits block (sgemm_splitk, the product of the composed route's ops.linear:
// the same logits) + nucleus_rows, or vocab_topk + nucleus_pick. top_p == 1 is "off": the plain launches, not a nucleus.
// greedy_stride (sample_key.h's vs_row_key; the capnet_*_greedy entries): g > 0 makes every g-th row the greedy decode of its
// group -- the loops only pass it to the draw; on the attention loop the caller runs m = g rows per image, so the greedy
// caption rides on the one read of the image's maps per step
// exclusions (ex; the capnet_*_excl entries): one more launch per step, sample_exclusion_mask, and the draw takes
// the mask -- vocab_sample / vocab_topk in their epilogues, the nucleus draw without top_k through mask_logits on its block ----
static size_t sample_ws_bytes(int nlayers, int rows, int H, int V, int top_k, bool nucleus) {
  const size_t draw = top_k > 0 ? vocab_topk_ws_bytes(rows, top_k, V)
                      : nucleus ? align16((size_t)rows * V * sizeof(float)) : vocab_sample_ws_bytes(rows, V);
  return draw ? token_decode_layout(nlayers, rows, H, top_k).draw + draw : 0;
}

// the exclusion mask lies behind a loop's own bytes: sample_loop places it there
static size_t mask_offset(size_t own) { return align16(own); }
static size_t with_mask(size_t own, int rows, int V, bool excl) {
  return own && excl ? mask_offset(own) + sample_mask_bytes(rows, V) : own;
}

size_t sample_decode_ws_bytes(int nlayers, int rows, int H, int V, int top_k, bool nucleus, bool excl) {
  return with_mask(sample_ws_bytes(nlayers, rows, H, V, top_k, nucleus), rows, V, excl);
}

// own: the bytes of ws in front of the mask (the family's size without exclusions)
template <class Step>
static int sample_loop(int nlayers, int rows, int H, int V, int steps, const long long* start_tokens, const float* Cw,
                       const float* Cb, const float* state0, const SampleOpts& o, void* ws, size_t own, float* slab,
                       size_t slab_floats, long long* ids, float* logp, float* state_out, hipStream_t s, Step&& step_fn) {
  const int top_k = o.top_k;
  const TokenDecodeWs w = token_decode_layout(nlayers, rows, H, top_k);
  const bool nucleus = o.top_p < 1.f;
  char* p = reinterpret_cast<char*>(ws);
  // ex: a launch of its own builds the step's exclusion mask from ids and the start tokens, and the step's draw reads it;
  // null: the launches as they were
  SampleExcl ex{};
  if (o.ex) {
    ex = *o.ex;
    ex.mask = reinterpret_cast<unsigned*>(p + mask_offset(own));
  }
  const unsigned* mask = ex.mask;
  float* tk_values = reinterpret_cast<float*>(p + w.tk_values);
  int* tk_index = reinterpret_cast<int*>(p + w.tk_index);
  float* tk_lse = reinterpret_cast<float*>(p + w.tk_lse);
  void* draw_ws = p + w.draw;
  float* logits = reinterpret_cast<float*>(p + w.draw);      // the nucleus draw without top_k
  return token_loop(w, nlayers, rows, H, steps, nucleus && top_k == 0 ? 0 : 1, start_tokens, state0, ws, state_out, s, step_fn,
                    [&](int t, const float* h_top, long long* tok) {
                      if (mask)
                        if (int rc = sample_exclusion_mask(ids, steps, start_tokens, rows, t, V, ex, ex.mask, s)) return rc;
                      if (top_k == 0 && !nucleus)
                        return vocab_sample(h_top, Cw, Cb, rows, H, V, o.inv_T, o.seed, (unsigned)t, 0, draw_ws, tok, ids + t,
                                            logp + t, steps, s, o.greedy_stride, mask);
                      if (top_k == 0) {
                        int rc = sgemm_splitk(false, true, rows, V, H, h_top, H, Cw, H, logits, V, Cb, 0, slab, slab_floats, s);
                        if (rc == kOk && mask) rc = mask_logits(logits, rows, V, V, mask, s);
                        if (rc != kOk) return rc;
                        return nucleus_rows(logits, rows, V, V, o.inv_T, o.top_p, o.seed, (unsigned)t, 0, tok, ids + t, logp + t,
                                            steps, s, o.greedy_stride);
                      }
                      const int rc = vocab_topk(h_top, Cw, Cb, rows, H, V, top_k, draw_ws, tk_values, tk_index, tk_lse, s, mask);
                      if (rc != kOk) return rc;
                      if (nucleus)
                        return nucleus_pick(tk_values, tk_index, rows, top_k, V, o.inv_T, o.top_p, o.seed, (unsigned)t, 0, tok,
                                            ids + t, logp + t, steps, s, o.greedy_stride);
                      return sample_pick(tk_values, tk_index, rows, top_k, V, o.inv_T, o.seed, (unsigned)t, 0, tok, ids + t,
                                         logp + t, steps, s, o.greedy_stride);
                    });
}

int sample_decode(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                  const long long* start_tokens, const float* emb, const float* const* wcat, const float* const* beff,
                  const float* Cw, const float* Cb, const float* state0, const SampleOpts& o, void* ws, float* slab,
                  size_t slab_floats, long long* ids, float* logp, float* state_out, int* err_flag, hipStream_t s) {
  return sample_loop(nlayers, rows, H, V, steps, start_tokens, Cw, Cb, state0, o, ws,
                     sample_ws_bytes(nlayers, rows, H, V, o.top_k, o.top_p < 1.f), slab, slab_floats, ids, logp, state_out, s,
                     [&](int t, const long long* tok, const float* sin, float* sout, float* h_top) {
                       const bool given = t == 0 && first_inputs;     // step 0 on the caller's rows
                       return stacked_decode_step(cell, nlayers, rows, E, H, V, given ? nullptr : tok, given ? first_inputs : emb,
                                                  wcat, beff, sin, sout, h_top, err_flag, s);
                     });
}

// ---- the same loop for the attention decoders: n images x m samples each, the step att_decode_step with k = m and every
// row continuing from itself (parent_rows null at every step), so an image's maps are read once per step for all its
// samples. No beam bookkeeping.
// ws: sample_decode's layout at n m rows, then att_decode_step's block (z | xa | escore)
static size_t att_sample_ws_bytes(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k, bool nucleus) {
  if (n < 1 || m < 1 || (long)n * m >= (1L << 24)) return 0;
  const size_t base = sample_ws_bytes(nlayers, n * m, H, V, top_k, nucleus), step = att_decode_step_ws_bytes(n, m, P, A, C, E);
  return base && step ? align16(base) + align16(step) : 0;
}

size_t att_sample_decode_ws_bytes(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k, bool nucleus,
                                  bool excl) {
  return with_mask(att_sample_ws_bytes(nlayers, n, m, P, A, C, E, H, V, top_k, nucleus), n * m, V, excl);
}

int att_sample_decode(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int steps,
                      const long long* start_tokens, const float* att1, const float* feat, const float* emb, const float* wz,
                      const float* bz, const float* wf, const float* bf, const float* const* wcat, const float* const* beff,
                      const float* Cw, const float* Cb, const float* state0, const SampleOpts& o, void* ws, float* slab,
                      size_t slab_floats, long long* ids, float* logp, float* state_out, int* err_flag, hipStream_t s) {
  const int rows = n * m;
  const bool nucleus = o.top_p < 1.f;
  void* step_ws = reinterpret_cast<char*>(ws) + align16(sample_ws_bytes(nlayers, rows, H, V, o.top_k, nucleus));
  return sample_loop(nlayers, rows, H, V, steps, start_tokens, Cw, Cb, state0, o, ws,
                     att_sample_ws_bytes(nlayers, n, m, P, A, C, E, H, V, o.top_k, nucleus), slab, slab_floats, ids, logp, state_out,
                     s, [&](int, const long long* tok, const float* sin, float* sout, float* h_top) {
                       return att_decode_step(cell, nlayers, n, m, P, A, C, E, H, V, att1, feat, tok, emb, wz, bz, wf, bf, wcat, beff,
                                              sin, nullptr, sout, h_top, step_ws, slab, slab_floats, err_flag, s);
                     });
}

// ---- the whole beam search of a plain stack: steps x (one gathered decode-step launch per layer + the vocabulary
// projection + one beam_advance launch), then beam_finish -- capnet.beam.beam_search_device's loop without its host side
// ws: [state A | state B] ([n k][2L][H] each) | h_top [n k][H] | logits [n k][V] | words A | words B | parent_rows (int64
// [n k] each) | the beam_state_bytes block; every part starts 16-B aligned. fused (capnet_lstm_beam_decode on
// capnet_vocab_topk): no logits block; in its place values f32 [n k][k] | index int32 [n k][k] | lse f32 [n k] |
// vocab_topk's workspace. fused under constraints: behind everything (at `total`, so no other offset moves and
// capnet_beam_nbest finds the state where it was) the step's selection mask, sample_mask_bytes(n k, V)
struct BeamDecodeWs {
  size_t state, h_top, logits, words, parent, beam, total;   // byte offsets (state B at state + (h_top - state) / 2)
  size_t tk_values, tk_index, tk_lse, tk_ws;                 // fused only
};
static BeamDecodeWs beam_decode_layout(int nlayers, int n, int k, int H, int V, int max_steps, bool fused = false,
                                       int groups = 1) {   // n: all sentences, groups x sentences per group
  const size_t nk = (size_t)n * k;
  BeamDecodeWs w;
  w.state = 0;
  w.h_top = 2 * align16(nk * 2 * nlayers * H * sizeof(float));
  w.logits = w.h_top + align16(nk * H * sizeof(float));
  w.words = w.logits + (fused ? 0 : align16(nk * V * sizeof(float)));
  w.tk_values = w.tk_index = w.tk_lse = w.tk_ws = 0;
  if (fused) {
    w.tk_values = w.words;
    w.tk_index = w.tk_values + align16(nk * k * sizeof(float));
    w.tk_lse = w.tk_index + align16(nk * k * sizeof(int));
    w.tk_ws = w.tk_lse + align16(nk * sizeof(float));
    w.words = w.tk_ws + align16(vocab_topk_groups_ws_bytes(groups, (int)nk / groups, k, V));
  }
  w.parent = w.words + 2 * align16(nk * 8);
  w.beam = w.parent + align16(nk * 8);
  w.total = w.beam + align16(beam_state_bytes(n, k, max_steps));
  return w;
}

size_t beam_decode_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps) {
  if (nlayers < 1 || nlayers > 8 || n < 1 || H < 1 || V < 1 || !beam_state_bytes(n, k, max_steps)) return 0;
  return beam_decode_layout(nlayers, n, k, H, V, max_steps).total;
}

// the loop of the one-call searches: step(tokens, parent rows or null, state_in, state_out, h_top) is the decode step
// (parent rows null: step 1). fused: the projection and the selection as vocab_topk + beam_advance_topk, no logits
// block and no slab; else sgemm_splitk on the slab + beam_advance. Cwg / Cbg (capnet_lstm_beam_decode_groups): n = groups x
// sentences per group, group-major, and group g's rows are projected on Cwg[g] / Cbg[g] -- fused, one vocab_topk_groups
// launch; else one sgemm_splitk per group into the group's row block of the logits, one after the other on the one slab
template <class Step>
static int beam_loop(int nlayers, int n, int k, int H, int V, int max_steps, long long start_token, long long end_token,
                     const float* Cw, const float* Cb, const float* state0, void* ws, float* slab, size_t slab_floats,
                     int poll_every, long long* seqs, int* lengths, int* steps_run, hipStream_t s, Step&& step_fn,
                     bool fused = false, int groups = 1, const float* const* Cwg = nullptr, const float* const* Cbg = nullptr,
                     void* trace = nullptr, int* trace_rows = nullptr,   // (the row trace: beam_advance's, logits form only)
                     const BeamConstraints* con = nullptr,   // (constraints: beam_advance's forms; fused: the select-only top-k)
                     const BeamTeams* dv = nullptr) {                     // (diverse search: the logits form only)
  // dv: the step still runs on n images of k rows; the beam state is that of n teams searches of k / teams beams and lies
  // in the caller's block dv->beam, not in the layout's slot (which is sized for (n, k))
  const int sn = dv ? n * dv->teams : n, sk = dv ? k / dv->teams : k;
  const int nk = n * k, rpg = nk / groups;
  const BeamDecodeWs w = beam_decode_layout(nlayers, n, k, H, V, max_steps, fused, groups);
  const size_t st_bytes = (size_t)nk * 2 * nlayers * H * sizeof(float);
  char* p = reinterpret_cast<char*>(ws);
  float* state[2] = {reinterpret_cast<float*>(p + w.state), reinterpret_cast<float*>(p + w.state + w.h_top / 2)};
  float* h_top = reinterpret_cast<float*>(p + w.h_top);
  float* logits = reinterpret_cast<float*>(p + w.logits);
  float* tk_values = reinterpret_cast<float*>(p + w.tk_values);
  int* tk_index = reinterpret_cast<int*>(p + w.tk_index);
  float* tk_lse = reinterpret_cast<float*>(p + w.tk_lse);
  void* tk_ws = p + w.tk_ws;
  long long* words[2] = {reinterpret_cast<long long*>(p + w.words),
                         reinterpret_cast<long long*>(p + w.words + (w.parent - w.words) / 2)};
  long long* parent = reinterpret_cast<long long*>(p + w.parent);
  void* beam = dv ? dv->beam : p + w.beam;
  // fused under constraints: one more launch per step writes what each row may not select, and vocab_topk's select-only
  // instance leaves those words out of its candidates (not out of lse); beam_advance_topk is the one it was
  unsigned* sel_mask = fused && con ? reinterpret_cast<unsigned*>(p + w.total) : nullptr;
  const int* live_total = nullptr;
  if (int rc = beam_live(beam, sn, sk, max_steps, &live_total, nullptr, nullptr)) return rc;
  if (state0) CAPNET_HIP_CHECK(hipMemcpyAsync(state[0], state0, st_bytes, hipMemcpyDeviceToDevice, s));
  else CAPNET_HIP_CHECK(hipMemsetAsync(state[0], 0, st_bytes, s));
  if (int rc = beam_init(beam, sn, sk, max_steps, start_token, words[0], s)) return rc;
  if (fused) CAPNET_HIP_CHECK(hipMemsetAsync(tk_ws, 0, 16 * (size_t)groups, s));   // vocab_topk's counters, one per group
  int issued = 0;
  for (int step = 1; step <= max_steps; ++step) {
    // step 1: every beam is at its own (initial) row; afterwards the rows the previous beam_advance chose
    int rc = step_fn(words[(step - 1) & 1], step == 1 ? nullptr : parent, state[(step - 1) & 1], state[step & 1], h_top);
    if (fused) {
      if (rc == kOk && sel_mask) rc = beam_exclusion_mask(beam, n, k, max_steps, step, V, end_token, *con, sel_mask, s);
      if (rc == kOk)
        rc = Cwg ? vocab_topk_groups(h_top, Cwg, Cbg, groups, rpg, H, V, k, tk_ws, tk_values, tk_index, tk_lse, s, sel_mask, true)
                 : vocab_topk(h_top, Cw, Cb, nk, H, V, k, tk_ws, tk_values, tk_index, tk_lse, s, sel_mask, true);
      if (rc == kOk)
        rc = beam_advance_topk(beam, tk_values, tk_index, tk_lse, V, n, k, max_steps, step, end_token, words[step & 1], parent, s);
    } else {
      for (int g = 0; Cwg && g < groups && rc == kOk; ++g)
        rc = sgemm_splitk(false, true, rpg, V, H, h_top + (size_t)g * rpg * H, H, Cwg[g], H, logits + (size_t)g * rpg * V, V,
                          Cbg ? Cbg[g] : nullptr, 0, slab, slab_floats, s);
      if (rc == kOk && !Cwg) rc = sgemm_splitk(false, true, nk, V, H, h_top, H, Cw, H, logits, V, Cb, 0, slab, slab_floats, s);
      if (rc == kOk)   // (the kernel by what is given: teams, forced words, constraints, none)
        rc = beam_advance("beam_advance", beam, logits, V, V, n, k, max_steps, step, end_token, con, dv, words[step & 1], parent, trace, s);
    }
    if (rc != kOk) return rc;
    issued = step;
    if (poll_every > 0 && step % poll_every == 0 && step < max_steps) {
      int live = 0;
      CAPNET_HIP_CHECK(hipMemcpyAsync(&live, live_total, sizeof(int), hipMemcpyDeviceToHost, s));
      CAPNET_HIP_CHECK(hipStreamSynchronize(s));
      if (!live) break;
    }
  }
  if (steps_run) *steps_run = issued;
  return beam_finish(beam, sn, sk, max_steps, end_token, seqs, lengths, s, trace, trace_rows);
}

int beam_decode(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                long long end_token, const float* emb, const float* const* wcat, const float* const* beff, const float* Cw,
                const float* Cb, const float* state0, void* ws, float* slab, size_t slab_floats, int poll_every,
                long long* seqs, int* lengths, int* steps_run, int* err_flag, hipStream_t s, int groups, const BeamConstraints* con,
                const BeamTeams* teams) {
  n *= groups;   // beam groups: weight groups x images, group-major
  BeamTeams dv{0, 0.f, nullptr};
  if (teams) dv = BeamTeams{teams->teams, teams->strength, reinterpret_cast<char*>(ws) + beam_decode_layout(nlayers, n, k, H, V, max_steps).total};
  return beam_loop(nlayers, n, k, H, V, max_steps, start_token, end_token, Cw, Cb, state0, ws, slab, slab_floats, poll_every, seqs,
                   lengths, steps_run, s,
                   [&](const long long* tok, const long long* parent, const float* sin, float* sout, float* h_top) {
                     return stacked_decode_step(cell, nlayers, n * k, E, H, V, tok, emb, wcat, beff, sin, sout, h_top, err_flag, s,
                                                parent, groups);
                   },
                   false, 1, nullptr, nullptr, nullptr, nullptr, con, teams ? &dv : nullptr);
}

// ---- capnet.seq2seq's beam search: the same loop from a given state, step 1 on given inputs (EncoderRNN's feature
// column) when first_inputs is set, the projection and selection fused (vocab_topk.hip) or as beam_decode's ----
// the selection mask of the fused constrained step lies behind a layout's own bytes (beam_loop places it there)
static size_t with_select_mask(size_t own, int nk, int V, bool fused, bool constrained) {
  return own && fused && constrained ? own + sample_mask_bytes(nk, V) : own;
}

size_t lstm_beam_decode_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk, bool constrained) {
  if (nlayers < 1 || nlayers > 8 || n < 1 || H < 1 || V < 1 || k > V || !beam_state_bytes(n, k, max_steps)) return 0;
  if ((long)n * k >= (1L << 24) || (fused_topk && !vocab_topk_supported(H, k, V))) return 0;
  return with_select_mask(beam_decode_layout(nlayers, n, k, H, V, max_steps, fused_topk != 0).total, n * k, V, fused_topk != 0,
                          constrained);
}

int lstm_beam_decode(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                     long long end_token, const float* first_inputs, const float* emb, const float* const* wcat,
                     const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* ws, float* slab,
                     size_t slab_floats, int fused_topk, int poll_every, long long* seqs, int* lengths, int* steps_run,
                     int* err_flag, hipStream_t s, const BeamConstraints* con) {
  return beam_loop(nlayers, n, k, H, V, max_steps, start_token, end_token, Cw, Cb, state0, ws, slab, slab_floats, poll_every, seqs,
                   lengths, steps_run, s,
                   [&](const long long* tok, const long long* parent, const float* sin, float* sout, float* h_top) {
                     const bool given = !parent && first_inputs;     // step 1 on the caller's rows
                     return stacked_decode_step(cell, nlayers, n * k, E, H, V, given ? nullptr : tok, given ? first_inputs : emb,
                                                wcat, beff, sin, sout, h_top, err_flag, s, parent);
                   },
                   fused_topk != 0, 1, nullptr, nullptr, nullptr, nullptr, con);
}

// ---- every emotion decoder of capnet.seq2seq in one search: groups x n sentences, group g on its own embedding, LSTM
// weights and projection (the decode step on a (H / 4, groups) grid with per-group tables, parents gathered in the kernel)
size_t lstm_beam_decode_groups_ws_bytes(int nlayers, int groups, int n, int k, int H, int V, int max_steps, int fused_topk,
                                        bool constrained) {
  if (groups < 1 || groups > 8 || n < 1 || n >= (1 << 24)) return 0;
  if (!lstm_beam_decode_ws_bytes(nlayers, groups * n, k, H, V, max_steps, fused_topk)) return 0;
  return with_select_mask(beam_decode_layout(nlayers, groups * n, k, H, V, max_steps, fused_topk != 0, groups).total,
                          groups * n * k, V, fused_topk != 0, constrained);
}

int lstm_beam_decode_groups(int cell, int nlayers, int groups, int n, int k, int E, int H, int V, int max_steps,
                            long long start_token, long long end_token, const float* const* emb, const float* const* wcat,
                            const float* const* beff, const float* const* Cw, const float* const* Cb, const float* state0,
                            void* ws, float* slab, size_t slab_floats, int fused_topk, int poll_every, long long* seqs,
                            int* lengths, int* steps_run, int* err_flag, hipStream_t s, const BeamConstraints* con) {
  const int nq = groups * n;
  return beam_loop(nlayers, nq, k, H, V, max_steps, start_token, end_token, nullptr, nullptr, state0, ws, slab, slab_floats,
                   poll_every, seqs, lengths, steps_run, s,
                   [&](const long long* tok, const long long* parent, const float* sin, float* sout, float* h_top) {
                     return stacked_decode_step(cell, nlayers, nq * k, E, H, V, tok, emb[0], wcat, beff, sin, sout, h_top, err_flag,
                                                s, parent, groups, emb);
                   },
                   fused_topk != 0, groups, Cw, Cb, nullptr, nullptr, con);
}

// ---- the same loop for the attention decoders: the step is att_decode_step (z, the two attention launches, layer 0 on
// [embedding | gated context], the upper layers) ----
// ws: beam_decode's layout, then att_decode_step's block (z | xa | escore)
// the maps of the winners out of the per-step history: workgroup (i, e) copies hist[e][rows[i][e]] -- the row hypothesis i
// occupied at step e + 1 -- to alphas[i][e]; a row of -1 (past the caption, nothing completed) or out of range gives zeros
__global__ __launch_bounds__(256) void alpha_gather_kernel(const float* __restrict__ hist, const int* __restrict__ rows, int nk,
                                                           int max_steps, int P, float* __restrict__ alphas) {
  const int i = blockIdx.x, e = blockIdx.y;
  const int r = rows[(long)i * max_steps + e];
  const bool ok = r >= 0 && r < nk;
  const float* src = hist + ((size_t)e * nk + (ok ? r : 0)) * P;
  float* dst = alphas + ((size_t)i * max_steps + e) * P;
  for (int p = threadIdx.x; p < P; p += 256) dst[p] = ok ? src[p] : 0.f;
}

size_t att_beam_decode_ws_bytes(int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps) {
  const size_t base = beam_decode_ws_bytes(nlayers, n, k, H, V, max_steps), step = att_decode_step_ws_bytes(n, k, P, A, C, E);
  return base && step ? base + align16(step) : 0;
}

int att_beam_decode(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                    long long start_token, long long end_token, const float* att1, const float* feat, const float* emb,
                    const float* wz, const float* bz, const float* wf, const float* bf, const float* const* wcat,
                    const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* ws, float* slab,
                    size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                    hipStream_t s, int groups, float* alphas, const BeamConstraints* con, const BeamTeams* teams) {
  const int nq = groups * n;   // beam groups: weight groups x images, group-major
  const int D = teams ? teams->teams : 1;
  char* p = reinterpret_cast<char*>(ws);
  void* step_ws = p + beam_decode_layout(nlayers, nq, k, H, V, max_steps).total;
  // the maps (alphas set): behind the search's own workspace, trace | rows int32 [nq][max_steps] | history
  // [max_steps][nq k][P] -- step e's attention writes slice e - 1, the advance records the rows, one gather at the end
  void* trace = nullptr;
  int* rows = nullptr;
  float* hist = nullptr;
  if (alphas) {
    p += att_beam_decode_ws_bytes(nlayers, nq, k, P, A, C, E, H, V, max_steps);
    trace = p;
    p += align16(beam_trace_bytes(nq, k, max_steps));
    rows = reinterpret_cast<int*>(p);
    p += align16((size_t)nq * max_steps * sizeof(int));
    hist = reinterpret_cast<float*>(p);
  }
  // diverse: behind everything above, the state of nq D searches of k / D beams | with the maps, the winners' rows
  // [nq D][max_steps] (the slot above holds nq of them only)
  BeamTeams dv{0, 0.f, nullptr};
  if (teams) {
    char* tail = reinterpret_cast<char*>(ws) + (alphas ? att_beam_decode_alphas_ws_bytes(nlayers, groups, n, k, P, A, C, E, H, V, max_steps)
                                                        : att_beam_decode_ws_bytes(nlayers, nq, k, P, A, C, E, H, V, max_steps));
    dv = BeamTeams{D, teams->strength, tail};
    if (alphas) rows = reinterpret_cast<int*>(tail + align16(beam_state_bytes(nq * D, k / D, max_steps)));
  }
  int calls = 0;   // the step the loop is at: it calls the step once per step, in order
  const int rc = beam_loop(
      nlayers, nq, k, H, V, max_steps, start_token, end_token, Cw, Cb, state0, ws, slab, slab_floats, poll_every, seqs, lengths,
      steps_run, s,
      [&](const long long* tok, const long long* parent, const float* sin, float* sout, float* h_top) {
        float* slice = hist ? hist + (size_t)calls++ * nq * k * P : nullptr;
        return att_decode_step(cell, nlayers, n, k, P, A, C, E, H, V, att1, feat, tok, emb, wz, bz, wf, bf, wcat, beff, sin, parent,
                               sout, h_top, step_ws, slab, slab_floats, err_flag, s, groups, slice);
      },
      false, 1, nullptr, nullptr, trace, rows, con, teams ? &dv : nullptr);
  if (rc != kOk || !alphas) return rc;
  hipLaunchKernelGGL(alpha_gather_kernel, dim3(nq * D, max_steps), dim3(256), 0, s, hist, rows, nq * k, max_steps, P, alphas);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

size_t att_beam_decode_alphas_ws_bytes(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                       int max_steps) {
  if (groups < 1 || groups > 8 || n < 1 || n >= (1 << 24)) return 0;
  const int nq = groups * n;
  const size_t base = att_beam_decode_ws_bytes(nlayers, nq, k, P, A, C, E, H, V, max_steps);
  if (!base) return 0;
  return base + align16(beam_trace_bytes(nq, k, max_steps)) + align16((size_t)nq * max_steps * sizeof(int)) +
         align16((size_t)max_steps * nq * k * P * sizeof(float));
}

// ---- what the searches leave in the caller's workspace (capnet_beam_nbest after the search returns) ----
size_t beam_decode_ws_beam_offset(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk, int groups) {
  if (!lstm_beam_decode_groups_ws_bytes(nlayers, groups, n, k, H, V, max_steps, fused_topk)) return 0;
  return beam_decode_layout(nlayers, groups * n, k, H, V, max_steps, fused_topk != 0, groups).beam;
}

size_t att_beam_decode_alphas_ws_trace_offset(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                              int max_steps) {
  if (!att_beam_decode_alphas_ws_bytes(nlayers, groups, n, k, P, A, C, E, H, V, max_steps)) return 0;
  return att_beam_decode_ws_bytes(nlayers, groups * n, k, P, A, C, E, H, V, max_steps);
}

size_t att_beam_decode_alphas_ws_hist_offset(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                             int max_steps) {
  const size_t trace = att_beam_decode_alphas_ws_trace_offset(nlayers, groups, n, k, P, A, C, E, H, V, max_steps);
  if (!trace) return 0;
  const int nq = groups * n;
  return trace + align16(beam_trace_bytes(nq, k, max_steps)) + align16((size_t)nq * max_steps * sizeof(int));
}

int alpha_gather(const float* hist, const int* rows, int captions, int nk, int max_steps, int P, float* alphas, hipStream_t s) {
  CAPNET_REQUIRE(hist && rows && alphas, "alpha_gather: null argument");
  CAPNET_REQUIRE((size_t)hist % 4 == 0 && (size_t)rows % 4 == 0 && (size_t)alphas % 4 == 0,
                 "alpha_gather: hist, rows and alphas must be 4-byte aligned");
  CAPNET_REQUIRE(captions >= 1 && nk >= 1 && max_steps >= 1 && max_steps <= 65535 && P >= 1,
                 "alpha_gather: captions=%d nk=%d max_steps=%d P=%d (all >= 1, max_steps <= 65535)", captions, nk, max_steps, P);
  hipLaunchKernelGGL(alpha_gather_kernel, dim3(captions, max_steps), dim3(256), 0, s, hist, rows, nk, max_steps, P, alphas);
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
