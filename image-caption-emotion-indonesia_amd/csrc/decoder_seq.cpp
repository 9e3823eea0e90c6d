// Sequence drivers for the caption decoders: one C call runs the whole scheduled-sampling
// recurrence (forward) or the whole BPTT (backward) as a chain of HIP launches on one stream.
//
// Follows DecoderFactoredLSTM.forward / forward_step (stylenet/model.py:115-196) and
// DecoderRNN.forward (nic/model.py:74-115):
//   * inputs are [image feature, dropout(B(w_0)), ..., dropout(B(w_{L-2}))], packed time-major
//     (pack_padded_sequence order, batch shrinking with `batch_sizes`);
//   * step t is teacher forced iff tf_mask[t] (the caller draws random.random() per step,
//     model.py:181); otherwise its input is B(argmax(C h_{t-1})) WITHOUT dropout (model.py:184),
//     or B(captions[:,0]) at t = 0;
//   * FactoredLSTM gate pre-activation = U_g(S_g(V_g(x))) + W_g(h); c = f*c + i*c~; h = o*c.
// MI355X mapping: the input chain of all teacher-forced rows is three batched MFMA GEMMs over
// N = sum(lengths) rows (gate-concatenated / gate-batched weights); only the recurrent
// 4H x H product and the pointwise gate update run per time step.
#include <vector>

#include "common.h"
#include "kernels.h"

#include "seq_layers.h"

namespace capnet {

namespace seqd {

std::vector<int> step_offsets(const int* batch_sizes, int steps) {
  std::vector<int> off(steps + 1, 0);
  for (int t = 0; t < steps; ++t) off[t + 1] = off[t] + batch_sizes[t];
  return off;
}

std::vector<int> with_state_step(int B, const int* batch_sizes, int steps) {
  std::vector<int> bse(steps + 1, B);
  for (int t = 0; t < steps; ++t) bse[t + 1] = batch_sizes[t];
  return bse;
}

int check_batch_sizes(const char* who, const int* batch_sizes, int steps, int B, int N) {
  CAPNET_REQUIRE(batch_sizes != nullptr, "%s: null batch_sizes", who);
  long n = 0;
  int prev = B;
  for (int t = 0; t < steps; ++t) {
    CAPNET_REQUIRE(batch_sizes[t] > 0 && batch_sizes[t] <= prev,
                   "%s: batch_sizes must be positive and non-increasing (step %d: %d after %d)", who, t, batch_sizes[t], prev);
    prev = batch_sizes[t];
    n += batch_sizes[t];
  }
  CAPNET_REQUIRE(n == N, "%s: sum(batch_sizes)=%ld != N=%d", who, n, N);
  return kOk;
}

int build_row_tables(const std::vector<int>& off, const unsigned char* tf_mask, int has_features, bool lead, int* row_sample,
                     int* row_col, int* row_token, int* prev_row, hipStream_t s) {
  SeqMeta m;
  m.steps = (int)off.size() - 1; m.N = off.back(); m.has_features = has_features;
  for (int t = 0; t <= m.steps; ++t) m.off[t] = off[t];
  if (lead) m.tf[0] = 1;
  for (int t = lead; t < m.steps; ++t) m.tf[t] = tf_mask[t - lead] ? 1 : 0;
  return build_rows(m, row_sample, row_col, row_token, prev_row, s);
}

Layout make_layout(const SeqDims& d) {
  Layout L;
  Carve take, itake;
  const size_t N = d.N, E = d.E, F = d.F, H = d.H;
  L.X = take(N * E);
  L.G = take(N * 4 * H);
  L.Cst = take(N * H);
  L.Wcat = take(4 * H * H);
  L.Wfrag = take(H % 16 == 0 ? lstm_wfrag_floats((int)H) : 4);
  L.Wp = take(H == 512 ? lstm_persist_w_floats() : 4);     // image of the persistent sequence kernel
  L.bUW = take(4 * H);
  if (d.cell == kCellFactored) {
    L.A1 = take(N * 4 * F);
    L.A2 = take(N * 4 * F);
    L.Vcat = take(4 * F * E);
    L.Scat = take(4 * F * F);
    L.Ucat = take(4 * H * F);
    L.bV = take(4 * F);
    L.bS = take(4 * F);
  } else {
    L.A1 = L.A2 = L.Scat = L.Ucat = L.bV = L.bS = 0;
    L.Vcat = take(4 * H * E);  // weight_ih copy (kept so backward sees the forward's weights)
  }
  L.total = take.o;
  L.row_sample = itake(N);
  L.row_col = itake(N);
  L.row_token = itake(N);
  L.prev_row = itake(N);
  L.ctl = itake(lstm_persist_ctl_ints());
  L.itotal = itake.o;
  return L;
}

// scratch of seq_backward_layer (lead: the chain's rows of all steps, for any batch_sizes[0])
BwdLayout make_bwd_layout(const SeqDims& d, int lead) {
  BwdLayout S;
  Carve take;
  const size_t N = d.N, F = d.F, H = d.H;
  const bool fac = d.cell == kCellFactored;
  S.dPre = take(N * 4 * H);
  S.Hprev = take(N * H);
  S.dh_rec = take((size_t)d.B * H);
  S.dc = take((size_t)d.B * H);
  S.dX = take(N * d.E);
  S.dA2 = take(fac ? N * 4 * F : 0);
  S.dA1 = take(fac ? N * 4 * F : 0);
  S.skws = take(kSplitKFloats);
  S.A1c = take(fac && lead ? N * 4 * F : 0);
  S.A2c = take(fac && lead ? N * 4 * F : 0);
  S.total = take.o;
  return S;
}

int check_dims(const SeqDims& d, const int* batch_sizes) {
  CAPNET_REQUIRE(d.B > 0 && d.T > 0 && d.steps > 0 && d.N > 0 && d.E > 0 && d.H > 0 && d.V > 0,
                 "decoder: bad dims B=%d T=%d steps=%d N=%d E=%d H=%d V=%d", d.B, d.T, d.steps, d.N, d.E, d.H, d.V);
  CAPNET_REQUIRE(d.cell == kCellLSTM || d.F > 0, "decoder: factored size");
  RC(check_batch_sizes("decoder", batch_sizes, d.steps, d.B, d.N));
  CAPNET_REQUIRE(d.steps <= d.T + (d.has_features ? 1 : 0),
                 "decoder: %d steps need more caption columns than T=%d", d.steps, d.T);
  return kOk;
}

int copy_d2d(float* dst, const float* src, size_t n, hipStream_t s) {
  CAPNET_HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return kOk;
}

static size_t nctr(const SkWs& k) { return k.ctr ? kSplitKCounters : 0; }

int chain_fwd(const Chain& c, const float* X, int n, float* A1, float* A2, float* out, long ldo, const float* bias, int accumulate,
              const SkWs& k, hipStream_t s) {
  const int XW = c.XW, F = c.F, H = c.H;
  RC(sgemm_splitk(false, true, n, 4 * F, XW, X, XW, c.Vcat, XW, A1, 4 * F, c.bV, 0, k.ws, k.floats, s, k.ctr, nctr(k)));
  RC(sgemm_splitk_batched(false, true, n, F, F, A1, 4 * F, c.Scat, F, A2, 4 * F, c.bS, 0, 4, F, (long)F * F, F, F, k.ws, k.floats,
                          s, k.ctr, nctr(k)));
  return sgemm_splitk_batched(false, true, n, H, F, A2, 4 * F, c.Ucat, F, out, ldo, bias, accumulate, 4, F, (long)H * F, H,
                              bias ? H : 0, k.ws, k.floats, s, k.ctr, nctr(k));
}

int chain_collapse(const Chain& c, float* US, float* Weff, float* c1, float* bias, const SkWs& k, hipStream_t s) {
  const int XW = c.XW, F = c.F, H = c.H;
  RC(sgemm(false, false, H, F, F, c.Ucat, F, c.Scat, F, US, F, nullptr, 0, 4, (long)H * F, (long)F * F, (long)H * F, 0, 0, s));
  RC(sgemm(false, false, H, XW, F, US, F, c.Vcat, XW, Weff, XW, nullptr, 0, 4, (long)H * F, (long)F * XW, (long)H * XW, 0, 0, s));
  RC(sgemm_splitk_batched(false, true, 1, F, F, c.bV, F, c.Scat, F, c1, F, c.bS, 0, 4, F, (long)F * F, F, F, k.ws, k.floats, s,
                          k.ctr, nctr(k)));
  return sgemm_splitk_batched(false, true, 1, H, F, c1, F, c.Ucat, F, bias, H, nullptr, 1, 4, F, (long)H * F, H, 0, k.ws, k.floats,
                              s, k.ctr, nctr(k));
}

int chain_rows(const Chain& c, const float* X, int n, float* A1, float* A2, const SkWs& k, hipStream_t s) {
  const int XW = c.XW, F = c.F;
  RC(sgemm_splitk(false, true, n, 4 * F, XW, X, XW, c.Vcat, XW, A1, 4 * F, c.bV, 0, k.ws, k.floats, s, k.ctr, nctr(k)));
  return sgemm(false, true, n, F, F, A1, 4 * F, c.Scat, F, A2, 4 * F, c.bS, 0, 4, F, (long)F * F, F, F, 0, s);
}

int chain_bwd_rows(const Chain& c, const float* dG, long ldg, int n, float* dA2, float* dA1, hipStream_t s) {
  const int F = c.F, H = c.H;
  RC(sgemm(false, false, n, F, H, dG, ldg, c.Ucat, F, dA2, 4 * F, nullptr, 0, 4, H, (long)H * F, F, 0, 0, s));
  return sgemm(false, false, n, F, F, dA2, 4 * F, c.Scat, F, dA1, 4 * F, nullptr, 0, 4, F, (long)F * F, F, 0, 0, s);
}

int chain_wgrads(const Chain& c, const float* dG, long ldg, const float* X, const float* A1, const float* A2, const float* dA2,
                 const float* dA1, int n, const ChainGrads& g, hipStream_t s) {
  const int XW = c.XW, F = c.F, H = c.H;
  // dU_g = dG_g^T . A2_g ; dS_g = dA2_g^T . A1_g ; dVcat = dA1^T . X
  RC(sgemm(true, false, H, F, n, dG, ldg, A2, 4 * F, g.dUcat, F, nullptr, 0, 4, H, F, (long)H * F, 0, 0, s));
  RC(colsum(dA2, 4 * F, n, 4 * F, g.dbS, 0, s));
  RC(sgemm(true, false, F, F, n, dA2, 4 * F, A1, 4 * F, g.dScat, F, nullptr, 0, 4, F, F, (long)F * F, 0, 0, s));
  RC(colsum(dA1, 4 * F, n, 4 * F, g.dbV, 0, s));
  return sgemm(true, false, 4 * F, XW, n, dA1, 4 * F, X, XW, g.dVcat, XW, nullptr, 0, 1, 0, 0, 0, 0, 0, s);
}

int lstm_input_wgrad(const float* dG, long ldg, const float* X, int XW, int H, int n, float* dWih, hipStream_t s) {
  return sgemm(true, false, 4 * H, XW, n, dG, ldg, X, XW, dWih, XW, nullptr, 0, 1, 0, 0, 0, 0, 0, s);
}

// ws: slab workspace of the per-step (few rows) products; the all-rows call up front has enough tiles for the plain kernel.
int input_chain(const SeqDims& d, const Layout& L, float* sv, int r0, int r1, const SkWs& k, hipStream_t s) {
  const int n = r1 - r0;
  if (n <= 0) return kOk;
  const int E = d.E, F = d.F, H = d.H;
  const SkWs kn{n <= 128 ? k.ws : nullptr, k.floats, k.ctr};
  const float* X = sv + L.X + (size_t)r0 * E;
  float* G = sv + L.G + (size_t)r0 * 4 * H;
  if (d.cell == kCellFactored)
    return chain_fwd(chain_of(d, L, sv), X, n, sv + L.A1 + (size_t)r0 * 4 * F, sv + L.A2 + (size_t)r0 * 4 * F, G, 4 * H, sv + L.bUW,
                     0, kn, s);
  // G = X . W_ih^T + (b_ih + b_hh)
  return sgemm_splitk(false, true, n, 4 * H, E, X, E, sv + L.Vcat, E, G, 4 * H, sv + L.bUW, 0, kn.ws, kn.floats, s, kn.ctr, nctr(kn));
}

int init_state(const float* mean, int B, int H, int C, const UpperInit& w, float* h0, float* c0, const SkWs& k, hipStream_t s) {
  // (B x 512 x 2048: a handful of 64 x 64 tiles walking the whole K took 80 us each at 12 rows; K-split: 9)
  RC(sgemm_splitk(false, true, B, H, C, mean, C, w.init_h_w, C, h0, H, w.init_h_b, 0, k.ws, k.floats, s, k.ctr, nctr(k)));
  return sgemm_splitk(false, true, B, H, C, mean, C, w.init_c_w, C, c0, H, w.init_c_b, 0, k.ws, k.floats, s, k.ctr, nctr(k));
}

int init_state_grad(const float* dh0, const float* dc0, const float* mean, int B, int H, int C, const UpperInitGrads& g, hipStream_t s) {
  RC(sgemm(true, false, H, C, B, dh0, H, mean, C, g.dWih, C, nullptr, 0, 1, 0, 0, 0, 0, 0, s));
  RC(colsum(dh0, H, B, H, g.dbih, 0, s));
  RC(sgemm(true, false, H, C, B, dc0, H, mean, C, g.dWic, C, nullptr, 0, 1, 0, 0, 0, 0, 0, s));
  return colsum(dc0, H, B, H, g.dbic, 0, s);
}

int feed_back(const Feedback& f, const float* h_prev, int b, int r0, float* X, long ldx, const SkWs& k, hipStream_t s) {
  RC(sgemm_splitk(false, true, b, f.V, f.H, h_prev, f.H, f.Cw, f.H, f.logits, f.V, f.Cb, 0, k.ws, k.floats, s, k.ctr, nctr(k)));
  RC(argmax_rows(f.logits, b, f.V, f.V, f.row_token + r0, s));
  return gather_inputs(f.captions, f.T, f.features, f.emb, f.E, f.V, f.row_sample, f.row_col, f.row_token, X, ldx, r0, r0 + b,
                       f.dropout_p, f.seed, 0, 1, f.err_flag, s);
}

}  // namespace seqd

using namespace seqd;

size_t seq_saved_floats(const SeqDims& d) { return make_layout(d).total; }
size_t seq_saved_ints(const SeqDims& d) { return make_layout(d).itotal; }
size_t seq_saved_cell_offset(const SeqDims& d) { return make_layout(d).Cst; }

size_t seq_fwd_scratch_floats(const SeqDims& d) { return (size_t)d.B * d.V + 64 + kSplitKFloats; }
size_t seq_bwd_scratch_floats(const SeqDims& d) { return make_bwd_layout(d, 0).total; }

namespace seqd {
int pack_layer(LayerCtx& c, const SeqWeights& w, const int* batch_sizes, hipStream_t s) {
  const SeqDims& d = c.d;
  const Layout& L = c.L;
  float* sv = c.sv;
  const int H = d.H;
  const GateOrder go = gate_order(d.cell);
  CopyTable ct;
  add_cell_copies(ct, w, d.cell, d.E, d.F, H, sv + L.Vcat, sv + L.Scat, sv + L.Ucat, sv + L.Wcat, sv + L.bV, sv + L.bS, sv + L.bUW);
  RC(multi_copy(ct, s));
  c.fused_step = H % 16 == 0 && lstm_step_fused_supported(batch_sizes[0], H);
  if (c.fused_step) RC(lstm_pack_wfrag(sv + L.Wcat, sv + L.Wfrag, H, go.gi, go.gf, go.go, go.gg, s));
  // runs of teacher-forced steps go to ONE launch of the persistent kernel (csrc/lstm_persist.hip)
  c.persist = lstm_persist_supported(batch_sizes[0], H);
  if (c.persist) {
    RC(lstm_persist_pack(sv + L.Wcat, sv + L.Wp, go.gi, go.gf, go.go, go.gg, s));
    CAPNET_HIP_CHECK(hipMemsetAsync(c.svi + L.ctl, 0, lstm_persist_ctl_ints() * sizeof(int), s));
  }
  c.segment = 0;
  return kOk;
}

// steps [t, t1) of one layer: step t's gate pre-activations (without the recurrent product) are in G, the following
// steps are teacher forced. One persistent launch where the kernel takes the size, else step by step.
int recur(LayerCtx& c, const std::vector<int>& off, const int* batch_sizes, int t, int t1, float* skws, int* skctr,
          int* err_flag, hipStream_t s) {
  const SeqDims& d = c.d;
  const Layout& L = c.L;
  float* sv = c.sv;
  const int H = d.H;
  const GateOrder go = gate_order(d.cell);
  const bool single_fused = t1 == t + 1 && t > 0 && c.fused_step;   // one free-running step: no weights to keep
  if (c.persist && !single_fused) {
    return lstm_persist_run(sv + L.Wp, sv + L.G, sv + L.Cst, c.hid, off.data(), batch_sizes, t, t1, H, go.gi, go.gf, go.go,
                            go.gg, go.tanh_out, ++c.segment, c.svi + L.ctl, err_flag, s, nullptr);
  }
  for (int u = t; u < t1; ++u) {
    const int b = batch_sizes[u], r0 = off[u];
    if (u > 0) {
      const float* h_prev = c.hid + (size_t)off[u - 1] * H;
      if (c.fused_step) {
        // gates += h_{t-1} . Wcat^T, activations and the c/h update in one launch
        RC(lstm_step_fused(h_prev, sv + L.Wfrag, sv + L.G + (size_t)r0 * 4 * H, 4 * H,
                           sv + L.Cst + (size_t)off[u - 1] * H, sv + L.Cst + (size_t)r0 * H,
                           c.hid + (size_t)r0 * H, b, H, go.gi, go.gf, go.go, go.gg, go.tanh_out, s));
        continue;
      }
      // G[rows] += h_{t-1} . Wcat^T
      RC(sgemm_splitk(false, true, b, 4 * H, H, h_prev, H, sv + L.Wcat, H,
                      sv + L.G + (size_t)r0 * 4 * H, 4 * H, nullptr, 1, skws, kSplitKWs, s, skctr, kSplitKCounters));
    }
    RC(lstm_pointwise_fwd(sv + L.G + (size_t)r0 * 4 * H, 4 * H,
                          u > 0 ? sv + L.Cst + (size_t)off[u - 1] * H : nullptr,
                          sv + L.Cst + (size_t)r0 * H, c.hid + (size_t)r0 * H, b, H, go.gi, go.gf,
                          go.go, go.gg, go.tanh_out, s));
  }
  return kOk;
}

// `training` is a bit set: bit 0 = training (dropout on), kSeqInputDropoutOnly = dropout on layer 0's token embeddings
// only and none between the layers (torch.nn.LSTM built without dropout=: capnet.seq2seq, seq2seq/model.py:46-49).
// The attention stack (decoder_att_seq.cpp) calls seq_backward_upper with 0 / 1 and is unchanged.
static bool between_layers(int training, float dropout_p) {
  return (training & 1) && !(training & kSeqInputDropoutOnly) && dropout_p > 0.f;
}

SeqDims upper_dims(const SeqDims& d0) {
  SeqDims d = d0;
  d.E = d0.H;               // a layer above the first reads the hidden state of the layer below
  d.has_features = 0;
  return d;
}
}  // namespace seqd

SeqDims seq_upper_dims(const SeqDims& d0) { return upper_dims(d0); }

// The decoder recurrence of 1 to nlayers cells. One layer is DecoderFactoredLSTM / DecoderRNN (either cell). More are the
// stacked cells of either kind (capnet.stacked, capnet.nic_stacked: SURVEY App. A-1's semantics -- the reference ignores
// num_layers, stylenet/model.py:37, nic/model.py:35): layer 0 is the single-layer cell on [feature, dropout(B(w))...];
// layer l > 0 is the same cell on dropout(hidden of layer l - 1) at the same step; the top layer's hidden feeds C on
// free-running steps. For the LSTM cell this is torch.nn.LSTM(num_layers) under teacher forcing.
// Runs of teacher-forced steps outside, layers inside: a run's rows go up the stack before the next run starts (a
// free-running step's input needs the TOP layer's previous hidden state).
int seq_forward_stacked(const SeqDims& d0, int nlayers, const int* batch_sizes, const unsigned char* tf_mask,
                        const long long* captions, const float* features, const float* emb, const SeqWeights* w,
                        const float* Cw, const float* Cb, float dropout_p, unsigned long long seed, int training,
                        float* const* saved, int* const* saved_i, float* scratch, float* const* hiddens, int* err_flag,
                        hipStream_t s) {
  RC(check_dims(d0, batch_sizes));
  CAPNET_REQUIRE(nlayers >= 1 && nlayers <= 8 && w && saved && saved_i && hiddens, "seq_forward_stacked: bad argument");
  CAPNET_REQUIRE(tf_mask && captions && emb && scratch && err_flag, "seq_forward: null argument");
  CAPNET_REQUIRE(!d0.has_features || features, "seq_forward: features missing");
  CAPNET_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "seq_forward: dropout p=%f", dropout_p);
  const int E = d0.E, N = d0.N, H = d0.H;
  bool any_free = false;
  for (int t = 1; t < d0.steps; ++t) any_free |= !tf_mask[t];
  CAPNET_REQUIRE(!any_free || (Cw && Cb), "seq_forward: output projection needed for free-running steps");
  CAPNET_REQUIRE(d0.steps <= kMaxSteps, "seq_forward: %d steps > %d", d0.steps, kMaxSteps);
  const std::vector<int> off = step_offsets(batch_sizes, d0.steps);

  std::vector<LayerCtx> lay(nlayers);
  for (int l = 0; l < nlayers; ++l) {
    CAPNET_REQUIRE(saved[l] && saved_i[l] && hiddens[l], "seq_forward: null buffer of layer %d", l);
    lay[l].d = l == 0 ? d0 : upper_dims(d0);
    lay[l].L = make_layout(lay[l].d);
    lay[l].sv = saved[l]; lay[l].svi = saved_i[l]; lay[l].hid = hiddens[l];
    RC(build_row_tables(off, tf_mask, d0.has_features, false, lay[l].svi + lay[l].L.row_sample, lay[l].svi + lay[l].L.row_col,
                        lay[l].svi + lay[l].L.row_token, lay[l].svi + lay[l].L.prev_row, s));
    RC(pack_layer(lay[l], w[l], batch_sizes, s));
  }
  LayerCtx& c0 = lay[0];
  LayerCtx& top = lay[nlayers - 1];

  // ---- layer 0: inputs + input chain for every row whose input is known up front
  CAPNET_HIP_CHECK(hipMemsetAsync(c0.sv + c0.L.X, 0, (size_t)N * E * sizeof(float), s));
  RC(gather_inputs(captions, d0.T, features, emb, E, d0.V, c0.svi + c0.L.row_sample, c0.svi + c0.L.row_col,
                   c0.svi + c0.L.row_token, c0.sv + c0.L.X, E, 0, N, dropout_p, seed, training && dropout_p > 0.f, 0,
                   err_flag, s));
  float* skws = scratch + (size_t)d0.B * d0.V + 64;
  int* skctr = reinterpret_cast<int*>(skws + kSplitKWs);
  const SkWs sk{skws, kSplitKWs, skctr};
  CAPNET_HIP_CHECK(hipMemsetAsync(skctr, 0, kSplitKCounters * sizeof(int), s));
  RC(input_chain(c0.d, c0.L, c0.sv, 0, N, sk, s));
  const Feedback fb{captions, features, emb, Cw, Cb, d0.T, E, d0.V, H, dropout_p, seed, c0.svi + c0.L.row_sample,
                    c0.svi + c0.L.row_col, c0.svi + c0.L.row_token, scratch, err_flag};

  // ---- recurrence, run by run
  for (int t = 0; t < d0.steps;) {
    int t1 = t + 1;
    while (t1 < d0.steps && tf_mask[t1]) ++t1;
    const int b = batch_sizes[t], r0 = off[t], r1 = off[t1];
    if (t > 0 && !tf_mask[t]) {
      // predicted = argmax(C h_{t-1}) of the TOP layer for the b surviving rows; then this step's input chain
      RC(feed_back(fb, top.hid + (size_t)off[t - 1] * H, b, r0, c0.sv + c0.L.X, E, sk, s));
      RC(input_chain(c0.d, c0.L, c0.sv, r0, r0 + b, sk, s));
    }
    for (int l = 0; l < nlayers; ++l) {
      LayerCtx& c = lay[l];
      if (l > 0) {
        // X_l = dropout(hidden of the layer below) for the run's rows (kSeqInputDropoutOnly: a plain copy), then its
        // input chain
        RC(rows_dropout(lay[l - 1].hid, c.sv + c.L.X, r0, r1, H, dropout_p, seed, l, between_layers(training, dropout_p), s));
        RC(input_chain(c.d, c.L, c.sv, r0, r1, sk, s));
      }
      RC(recur(c, off, batch_sizes, t, t1, skws, skctr, err_flag, s));
    }
    t = t1;
  }
  return kOk;
}

// layer > 0 (a stacked layer above the first): the input gradient goes to dH_below = d hidden of the layer below (through
// the dropout between the layers) instead of the embedding / feature scatter.
// lead = 1: step 0 is the layer's given initial state (seq_backward_upper); lead = 0: the state starts at zero.
static int seq_backward_layer(const SeqDims& d, const int* batch_sizes, const float* dH, const float* hiddens,
                              const float* saved, const int* saved_i, float* scratch, const SeqGrads& g,
                              float dropout_p, unsigned long long seed, int training, int layer, float* dH_below,
                              hipStream_t s, int lead = 0, float* dh0 = nullptr, float* dc0 = nullptr) {
  RC(check_dims(d, batch_sizes));
  CAPNET_REQUIRE(dH && hiddens && saved && saved_i && scratch, "seq_backward: null argument");
  CAPNET_REQUIRE(g.dWcat && g.dbUW && g.dVcat && (layer > 0 ? dH_below != nullptr : g.dEmb != nullptr), "seq_backward: null gradient buffer");
  CAPNET_REQUIRE(lead == 0 || (layer > 0 && d.steps > 1 && dh0 && dc0), "seq_backward: leading state step");
  const Layout L = make_layout(d);
  const BwdLayout S = make_bwd_layout(d, lead);
  const int E = d.E, F = d.F, H = d.H, N = d.N;
  const bool fac = d.cell == kCellFactored;
  const GateOrder go = gate_order(d.cell);
  const std::vector<int> off = step_offsets(batch_sizes, d.steps);
  const int R0 = off[lead], Nr = N - R0;       // rows computed by the forward (the leading state step's are given)
  float *dPre = scratch + S.dPre, *Hprev = scratch + S.Hprev, *dh_rec = scratch + S.dh_rec, *dc = scratch + S.dc;
  float *dX = scratch + S.dX, *dA2 = scratch + S.dA2, *dA1 = scratch + S.dA1, *skws = scratch + S.skws;
  const float* sv = saved;
  CAPNET_HIP_CHECK(hipMemsetAsync(dh_rec, 0, (size_t)d.B * H * sizeof(float), s));
  CAPNET_HIP_CHECK(hipMemsetAsync(dc, 0, (size_t)d.B * H * sizeof(float), s));

  int slabs = 0;   // > 0: dh of the following step is still in `skws` as K-chunk slabs
  for (int t = d.steps - 1; t >= lead; --t) {
    const int b = batch_sizes[t], r0 = off[t];
    const int b_next = (t + 1 < d.steps) ? batch_sizes[t + 1] : 0;
    RC(lstm_pointwise_bwd(sv + L.G + (size_t)r0 * 4 * H, 4 * H, sv + L.Cst + (size_t)r0 * H,
                          t > 0 ? sv + L.Cst + (size_t)off[t - 1] * H : nullptr,
                          dH + (size_t)(r0 - R0) * H, slabs > 0 ? skws : dh_rec, dc, dPre + (size_t)r0 * 4 * H,
                          4 * H, b, b_next, H, go.gi, go.gf, go.go, go.gg, go.tanh_out, s, slabs,
                          (long)b_next * H));
    slabs = 0;
    if (t > 0) {
      // dh_{t-1}[0:b] = dPre_t . Wcat     (rows b..b_{t-1} of step t-1 have no successor);
      // the K-chunk partials stay in slabs and are summed by the next gate kernel
      RC(sgemm_splitk_slabs(false, b, H, 4 * H, dPre + (size_t)r0 * 4 * H, 4 * H, sv + L.Wcat, H, skws,
                            kSplitKFloats, &slabs, s));
      if (slabs == 0)
        RC(sgemm_splitk(false, false, b, H, 4 * H, dPre + (size_t)r0 * 4 * H, 4 * H, sv + L.Wcat, H,
                        dh_rec, H, nullptr, 0, skws, kSplitKFloats, s));
    }
  }
  if (lead) {
    // d h0 (all rows of the first step are alive), d c0
    if (slabs) RC(reduce_slabs(skws, slabs, batch_sizes[0], H, dh_rec, H, nullptr, 0, s));
    RC(copy_d2d(dh0, dh_rec, (size_t)batch_sizes[0] * H, s));
    RC(copy_d2d(dc0, dc, (size_t)batch_sizes[0] * H, s));
  }
  const float* X = sv + L.X + (size_t)R0 * E;
  // the factored chain's intermediate rows: saved by the forward, or (lead) formed here over all rows
  const float* A1 = lead ? scratch + S.A1c : sv + L.A1;
  const float* A2 = lead ? scratch + S.A2c : sv + L.A2;
  const Chain ch = chain_of(d, L, sv);
  if (fac && lead) RC(chain_rows(ch, X, Nr, scratch + S.A1c, scratch + S.A2c, SkWs{skws, kSplitKFloats, nullptr}, s));
  // recurrent weight gradient over all steps at once: dWcat = dPre^T . h_{t-1}
  dPre += (size_t)R0 * 4 * H;
  RC(gather_rows(hiddens, saved_i + L.prev_row + R0, Hprev, Nr, H, s));
  RC(sgemm_splitk(true, false, 4 * H, H, Nr, dPre, 4 * H, Hprev, H, g.dWcat, H, nullptr, 0, skws, kSplitKFloats, s));
  RC(colsum(dPre, 4 * H, Nr, 4 * H, g.dbUW, 0, s));
  if (fac) {
    CAPNET_REQUIRE(g.dUcat && g.dScat && g.dbS && g.dbV, "seq_backward: null factored gradient buffer");
    RC(chain_bwd_rows(ch, dPre, 4 * H, Nr, dA2, dA1, s));
    RC(chain_wgrads(ch, dPre, 4 * H, X, A1, A2, dA2, dA1, Nr, ChainGrads{g.dVcat, g.dbV, g.dScat, g.dbS, g.dUcat}, s));
  } else {
    RC(lstm_input_wgrad(dPre, 4 * H, X, E, H, Nr, g.dVcat, s));
  }
  // dX = (dA1 | dPre) . (Vcat | weight_ih)
  const int K = fac ? 4 * F : 4 * H;
  RC(sgemm_splitk(false, false, Nr, E, K, fac ? dA1 : dPre, K, sv + L.Vcat, E, dX, E, nullptr, 0, skws, kSplitKFloats, s));
  if (layer > 0) return rows_dropout(dX, dH_below, 0, Nr, E, dropout_p, seed, layer, between_layers(training, dropout_p), s);
  CAPNET_HIP_CHECK(hipMemsetAsync(g.dEmb, 0, (size_t)d.V * E * sizeof(float), s));
  if (g.dFeat) CAPNET_HIP_CHECK(hipMemsetAsync(g.dFeat, 0, (size_t)d.B * E * sizeof(float), s));
  // (the split-K slab area is free by now: the scatter's two integer tables over the vocabulary go there)
  return scatter_input_grad(dX, E, N, E, saved_i + L.row_sample, saved_i + L.row_col, saved_i + L.row_token, g.dEmb, g.dFeat, d.V,
                            dropout_p, seed, training && dropout_p > 0.f, s, reinterpret_cast<int*>(skws), kSplitKFloats);
}

int seqd::seq_backward_upper(const SeqDims& d, const int* batch_sizes, const float* dH, const float* hiddens,
                             const float* saved, const int* saved_i, float* scratch, const SeqGrads& g, float dropout_p,
                             unsigned long long seed, int training, int layer, float* dH_below, float* dh0, float* dc0,
                             hipStream_t s) {
  return seq_backward_layer(d, batch_sizes, dH, hiddens, saved, saved_i, scratch, g, dropout_p, seed, training, layer,
                            dH_below, s, 1, dh0, dc0);
}

// BPTT of seq_forward_stacked, top layer first: a layer's whole backward through time, then its input gradient becomes the
// hidden-state gradient of the layer below (only the top layer's hiddens have consumers outside the stack).
// dH_work: nlayers - 1 buffers [N][H]; grads: one SeqGrads per layer (dEmb / dFeat of layer 0 only).
int seq_backward_stacked(const SeqDims& d0, int nlayers, const int* batch_sizes, const float* dH_top,
                         const float* const* hiddens, const float* const* saved, const int* const* saved_i, float* scratch,
                         float* const* dH_work, const SeqGrads* g, float dropout_p, unsigned long long seed, int training,
                         hipStream_t s) {
  CAPNET_REQUIRE(nlayers >= 1 && nlayers <= 8 && hiddens && saved && saved_i && g && (nlayers == 1 || dH_work),
                 "seq_backward_stacked: bad argument");
  const float* dH = dH_top;
  for (int l = nlayers - 1; l >= 0; --l) {
    const SeqDims d = l == 0 ? d0 : upper_dims(d0);
    float* below = l > 0 ? dH_work[l - 1] : nullptr;
    RC(seq_backward_layer(d, batch_sizes, dH, hiddens[l], saved[l], saved_i[l], scratch, g[l], dropout_p, seed, training, l,
                          below, s));
    dH = below;
  }
  return kOk;
}

}  // namespace capnet
