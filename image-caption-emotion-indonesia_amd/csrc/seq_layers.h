// What the two sequence drivers (decoder_seq.cpp, decoder_att_seq.cpp) share: the step bookkeeping of a packed batch, the
// factored input chain in all its forms, a layer's saved-buffer layout, weight packing and recurrence, the backward
// scratch layout, the initial state from the pixel mean and the free-running feedback. Defined in decoder_seq.cpp.
#pragma once
#include <vector>

#include "common.h"
#include "kernels.h"

#define RC(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

namespace capnet {

constexpr size_t kSplitKFloats = 32ull * 64 * 2048;  // slabs for the per-step skinny GEMMs (16 MB)
constexpr size_t kSplitKWs = kSplitKFloats - kSplitKCounters;   // slabs | tile counters of the one-launch products (<= 16 rows)

namespace seqd {

// walks a buffer in 4-float-aligned pieces: a layout's offsets and, at the end, its total
struct Carve {
  size_t o = 0;
  size_t operator()(size_t n) { const size_t r = o; o += (n + 3) / 4 * 4; return r; }
};

// column block of each gate role: FactoredLSTM packs i,f,o,c~ ; nn.LSTMCell stores i,f,g,o and h = o tanh(c)
struct GateOrder { int gi, gf, go, gg, tanh_out; };
inline GateOrder gate_order(int cell) { return cell == kCellFactored ? GateOrder{0, 1, 2, 3, 0} : GateOrder{0, 1, 3, 2, 1}; }

// first packed row of every step (and N at the end)
std::vector<int> step_offsets(const int* batch_sizes, int steps);
// batch_sizes with a leading state step of B rows in front
std::vector<int> with_state_step(int B, const int* batch_sizes, int steps);
// batch_sizes: positive, non-increasing from B, summing to N
int check_batch_sizes(const char* who, const int* batch_sizes, int steps, int B, int N);
// the row tables (sample, caption column, token, previous row) of the packed rows `off`, built on the device from kernel
// arguments (no copy, no sync). lead: step 0 of `off` is a leading state step and tf_mask starts at step 1.
int build_row_tables(const std::vector<int>& off, const unsigned char* tf_mask, int has_features, bool lead, int* row_sample,
                     int* row_col, int* row_token, int* prev_row, hipStream_t s);

// slab workspace of the skinny products with its tile counters (ctr may be null: the product takes the plain hand-off)
struct SkWs { float* ws; size_t floats; int* ctr; };

// ---- the factored input chain G_g = U_g (S_g (V_g x + bV_g) + bS_g): gate-concatenated weights of either layout
struct Chain { const float *Vcat, *Scat, *Ucat, *bV, *bS; int XW, F, H; };   // XW: input width
struct ChainGrads { float *dVcat, *dbV, *dScat, *dbS, *dUcat; };
// n rows: A1 = X Vcat^T + bV, A2_g = A1_g S_g^T + bS_g, out_g = A2_g U_g^T + bias_g (or += where accumulate)
int chain_fwd(const Chain& c, const float* X, int n, float* A1, float* A2, float* out, long ldo, const float* bias, int accumulate,
              const SkWs& k, hipStream_t s);
// the chain as one matrix: US_g = U_g S_g, Weff_g = US_g V_g, c1_g = S_g bV_g + bS_g, bias_g += U_g c1_g
int chain_collapse(const Chain& c, float* US, float* Weff, float* c1, float* bias, const SkWs& k, hipStream_t s);
// all n rows after the loop: the intermediate rows A1, A2; their gradients dA2_g = dG_g U_g, dA1_g = dA2_g S_g; the five
// weight gradients (dG: the gates' gradient, leading dimension ldg)
int chain_rows(const Chain& c, const float* X, int n, float* A1, float* A2, const SkWs& k, hipStream_t s);
int chain_bwd_rows(const Chain& c, const float* dG, long ldg, int n, float* dA2, float* dA1, hipStream_t s);
int chain_wgrads(const Chain& c, const float* dG, long ldg, const float* X, const float* A1, const float* A2, const float* dA2,
                 const float* dA1, int n, const ChainGrads& g, hipStream_t s);
// nn.LSTMCell instead of the chain: d weight_ih [4H][XW] = dG^T X
int lstm_input_wgrad(const float* dG, long ldg, const float* X, int XW, int H, int n, float* dWih, hipStream_t s);

struct Layout {
  // saved float buffer
  size_t X, A1, A2, G, Cst, Vcat, Scat, Ucat, Wcat, Wfrag, Wp, bV, bS, bUW, total;
  // int buffer
  size_t row_sample, row_col, row_token, prev_row, ctl, itotal;
};
Layout make_layout(const SeqDims& d);
inline Chain chain_of(const SeqDims& d, const Layout& L, const float* sv) {
  return {sv + L.Vcat, sv + L.Scat, sv + L.Ucat, sv + L.bV, sv + L.bS, d.E, d.F, d.H};
}

// gate pre-activations (without the recurrent product) of rows [r0, r1) from their inputs X
int input_chain(const SeqDims& d, const Layout& L, float* sv, int r0, int r1, const SkWs& k, hipStream_t s);

// one layer of the (possibly stacked) recurrence: its dims (E = its input width), saved buffers and output rows
struct LayerCtx {
  SeqDims d;
  Layout L;
  float* sv; int* svi; float* hid;
  bool fused_step = false, persist = false;
  int segment = 0;
};
// a cell's gate-concatenated weight copies as items of one multi_copy launch: V, S, U, the recurrent W, bV, bS and bU + bW
// (nn.LSTMCell: weight_ih, weight_hh and bias_ih + bias_hh). W: SeqWeights or the cell part of AttWeights.
template <class W>
void add_cell_copies(CopyTable& ct, const W& w, int cell, size_t XW, size_t F, size_t H, float* Vcat, float* Scat, float* Ucat,
                     float* Wrec, float* bV, float* bS, float* brec) {
  if (cell != kCellFactored) {
    ct.add(Vcat, w.Vw[0], 4 * H * XW);
    ct.add(Wrec, w.Ww[0], 4 * H * H);
    ct.add(brec, w.Vb[0], 4 * H, w.Wb[0]);
    return;
  }
  for (int g = 0; g < 4; ++g) {
    ct.add(Vcat + g * F * XW, w.Vw[g], F * XW);
    ct.add(Scat + g * F * F, w.Sw[g], F * F);
    ct.add(Ucat + g * H * F, w.Uw[g], H * F);
    ct.add(Wrec + g * H * H, w.Ww[g], H * H);
    ct.add(bV + g * F, w.Vb[g], F);
    ct.add(bS + g * F, w.Sb[g], F);
    ct.add(brec + g * H, w.Ub[g], H, w.Wb[g]);
  }
}
// the layer's weight copies (one launch), the fused-step fragment image and the persistent kernel's image
int pack_layer(LayerCtx& c, const SeqWeights& w, const int* batch_sizes, hipStream_t s);
// steps [t, t1) of one layer whose gate pre-activations (without the recurrent product) are in G
int recur(LayerCtx& c, const std::vector<int>& off, const int* batch_sizes, int t, int t1, float* skws, int* skctr,
          int* err_flag, hipStream_t s);

// h0, c0 [B][H] = init_h / init_c (mean [B][C]), and the gradient of the four parameters from d h0, d c0
int init_state(const float* mean, int B, int H, int C, const UpperInit& w, float* h0, float* c0, const SkWs& k, hipStream_t s);
int init_state_grad(const float* dh0, const float* dc0, const float* mean, int B, int H, int C, const UpperInitGrads& g,
                    hipStream_t s);

// a free-running step: tokens of rows [r0, r0 + b) = argmax(h_prev C^T + Cb) (logits [b][V] is scratch), then their
// embeddings WITHOUT dropout into X
struct Feedback {
  const long long* captions;
  const float *features, *emb, *Cw, *Cb;
  int T, E, V, H;
  float dropout_p; unsigned long long seed;
  const int *row_sample, *row_col; int* row_token;
  float* logits; int* err_flag;
};
int feed_back(const Feedback& f, const float* h_prev, int b, int r0, float* X, long ldx, const SkWs& k, hipStream_t s);

// scratch of one layer's backward. lead: the layer has a leading state step and forms the chain's rows A1c, A2c itself.
struct BwdLayout { size_t dPre, Hprev, dh_rec, dc, dX, dA2, dA1, skws, A1c, A2c, total; };
BwdLayout make_bwd_layout(const SeqDims& d, int lead);

// Backward of one layer above the first with a LEADING STATE STEP: step 0 of `d` / `batch_sizes` holds the layer's
// initial state (bs[0] = B rows of h0 in hiddens, of c0 in the saved Cst) and is not computed; the real steps are
// 1 .. steps-1, and dH / dH_below are packed without it (row r there = row bs[0] + r here). The chain's intermediate
// rows A1, A2 are formed here over all rows (the fused upper step does not write them). dh0 / dc0 [B][H] receive the
// gradient of the initial state. Scratch: make_bwd_layout(d, 1).
int seq_backward_upper(const SeqDims& d, const int* batch_sizes, const float* dH, const float* hiddens, const float* saved,
                       const int* saved_i, float* scratch, const SeqGrads& g, float dropout_p, unsigned long long seed,
                       int training, int layer, float* dH_below, float* dh0, float* dc0, hipStream_t s);

}  // namespace seqd
}  // namespace capnet
