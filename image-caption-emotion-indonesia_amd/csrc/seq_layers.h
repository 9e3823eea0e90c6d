// Layer machinery of the factored-LSTM sequence driver (decoder_seq.cpp), shared with the stacked attention driver
// (decoder_att_seq.cpp): a layer's saved-buffer layout, its weight packing, its input chain and its recurrence run by run.
#pragma once
#include <vector>

#include "common.h"
#include "kernels.h"

#define RC(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

namespace capnet {

constexpr size_t kSplitKFloats = 32ull * 64 * 2048;  // slabs for the per-step skinny GEMMs (16 MB)
constexpr size_t kSplitKWs = kSplitKFloats - kSplitKCounters;   // slabs | tile counters of the one-launch products (<= 16 rows)

namespace seqd {

struct Layout {
  // saved float buffer
  size_t X, A1, A2, G, Cst, Vcat, Scat, Ucat, Wcat, Wfrag, Wp, bV, bS, bUW, total;
  // int buffer
  size_t row_sample, row_col, row_token, prev_row, ctl, itotal;
};
Layout make_layout(const SeqDims& d);

struct GateOrder { int gi, gf, go, gg, tanh_out; };
GateOrder gate_order(int cell);

// gate pre-activations (without the recurrent product) of rows [r0, r1) from their inputs X
int input_chain(const SeqDims& d, const Layout& L, float* sv, int r0, int r1, float* ws, size_t ws_floats, hipStream_t s,
                int* ctr = nullptr);

// one layer of the (possibly stacked) recurrence: its dims (E = its input width), saved buffers and output rows
struct LayerCtx {
  SeqDims d;
  Layout L;
  float* sv;
  int* svi;
  float* hid;
  bool fused_step = false, persist = false;
  int segment = 0;
};

// gate-concatenated weight copies, the fused-step fragment image and the persistent kernel's image
int pack_layer(LayerCtx& c, const SeqWeights& w, const int* batch_sizes, hipStream_t s);
// steps [t, t1) of one layer whose gate pre-activations (without the recurrent product) are in G
int recur(LayerCtx& c, const std::vector<int>& off, const int* batch_sizes, int t, int t1, float* skws, int* skctr,
          int* err_flag, hipStream_t s);

// Backward of one layer above the first with a LEADING STATE STEP: step 0 of `d` / `batch_sizes` holds the layer's
// initial state (bs[0] = B rows of h0 in hiddens, of c0 in the saved Cst) and is not computed; the real steps are
// 1 .. steps-1, and dH / dH_below are packed without it (row r there = row bs[0] + r here). The chain's intermediate
// rows A1, A2 are formed here over all rows (the fused upper step does not write them). dh0 / dc0 [B][H] receive the
// gradient of the initial state.
int seq_backward_upper(const SeqDims& d, const int* batch_sizes, const float* dH, const float* hiddens, const float* saved,
                       const int* saved_i, float* scratch, const SeqGrads& g, float dropout_p, unsigned long long seed,
                       int training, int layer, float* dH_below, float* dh0, float* dc0, hipStream_t s);
size_t seq_bwd_upper_scratch_floats(const SeqDims& d);

}  // namespace seqd
}  // namespace capnet
