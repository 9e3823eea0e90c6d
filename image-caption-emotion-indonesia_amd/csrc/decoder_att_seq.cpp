// Sequence driver of the attention decoders: DecoderFactoredLSTMAtt.forward
// (stylenet/model_att.py:238-305) and nic DecoderRNNAtt.forward (nic/model_att.py:152-202, the
// same loop around nn.LSTMCell(E + C, H)) and their BPTT, one C call each.
//
// Per step t (rows = batch_sizes[t], previous state h, c -- the initial state is
// init_h/init_c(mean over pixels of the feature map), :185-194,260):
//   alpha, awe = attention(features, h)          (:279-280, Attention.forward :51-70)
//   gate = sigmoid(f_beta(h)); awe = gate * awe  (:283-284)
//   x = teacher forced ? dropout(B(w_t)) : B(argmax(C h))   (:285-288)
//   h, c = factored_lstm_step(cat[x, awe], h, c)             (:290-293, forward_step :196-236)
//   alphas[:rows, t] = alpha                                 (:296)
// MI355X mapping. Every product with h_{t-1} is ONE skinny GEMM per step against the stacked
// weight Wz = [W_i; W_f; W_o; W_c; decoder_att; f_beta] ([4H+A+C] x H): the forward writes
// Z = [gate pre-acts | att2 | f_beta(h)] rows, the backward reads dZ rows and gets dh in one
// product; the weight gradients of all six matrices are one TN GEMM over all packed rows after
// the loop. With cell = kCellLSTM the V/S/U chain is the single product [x | ctx] . weight_ih^T
// (gate order i,f,g,o; h = o tanh(c)) and Wz = [weight_hh; decoder_att; f_beta].
// encoder_att(features) is hoisted out of the time loop (the reference recomputes it
// every step) and its weight gradient is accumulated per sample and reduced by one GEMM.
#include <cstdlib>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "seq_layers.h"

namespace capnet {

using seqd::Carve; using seqd::Chain; using seqd::GateOrder; using seqd::SkWs;

namespace {

struct ALayout {
  size_t XA, Zf, A1, A2, Cst, alpha, awe, att1, mean, h0, c0, Vcat, Scat, Ucat, Wz, bV, bS, bz, US, Weff, c1, total;
  size_t row_sample, row_col, row_token, prev_row, itotal;
  int ZW, XW;
};

ALayout make_alayout(const AttDims& d) {
  ALayout L;
  L.ZW = 4 * d.H + d.A + d.C;
  L.XW = d.E + d.C;
  Carve take, itake;
  const size_t N = d.N, F = d.F, H = d.H;
  const bool fac = d.cell == kCellFactored;
  L.XA = take(N * L.XW);
  L.Zf = take(N * L.ZW);
  L.A1 = take(fac ? N * 4 * F : 4);
  L.A2 = take(fac ? N * 4 * F : 4);
  L.Cst = take(N * H);
  L.alpha = take(N * d.P);
  L.awe = take(N * d.C);
  L.att1 = take((size_t)d.B * d.P * d.A);
  L.mean = take((size_t)d.B * d.C);
  L.h0 = take((size_t)d.B * H);
  L.c0 = take((size_t)d.B * H);
  L.Vcat = take(fac ? 4 * F * L.XW : 4 * H * L.XW);   // LSTM: weight_ih [4H][E+C]
  L.Scat = take(fac ? 4 * F * F : 4);
  L.Ucat = take(fac ? 4 * H * F : 4);
  L.Wz = take((size_t)L.ZW * H);
  L.bV = take(4 * F);
  L.bS = take(4 * F);
  L.bz = take(L.ZW);
  // the factored chain as ONE matrix (steps of few rows, see chain_collapsed): U_g S_g [H][F], U_g S_g V_g [4H][E+C], S_g bV_g + bS_g
  L.US = take(fac ? 4 * H * F : 4);
  L.Weff = take(fac ? 4 * H * L.XW : 4);
  L.c1 = take(4 * F);
  L.total = take.o;
  L.row_sample = itake(N);
  L.row_col = itake(N);
  L.row_token = itake(N);
  L.prev_row = itake(N);
  L.itotal = itake.o;
  return L;
}
Chain chain_of(const AttDims& d, const ALayout& L, const float* sv) {
  return {sv + L.Vcat, sv + L.Scat, sv + L.Ucat, sv + L.bV, sv + L.bS, L.XW, d.F, d.H};
}

// Steps of at most 16 rows are a chain of dependent launches of 8-12 us each, whatever they compute (NOTEBOOK 4l): the
// factored input product U_g (S_g (V_g x + bV_g) + bS_g) is three of them per step and three more on the way back. With
// few rows the chain is run as ONE product per step against W_g = U_g S_g V_g (formed once per call: a 512 x 512 x 512
// and a 512 x 512 x 2348 product per gate, ~5 GFLOP, where the steps' own products are 0.05 GFLOP each) and bias
// U_g (S_g bV_g + bS_g); the intermediate rows A1 = V x + bV, A2 = S A1 + bS the weight gradients need, and their
// gradients dA2 = dgates U, dA1 = dA2 S, are formed for ALL rows at once after the backward loop -- the same sums in another
// association (fp32 rounding apart: the fixtures of the reference's own class hold either way). It pays up to the 128 rows
// the K-split step products take (64 / 96 rows: +5.4 % / +4.1 % images per second). 0 = by shape (B <= 128), 1 = always,
// -1 = never.
int g_att_chain_mode = [] {
  const char* e = getenv("CAPNET_ATT_CHAIN");        // "3": three products per step everywhere, "1": one everywhere (A/B)
  return e && e[0] == '3' ? -1 : (e && e[0] == '1' ? 1 : 0);
}();
bool chain_collapsed(const AttDims& d) {
  if (d.cell != kCellFactored || g_att_chain_mode < 0) return false;
  return g_att_chain_mode > 0 || d.B <= 128;
}

// The K-chunk partials of a step product, left for its consumer to sum: slab[k][M][N], k < *n (0: the shape qualifies
// for neither kernel and the caller takes the summed form).
int product_slabs(bool tb, int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* ws, size_t ws_floats,
                  int* n, hipStream_t s) {
  const int rc = sgemm_rows16_slabs(tb, M, N, K, A, lda, B, ldb, ws, ws_floats, n, s);
  if (rc || *n) return rc;
  return sgemm_splitk_slabs(tb, M, N, K, A, lda, B, ldb, ws, ws_floats, n, s);
}

constexpr size_t kAttSplitKFloats = 32ull * 64 * 4608;
constexpr size_t kAttSplitKWs = kAttSplitKFloats - kSplitKCounters;   // slabs | tile counters

int check(const AttDims& d, const int* bs) {
  CAPNET_REQUIRE(d.cell == kCellFactored || d.cell == kCellLSTM, "att decoder: unknown cell %d", d.cell);
  CAPNET_REQUIRE(d.B > 0 && d.T > 0 && d.steps > 0 && d.N > 0 && d.E > 0 && d.F > 0 && d.H > 0 &&
                     d.V > 0 && d.A > 0 && d.P > 0 && d.C > 0,
                 "att decoder: bad dims");
  CAPNET_REQUIRE(d.E % 4 == 0 && d.H % 4 == 0 && d.A % 4 == 0 && d.C % 512 == 0 && d.F % 4 == 0,
                 "att decoder: E, H, A, F must be multiples of 4 and the feature size of 512 "
                 "(E=%d H=%d A=%d F=%d C=%d)", d.E, d.H, d.A, d.F, d.C);
  CAPNET_REQUIRE(bs != nullptr && d.steps <= kMaxSteps && d.steps <= d.T, "att decoder: steps");
  CAPNET_REQUIRE(bs[0] == d.B, "att decoder: batch_sizes[0] must equal the batch");
  return seqd::check_batch_sizes("att decoder", bs, d.steps, d.B, d.N);
}

// Backward scratch. The chain's rows A1c, A2c have their full size whatever the chain mode, so that the size does not
// depend on a switch that can change between the size query and the call.
struct ABwdLayout {
  size_t Zb, dA2, dA1, A1c, A2c, dXA, Hprev, dh_rec, dc, dalpha_part, datt1, dwf_rows, dbf_rows, de_all, skws, dh_slabs, total;
  size_t dh_ws_floats;
};
ABwdLayout make_abwd_layout(const AttDims& d) {
  ABwdLayout S;
  Carve take;
  const ALayout L = make_alayout(d);
  const size_t N = d.N, B = d.B, rows4F = d.cell == kCellFactored ? N * 4 * d.F : 4;
  S.Zb = take(N * L.ZW);
  S.dA2 = take(rows4F);
  S.dA1 = take(rows4F);
  S.A1c = take(rows4F);     // the chain's intermediate rows, formed in the backward where the forward ran one product
  S.A2c = take(rows4F);
  S.dXA = take(N * L.XW);
  S.Hprev = take(N * d.H);
  S.dh_rec = take(B * d.H);
  S.dc = take(B * d.H);
  S.dalpha_part = take(B * (d.C / 256) * d.P);
  S.datt1 = take(B * d.P * d.A);
  S.dwf_rows = take(N * d.A);
  S.dbf_rows = take(N);
  S.de_all = take(N * d.P);   // softmax-backward scores of every row
  S.skws = take(kAttSplitKFloats);
  // dh_{t-1} = dZ_t . Wz has K = 4H + A + C: eighteen 256-k chunks. Its partials stay in the slab area and the gate kernel of
  // step t - 1 -- the next launch -- sums them (<= 16 rows: the hand-off inside the launch was 8 of the product's 12.6 us;
  // up to 128 rows: a splitk_reduce launch less per step)
  S.dh_ws_floats = d.B <= 128 ? (size_t)cdiv(L.ZW, 64) * B * d.H : 4;
  S.dh_slabs = take(S.dh_ws_floats);
  S.total = take.o;
  return S;
}

}  // namespace

int att_set_chain_mode(int mode) {
  const int old = g_att_chain_mode;
  g_att_chain_mode = mode < 0 ? -1 : (mode > 0 ? 1 : 0);
  return old;
}

size_t att_saved_floats(const AttDims& d) { return make_alayout(d).total; }
size_t att_saved_ints(const AttDims& d) { return make_alayout(d).itotal; }
size_t att_fwd_scratch_floats(const AttDims& d) {
  return (size_t)d.B * d.V + 64 + kAttSplitKFloats + (size_t)d.B * d.P + 64;
}
size_t att_bwd_scratch_floats(const AttDims& d) { return make_abwd_layout(d).total; }

namespace {
// one forward call of the attention cell: what its steps share (att_fwd_begin), so that the single-layer driver and the
// stacked one step through the same code
struct AttFwd {
  AttDims d;
  ALayout L;
  std::vector<int> off;
  const unsigned char* tf;
  seqd::Feedback fb;       // a free-running step's token from the top layer's hidden state
  const float *feat, *w_full, *b_full;
  float *sv, *escore, *hiddens, *alphas_bt;
  SkWs sk;
  bool one_product;
  hipStream_t s;
};

// row bookkeeping, weight packing, the collapsed chain, the time-invariant products and the teacher-forced inputs
int att_fwd_begin(AttFwd& f, const AttDims& d, const int* bs, const unsigned char* tf, const long long* captions,
                  const float* feat, const float* emb, const AttWeights& w, const float* Cw, const float* Cb,
                  float dropout_p, unsigned long long seed, int training, float* saved, int* saved_i, float* scratch,
                  float* hiddens, float* alphas_bt, int* err_flag, hipStream_t s) {
  RC(check(d, bs));
  CAPNET_REQUIRE(tf && captions && feat && emb && Cw && Cb && saved && saved_i && scratch && hiddens && alphas_bt && err_flag,
                 "att_seq_forward: null argument");
  CAPNET_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "att_seq_forward: dropout p");
  f.d = d;
  f.L = make_alayout(d);
  const ALayout& L = f.L;
  const int E = d.E, F = d.F, H = d.H, N = d.N, A = d.A, P = d.P, C = d.C, XW = L.XW;
  float* sv = saved;
  f.off = seqd::step_offsets(bs, d.steps);
  RC(seqd::build_row_tables(f.off, tf, 0, false, saved_i + L.row_sample, saved_i + L.row_col, saved_i + L.row_token,
                            saved_i + L.prev_row, s));
  float* skws = scratch + (size_t)d.B * d.V + 64;
  float* escore = skws + kAttSplitKFloats;   // raw attention scores of the current step [b][P]
  // tile counters of the one-launch products for steps of <= 16 rows (gemm_rows16_kernel): the tail of the slab area
  int* skctr = reinterpret_cast<int*>(skws + kAttSplitKWs);
  const SkWs sk{skws, kAttSplitKWs, skctr};
  CAPNET_HIP_CHECK(hipMemsetAsync(skctr, 0, kSplitKCounters * sizeof(int), s));
  // ---- pack weights
  CopyTable ct;      // one launch for the whole packing
  seqd::add_cell_copies(ct, w, d.cell, XW, F, H, sv + L.Vcat, sv + L.Scat, sv + L.Ucat, sv + L.Wz, sv + L.bV, sv + L.bS, sv + L.bz);
  ct.add(sv + L.Wz + (size_t)4 * H * H, w.dec_att_w, (size_t)A * H);
  ct.add(sv + L.Wz + (size_t)(4 * H + A) * H, w.f_beta_w, (size_t)C * H);
  ct.add(sv + L.bz + 4 * H, w.dec_att_b, A);
  ct.add(sv + L.bz + 4 * H + A, w.f_beta_b, C);
  RC(multi_copy(ct, s));
  const bool one_product = chain_collapsed(d);
  // bz[gate g] += U_g (S_g bV_g + bS_g)
  if (one_product) RC(seqd::chain_collapse(chain_of(d, L, sv), sv + L.US, sv + L.Weff, sv + L.c1, sv + L.bz, sk, s));

  // ---- time-invariant parts
  RC(global_avgpool(feat, sv + L.mean, d.B, P, C, s));
  RC(seqd::init_state(sv + L.mean, d.B, H, C, UpperInit{w.init_h_w, w.init_h_b, w.init_c_w, w.init_c_b}, sv + L.h0, sv + L.c0,
                      sk, s));
  // (through the K-split entry: with few images its 128 x 128 tiles are few and the product is cut over the chip)
  RC(sgemm_splitk(false, true, d.B * P, A, C, feat, C, w.enc_att_w, C, sv + L.att1, A, w.enc_att_b, 0, skws, kAttSplitKWs, s,
                  skctr, kSplitKCounters));
  CAPNET_HIP_CHECK(hipMemsetAsync(sv + L.XA, 0, (size_t)N * XW * sizeof(float), s));
  CAPNET_HIP_CHECK(hipMemsetAsync(alphas_bt, 0, (size_t)d.B * d.steps * P * sizeof(float), s));
  RC(gather_inputs(captions, d.T, nullptr, emb, E, d.V, saved_i + L.row_sample, saved_i + L.row_col, saved_i + L.row_token,
                   sv + L.XA, XW, 0, N, dropout_p, seed, training && dropout_p > 0.f, 0, err_flag, s));
  f.tf = tf; f.feat = feat; f.w_full = w.full_att_w; f.b_full = w.full_att_b;
  f.fb = seqd::Feedback{captions, nullptr, emb, Cw, Cb, d.T, E, d.V, H, dropout_p, seed, saved_i + L.row_sample,
                        saved_i + L.row_col, saved_i + L.row_token, scratch, err_flag};
  f.sv = sv; f.sk = sk; f.escore = escore; f.hiddens = hiddens; f.alphas_bt = alphas_bt;
  f.one_product = one_product; f.s = s;
  return kOk;
}

// step t of the attention cell. h_feed: the rows of step t - 1 whose argmax(C h) is fed back when step t is free running
// (the cell's own hiddens; the top layer's in a stack)
int att_fwd_step(AttFwd& f, int t, const float* h_feed) {
  const AttDims& d = f.d;
  const ALayout& L = f.L;
  const std::vector<int>& off = f.off;
  const int E = d.E, F = d.F, H = d.H, A = d.A, P = d.P, C = d.C, ZW = L.ZW, XW = L.XW;
  float* sv = f.sv;
  float* skws = f.sk.ws;
  int* skctr = f.sk.ctr;
  const bool fac = d.cell == kCellFactored, one_product = f.one_product;
  const GateOrder go = seqd::gate_order(d.cell);
  hipStream_t s = f.s;
  const int b = off[t + 1] - off[t], r0 = off[t];
  const float* hprev = t > 0 ? f.hiddens + (size_t)off[t - 1] * H : sv + L.h0;
  const float* cprev = t > 0 ? sv + L.Cst + (size_t)off[t - 1] * H : sv + L.c0;
  float* Z = sv + L.Zf + (size_t)r0 * ZW;
  // Z = h . Wz^T + bz  ->  [recurrent gate pre-acts | att2 | f_beta(h)]
  RC(sgemm_splitk(false, true, b, ZW, H, hprev, H, sv + L.Wz, H, Z, ZW, sv + L.bz, 0, skws, kAttSplitKWs, s, skctr, kSplitKCounters));
  RC(att_step_fwd(sv + L.att1, f.feat, Z + 4 * H, Z + 4 * H + A, ZW, f.w_full, f.b_full, b, P,
                  A, C, sv + L.alpha + (size_t)r0 * P, f.alphas_bt, d.steps, t,
                  sv + L.awe + (size_t)r0 * C, sv + L.XA + (size_t)r0 * XW + E, XW, f.escore, s));
  if (t > 0 && !f.tf[t]) RC(seqd::feed_back(f.fb, h_feed, b, r0, sv + L.XA, XW, f.sk, s));
  int x_slabs = 0;      // the input product's K-chunk partials, summed by the gate kernel (no hand-off inside the product's launch)
  // one product per step: [x | gated context] . Wx^T with Wx = U S V (the collapsed chain) or nn.LSTMCell's weight_ih
  const float* Wx = one_product ? sv + L.Weff : (fac ? nullptr : sv + L.Vcat);
  if (Wx) {
    RC(product_slabs(true, b, 4 * H, XW, sv + L.XA + (size_t)r0 * XW, XW, Wx, XW, skws, kAttSplitKWs, &x_slabs, s));
    if (!x_slabs)
      RC(sgemm_splitk(false, true, b, 4 * H, XW, sv + L.XA + (size_t)r0 * XW, XW, Wx, XW, Z, ZW, nullptr, 1, skws,
                      kAttSplitKWs, s, skctr, kSplitKCounters));
  } else {
    // factored chain on [x | gated context], added to the recurrent product in Z
    RC(seqd::chain_fwd(chain_of(d, L, sv), sv + L.XA + (size_t)r0 * XW, b, sv + L.A1 + (size_t)r0 * 4 * F,
                       sv + L.A2 + (size_t)r0 * 4 * F, Z, ZW, nullptr, 1, f.sk, s));
  }
  RC(lstm_pointwise_fwd(Z, ZW, cprev, sv + L.Cst + (size_t)r0 * H, f.hiddens + (size_t)r0 * H, b, H,
                        go.gi, go.gf, go.go, go.gg, go.tanh_out, s, x_slabs ? skws : nullptr, x_slabs));
  return kOk;
}
}  // namespace

int att_seq_backward(const AttDims& d, const int* bs, const float* dH, const float* dalphas_bt,
                     const float* hiddens, const float* feat, const AttWeights& w,
                     const float* saved, const int* saved_i, float* scratch, const AttGrads& g,
                     float dropout_p, unsigned long long seed, int training, hipStream_t s) {
  RC(check(d, bs));
  CAPNET_REQUIRE(dH && hiddens && feat && saved && saved_i && scratch, "att_seq_backward: null argument");
  const bool fac = d.cell == kCellFactored;
  const GateOrder go = seqd::gate_order(d.cell);
  CAPNET_REQUIRE(g.dVcat && g.dWz && g.dbz && g.dWe && g.dbe && g.dwf && g.dbf && g.dWih && g.dbih &&
                     g.dWic && g.dbic && g.dEmb && (!fac || (g.dbV && g.dScat && g.dbS && g.dUcat)),
                 "att_seq_backward: null gradient buffer");
  const ALayout L = make_alayout(d);
  const ABwdLayout S = make_abwd_layout(d);
  const int E = d.E, F = d.F, H = d.H, N = d.N, A = d.A, P = d.P, C = d.C, ZW = L.ZW, XW = L.XW;
  const float* sv = saved;
  const std::vector<int> off = seqd::step_offsets(bs, d.steps);
  const bool one_product = chain_collapsed(d);
  const Chain ch = chain_of(d, L, sv);
  float *Zb = scratch + S.Zb, *dA2 = scratch + S.dA2, *dA1 = scratch + S.dA1, *dXA = scratch + S.dXA, *Hprev = scratch + S.Hprev;
  float *dh_rec = scratch + S.dh_rec, *dc = scratch + S.dc, *dalpha_part = scratch + S.dalpha_part, *datt1 = scratch + S.datt1;
  float *dwf_rows = scratch + S.dwf_rows, *dbf_rows = scratch + S.dbf_rows, *de_all = scratch + S.de_all;
  float *skws = scratch + S.skws, *dh_slabs_ws = scratch + S.dh_slabs;
  const size_t dh_ws_floats = S.dh_ws_floats;
  const float* A1 = one_product ? scratch + S.A1c : sv + L.A1;
  const float* A2 = one_product ? scratch + S.A2c : sv + L.A2;
  int* skctr = reinterpret_cast<int*>(skws + kAttSplitKWs);
  CAPNET_HIP_CHECK(hipMemsetAsync(skctr, 0, kSplitKCounters * sizeof(int), s));
  CAPNET_HIP_CHECK(hipMemsetAsync(dh_rec, 0, (size_t)d.B * H * sizeof(float), s));
  CAPNET_HIP_CHECK(hipMemsetAsync(dc, 0, (size_t)d.B * H * sizeof(float), s));

  int dh_slabs = 0;
  for (int t = d.steps - 1; t >= 0; --t) {
    const int b = bs[t], r0 = off[t];
    const int b_next = (t + 1 < d.steps) ? bs[t + 1] : 0;
    const float* cprev = t > 0 ? sv + L.Cst + (size_t)off[t - 1] * H : sv + L.c0;
    const float* Zf = sv + L.Zf + (size_t)r0 * ZW;
    float* Z = Zb + (size_t)r0 * ZW;
    RC(lstm_pointwise_bwd(Zf, ZW, sv + L.Cst + (size_t)r0 * H, cprev, dH + (size_t)r0 * H, dh_slabs ? dh_slabs_ws : dh_rec, dc,
                          Z, ZW, b, b_next, H, go.gi, go.gf, go.go, go.gg, go.tanh_out, s, dh_slabs, (long)b_next * H));
    int dx_slabs = 0;     // d[x | ctx] as K-chunk partials: the context kernel -- the next launch -- sums them
    const float* Wx = one_product ? sv + L.Weff : (fac ? nullptr : sv + L.Vcat);
    if (Wx) {
      // d[x | ctx] = d gates . Wx
      RC(product_slabs(false, b, XW, 4 * H, Z, ZW, Wx, XW, skws, kAttSplitKWs, &dx_slabs, s));
      if (!dx_slabs)
        RC(sgemm_splitk(false, false, b, XW, 4 * H, Z, ZW, Wx, XW, dXA + (size_t)r0 * XW, XW,
                        nullptr, 0, skws, kAttSplitKWs, s, skctr, kSplitKCounters));
    } else {
      RC(sgemm_splitk_batched(false, false, b, F, H, Z, ZW, sv + L.Ucat, F, dA2 + (size_t)r0 * 4 * F,
                              4 * F, nullptr, 0, 4, H, (long)H * F, F, 0, skws, kAttSplitKWs, s, skctr, kSplitKCounters));
      RC(sgemm_splitk_batched(false, false, b, F, F, dA2 + (size_t)r0 * 4 * F, 4 * F, sv + L.Scat, F,
                              dA1 + (size_t)r0 * 4 * F, 4 * F, nullptr, 0, 4, F, (long)F * F, F, 0,
                              skws, kAttSplitKWs, s, skctr, kSplitKCounters));
      RC(sgemm_splitk(false, false, b, XW, 4 * F, dA1 + (size_t)r0 * 4 * F, 4 * F, sv + L.Vcat, XW,
                      dXA + (size_t)r0 * XW, XW, nullptr, 0, skws, kAttSplitKWs, s, skctr, kSplitKCounters));
    }
    RC(att_step_bwd(sv + L.att1, feat, Zf + 4 * H, ZW, Zf + 4 * H + A, ZW, sv + L.awe + (size_t)r0 * C,
                    sv + L.alpha + (size_t)r0 * P, w.full_att_w, dXA + (size_t)r0 * XW + E, XW,
                    dalphas_bt, d.steps, t, b, P, A, C, dalpha_part, Z + 4 * H + A, Z + 4 * H, ZW,
                    de_all + (size_t)r0 * P, dwf_rows + (size_t)r0 * A, dbf_rows + r0, s, dx_slabs ? skws : nullptr, dx_slabs, E));
    // dh_{t-1} (or dh0) = dZ . Wz
    dh_slabs = 0;
    if (d.B <= 128) RC(product_slabs(false, b, H, ZW, Z, ZW, sv + L.Wz, H, dh_slabs_ws, dh_ws_floats, &dh_slabs, s));
    if (!dh_slabs)
      RC(sgemm_splitk(false, false, b, H, ZW, Z, ZW, sv + L.Wz, H, dh_rec, H, nullptr, 0, skws, kAttSplitKWs, s, skctr, kSplitKCounters));
  }
  if (dh_slabs) RC(reduce_slabs(dh_slabs_ws, dh_slabs, d.B, H, dh_rec, H, nullptr, 0, s));      // dh0: all B rows are alive at t = 0
  // ---- weight gradients over all rows at once
  RC(gather_prev_rows(hiddens, saved_i + L.prev_row, sv + L.h0, saved_i + L.row_sample, Hprev, N, H, s));
  RC(sgemm_splitk(true, false, ZW, H, N, Zb, ZW, Hprev, H, g.dWz, H, nullptr, 0, skws, kAttSplitKWs, s));
  RC(colsum(Zb, ZW, N, ZW, g.dbz, 0, s));
  if (one_product) {
    // the rows the steps did not form: A1, A2 and their gradients
    RC(seqd::chain_rows(ch, sv + L.XA, N, scratch + S.A1c, scratch + S.A2c, SkWs{skws, kAttSplitKWs, skctr}, s));
    RC(seqd::chain_bwd_rows(ch, Zb, ZW, N, dA2, dA1, s));
  }
  if (fac) RC(seqd::chain_wgrads(ch, Zb, ZW, sv + L.XA, A1, A2, dA2, dA1, N, seqd::ChainGrads{g.dVcat, g.dbV, g.dScat, g.dbS, g.dUcat}, s));
  else RC(seqd::lstm_input_wgrad(Zb, ZW, sv + L.XA, XW, H, N, g.dVcat, s));     // (d bias_ih = d bias_hh = dbz[0:4H])
  RC(colsum(dwf_rows, A, N, A, g.dwf, 0, s));
  RC(colsum(dbf_rows, 1, N, 1, g.dbf, 0, s));
  // encoder_att: d att1 summed per sample over its steps in one pass over att1
  RC(att_datt1(sv + L.att1, sv + L.Zf + 4 * H, ZW, de_all, w.full_att_w, off.data(), d.steps, d.B, P, A,
               datt1, s));
  RC(sgemm_splitk(true, false, A, C, d.B * P, datt1, A, feat, C, g.dWe, C, nullptr, 0, skws, kAttSplitKWs, s));
  RC(colsum(datt1, A, d.B * P, A, g.dbe, 0, s, skws, kAttSplitKWs));
  // init_h / init_c: dh0 = dh_rec, dc0 = dc (all B rows are alive at t = 0)
  RC(seqd::init_state_grad(dh_rec, dc, sv + L.mean, d.B, H, C, UpperInitGrads{g.dWih, g.dbih, g.dWic, g.dbic}, s));
  CAPNET_HIP_CHECK(hipMemsetAsync(g.dEmb, 0, (size_t)d.V * E * sizeof(float), s));
  return scatter_input_grad(dXA, XW, N, E, saved_i + L.row_sample, saved_i + L.row_col, saved_i + L.row_token, g.dEmb, nullptr, d.V,
                            dropout_p, seed, training && dropout_p > 0.f, s, reinterpret_cast<int*>(skws), kAttSplitKWs);
}

// ---- stacked attention decoder (capnet.stacked_att) -------------------------------------------------------------------
// PERF-ONLY, PARITY UNPINNED: the reference accepts num_layers and ignores it (stylenet/model_att.py:81, nic/model_att.py:79).
// Layer 0 is the cell above, unchanged; its attention and f_beta gate read layer 0's own h^0_{t-1}. Layer l > 0 is layer 0's
// cell (factored: capnet.stacked_att; nn.LSTMCell(H, H): capnet.nic_stacked) on
// dropout_l(h^{l-1}_t) with its own parameters and initial state init_h{l} / init_c{l}(mean over pixels); only the top
// layer feeds C. As the attention stays inside layer 0, a run of teacher-forced steps goes up the stack run by run: layer
// 0 steps through the run, then each upper layer takes the run's rows (decoder_seq.cpp's layer machinery: one persistent
// launch per run, or per lone step the fused upper step below). An upper layer's buffers carry a LEADING STATE STEP: step
// 0 of its rows is the initial state (B rows), packed row r of the decoder is its row B + r.
namespace {
SeqDims upper_ext_dims(const AttDims& d) {
  SeqDims u;
  u.B = d.B; u.T = d.T + 1; u.steps = d.steps + 1; u.N = d.N + d.B; u.E = d.H; u.F = d.F; u.H = d.H; u.V = d.V;
  u.has_features = 0; u.cell = d.cell;           // the upper layers are layer 0's cell
  return u;
}
// after the layer's seq layout: the collapsed chain of the fused upper step, Weff [4H][H] = U_g S_g V_g, US [4H][F],
// c1 [4F] = S_g bV_g + bS_g, beff [4H] = U_g c1_g + bU_g + bW_g. The LSTM cell has no chain: its Weff is the layout's
// weight_ih copy (Vcat) and its beff the summed biases (bUW), nothing is added.
struct UpperExtra { size_t Weff, US, c1, beff, total; };
UpperExtra upper_extra(const SeqDims& u) {
  const seqd::Layout L = seqd::make_layout(u);
  const size_t base = L.total, H = u.H, F = u.F;
  UpperExtra x;
  if (u.cell != kCellFactored) {
    x.Weff = L.Vcat; x.beff = L.bUW; x.US = x.c1 = 0; x.total = base;
    return x;
  }
  x.Weff = base;
  x.US = x.Weff + 4 * H * H;
  x.c1 = x.US + 4 * H * F;
  x.beff = x.c1 + (4 * F + 3) / 4 * 4;
  x.total = x.beff + 4 * H;
  return x;
}
bool fused_upper_enabled() {        // read at every call: CAPNET_NO_FUSED_UPPER_STEP=1 takes the composed step
  const char* e = getenv("CAPNET_NO_FUSED_UPPER_STEP");
  return !(e && e[0] == '1');
}
}  // namespace

size_t att_stacked_saved_floats(const AttDims& d, int layer) {
  return layer == 0 ? att_saved_floats(d) : upper_extra(upper_ext_dims(d)).total;
}
size_t att_stacked_saved_ints(const AttDims& d, int layer) {
  return layer == 0 ? att_saved_ints(d) : seqd::make_layout(upper_ext_dims(d)).itotal;
}
size_t att_stacked_fwd_scratch_floats(const AttDims& d, int nlayers) {
  (void)nlayers;           // the upper layers work in the attention cell's slab area
  return att_fwd_scratch_floats(d);
}
// scratch of the stacked backward: layer 0's or an upper layer's, whichever is larger, then the gradient of an upper
// layer's initial state
struct StackedBwdLayout { size_t dh0, dc0, total; };
static StackedBwdLayout make_stacked_bwd_layout(const AttDims& d) {
  Carve take;
  const size_t a = make_abwd_layout(d).total, u = seqd::make_bwd_layout(upper_ext_dims(d), 1).total;
  take(a > u ? a : u);
  StackedBwdLayout S;
  S.dh0 = take((size_t)d.B * d.H);
  S.dc0 = take((size_t)d.B * d.H);
  S.total = take.o;
  return S;
}
size_t att_stacked_bwd_scratch_floats(const AttDims& d, int nlayers) {
  return nlayers > 1 ? make_stacked_bwd_layout(d).total : att_bwd_scratch_floats(d);
}

int att_seq_forward_stacked(const AttDims& d, int nlayers, const int* bs, const unsigned char* tf, const long long* captions,
                            const float* feat, const float* emb, const AttWeights& w0, const SeqWeights* wu,
                            const UpperInit* iu, const float* Cw, const float* Cb, float dropout_p, unsigned long long seed,
                            int training, float* const* saved, int* const* saved_i, float* scratch, float* const* hiddens,
                            float* alphas_bt, int* err_flag, hipStream_t s) {
  CAPNET_REQUIRE(nlayers >= 1 && nlayers <= 8 && saved && saved_i && hiddens && (nlayers == 1 || (wu && iu)),
                 "att_seq_forward_stacked: bad argument (layers %d)", nlayers);
  CAPNET_REQUIRE(nlayers == 1 || d.steps + 1 <= kMaxSteps, "att_seq_forward_stacked: %d steps", d.steps);
  for (int l = 0; l < nlayers; ++l)
    CAPNET_REQUIRE(saved[l] && saved_i[l] && hiddens[l], "att_seq_forward_stacked: null buffer of layer %d", l);
  AttFwd f;
  RC(att_fwd_begin(f, d, bs, tf, captions, feat, emb, w0, Cw, Cb, dropout_p, seed, training, saved[0], saved_i[0], scratch,
                   hiddens[0], alphas_bt, err_flag, s));
  const int B = d.B, H = d.H, C = d.C;
  if (nlayers == 1) {
    for (int t = 0; t < d.steps; ++t) RC(att_fwd_step(f, t, t > 0 ? hiddens[0] + (size_t)f.off[t - 1] * H : nullptr));
    return kOk;
  }
  const SeqDims ud = upper_ext_dims(d);
  const UpperExtra ux = upper_extra(ud);
  const std::vector<int> bse = seqd::with_state_step(B, bs, d.steps), offe = seqd::step_offsets(bse.data(), ud.steps);
  const bool fused = fused_upper_enabled();
  const bool drop = training && dropout_p > 0.f;
  const float* mean = f.sv + f.L.mean;
  std::vector<seqd::LayerCtx> up(nlayers);
  for (int l = 1; l < nlayers; ++l) {
    seqd::LayerCtx& c = up[l];
    c.d = ud;
    c.L = seqd::make_layout(ud);
    c.sv = saved[l]; c.svi = saved_i[l]; c.hid = hiddens[l];
    RC(seqd::build_row_tables(offe, tf, 0, true, c.svi + c.L.row_sample, c.svi + c.L.row_col, c.svi + c.L.row_token,
                              c.svi + c.L.prev_row, s));
    RC(seqd::pack_layer(c, wu[l - 1], bse.data(), s));
    // the leading state step: h0 = init_h{l}(mean), c0 = init_c{l}(mean)
    RC(seqd::init_state(mean, B, H, C, iu[l - 1], c.hid, c.sv + c.L.Cst, f.sk, s));
    if (fused && d.cell == kCellFactored) {
      // beff = bU + bW, then += U_g c1_g
      float* sv = c.sv;
      CAPNET_HIP_CHECK(hipMemcpyAsync(sv + ux.beff, sv + c.L.bUW, (size_t)4 * H * sizeof(float), hipMemcpyDeviceToDevice, s));
      RC(seqd::chain_collapse(seqd::chain_of(ud, c.L, sv), sv + ux.US, sv + ux.Weff, sv + ux.c1, sv + ux.beff, f.sk, s));
    }
  }
  const seqd::LayerCtx& top = up[nlayers - 1];
  for (int t = 0; t < d.steps;) {
    int t1 = t + 1;
    while (t1 < d.steps && tf[t1]) ++t1;
    // layer 0 through the run (only its first step can be free running: it feeds back argmax(C h^top_{t-1}))
    for (int u = t; u < t1; ++u) RC(att_fwd_step(f, u, u > 0 ? top.hid + (size_t)offe[u] * H : nullptr));
    const int b = bs[t], r0 = f.off[t], r1 = f.off[t1];
    for (int l = 1; l < nlayers; ++l) {
      seqd::LayerCtx& c = up[l];
      const float* below = l == 1 ? hiddens[0] : up[l - 1].hid + (size_t)B * H;     // packed row 0 of the layer below
      if (fused && t1 == t + 1 && lstm_upper_step_supported(b, H)) {
        const size_t pr = offe[t + 1], cr = offe[t];     // this step's rows; the previous step's (or the initial state)
        RC(lstm_upper_step(below + (size_t)r0 * H, c.hid + cr * H, c.sv + c.L.Cst + cr * H, c.sv + ux.Weff, c.sv + c.L.Wcat,
                           c.sv + ux.beff, c.sv + c.L.X + pr * H, c.sv + c.L.G + pr * 4 * H, c.sv + c.L.Cst + pr * H,
                           c.hid + pr * H, b, H, r0, dropout_p, seed, l, drop, s, d.cell));
        continue;
      }
      RC(rows_dropout(below, c.sv + c.L.X + (size_t)B * H, r0, r1, H, dropout_p, seed, l, drop, s));
      RC(seqd::input_chain(c.d, c.L, c.sv, B + r0, B + r1, SkWs{f.sk.ws, kSplitKWs, f.sk.ctr}, s));
      RC(seqd::recur(c, offe, bse.data(), t + 1, t1 + 1, f.sk.ws, f.sk.ctr, err_flag, s));
    }
    t = t1;
  }
  return kOk;
}

// BPTT of att_seq_forward_stacked, top layer first: a layer's input gradient is the hidden-state gradient of the layer
// below (only the top layer feeds C); layer 0's backward is att_seq_backward on it.
int att_seq_backward_stacked(const AttDims& d, int nlayers, const int* bs, const float* dH_top, const float* dalphas_bt,
                             const float* const* hiddens, const float* feat, const AttWeights& w0,
                             const float* const* saved, const int* const* saved_i, float* scratch, float* const* dH_work,
                             const AttGrads& g0, const SeqGrads* gu, const UpperInitGrads* giu, float dropout_p,
                             unsigned long long seed, int training, hipStream_t s) {
  CAPNET_REQUIRE(nlayers >= 1 && nlayers <= 8 && hiddens && saved && saved_i && scratch &&
                     (nlayers == 1 || (dH_work && gu && giu)),
                 "att_seq_backward_stacked: bad argument (layers %d)", nlayers);
  const float* dH = dH_top;
  if (nlayers > 1) {
    RC(check(d, bs));
    const SeqDims ud = upper_ext_dims(d);
    const int B = d.B, H = d.H, C = d.C;
    const std::vector<int> bse = seqd::with_state_step(B, bs, d.steps);
    const StackedBwdLayout S = make_stacked_bwd_layout(d);
    float *dh0 = scratch + S.dh0, *dc0 = scratch + S.dc0;
    const float* mean = saved[0] + make_alayout(d).mean;
    for (int l = nlayers - 1; l >= 1; --l) {
      CAPNET_REQUIRE(dH_work[l - 1] && hiddens[l] && saved[l] && saved_i[l], "att_seq_backward_stacked: null buffer of layer %d", l);
      const UpperInitGrads& gi = giu[l - 1];
      CAPNET_REQUIRE(gi.dWih && gi.dbih && gi.dWic && gi.dbic, "att_seq_backward_stacked: null initial-state gradient");
      RC(seqd::seq_backward_upper(ud, bse.data(), dH, hiddens[l], saved[l], saved_i[l], scratch, gu[l - 1], dropout_p, seed,
                                  training, l, dH_work[l - 1], dh0, dc0, s));
      // init_h{l} / init_c{l}: all B rows are alive at the first step
      RC(seqd::init_state_grad(dh0, dc0, mean, B, H, C, gi, s));
      dH = dH_work[l - 1];
    }
  }
  return att_seq_backward(d, bs, dH, dalphas_bt, hiddens[0], feat, w0, saved[0], saved_i[0], scratch, g0, dropout_p, seed,
                          training, s);
}

}  // namespace capnet
