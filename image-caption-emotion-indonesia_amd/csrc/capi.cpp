// extern "C" boundary of libcapnet_hip.so (declared in include/capnet.h).
#include "../../include/capnet.h"

#include "common.h"
#include "kernels.h"

using namespace capnet;

static inline hipStream_t S(capnet_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

static SeqDims to_dims(const int* d) {
  SeqDims r;
  r.B = d[0]; r.T = d[1]; r.steps = d[2]; r.N = d[3]; r.E = d[4]; r.F = d[5]; r.H = d[6];
  r.V = d[7]; r.has_features = d[8]; r.cell = d[9];
  return r;
}

// the slots of a layer's 32-entry weight table its cell reads: all of the factored cell's; nn.LSTMCell's weight_ih,
// bias_ih, weight_hh, bias_hh sit in slots 0 / 4 / 24 / 28 (V w, V b, W w, W b of the first gate)
static bool weight_used(int cell, int i) { return cell == kCellFactored || i == 0 || i == 4 || i == 24 || i == 28; }
template <class Weights>           // SeqWeights, or the cell part of AttWeights
static void to_weights(const float* const* weights, Weights& w) {
  for (int g = 0; g < 4; ++g) {
    w.Vw[g] = weights[0 + g];  w.Vb[g] = weights[4 + g];
    w.Sw[g] = weights[8 + g];  w.Sb[g] = weights[12 + g];
    w.Uw[g] = weights[16 + g]; w.Ub[g] = weights[20 + g];
    w.Ww[g] = weights[24 + g]; w.Wb[g] = weights[28 + g];
  }
}
static void to_grads(float* const* q, SeqGrads& g) {
  g.dVcat = q[0]; g.dbV = q[1]; g.dScat = q[2]; g.dbS = q[3]; g.dUcat = q[4];
  g.dbUW = q[5]; g.dWcat = q[6]; g.dEmb = q[7]; g.dFeat = q[8];
}

static AttDims to_adims(const int* d) {
  AttDims r;
  r.B = d[0]; r.T = d[1]; r.steps = d[2]; r.N = d[3]; r.E = d[4]; r.F = d[5]; r.H = d[6];
  r.V = d[7]; r.A = d[8]; r.P = d[9]; r.C = d[10]; r.cell = d[11];
  return r;
}
static int to_aweights(const float* const* p, AttWeights* w, int cell) {
  CAPNET_REQUIRE(p != nullptr, "att decoder: null weight table");
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "att decoder: unknown cell %d", cell);
  for (int i = 0; i < 44; ++i)
    CAPNET_REQUIRE(p[i] || (i < 32 && !weight_used(cell, i)), "att decoder: weight %d is null", i);
  to_weights(p, *w);
  w->init_h_w = p[32]; w->init_h_b = p[33]; w->init_c_w = p[34]; w->init_c_b = p[35];
  w->enc_att_w = p[36]; w->enc_att_b = p[37]; w->dec_att_w = p[38]; w->dec_att_b = p[39];
  w->full_att_w = p[40]; w->full_att_b = p[41]; w->f_beta_w = p[42]; w->f_beta_b = p[43];
  return kOk;
}
static void to_agrads(float* const* q, AttGrads& g) {
  g.dVcat = q[0]; g.dbV = q[1]; g.dScat = q[2]; g.dbS = q[3]; g.dUcat = q[4];
  g.dWz = q[5]; g.dbz = q[6]; g.dWe = q[7]; g.dbe = q[8]; g.dwf = q[9];
  g.dbf = q[10]; g.dWih = q[11]; g.dbih = q[12]; g.dWic = q[13]; g.dbic = q[14];
  g.dEmb = q[15];
}

extern "C" {

const char* capnet_last_error(void) { return last_error(); }
int capnet_abi_version(void) { return 1; }

int capnet_sgemm(int transA, int transB, int M, int N, int K, const float* A, long lda,
                 const float* B, long ldb, float* C, long ldc, const float* bias, int accumulate,
                 int batch, long strideA, long strideB, long strideC, long strideBias,
                 int force_tile, capnet_stream_t stream) {
  return sgemm(transA != 0, transB != 0, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, batch,
               strideA, strideB, strideC, strideBias, force_tile, S(stream));
}

int capnet_sgemm_b3(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                    float* C, long ldc, const float* bias, int accumulate, int batch, long strideA, long strideB,
                    long strideC, long strideBias, float* ws, size_t ws_floats, capnet_stream_t stream) {
  return sgemm_b3(transA != 0, transB != 0, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, batch, strideA, strideB,
                  strideC, strideBias, S(stream), ws, ws_floats);
}
int capnet_sgemm_b3_eligible(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                             const float* C, long ldc, const float* bias, int batch, long strideA, long strideB,
                             long strideC, long strideBias) {
  return sgemm_b3_eligible(transA != 0, transB != 0, M, N, K, A, lda, B, ldb, C, ldc, bias, batch, strideA, strideB, strideC,
                           strideBias) ? 1 : 0;
}

int capnet_sgemm_nt_dma_eligible(int M, int N, int K, const float* A, long lda, const float* B,
                                 long ldb, const float* C, long ldc) {
  return sgemm_nt_dma_eligible(M, N, K, A, lda, B, ldb, C, ldc) ? 1 : 0;
}
int capnet_sgemm_nt_dma(int M, int N, int K, const float* A, long lda, const float* B, float* C,
                        const float* bias, capnet_stream_t stream) {
  CAPNET_REQUIRE(A && B && C, "sgemm_nt_dma: null operand");
  return sgemm_nt_dma(M, N, K, A, lda, B, C, bias, S(stream));
}
int capnet_conv1x1_tiles_m(long M) { return conv1x1_tiles_m(M); }
int capnet_conv1x1_fwd_dma(const float* x, long sxb, long sxh, long sxw, const float* w_oi, float* y,
                           float* part_sum, float* part_sq, int B, int H, int W, int Cin, int Cout,
                           int stride, const float* out_scale, const float* out_shift, const float* res,
                           int relu_out, capnet_stream_t stream) {
  return conv1x1_fwd_dma(x, sxb, sxh, sxw, w_oi, y, part_sum, part_sq, B, H, W, Cin, Cout, stride,
                         S(stream), out_scale, out_shift, res, relu_out);
}

int capnet_conv1x1_fwd_areg(const float* x, const unsigned* image, int bn, float* y, const float* in_scale,
                            const float* in_shift, int relu_in, float* part_sum, float* part_sq, long M, int Cin, int Cout,
                            int in_exp, capnet_stream_t stream) {
  return conv1x1_fwd_areg(x, image, bn, y, in_scale, in_shift, relu_in, part_sum, part_sq, M, Cin, Cout, in_exp, S(stream));
}
size_t capnet_conv1x1_f16x3_weight_words(int Cin, int Cout) { return conv1x1_f16x3_weight_words(Cin, Cout); }
int capnet_conv1x1_f16x3_bn(long M, int Cout) { return conv1x1_f16x3_bn(M, Cout); }
int capnet_conv1x1_f16x3_pack(const float* w_oi, unsigned* image, int Cout, int Cin, int bn,
                              capnet_stream_t stream) {
  return conv1x1_f16x3_pack(w_oi, image, Cout, Cin, bn, S(stream));
}
int capnet_conv1x1_fwd_f16x3(const float* x, long sxb, long sxh, long sxw, const unsigned* image, int bn,
                             float* y, const float* in_scale, const float* in_shift, int relu_in,
                             float* part_sum, float* part_sq, int B, int H, int W, int Cin, int Cout,
                             int stride, const float* out_scale, const float* out_shift,
                             const float* res, int relu_out, capnet_stream_t stream) {
  CAPNET_REQUIRE(conv1x1_f16x3_eligible(x, sxb, sxh, sxw, 1, B, H, W, Cin, Cout, stride, in_scale, in_shift),
                 "capnet_conv1x1_fwd_f16x3: operands not eligible (Cin %% 64, Cout %% 64, 16-B aligned rows, Cin <= 512 with a folded input)");
  return conv1x1_fwd_f16x3(x, sxb, sxh, sxw, image, bn, y, in_scale, in_shift, relu_in, part_sum, part_sq, B,
                           H, W, Cin, Cout, stride, S(stream), out_scale, out_shift, res, relu_out);
}

size_t capnet_conv_f16x3_weight_words(int Cin, int Cout, int k) { return conv_f16x3_weight_words(Cin, Cout, k); }
int capnet_conv_f16x3_pack(const float* w_oihw, unsigned* image, int Cout, int Cin, int k, int bn,
                           capnet_stream_t stream) {
  return conv_f16x3_pack(w_oihw, image, Cout, Cin, k, bn, S(stream));
}
int capnet_conv2d_fwd_f16x3(const float* x, long sxb, long sxh, long sxw, const unsigned* image, int bn, float* y,
                            const float* in_scale, const float* in_shift, int relu_in, float* part_sum,
                            float* part_sq, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                            const float* out_scale, const float* out_shift, const float* res, int relu_out,
                            capnet_stream_t stream) {
  CAPNET_REQUIRE(conv_f16x3_eligible(x, sxb, sxh, sxw, 1, B, H, W, Cin, Cout, k, stride, pad, in_scale, in_shift),
                 "capnet_conv2d_fwd_f16x3: operands not eligible (k = 1 / pad 0 or k = 3 / pad 1, Cin %% 64, Cout %% 64, 16-B aligned rows, Cin <= 512 with a folded input)");
  return conv_fwd_f16x3(x, sxb, sxh, sxw, image, bn, y, in_scale, in_shift, relu_in, part_sum, part_sq, B, H, W,
                        Cin, Cout, k, stride, pad, S(stream), out_scale, out_shift, res, relu_out);
}

int capnet_conv3x3_fwd_patch(const float* x, const unsigned* image, int bn, float* y, const float* in_scale,
                             const float* in_shift, int relu_in, float* part_sum, float* part_sq, int B, int H, int W,
                             int Cin, int Cout, int shared_chip, capnet_stream_t stream) {
  return conv3x3_fwd_patch(x, image, bn, y, in_scale, in_shift, relu_in, part_sum, part_sq, B, H, W, Cin, Cout, S(stream),
                           shared_chip != 0);
}
int capnet_conv1x1_fwd_tail(const float* y3, const float* s1, const float* t1, const float* res, const float* s2, const
                            float* t2, float* tail_out, const unsigned* image, int bn, float* y, float* part_sum, float*
                            part_sq, long M, int Cin, int Cout, capnet_stream_t stream) {
  return conv1x1_fwd_tail(y3, s1, t1, res, s2, t2, tail_out, image, bn, y, part_sum, part_sq, M, Cin, Cout, S(stream));
}
// the same three with the input's power-of-two prescale (capnet.h)
int capnet_conv2d_fwd_f16x3_scaled(const float* x, long sxb, long sxh, long sxw, const unsigned* image, int bn, float* y,
                                   const float* in_scale, const float* in_shift, int relu_in, float* part_sum,
                                   float* part_sq, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                   int in_exp, capnet_stream_t stream) {
  CAPNET_REQUIRE(conv_f16x3_eligible(x, sxb, sxh, sxw, 1, B, H, W, Cin, Cout, k, stride, pad, in_scale, in_shift),
                 "capnet_conv2d_fwd_f16x3_scaled: operands not eligible");
  return conv_fwd_f16x3(x, sxb, sxh, sxw, image, bn, y, in_scale, in_shift, relu_in, part_sum, part_sq, B, H, W,
                        Cin, Cout, k, stride, pad, S(stream), nullptr, nullptr, nullptr, 0, in_exp);
}
int capnet_conv3x3_fwd_patch_scaled(const float* x, const unsigned* image, int bn, float* y, const float* in_scale,
                                    const float* in_shift, int relu_in, float* part_sum, float* part_sq, int B, int H,
                                    int W, int Cin, int Cout, int shared_chip, int in_exp, capnet_stream_t stream) {
  return conv3x3_fwd_patch(x, image, bn, y, in_scale, in_shift, relu_in, part_sum, part_sq, B, H, W, Cin, Cout, S(stream),
                           shared_chip != 0, in_exp);
}
int capnet_conv1x1_fwd_tail_scaled(const float* y3, const float* s1, const float* t1, const float* res, const float* s2,
                                   const float* t2, float* tail_out, const unsigned* image, int bn, float* y, float*
                                   part_sum, float* part_sq, long M, int Cin, int Cout, int in_exp, capnet_stream_t stream) {
  return conv1x1_fwd_tail(y3, s1, t1, res, s2, t2, tail_out, image, bn, y, part_sum, part_sq, M, Cin, Cout, S(stream),
                          in_exp);
}
size_t capnet_conv_stem_f16x3_weight_words(void) { return conv_stem_f16x3_weight_words(); }
int capnet_conv_stem_f16x3_part_rows(int B, int H, int W) { return conv_stem_f16x3_part_rows(B, H, W); }
int capnet_conv_stem_f16x3_pack(const float* w_oihw, unsigned* image, capnet_stream_t stream) {
  return conv_stem_f16x3_pack(w_oihw, image, S(stream));
}
int capnet_conv_stem_fwd_f16x3(const float* x, long sxb, long sxc, long sxh, const unsigned* image, float* y,
                               float* part_sum, float* part_sq, int B, int H, int W, capnet_stream_t stream) {
  return conv_stem_fwd_f16x3(x, sxb, sxc, sxh, image, y, part_sum, part_sq, B, H, W, S(stream));
}

// the convolution kernels' own eligibility predicates (host code, no device)
int capnet_conv_v2_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int B, int Cin, int Cout,
                            const float* in_scale, const float* in_shift) {
  return conv_v2_eligible(x, sxb, sxh, sxw, sxc, B, Cin, Cout, in_scale, in_shift) ? 1 : 0;
}
int capnet_conv1x1_dma_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int B, int H, int W, int Cin,
                                int Cout, int stride) {
  return conv1x1_dma_eligible(x, sxb, sxh, sxw, sxc, B, H, W, Cin, Cout, stride) ? 1 : 0;
}
int capnet_conv_f16x3_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int B, int H, int W, int Cin,
                               int Cout, int k, int stride, int pad, const float* in_scale, const float* in_shift) {
  return conv_f16x3_eligible(x, sxb, sxh, sxw, sxc, B, H, W, Cin, Cout, k, stride, pad, in_scale, in_shift) ? 1 : 0;
}
int capnet_conv3x3_patch_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int B, int H, int W, int Cin,
                                  int Cout, int k, int stride, int pad, const float* in_scale, const float* in_shift) {
  return conv3x3_patch_eligible(x, sxb, sxh, sxw, sxc, B, H, W, Cin, Cout, k, stride, pad, in_scale, in_shift) ? 1 : 0;
}
int capnet_conv1x1_areg_eligible(const float* x, long M, int Cin, int Cout, int bn, const float* in_scale,
                                 const float* in_shift) {
  return conv1x1_areg_eligible(x, M, Cin, Cout, bn, in_scale, in_shift) ? 1 : 0;
}
int capnet_conv1x1_tail_eligible(const float* y3, const float* res, long M, int Cin, int Cout) {
  return conv1x1_tail_eligible(y3, res, M, Cin, Cout) ? 1 : 0;
}
int capnet_conv_stem_f16x3_eligible(const float* x, long sxb, long sxc, long sxh, long sxw, int B, int H, int W, int Cin,
                                    int Cout, int k, int stride, int pad) {
  return conv_stem_f16x3_eligible(x, sxb, sxc, sxh, sxw, B, H, W, Cin, Cout, k, stride, pad) ? 1 : 0;
}

int capnet_sgemm_splitk(int transA, int transB, int M, int N, int K, const float* A, long lda,
                        const float* B, long ldb, float* C, long ldc, const float* bias,
                        int accumulate, float* workspace, size_t workspace_floats,
                        capnet_stream_t stream) {
  CAPNET_REQUIRE(M >= 0 && N >= 0 && K >= 0, "sgemm_splitk: negative dimension");
  return sgemm_splitk(transA != 0, transB != 0, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate,
                      workspace, workspace_floats, S(stream));
}
int capnet_sgemm_splitk_fused(int transA, int transB, int M, int N, int K, const float* A, long lda,
                              const float* B, long ldb, float* C, long ldc, const float* bias,
                              int accumulate, float* workspace, size_t workspace_floats, int* counters,
                              size_t n_counters, capnet_stream_t stream) {
  CAPNET_REQUIRE(M >= 0 && N >= 0 && K >= 0, "sgemm_splitk_fused: negative dimension");
  return sgemm_splitk(transA != 0, transB != 0, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate,
                      workspace, workspace_floats, S(stream), counters, n_counters);
}
int capnet_colsum(const float* x, long ld, int rows, int C, float* out, int accumulate,
                  capnet_stream_t stream) {
  return colsum(x, ld, rows, C, out, accumulate, S(stream));
}

int capnet_colsum_ws(const float* x, long ld, int rows, int C, float* out, int accumulate, float* workspace,
                     size_t workspace_floats, capnet_stream_t stream) {
  CAPNET_REQUIRE(x && out && C > 0 && rows >= 0, "colsum: bad argument");
  CAPNET_REQUIRE(ld >= C, "colsum: leading dimension too small (ld=%ld C=%d)", ld, C);
  return colsum(x, ld, rows, C, out, accumulate, S(stream), workspace, workspace_floats);
}
int capnet_reduce_slabs(const float* slab, int count, int M, int N, float* out, long ldc, const float* bias,
                        int accumulate, capnet_stream_t stream) {
  CAPNET_REQUIRE(slab && out && count > 0 && M > 0 && N > 0, "reduce_slabs: bad argument");
  CAPNET_REQUIRE(ldc >= N, "reduce_slabs: leading dimension too small (ldc=%ld N=%d)", ldc, N);
  return reduce_slabs(slab, count, M, N, out, ldc, bias, accumulate, S(stream));
}
int capnet_sgemm_splitk_batched(int transA, int transB, int M, int N, int K, const float* A, long lda,
                                const float* B, long ldb, float* C, long ldc, const float* bias, int accumulate,
                                int batch, long strideA, long strideB, long strideC, long strideBias,
                                float* workspace, size_t workspace_floats, int* counters, size_t n_counters,
                                capnet_stream_t stream) {
  CAPNET_REQUIRE(M >= 0 && N >= 0 && K >= 0 && batch >= 0, "sgemm_splitk_batched: bad argument (negative dimension)");
  if (M == 0 || N == 0 || batch == 0) return kOk;
  CAPNET_REQUIRE(A && B && C, "sgemm_splitk_batched: bad argument (null operand)");
  CAPNET_REQUIRE(lda >= (transA ? M : K) && ldb >= (transB ? K : N) && ldc >= N,
                 "sgemm_splitk_batched: leading dimension too small (lda=%ld ldb=%ld ldc=%ld M=%d N=%d K=%d)", lda, ldb,
                 ldc, M, N, K);
  return sgemm_splitk_batched(transA != 0, transB != 0, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, batch,
                              strideA, strideB, strideC, strideBias, workspace, workspace_floats, S(stream), counters,
                              n_counters);
}
int capnet_sgemm_splitk_slabs(int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                              float* workspace, size_t workspace_floats, int* n_slabs, capnet_stream_t stream) {
  CAPNET_REQUIRE(n_slabs && A && B && M >= 0 && N >= 0 && K >= 0, "sgemm_splitk_slabs: bad argument");
  CAPNET_REQUIRE(lda >= K && ldb >= (transB ? K : N), "sgemm_splitk_slabs: leading dimension too small (lda=%ld ldb=%ld)",
                 lda, ldb);
  return sgemm_splitk_slabs(transB != 0, M, N, K, A, lda, B, ldb, workspace, workspace_floats, n_slabs, S(stream));
}
int capnet_sgemm_rows16_slabs(int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                              float* workspace, size_t workspace_floats, int* n_slabs, capnet_stream_t stream) {
  CAPNET_REQUIRE(n_slabs && A && B && M >= 0 && N >= 0 && K >= 0, "sgemm_rows16_slabs: bad argument");
  CAPNET_REQUIRE(lda >= K && ldb >= (transB ? K : N), "sgemm_rows16_slabs: leading dimension too small (lda=%ld ldb=%ld)",
                 lda, ldb);
  return sgemm_rows16_slabs(transB != 0, M, N, K, A, lda, B, ldb, workspace, workspace_floats, n_slabs, S(stream));
}

static void route_detail(int* detail, bool vec, int splits, int chunk, int tiles) {
  if (!detail) return;
  detail[0] = vec ? 1 : 0; detail[1] = splits; detail[2] = chunk; detail[3] = tiles;
}
int capnet_sgemm_route(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                       const float* C, long ldc, const float* bias, int accumulate, int batch, long strideA,
                       long strideB, long strideC, long strideBias, int force_tile, int* detail) {
  SgemmPlan p;
  const int rc = sgemm_plan(transA != 0, transB != 0, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, batch, strideA,
                            strideB, strideC, strideBias, force_tile, &p);
  if (rc != kOk) return rc;
  route_detail(detail, p.vec, 1, 0, p.tiles_m * p.tiles_n);
  return p.route;
}
int capnet_sgemm_splitk_route(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B,
                              long ldb, const float* C, long ldc, const float* bias, int accumulate, int batch,
                              long strideA, long strideB, long strideC, long strideBias, const float* workspace,
                              size_t workspace_floats, const int* counters, size_t n_counters, int* detail) {
  SplitkPlan p;
  const int rc = sgemm_splitk_plan(transA != 0, transB != 0, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, batch,
                                   strideA, strideB, strideC, strideBias, workspace, workspace_floats, counters,
                                   n_counters, true, &p);
  if (rc != kOk) return rc;
  if (p.route == kRouteFellThrough) {
    route_detail(detail, p.inner.vec, 1, 0, p.inner.tiles_m * p.inner.tiles_n);
    return p.inner.route == kRouteNone ? kRouteNone : (kRouteFellThrough | p.inner.route);
  }
  route_detail(detail, p.vec, p.splits, p.chunk, p.tiles);
  return p.route;
}

int capnet_argmax_rows(const float* x, int rows, int ld, int V, int* out, capnet_stream_t stream) {
  CAPNET_REQUIRE(x && out && ld >= V && V > 0, "argmax_rows: bad argument");
  return argmax_rows(x, rows, ld, V, out, S(stream));
}

int capnet_trunk_create(int batch, int height, int width, capnet_trunk_t** out) {
  return trunk_create(batch, height, width, reinterpret_cast<Trunk**>(out));
}
void capnet_trunk_destroy(capnet_trunk_t* t) { trunk_destroy(reinterpret_cast<Trunk*>(t)); }
size_t capnet_trunk_workspace_bytes(const capnet_trunk_t* t) {
  return trunk_workspace_bytes(reinterpret_cast<const Trunk*>(t));
}
int capnet_trunk_num_convs(const capnet_trunk_t* t) {
  return trunk_num_convs(reinterpret_cast<const Trunk*>(t));
}
int capnet_trunk_final_side(const capnet_trunk_t* t) {
  return trunk_final_side(reinterpret_cast<const Trunk*>(t));
}
double capnet_trunk_flops(const capnet_trunk_t* t) {
  return trunk_flops(reinterpret_cast<const Trunk*>(t));
}
int capnet_trunk_conv_shape(const capnet_trunk_t* t, int i, int* cout, int* cin, int* ksize,
                            int* stride, int* row_stride) {
  CAPNET_REQUIRE(t && cout && cin && ksize && stride && row_stride, "trunk_conv_shape: null");
  return trunk_conv_shape(reinterpret_cast<const Trunk*>(t), i, cout, cin, ksize, stride,
                          row_stride);
}
int capnet_trunk_forward(const capnet_trunk_t* t, const float* images_nchw,
                         const float* const* w_packed, const float* const* bn_weight,
                         const float* const* bn_bias, float* const* bn_running_mean,
                         float* const* bn_running_var, int train, float momentum, float eps,
                         void* workspace, float* out_pooled, float* out_map,
                         const int* input_exponents, int* err_flag, capnet_stream_t stream) {
  return trunk_forward(reinterpret_cast<Trunk*>(const_cast<capnet_trunk_t*>(t)), images_nchw, w_packed, bn_weight,
                       bn_bias, bn_running_mean, bn_running_var, train, momentum, eps,
                       reinterpret_cast<float*>(workspace), out_pooled, out_map, input_exponents, err_flag, S(stream));
}
int capnet_trunk_set_tail_balance(const capnet_trunk_t* t, int on) {
  return trunk_set_tail_balance(reinterpret_cast<Trunk*>(const_cast<capnet_trunk_t*>(t)), on);
}
int capnet_trunk_update_running(const capnet_trunk_t* t, const void* workspace,
                                float* const* bn_running_mean, float* const* bn_running_var,
                                float momentum, capnet_stream_t stream) {
  return trunk_update_running(reinterpret_cast<Trunk*>(const_cast<capnet_trunk_t*>(t)),
                              reinterpret_cast<const float*>(workspace), bn_running_mean, bn_running_var,
                              momentum, S(stream));
}
double capnet_trunk_conv_flops(const capnet_trunk_t* t, int i) {
  return trunk_conv_flops(reinterpret_cast<const Trunk*>(t), i);
}
int capnet_trunk_conv_kmajor(const capnet_trunk_t* t, int i) {
  return trunk_conv_kmajor(reinterpret_cast<const Trunk*>(t), i);
}
int capnet_trunk_conv_tile_n(const capnet_trunk_t* t, int i) { return trunk_conv_tile_n(reinterpret_cast<const Trunk*>(t), i); }
int capnet_pack_conv_weight_kmajor(const float* w_oihw, float* out, int Cout, int Cin, int KH,
                                   int KW, int k_rows, capnet_stream_t stream) {
  return pack_conv_weight_kmajor(w_oihw, out, Cout, Cin, KH, KW, k_rows, S(stream));
}
int capnet_conv2d_fwd_kmajor(const float* x, long sxb, long sxh, long sxw, const float* w_kmajor,
                             int k_rows, float* y, const float* in_scale, const float* in_shift,
                             int relu_in, float* part_sum, float* part_sq, int B, int H, int W,
                             int Cin, int Cout, int KH, int KW, int stride, int pad, int tile,
                             float* slabs, capnet_stream_t stream) {
  return conv2d_fwd_v2(x, sxb, sxh, sxw, w_kmajor, k_rows, y, in_scale, in_shift, relu_in, part_sum,
                       part_sq, B, H, W, Cin, Cout, KH, KW, stride, pad, tile, slabs, S(stream));
}
size_t capnet_conv_kmajor_slab_floats(int M, int Cout, int k_rows, int tile) {
  return conv_v2_slab_floats(M, Cout, k_rows, tile);
}
int capnet_pack_conv_weight(const float* w_oihw, float* out, int Cout, int Cin, int KH, int KW,
                            int row_stride, capnet_stream_t stream) {
  return pack_conv_weight(w_oihw, out, Cout, Cin, KH, KW, row_stride, S(stream));
}
int capnet_adaptive_pool_replicate(const float* x, float* out, int B, int side, int out_side,
                                   int C, capnet_stream_t stream) {
  return adaptive_pool_replicate(x, out, B, side, out_side, C, S(stream));
}

int capnet_conv2d_fwd(const float* x, long sxb, long sxh, long sxw, long sxc,
                      const float* w_packed, int row_stride, float* y, const float* in_scale,
                      const float* in_shift, int relu_in, float* part_sum, float* part_sq, int B,
                      int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                      int tile, capnet_stream_t stream) {
  return conv2d_fwd(x, sxb, sxh, sxw, sxc, w_packed, row_stride, y, in_scale, in_shift, relu_in,
                    part_sum, part_sq, B, H, W, Cin, Cout, KH, KW, stride, pad, tile, S(stream));
}
int capnet_conv_tiles_m(int M, int Cout, int tile) {
  if (tile == 0) tile = conv_auto_tile(M, Cout);
  return conv_tiles_m(M, tile);
}
void capnet_conv_kmajor_plan(int M, int Cout, int k_rows, int tile, int* out5) {
  conv_v2_plan(M, Cout, k_rows, tile, out5);
}
int capnet_conv_kmajor_tiles_m(int M, int Cout, int k_rows, int tile) {
  int plan[5];
  conv_v2_plan(M, Cout, k_rows, tile, plan);   // normalises the tile exactly as the launcher does
  return conv_tiles_m(M, plan[0]);
}
int capnet_bn_finalize(const float* part_sum, const float* part_sq, int tiles, int C, long count,
                       const float* gamma, const float* beta, float* running_mean,
                       float* running_var, float momentum, float eps, float* scale, float* shift,
                       capnet_stream_t stream) {
  return bn_finalize(part_sum, part_sq, tiles, C, count, gamma, beta, running_mean, running_var,
                     momentum, eps, scale, shift, S(stream));
}
int capnet_bn_add_relu(const float* y, const float* s1, const float* t1, const float* res,
                       const float* s2, const float* t2, float* out, long rows, int C,
                       capnet_stream_t stream) {
  return bn_add_relu(y, s1, t1, res, s2, t2, out, rows, C, S(stream));
}
int capnet_bn_relu_maxpool(const float* y, const float* scale, const float* shift, float* out,
                           int B, int H, int W, int C, capnet_stream_t stream) {
  return bn_relu_maxpool(y, scale, shift, out, B, H, W, C, S(stream));
}
int capnet_global_avgpool(const float* x, float* out, int B, int HW, int C,
                          capnet_stream_t stream) {
  return global_avgpool(x, out, B, HW, C, S(stream));
}

int capnet_bn1d_fwd(const float* x, int B, int C, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int train, float momentum, float eps,
                    float* y, float* save_mean, float* save_invstd, capnet_stream_t stream) {
  return bn1d_fwd(x, B, C, gamma, beta, running_mean, running_var, train, momentum, eps, y,
                  save_mean, save_invstd, S(stream));
}
int capnet_bn1d_bwd(const float* dy, const float* x, int B, int C, const float* gamma,
                    const float* save_mean, const float* save_invstd, float* dx, float* dgamma,
                    float* dbeta, capnet_stream_t stream) {
  return bn1d_bwd(dy, x, B, C, gamma, save_mean, save_invstd, dx, dgamma, dbeta, S(stream));
}

int capnet_embedding_fwd(const long long* idx, int n, const float* emb, int E, int V, float* out,
                         int* err_flag, capnet_stream_t stream) {
  return embedding_fwd(idx, n, emb, E, V, out, err_flag, S(stream));
}
int capnet_lstm_pointwise_fwd(float* pre, const float* c_prev, float* c_out, float* h_out, int b,
                              int H, int cell, capnet_stream_t stream) {
  CAPNET_REQUIRE(pre && c_out && h_out && b >= 0 && H > 0, "lstm_pointwise_fwd: bad argument");
  if (cell == kCellFactored)
    return lstm_pointwise_fwd(pre, 4L * H, c_prev, c_out, h_out, b, H, 0, 1, 2, 3, 0, S(stream));
  CAPNET_REQUIRE(cell == kCellLSTM, "lstm_pointwise_fwd: unknown cell %d", cell);
  return lstm_pointwise_fwd(pre, 4L * H, c_prev, c_out, h_out, b, H, 0, 1, 3, 2, 1, S(stream));
}

// what capnet_stacked_decode_step_gather and capnet_stacked_decode_step_groups check alike
static int stacked_step_check(int cell, int nlayers, int rows, int E, int H, int V, const long long* tokens, const float* x,
                              const float* const* wcat, const float* const* beff, const float* state_in,
                              const long long* parent_rows, const float* state_out, const float* h_top, const int* err_flag) {
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "stacked_decode_step: unknown cell %d", cell);
  CAPNET_REQUIRE(nlayers >= 1 && nlayers <= 8, "stacked_decode_step: layers %d (1..8)", nlayers);
  CAPNET_REQUIRE(rows >= 1, "stacked_decode_step: rows %d", rows);
  CAPNET_REQUIRE(stacked_decode_supported(E, H), "stacked_decode_step: unsupported E=%d H=%d", E, H);
  CAPNET_REQUIRE(x && wcat && beff && state_in && state_out && h_top, "stacked_decode_step: null argument");
  CAPNET_REQUIRE(!tokens || (err_flag && V >= 1), "stacked_decode_step: token ids need err_flag and V >= 1");
  CAPNET_REQUIRE(!parent_rows || err_flag, "stacked_decode_step: parent rows need err_flag");
  CAPNET_REQUIRE(state_in != state_out, "stacked_decode_step: state_in and state_out must differ");
  CAPNET_REQUIRE(aligned16(state_in) && aligned16(state_out), "stacked_decode_step: state alignment");
  for (int l = 0; l < nlayers; ++l) {
    CAPNET_REQUIRE(wcat[l] && beff[l], "stacked_decode_step: weights of layer %d are null", l);
    CAPNET_REQUIRE(aligned16(wcat[l]), "stacked_decode_step: weights of layer %d not 16-B aligned", l);
  }
  return kOk;
}

int capnet_stacked_decode_step_gather(int cell, int nlayers, int rows, int E, int H, int V, const long long* tokens,
                                      const float* x, const float* const* wcat, const float* const* beff,
                                      const float* state_in, const long long* parent_rows, float* state_out, float* h_top,
                                      int* err_flag, capnet_stream_t stream) {
  if (int rc = stacked_step_check(cell, nlayers, rows, E, H, V, tokens, x, wcat, beff, state_in, parent_rows, state_out, h_top,
                                  err_flag))
    return rc;
  return stacked_decode_step(cell, nlayers, rows, E, H, V, tokens, x, wcat, beff, state_in, state_out, h_top, err_flag,
                             S(stream), parent_rows);
}

// (a group's weights follow the group before it at 4H (kin + H) floats, a multiple of 16 bytes: layer l's alignment is group 0's)
int capnet_stacked_decode_step_groups(int cell, int nlayers, int groups, int rows_per_group, int E, int H, int V,
                                      const long long* tokens, const float* x, const float* const* wcat,
                                      const float* const* beff, const float* state_in, const long long* parent_rows,
                                      float* state_out, float* h_top, int* err_flag, capnet_stream_t stream) {
  CAPNET_REQUIRE(groups >= 1 && groups <= 8, "stacked_decode_step: groups %d (1..8)", groups);
  CAPNET_REQUIRE(rows_per_group >= 1 && rows_per_group < (1 << 24), "stacked_decode_step: rows per group %d", rows_per_group);
  if (int rc = stacked_step_check(cell, nlayers, groups * rows_per_group, E, H, V, tokens, x, wcat, beff, state_in, parent_rows,
                                  state_out, h_top, err_flag))
    return rc;
  return stacked_decode_step(cell, nlayers, groups * rows_per_group, E, H, V, tokens, x, wcat, beff, state_in, state_out, h_top,
                             err_flag, S(stream), parent_rows, groups);
}

int capnet_stacked_decode_step_tables(int cell, int nlayers, int groups, int rows_per_group, int E, int H, int V,
                                      const long long* tokens, const float* const* tables, const float* const* wcat,
                                      const float* const* beff, const float* state_in, const long long* parent_rows,
                                      float* state_out, float* h_top, int* err_flag, capnet_stream_t stream) {
  CAPNET_REQUIRE(groups >= 1 && groups <= 8, "stacked_decode_step: groups %d (1..8)", groups);
  CAPNET_REQUIRE(rows_per_group >= 1 && rows_per_group < (1 << 24), "stacked_decode_step: rows per group %d", rows_per_group);
  CAPNET_REQUIRE(tokens && tables, "stacked_decode_step: per-group tables need token ids");
  for (int g = 0; g < groups; ++g) CAPNET_REQUIRE(tables[g], "stacked_decode_step: table of group %d is null", g);
  if (int rc = stacked_step_check(cell, nlayers, groups * rows_per_group, E, H, V, tokens, tables[0], wcat, beff, state_in,
                                  parent_rows, state_out, h_top, err_flag))
    return rc;
  return stacked_decode_step(cell, nlayers, groups * rows_per_group, E, H, V, tokens, tables[0], wcat, beff, state_in, state_out,
                             h_top, err_flag, S(stream), parent_rows, groups, tables);
}

int capnet_stacked_decode_step_cell(int cell, int nlayers, int rows, int E, int H, int V, const long long* tokens,
                                    const float* x, const float* const* wcat, const float* const* beff,
                                    const float* state_in, float* state_out, float* h_top, int* err_flag,
                                    capnet_stream_t stream) {
  return capnet_stacked_decode_step_gather(cell, nlayers, rows, E, H, V, tokens, x, wcat, beff, state_in, nullptr, state_out,
                                           h_top, err_flag, stream);
}

int capnet_stacked_decode_step(int nlayers, int rows, int E, int H, int V, const long long* tokens, const float* x,
                               const float* const* wcat, const float* const* beff, const float* state_in,
                               float* state_out, float* h_top, int* err_flag, capnet_stream_t stream) {
  return capnet_stacked_decode_step_cell(kCellFactored, nlayers, rows, E, H, V, tokens, x, wcat, beff, state_in, state_out,
                                         h_top, err_flag, stream);
}
size_t capnet_vocab_argmax_ws_bytes(int rows, int V) { return rows >= 1 && V >= 1 ? vocab_argmax_ws_bytes(rows, V) : 0; }

int capnet_vocab_argmax(const float* h, const float* w, const float* b, int rows, int H, int V, void* workspace,
                        long long* tokens, capnet_stream_t stream) {
  CAPNET_REQUIRE(rows >= 1 && V >= 1, "vocab_argmax: rows %d, V %d", rows, V);
  CAPNET_REQUIRE(vocab_argmax_supported(H), "vocab_argmax: unsupported H=%d", H);
  CAPNET_REQUIRE(h && w && workspace && tokens, "vocab_argmax: null argument");
  CAPNET_REQUIRE(aligned16(h) && aligned16(w) && aligned16(workspace), "vocab_argmax: h, w and the workspace must be 16-B aligned");
  return vocab_argmax(h, w, b, rows, H, V, workspace, tokens, nullptr, 0, S(stream));
}

size_t capnet_vocab_argmax_groups_ws_bytes(int groups, int rows_per_group, int V) {
  return groups >= 1 && groups <= 8 && rows_per_group >= 1 && V >= 1 ? vocab_argmax_groups_ws_bytes(groups, rows_per_group, V) : 0;
}

int capnet_vocab_argmax_groups(const float* h, const float* const* w, const float* const* b, int groups, int rows_per_group,
                               int H, int V, void* workspace, long long* tokens, capnet_stream_t stream) {
  CAPNET_REQUIRE(groups >= 1 && groups <= 8, "vocab_argmax: groups %d (1..8)", groups);
  CAPNET_REQUIRE(rows_per_group >= 1 && rows_per_group < (1 << 24) && V >= 1, "vocab_argmax: rows per group %d, V %d",
                 rows_per_group, V);
  CAPNET_REQUIRE(vocab_argmax_supported(H), "vocab_argmax: unsupported H=%d", H);
  CAPNET_REQUIRE(h && w && workspace && tokens, "vocab_argmax: null argument");
  CAPNET_REQUIRE(aligned16(h) && aligned16(workspace), "vocab_argmax: h, w and the workspace must be 16-B aligned");
  for (int g = 0; g < groups; ++g)
    CAPNET_REQUIRE(w[g] && aligned16(w[g]), "vocab_argmax: projection of group %d is null or not 16-B aligned", g);
  return vocab_argmax_groups(h, w, b, groups, rows_per_group, H, V, workspace, tokens, nullptr, 0, S(stream));
}

size_t capnet_lstm_greedy_decode_ws_bytes(int nlayers, int rows, int H, int V) {
  return nlayers >= 1 && nlayers <= 8 && rows >= 1 && H >= 1 && V >= 1 ? lstm_greedy_decode_ws_bytes(nlayers, rows, H, V) : 0;
}

size_t capnet_lstm_greedy_decode_groups_ws_bytes(int nlayers, int groups, int rows_per_group, int H, int V) {
  return nlayers >= 1 && nlayers <= 8 && groups >= 1 && groups <= 8 && rows_per_group >= 1 && H >= 1 && V >= 1
             ? lstm_greedy_decode_groups_ws_bytes(nlayers, groups, rows_per_group, H, V) : 0;
}

// the per-layer weights of every one-call decode: wcat[l] and beff[l] given, wcat[l] 16-B aligned
static int layer_weights_check(const char* who, int nlayers, const float* const* wcat, const float* const* beff) {
  for (int l = 0; l < nlayers; ++l) {
    CAPNET_REQUIRE(wcat[l] && beff[l], "%s: weights of layer %d are null", who, l);
    CAPNET_REQUIRE(aligned16(wcat[l]), "%s: weights of layer %d not 16-B aligned", who, l);
  }
  return kOk;
}

// what the plain stacks' one-call beam searches check alike: `groups` weight groups of n sentences (images) each on `tables`
// embeddings and projections (1: one of each for every group; groups: one per group); fused_topk: no slab is needed
static int stack_decode_check(const char* who, int cell, int nlayers, int groups, int n, int k, int E, int H, int V, int max_steps,
                              long long start_token, int poll_every, int fused_topk, int tables, const float* const* emb,
                              const float* const* wcat, const float* const* beff, const float* const* Cw, const float* state0,
                              const void* workspace, const float* slab, size_t slab_floats, const long long* seqs,
                              const int* lengths, const int* err_flag) {
  CAPNET_REQUIRE(groups >= 1 && groups <= 8, "%s: groups %d (1..8)", who, groups);
  const long nq = n >= 1 && n < (1 << 24) ? (long)groups * n : 0;      // the beam groups
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "%s: unknown cell %d", who, cell);
  CAPNET_REQUIRE(nlayers >= 1 && nlayers <= 8, "%s: layers %d (1..8)", who, nlayers);
  CAPNET_REQUIRE(nq >= 1 && max_steps >= 1 && V >= 1 && poll_every >= 0, "%s: n %d, max_steps %d, V %d, poll_every %d", who, n,
                 max_steps, V, poll_every);
  CAPNET_REQUIRE(k >= 1 && k <= 16 && k <= V, "%s: k=%d (1 <= k <= 16, k <= V = %d)", who, k, V);
  CAPNET_REQUIRE(nq * k * (max_steps + 2) < (1L << 28) && nq * k * V < (1L << 31), "%s: n k too large", who);
  CAPNET_REQUIRE(stacked_decode_supported(E, H), "%s: unsupported E=%d H=%d", who, E, H);
  CAPNET_REQUIRE(!fused_topk || vocab_topk_supported(H, k, V), "%s: the fused top-k does not take H=%d", who, H);
  CAPNET_REQUIRE(start_token >= 0 && start_token <= 0x7fffffffLL, "%s: start_token %lld", who, start_token);
  CAPNET_REQUIRE(emb && wcat && beff && Cw && workspace && seqs && lengths && err_flag, "%s: null argument", who);
  CAPNET_REQUIRE(aligned16(workspace) && (!state0 || aligned16(state0)), "%s: workspace, Cw and state0 must be 16-B aligned", who);
  for (int g = 0; g < tables; ++g) {
    CAPNET_REQUIRE(emb[g] && Cw[g], "%s: null argument (embedding or projection of group %d)", who, g);
    CAPNET_REQUIRE(aligned16(Cw[g]), "%s: workspace, Cw and state0 must be 16-B aligned (Cw of group %d)", who, g);
  }
  CAPNET_REQUIRE((size_t)seqs % 8 == 0 && (size_t)lengths % 4 == 0, "%s: seqs / lengths alignment", who);
  if (!fused_topk) {
    CAPNET_REQUIRE(slab, "%s: null argument (without the fused top-k the slab is required)", who);
    CAPNET_REQUIRE(aligned16(slab), "%s: the slab must be 16-B aligned", who);
    CAPNET_REQUIRE(slab_floats >= (size_t)nq * k * V, "%s: the slab holds %zu floats, one [n k][V] block is %zu", who, slab_floats,
                   (size_t)nq * k * V);
  }
  return layer_weights_check(who, nlayers, wcat, beff);
}

// what the two greedy entries check alike (features only with one group)
static int greedy_check(int nlayers, int groups, int rpg, int E, int H, int V, int steps, const float* features,
                        const long long* start_tokens, const float* const* emb, const float* const* wcat,
                        const float* const* beff, const float* const* Cw, const float* const* Cb, const float* state0,
                        const void* workspace, const long long* ids, const float* state_out, const int* err_flag) {
  CAPNET_REQUIRE(nlayers >= 1 && nlayers <= 8, "lstm_greedy_decode: layers %d (1..8)", nlayers);
  CAPNET_REQUIRE(groups >= 1 && groups <= 8, "lstm_greedy_decode: groups %d (1..8)", groups);
  CAPNET_REQUIRE(rpg >= 1 && rpg < (1 << 24) && steps >= 1 && V >= 1, "lstm_greedy_decode: rows %d, steps %d, V %d", rpg, steps, V);
  CAPNET_REQUIRE(stacked_decode_supported(E, H) && vocab_argmax_supported(H), "lstm_greedy_decode: unsupported E=%d H=%d", E, H);
  CAPNET_REQUIRE((features != nullptr) != (start_tokens != nullptr),
                 "lstm_greedy_decode: the first input is either features or start_tokens");
  CAPNET_REQUIRE(emb && wcat && beff && Cw && Cb && workspace && ids && state_out && err_flag, "lstm_greedy_decode: null argument");
  CAPNET_REQUIRE(aligned16(workspace) && (!state0 || aligned16(state0)) && aligned16(state_out),
                 "lstm_greedy_decode: workspace, Cw and the states must be 16-B aligned");
  for (int g = 0; g < groups; ++g) {
    CAPNET_REQUIRE(emb[g] && Cw[g], "lstm_greedy_decode: null argument (embedding or projection of group %d)", g);
    CAPNET_REQUIRE(aligned16(Cw[g]), "lstm_greedy_decode: workspace, Cw and the states must be 16-B aligned (group %d)", g);
  }
  return layer_weights_check("lstm_greedy_decode", nlayers, wcat, beff);
}

int capnet_lstm_greedy_decode_groups(int nlayers, int groups, int rows_per_group, int E, int H, int V, int steps,
                                     const long long* start_tokens, const float* const* emb, const float* const* wcat,
                                     const float* const* beff, const float* const* Cw, const float* const* Cb,
                                     const float* state0, void* workspace, long long* ids, float* state_out, int* err_flag,
                                     capnet_stream_t stream) {
  const float* no_bias[8] = {};
  CAPNET_REQUIRE(groups >= 1 && groups <= 8, "lstm_greedy_decode: groups %d (1..8)", groups);
  for (int g = 0; Cb && g < groups; ++g) CAPNET_REQUIRE(Cb[g], "lstm_greedy_decode: null argument (bias of group %d)", g);
  if (!Cb) Cb = no_bias;
  if (int rc = greedy_check(nlayers, groups, rows_per_group, E, H, V, steps, nullptr, start_tokens, emb, wcat, beff, Cw, Cb,
                            state0, workspace, ids, state_out, err_flag))
    return rc;
  return lstm_greedy_decode_groups(nlayers, groups, rows_per_group, E, H, V, steps, nullptr, start_tokens, emb, wcat, beff, Cw,
                                   Cb, state0, workspace, ids, state_out, err_flag, S(stream));
}

int capnet_lstm_greedy_decode(int nlayers, int rows, int E, int H, int V, int steps, const float* features,
                              const long long* start_tokens, const float* emb, const float* const* wcat,
                              const float* const* beff, const float* Cw, const float* Cb, const float* state0,
                              void* workspace, long long* ids, float* state_out, int* err_flag, capnet_stream_t stream) {
  if (int rc = greedy_check(nlayers, 1, rows, E, H, V, steps, features, start_tokens, &emb, wcat, beff, &Cw, &Cb, state0,
                            workspace, ids, state_out, err_flag))
    return rc;
  return lstm_greedy_decode_groups(nlayers, 1, rows, E, H, V, steps, features, start_tokens, &emb, wcat, beff, &Cw, &Cb, state0,
                                   workspace, ids, state_out, err_flag, S(stream));
}

size_t capnet_beam_decode_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps) {
  return beam_decode_ws_bytes(nlayers, n, k, H, V, max_steps);
}

// the teams of a diverse one-call search (capnet_beam_decode_diverse, capnet_att_beam_decode_diverse): beam_teams_check, and
// the state of n teams searches of k / teams beams must exist
static int decode_teams_check(const char* who, int n, int k, const BeamTeams& t, int max_steps) {
  if (int rc = beam_teams_check(who, k, t.teams, t.strength)) return rc;
  CAPNET_REQUIRE(n >= 1 && (long)n * t.teams < (1L << 24) && beam_state_bytes(n * t.teams, k / t.teams, max_steps), "%s: n=%d teams=%d",
                 who, n, t.teams);
  return kOk;
}

// every capnet_beam_decode* entry: stack_decode_check, then the checks of what is given. n: the images of one group
static int beam_decode_entry(const char* who, int cell, int nlayers, int groups, int n, int k, int E, int H, int V, int max_steps,
                             long long start_token, long long end_token, const float* emb, const float* const* wcat,
                             const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* workspace,
                             float* slab, size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run,
                             int* err_flag, capnet_stream_t stream, const BeamConstraints* con = nullptr,
                             const BeamTeams* teams = nullptr) {
  if (int rc = stack_decode_check(who, cell, nlayers, groups, n, k, E, H, V, max_steps, start_token, poll_every, 0, 1, &emb, wcat, beff,
                                  &Cw, state0, workspace, slab, slab_floats, seqs, lengths, err_flag))
    return rc;
  if (teams)
    if (int rc = decode_teams_check(who, groups * n, k, *teams, max_steps)) return rc;
  if (con)
    if (int rc = beam_constraints_check(who, *con)) return rc;
  if (con && con->n_forced)
    if (int rc = beam_forced_check(who, *con)) return rc;
  return beam_decode(cell, nlayers, n, k, E, H, V, max_steps, start_token, end_token, emb, wcat, beff, Cw, Cb, state0, workspace,
                     slab, slab_floats, poll_every, seqs, lengths, steps_run, err_flag, S(stream), groups, con, teams);
}

int capnet_beam_decode(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                       long long end_token, const float* emb, const float* const* wcat, const float* const* beff,
                       const float* Cw, const float* Cb, const float* state0, void* workspace, float* slab,
                       size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                       capnet_stream_t stream) {
  return beam_decode_entry("beam_decode", cell, nlayers, 1, n, k, E, H, V, max_steps, start_token, end_token, emb, wcat, beff, Cw, Cb,
                           state0, workspace, slab, slab_floats, poll_every, seqs, lengths, steps_run, err_flag, stream);
}

int capnet_beam_decode_groups(int cell, int nlayers, int groups, int n_images, int k, int E, int H, int V, int max_steps,
                              long long start_token, long long end_token, const float* emb, const float* const* wcat,
                              const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* workspace,
                              float* slab, size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run,
                              int* err_flag, capnet_stream_t stream) {
  return beam_decode_entry("beam_decode", cell, nlayers, groups, n_images, k, E, H, V, max_steps, start_token, end_token, emb, wcat,
                           beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths, steps_run, err_flag, stream);
}

int capnet_beam_decode_constrained(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                                   long long end_token, const float* emb, const float* const* wcat, const float* const* beff,
                                   const float* Cw, const float* Cb, const float* state0, void* workspace, float* slab,
                                   size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run,
                                   int* err_flag, capnet_stream_t stream, int no_repeat_ngram, int min_words, const int* banned,
                                   int n_banned) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned};
  return beam_decode_entry("beam_decode_constrained", cell, nlayers, 1, n, k, E, H, V, max_steps, start_token, end_token, emb, wcat,
                           beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths, steps_run, err_flag, stream,
                           &con);
}

int capnet_beam_decode_forced(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                              long long end_token, const float* emb, const float* const* wcat, const float* const* beff,
                              const float* Cw, const float* Cb, const float* state0, void* workspace, float* slab,
                              size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                              capnet_stream_t stream, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                              const int* forced, int n_forced) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned, forced, n_forced};
  if (int rc = beam_forced_check("beam_decode_forced", con)) return rc;   // (n_forced == 0 would be the constrained search)
  return beam_decode_entry("beam_decode_forced", cell, nlayers, 1, n, k, E, H, V, max_steps, start_token, end_token, emb, wcat, beff,
                           Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths, steps_run, err_flag, stream, &con);
}

int capnet_beam_decode_rules(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                             long long end_token, const float* emb, const float* const* wcat, const float* const* beff,
                             const float* Cw, const float* Cb, const float* state0, void* workspace, float* slab,
                             size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                             capnet_stream_t stream, const int* rules) {
  if (int rc = beam_rules_check("beam_decode_rules", rules)) return rc;   // (NULL would be the plain search)
  BeamConstraints con{0, 0, nullptr, 0};
  con.rules = rules;
  return beam_decode_entry("beam_decode_rules", cell, nlayers, 1, n, k, E, H, V, max_steps, start_token, end_token, emb, wcat, beff,
                           Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths, steps_run, err_flag, stream, &con);
}

int capnet_beam_decode_diverse(int cell, int nlayers, int n, int k, int teams, float strength, int E, int H, int V, int max_steps,
                               long long start_token, long long end_token, const float* emb, const float* const* wcat,
                               const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* workspace,
                               float* slab, size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run,
                               int* err_flag, capnet_stream_t stream, int no_repeat_ngram, int min_words, const int* banned,
                               int n_banned) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned};
  const BeamTeams dv{teams, strength, nullptr};
  return beam_decode_entry("beam_decode_diverse", cell, nlayers, 1, n, k, E, H, V, max_steps, start_token, end_token, emb, wcat, beff,
                           Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths, steps_run, err_flag, stream, &con,
                           &dv);
}

size_t capnet_vocab_topk_ws_bytes(int rows, int k, int V) { return vocab_topk_ws_bytes(rows, k, V); }

static int vocab_topk_tail(const float* h, const float* w, const float* b, int rows, int H, int V, int k, void* workspace,
                           float* values, int* index, float* lse, capnet_stream_t stream, const unsigned* mask,
                           bool select_only = false) {
  CAPNET_REQUIRE(rows >= 1 && rows < (1 << 24) && V >= 1, "vocab_topk: rows %d, V %d", rows, V);
  CAPNET_REQUIRE(k >= 1 && k <= 16 && k <= V, "vocab_topk: k=%d (1 <= k <= 16, k <= V = %d)", k, V);
  CAPNET_REQUIRE(vocab_topk_supported(H, k, V), "vocab_topk: unsupported H=%d", H);
  CAPNET_REQUIRE(h && w && workspace && values && index && lse, "vocab_topk: null argument");
  CAPNET_REQUIRE(aligned16(h) && aligned16(w) && aligned16(workspace), "vocab_topk: h, w and the workspace must be 16-B aligned");
  CAPNET_REQUIRE((size_t)values % 4 == 0 && (size_t)index % 4 == 0 && (size_t)lse % 4 == 0, "vocab_topk: output alignment");
  return vocab_topk(h, w, b, rows, H, V, k, workspace, values, index, lse, S(stream), mask, select_only);
}
int capnet_vocab_topk(const float* h, const float* w, const float* b, int rows, int H, int V, int k, void* workspace,
                      float* values, int* index, float* lse, capnet_stream_t stream) {
  return vocab_topk_tail(h, w, b, rows, H, V, k, workspace, values, index, lse, stream, nullptr);
}

// ---- sampled decoding (vocab_sample.hip) ----
float capnet_sample_uniform(unsigned long long seed, unsigned step, unsigned row, unsigned v) {
  return sample_uniform_host(seed, step, row, v);
}

// what every sampling entry checks alike; sets inv_T
static int sample_check(const char* who, int rows, int V, float temperature, unsigned step, unsigned row0, float* inv_T) {
  CAPNET_REQUIRE(rows >= 1 && rows < (1 << 24) && V >= 1 && V <= (1 << 24), "%s: rows %d, V %d (rows < 2^24, V <= 2^24)", who, rows, V);
  CAPNET_REQUIRE(temperature > 0.f && temperature <= 3.0e38f, "%s: temperature %g (finite, > 0)", who, (double)temperature);
  CAPNET_REQUIRE(step <= 65535u && (unsigned long long)row0 + (unsigned)rows <= (1u << 24),
                 "%s: step %u (<= 65535), row0 %u + rows %d (<= 2^24)", who, step, row0, rows);
  *inv_T = 1.0f / temperature;
  return kOk;
}

// greedy_stride of the capnet_*_greedy entries (sample_key.h's vs_row_key): 0 = off; the loops: the rows come in whole groups
// (rows % stride == 0; the attention loops: the stride IS the rows per image)
static int greedy_stride_check(const char* who, int rows, unsigned greedy_stride, int per_image) {
  CAPNET_REQUIRE(greedy_stride < (1u << 24), "%s: greedy_stride %u (< 2^24)", who, greedy_stride);
  CAPNET_REQUIRE(!greedy_stride || !rows || rows % (int)greedy_stride == 0, "%s: %d rows in groups of greedy_stride %u", who, rows,
                 greedy_stride);
  CAPNET_REQUIRE(!greedy_stride || !per_image || per_image == (int)greedy_stride, "%s: greedy_stride %u with %d rows per image", who,
                 greedy_stride, per_image);
  return kOk;
}

size_t capnet_vocab_sample_ws_bytes(int rows, int V) { return rows >= 1 && V >= 1 ? vocab_sample_ws_bytes(rows, V) : 0; }

static int vocab_sample_tail(const float* h, const float* w, const float* b, int rows, int H, int V, float temperature,
                             unsigned long long seed, unsigned step, unsigned row0, void* workspace, long long* tokens,
                             float* logp, capnet_stream_t stream, unsigned greedy_stride, const unsigned* mask = nullptr) {
  if (int rc = greedy_stride_check("vocab_sample", 0, greedy_stride, 0)) return rc;
  float inv_T = 0.f;
  if (int rc = sample_check("vocab_sample", rows, V, temperature, step, row0, &inv_T)) return rc;
  CAPNET_REQUIRE(vocab_sample_supported(H), "vocab_sample: unsupported H=%d", H);
  CAPNET_REQUIRE(h && w && workspace && tokens && logp, "vocab_sample: null argument");
  CAPNET_REQUIRE(aligned16(h) && aligned16(w) && aligned16(workspace), "vocab_sample: h, w and the workspace must be 16-B aligned");
  CAPNET_REQUIRE((size_t)tokens % 8 == 0 && (size_t)logp % 4 == 0, "vocab_sample: output alignment");
  return vocab_sample(h, w, b, rows, H, V, inv_T, seed, step, row0, workspace, tokens, nullptr, logp, 1, S(stream), greedy_stride, mask);
}
int capnet_vocab_sample(const float* h, const float* w, const float* b, int rows, int H, int V, float temperature,
                        unsigned long long seed, unsigned step, unsigned row0, void* workspace, long long* tokens,
                        float* logp, capnet_stream_t stream) {
  return vocab_sample_tail(h, w, b, rows, H, V, temperature, seed, step, row0, workspace, tokens, logp, stream, 0);
}
int capnet_vocab_sample_greedy(const float* h, const float* w, const float* b, int rows, int H, int V, float temperature,
                               unsigned long long seed, unsigned step, unsigned row0, void* workspace, long long* tokens,
                               float* logp, unsigned greedy_stride, capnet_stream_t stream) {
  return vocab_sample_tail(h, w, b, rows, H, V, temperature, seed, step, row0, workspace, tokens, logp, stream,
                           greedy_stride);
}

// nucleus (top-p) sampling (vocab_nucleus.hip): top_p == 1 is "off" -- the stand-alone draws then ARE the plain ones and
// report under their names, the _nucleus loops leave it to the plain loops (allow_one false)
static int top_p_check(const char* who, float top_p, bool allow_one) {
  CAPNET_REQUIRE(top_p > 0.f && (top_p < 1.f || (allow_one && top_p == 1.f)), "%s: top_p %g (0 < top_p %s 1)", who, (double)top_p,
                 allow_one ? "<=" : "<");
  return kOk;
}

// capnet_sample_pick* (who "sample_pick", top_p 1) and capnet_nucleus_pick* (who "nucleus_pick")
static int pick_tail(const char* who, const float* values, const int* index, int rows, int k, int V, float temperature, float top_p,
                     unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp, capnet_stream_t stream,
                     unsigned greedy_stride) {
  if (int rc = greedy_stride_check(who, 0, greedy_stride, 0)) return rc;
  if (int rc = top_p_check(who, top_p, true)) return rc;
  if (top_p == 1.f) who = "sample_pick";
  float inv_T = 0.f;
  if (int rc = sample_check(who, rows, V, temperature, step, row0, &inv_T)) return rc;
  CAPNET_REQUIRE(k >= 1 && k <= 16, "%s: k=%d (1 <= k <= 16)", who, k);
  CAPNET_REQUIRE(values && index && tokens && logp, "%s: null argument", who);
  CAPNET_REQUIRE((size_t)values % 4 == 0 && (size_t)index % 4 == 0 && (size_t)tokens % 8 == 0 && (size_t)logp % 4 == 0,
                 "%s: alignment", who);
  if (top_p == 1.f) return sample_pick(values, index, rows, k, V, inv_T, seed, step, row0, tokens, nullptr, logp, 1, S(stream), greedy_stride);
  return nucleus_pick(values, index, rows, k, V, inv_T, top_p, seed, step, row0, tokens, nullptr, logp, 1, S(stream), greedy_stride);
}
int capnet_sample_pick(const float* values, const int* index, int rows, int k, int V, float temperature,
                       unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp,
                       capnet_stream_t stream) {
  return pick_tail("sample_pick", values, index, rows, k, V, temperature, 1.f, seed, step, row0, tokens, logp, stream, 0);
}
int capnet_sample_pick_greedy(const float* values, const int* index, int rows, int k, int V, float temperature,
                              unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp,
                              unsigned greedy_stride, capnet_stream_t stream) {
  return pick_tail("sample_pick", values, index, rows, k, V, temperature, 1.f, seed, step, row0, tokens, logp, stream, greedy_stride);
}
int capnet_nucleus_pick(const float* values, const int* index, int rows, int k, int V, float temperature, float top_p,
                        unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp,
                        capnet_stream_t stream) {
  return pick_tail("nucleus_pick", values, index, rows, k, V, temperature, top_p, seed, step, row0, tokens, logp, stream, 0);
}
int capnet_nucleus_pick_greedy(const float* values, const int* index, int rows, int k, int V, float temperature, float top_p,
                               unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp,
                               unsigned greedy_stride, capnet_stream_t stream) {
  return pick_tail("nucleus_pick", values, index, rows, k, V, temperature, top_p, seed, step, row0, tokens, logp, stream, greedy_stride);
}

// capnet_sample_rows* (who "sample_rows", top_p 1) and capnet_nucleus_rows* (who "nucleus_rows")
static int rows_tail(const char* who, const float* logits, int rows, long ld, int V, float temperature, float top_p,
                     unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp, capnet_stream_t stream,
                     unsigned greedy_stride) {
  if (int rc = greedy_stride_check(who, 0, greedy_stride, 0)) return rc;
  if (int rc = top_p_check(who, top_p, true)) return rc;
  if (top_p == 1.f) who = "sample_rows";
  float inv_T = 0.f;
  if (int rc = sample_check(who, rows, V, temperature, step, row0, &inv_T)) return rc;
  CAPNET_REQUIRE(ld >= V, "%s: ld %ld < V %d", who, ld, V);
  CAPNET_REQUIRE(logits && tokens && logp, "%s: null argument", who);
  CAPNET_REQUIRE((size_t)logits % 4 == 0 && (size_t)tokens % 8 == 0 && (size_t)logp % 4 == 0, "%s: alignment", who);
  if (top_p == 1.f) return sample_rows(logits, rows, ld, V, inv_T, seed, step, row0, tokens, nullptr, logp, 1, S(stream), greedy_stride);
  return nucleus_rows(logits, rows, ld, V, inv_T, top_p, seed, step, row0, tokens, nullptr, logp, 1, S(stream), greedy_stride);
}
int capnet_sample_rows(const float* logits, int rows, long ld, int V, float temperature, unsigned long long seed,
                       unsigned step, unsigned row0, long long* tokens, float* logp, capnet_stream_t stream) {
  return rows_tail("sample_rows", logits, rows, ld, V, temperature, 1.f, seed, step, row0, tokens, logp, stream, 0);
}
int capnet_sample_rows_greedy(const float* logits, int rows, long ld, int V, float temperature, unsigned long long seed,
                              unsigned step, unsigned row0, long long* tokens, float* logp, unsigned greedy_stride,
                              capnet_stream_t stream) {
  return rows_tail("sample_rows", logits, rows, ld, V, temperature, 1.f, seed, step, row0, tokens, logp, stream, greedy_stride);
}
int capnet_nucleus_rows(const float* logits, int rows, long ld, int V, float temperature, float top_p,
                        unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp,
                        capnet_stream_t stream) {
  return rows_tail("nucleus_rows", logits, rows, ld, V, temperature, top_p, seed, step, row0, tokens, logp, stream, 0);
}
int capnet_nucleus_rows_greedy(const float* logits, int rows, long ld, int V, float temperature, float top_p,
                               unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp,
                               unsigned greedy_stride, capnet_stream_t stream) {
  return rows_tail("nucleus_rows", logits, rows, ld, V, temperature, top_p, seed, step, row0, tokens, logp, stream, greedy_stride);
}

// ---- the sampled decode of a plain stack in one call (decode_loops.hip) ----
size_t capnet_sample_decode_ws_bytes(int nlayers, int rows, int H, int V, int top_k) {
  if (nlayers < 1 || nlayers > 8 || rows < 1 || rows >= (1 << 24) || H < 1 || V < 1 || top_k < 0 || top_k > 16 || top_k > V) return 0;
  return sample_decode_ws_bytes(nlayers, rows, H, V, top_k, false, false);
}
size_t capnet_sample_decode_nucleus_ws_bytes(int nlayers, int rows, int H, int V, int top_k) {
  if (!capnet_sample_decode_ws_bytes(nlayers, rows, H, V, top_k)) return 0;
  return sample_decode_ws_bytes(nlayers, rows, H, V, top_k, true, false);
}
size_t capnet_sample_decode_excl_ws_bytes(int nlayers, int rows, int H, int V, int top_k, float top_p) {
  if (!capnet_sample_decode_ws_bytes(nlayers, rows, H, V, top_k) || !(top_p > 0.f && top_p <= 1.f)) return 0;
  return sample_decode_ws_bytes(nlayers, rows, H, V, top_k, top_p < 1.f, true);
}

// every capnet_sample_decode* entry. top_p_one: whether the entry admits top_p == 1 (the plain entries pass 1, the _nucleus
// entries leave it to them, the _excl entry takes both draws); ex: the _excl entry's exclusions, which need the start tokens
static int sample_decode_entry(const char* who, int cell, int nlayers, int rows, int E, int H, int V, int steps,
                               const float* first_inputs, const long long* start_tokens, const float* emb,
                               const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                               const float* state0, float temperature, int top_k, float top_p, bool top_p_one,
                               unsigned long long seed, void* workspace, float* slab, size_t slab_floats, long long* ids,
                               float* logp, float* state_out, int* err_flag, capnet_stream_t stream, unsigned greedy_stride,
                               const SampleExcl* ex = nullptr) {
  if (int rc = greedy_stride_check(who, rows, greedy_stride, 0)) return rc;
  float inv_T = 0.f;
  if (int rc = top_p_check(who, top_p, top_p_one)) return rc;
  if (ex) {
    if (int rc = sample_excl_check(who, *ex)) return rc;
    CAPNET_REQUIRE(start_tokens, "%s: start_tokens is required (the hypotheses begin with them)", who);
  }
  CAPNET_REQUIRE(steps >= 1 && steps <= 65535, "%s: steps %d (1..65535)", who, steps);
  if (int rc = sample_check(who, rows, V, temperature, 0, 0, &inv_T)) return rc;
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "%s: unknown cell %d", who, cell);
  CAPNET_REQUIRE(nlayers >= 1 && nlayers <= 8, "%s: layers %d (1..8)", who, nlayers);
  CAPNET_REQUIRE(top_k >= 0 && top_k <= 16 && top_k <= V, "%s: top_k=%d (0 = off, 1 .. 16, <= V = %d)", who, top_k, V);
  CAPNET_REQUIRE(stacked_decode_supported(E, H) && vocab_sample_supported(H), "%s: unsupported E=%d H=%d", who, E, H);
  CAPNET_REQUIRE((first_inputs != nullptr) != (start_tokens != nullptr), "%s: the first input is either first_inputs or start_tokens",
                 who);
  CAPNET_REQUIRE(emb && wcat && beff && Cw && workspace && ids && logp && err_flag, "%s: null argument", who);
  CAPNET_REQUIRE(top_k > 0 || top_p == 1.f || (slab && aligned16(slab) && slab_floats > 0),
                 "%s: the split-K slab (16-B aligned) is required", who);
  CAPNET_REQUIRE(aligned16(workspace) && aligned16(Cw) && (!state0 || aligned16(state0)) && (!state_out || aligned16(state_out)),
                 "%s: workspace, Cw and the states must be 16-B aligned", who);
  CAPNET_REQUIRE((size_t)ids % 8 == 0 && (size_t)logp % 4 == 0, "%s: ids / logp alignment", who);
  if (int rc = layer_weights_check(who, nlayers, wcat, beff)) return rc;
  return sample_decode(cell, nlayers, rows, E, H, V, steps, first_inputs, start_tokens, emb, wcat, beff, Cw, Cb, state0,
                       SampleOpts{inv_T, top_k, top_p, seed, greedy_stride, ex}, workspace, slab, slab_floats, ids, logp, state_out,
                       err_flag, S(stream));
}
int capnet_sample_decode(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                         const long long* start_tokens, const float* emb, const float* const* wcat, const float* const* beff,
                         const float* Cw, const float* Cb, const float* state0, float temperature, int top_k,
                         unsigned long long seed, void* workspace, long long* ids, float* logp, float* state_out,
                         int* err_flag, capnet_stream_t stream) {
  return sample_decode_entry("sample_decode", cell, nlayers, rows, E, H, V, steps, first_inputs, start_tokens, emb, wcat, beff, Cw, Cb,
                             state0, temperature, top_k, 1.f, true, seed, workspace, nullptr, 0, ids, logp, state_out, err_flag, stream,
                             0);
}
int capnet_sample_decode_greedy(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                                const long long* start_tokens, const float* emb, const float* const* wcat,
                                const float* const* beff, const float* Cw, const float* Cb, const float* state0,
                                float temperature, int top_k, unsigned long long seed, void* workspace, long long* ids,
                                float* logp, float* state_out, int* err_flag, unsigned greedy_stride,
                                capnet_stream_t stream) {
  return sample_decode_entry("sample_decode", cell, nlayers, rows, E, H, V, steps, first_inputs, start_tokens, emb, wcat, beff, Cw, Cb,
                             state0, temperature, top_k, 1.f, true, seed, workspace, nullptr, 0, ids, logp, state_out, err_flag, stream,
                             greedy_stride);
}
int capnet_sample_decode_nucleus(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                                 const long long* start_tokens, const float* emb, const float* const* wcat,
                                 const float* const* beff, const float* Cw, const float* Cb, const float* state0,
                                 float temperature, int top_k, float top_p, unsigned long long seed, void* workspace,
                                 float* slab, size_t slab_floats, long long* ids, float* logp, float* state_out,
                                 int* err_flag, capnet_stream_t stream) {
  return sample_decode_entry("sample_decode_nucleus", cell, nlayers, rows, E, H, V, steps, first_inputs, start_tokens, emb, wcat, beff,
                             Cw, Cb, state0, temperature, top_k, top_p, false, seed, workspace, slab, slab_floats, ids, logp,
                             state_out, err_flag, stream, 0);
}
int capnet_sample_decode_nucleus_greedy(int cell, int nlayers, int rows, int E, int H, int V, int steps,
                                        const float* first_inputs, const long long* start_tokens, const float* emb,
                                        const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                        const float* state0, float temperature, int top_k, float top_p,
                                        unsigned long long seed, void* workspace, float* slab, size_t slab_floats,
                                        long long* ids, float* logp, float* state_out, int* err_flag, unsigned greedy_stride,
                                        capnet_stream_t stream) {
  return sample_decode_entry("sample_decode_nucleus", cell, nlayers, rows, E, H, V, steps, first_inputs, start_tokens, emb, wcat, beff,
                             Cw, Cb, state0, temperature, top_k, top_p, false, seed, workspace, slab, slab_floats, ids, logp,
                             state_out, err_flag, stream, greedy_stride);
}
int capnet_sample_decode_excl(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                              const long long* start_tokens, const float* emb, const float* const* wcat,
                              const float* const* beff, const float* Cw, const float* Cb, const float* state0, float temperature,
                              int top_k, float top_p, unsigned long long seed, void* workspace, float* slab, size_t slab_floats,
                              long long* ids, float* logp, float* state_out, int* err_flag, unsigned greedy_stride,
                              long long end_token, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                              capnet_stream_t stream) {
  const SampleExcl ex{end_token, no_repeat_ngram, min_words, banned, n_banned, nullptr};
  return sample_decode_entry("sample_decode_excl", cell, nlayers, rows, E, H, V, steps, first_inputs, start_tokens, emb, wcat, beff, Cw,
                             Cb, state0, temperature, top_k, top_p, true, seed, workspace, slab, slab_floats, ids, logp, state_out,
                             err_flag, stream, greedy_stride, &ex);
}

// ---- the exclusions' own entries (sample_exclude.hip) ----
int capnet_sample_exclusion_mask(const long long* ids, long ld, int steps, const long long* start_tokens, int rows, int t, int V,
                                 long long end_token, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                                 unsigned* mask, capnet_stream_t stream) {
  const char* who = "sample_exclusion_mask";
  const SampleExcl c{end_token, no_repeat_ngram, min_words, banned, n_banned, mask};
  if (int rc = sample_excl_check(who, c)) return rc;
  CAPNET_REQUIRE(rows >= 1 && rows < (1 << 24) && V >= 1 && V <= (1 << 24), "%s: rows %d, V %d (rows < 2^24, V <= 2^24)", who, rows, V);
  CAPNET_REQUIRE(steps >= 1 && steps <= 65535 && ld >= steps, "%s: steps %d (1..65535), ld %ld (>= steps)", who, steps, ld);
  CAPNET_REQUIRE(t >= 0 && t <= steps, "%s: t=%d lies beyond steps %d", who, t, steps);
  CAPNET_REQUIRE(mask && (size_t)mask % 4 == 0, "%s: mask is null or not 4-byte aligned", who);
  CAPNET_REQUIRE((ids || !t) && (size_t)ids % 8 == 0 && (size_t)start_tokens % 8 == 0,
                 "%s: ids is null (required from t = 1) or ids / start_tokens not 8-byte aligned", who);
  return sample_exclusion_mask(ids, ld, start_tokens, rows, t, V, c, mask, S(stream));
}

int capnet_mask_logits(float* logits, int rows, long ld, int V, const unsigned* mask, capnet_stream_t stream) {
  CAPNET_REQUIRE(rows >= 1 && rows < (1 << 24) && V >= 1 && V <= (1 << 24) && ld >= V, "mask_logits: rows %d, V %d, ld %ld (>= V)", rows,
                 V, ld);
  CAPNET_REQUIRE(logits && (size_t)logits % 4 == 0, "mask_logits: logits is null or not 4-byte aligned");
  CAPNET_REQUIRE(mask && (size_t)mask % 4 == 0, "mask_logits: mask is null or not 4-byte aligned");
  return mask_logits(logits, rows, ld, V, mask, S(stream));
}

int capnet_vocab_sample_masked(const float* h, const float* w, const float* b, int rows, int H, int V, float temperature,
                               unsigned long long seed, unsigned step, unsigned row0, const unsigned* mask, void* workspace,
                               long long* tokens, float* logp, unsigned greedy_stride, capnet_stream_t stream) {
  CAPNET_REQUIRE(mask && (size_t)mask % 4 == 0, "vocab_sample_masked: mask is null or not 4-byte aligned");
  return vocab_sample_tail(h, w, b, rows, H, V, temperature, seed, step, row0, workspace, tokens, logp, stream, greedy_stride, mask);
}

int capnet_vocab_topk_masked(const float* h, const float* w, const float* b, int rows, int H, int V, int k, const unsigned* mask,
                             void* workspace, float* values, int* index, float* lse, capnet_stream_t stream) {
  CAPNET_REQUIRE(mask && (size_t)mask % 4 == 0, "vocab_topk_masked: mask is null or not 4-byte aligned");
  return vocab_topk_tail(h, w, b, rows, H, V, k, workspace, values, index, lse, stream, mask);
}

// ---- the fused beam step under constraints: the mask of a device beam's rows, and vocab_topk's select-only instance ----
int capnet_beam_exclusion_mask(const void* beam, int n, int k, int max_steps, int step, int V, long long end_token,
                               int no_repeat_ngram, int min_words, const int* banned, int n_banned, unsigned* mask,
                               capnet_stream_t stream) {
  const char* who = "beam_exclusion_mask";
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned};
  if (int rc = beam_constraints_check(who, con)) return rc;
  CAPNET_REQUIRE(beam && (size_t)beam % 4 == 0, "%s: the beam state is null or not 4-byte aligned", who);
  CAPNET_REQUIRE(n >= 1 && k >= 1 && k <= 16 && max_steps >= 1 && (long)n * k < (1L << 24) &&
                     (long)n * k * (max_steps + 2) < (1L << 28),
                 "%s: n=%d k=%d max_steps=%d (n, max_steps >= 1; 1 <= k <= 16; n k < 2^24)", who, n, k, max_steps);
  CAPNET_REQUIRE(V >= 1 && V <= (1 << 24), "%s: V %d (1 .. 2^24)", who, V);
  CAPNET_REQUIRE(step >= 1 && step <= max_steps, "%s: step=%d (1 <= step <= max_steps = %d)", who, step, max_steps);
  CAPNET_REQUIRE(mask && (size_t)mask % 4 == 0, "%s: mask is null or not 4-byte aligned", who);
  return beam_exclusion_mask(beam, n, k, max_steps, step, V, end_token, con, mask, S(stream));
}

int capnet_vocab_topk_select(const float* h, const float* w, const float* b, int rows, int H, int V, int k, const unsigned* mask,
                             void* workspace, float* values, int* index, float* lse, capnet_stream_t stream) {
  CAPNET_REQUIRE(mask && (size_t)mask % 4 == 0, "vocab_topk_select: mask is null or not 4-byte aligned");
  return vocab_topk_tail(h, w, b, rows, H, V, k, workspace, values, index, lse, stream, mask, true);
}

size_t capnet_vocab_topk_groups_ws_bytes(int groups, int rows_per_group, int k, int V) {
  return vocab_topk_groups_ws_bytes(groups, rows_per_group, k, V);
}

static int vocab_topk_groups_tail(const float* h, const float* const* w, const float* const* b, int groups, int rows_per_group,
                                  int H, int V, int k, void* workspace, float* values, int* index, float* lse,
                                  capnet_stream_t stream, const unsigned* mask, bool select_only) {
  CAPNET_REQUIRE(groups >= 1 && groups <= 8, "vocab_topk: groups %d (1..8)", groups);
  CAPNET_REQUIRE(rows_per_group >= 1 && rows_per_group < (1 << 24) && V >= 1, "vocab_topk: rows per group %d, V %d",
                 rows_per_group, V);
  CAPNET_REQUIRE(k >= 1 && k <= 16 && k <= V, "vocab_topk: k=%d (1 <= k <= 16, k <= V = %d)", k, V);
  CAPNET_REQUIRE(vocab_topk_supported(H, k, V), "vocab_topk: unsupported H=%d", H);
  CAPNET_REQUIRE(h && w && workspace && values && index && lse, "vocab_topk: null argument");
  CAPNET_REQUIRE(aligned16(h) && aligned16(workspace), "vocab_topk: h, w and the workspace must be 16-B aligned");
  CAPNET_REQUIRE((size_t)values % 4 == 0 && (size_t)index % 4 == 0 && (size_t)lse % 4 == 0, "vocab_topk: output alignment");
  for (int g = 0; g < groups; ++g)
    CAPNET_REQUIRE(w[g] && aligned16(w[g]), "vocab_topk: projection of group %d is null or not 16-B aligned", g);
  return vocab_topk_groups(h, w, b, groups, rows_per_group, H, V, k, workspace, values, index, lse, S(stream), mask, select_only);
}
int capnet_vocab_topk_groups(const float* h, const float* const* w, const float* const* b, int groups, int rows_per_group,
                             int H, int V, int k, void* workspace, float* values, int* index, float* lse,
                             capnet_stream_t stream) {
  return vocab_topk_groups_tail(h, w, b, groups, rows_per_group, H, V, k, workspace, values, index, lse, stream, nullptr, false);
}
int capnet_vocab_topk_groups_masked(const float* h, const float* const* w, const float* const* b, int groups, int rows_per_group,
                                    int H, int V, int k, const unsigned* mask, int select_only, void* workspace, float* values,
                                    int* index, float* lse, capnet_stream_t stream) {
  CAPNET_REQUIRE(mask && (size_t)mask % 4 == 0, "vocab_topk_groups_masked: mask is null or not 4-byte aligned");
  CAPNET_REQUIRE(select_only == 0 || select_only == 1, "vocab_topk_groups_masked: select_only=%d (0 or 1)", select_only);
  return vocab_topk_groups_tail(h, w, b, groups, rows_per_group, H, V, k, workspace, values, index, lse, stream, mask,
                                select_only != 0);
}

size_t capnet_lstm_beam_decode_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk) {
  return lstm_beam_decode_ws_bytes(nlayers, n, k, H, V, max_steps, fused_topk);
}

// the constraints of capnet_lstm_beam_decode[_groups]_constrained: the two existing checks, and no forced words on the fused step
static int lstm_constraints_check(const char* who, const BeamConstraints& con, int fused_topk) {
  if (int rc = beam_constraints_check(who, con)) return rc;
  if (con.n_forced)      // (0: none, whatever `forced` points at)
    if (int rc = beam_forced_check(who, con)) return rc;
  CAPNET_REQUIRE(!(fused_topk && con.n_forced), "%s: forced words take the unfused step (fused_topk = 0)", who);
  return kOk;
}

static int lstm_beam_decode_entry(const char* who, int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps,
                                  long long start_token, long long end_token, const float* first_inputs, const float* emb,
                                  const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                  const float* state0, void* workspace, float* slab, size_t slab_floats, int fused_topk,
                                  int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                  capnet_stream_t stream, const BeamConstraints* con = nullptr) {
  if (int rc = stack_decode_check(who, cell, nlayers, 1, n, k, E, H, V, max_steps, start_token, poll_every,
                                  fused_topk, 1, &emb, wcat, beff, &Cw, state0, workspace, slab, slab_floats, seqs, lengths,
                                  err_flag))
    return rc;
  CAPNET_REQUIRE((long)n * k < (1L << 24), "%s: n k too large", who);
  CAPNET_REQUIRE(!first_inputs || aligned16(first_inputs), "%s: first_inputs must be 16-B aligned", who);
  if (con)
    if (int rc = lstm_constraints_check(who, *con, fused_topk)) return rc;
  return lstm_beam_decode(cell, nlayers, n, k, E, H, V, max_steps, start_token, end_token, first_inputs, emb, wcat, beff, Cw, Cb,
                          state0, workspace, slab, slab_floats, fused_topk, poll_every, seqs, lengths, steps_run, err_flag,
                          S(stream), con);
}

int capnet_lstm_beam_decode(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                            long long end_token, const float* first_inputs, const float* emb, const float* const* wcat,
                            const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* workspace,
                            float* slab, size_t slab_floats, int fused_topk, int poll_every, long long* seqs, int* lengths,
                            int* steps_run, int* err_flag, capnet_stream_t stream) {
  return lstm_beam_decode_entry("lstm_beam_decode", cell, nlayers, n, k, E, H, V, max_steps, start_token, end_token, first_inputs, emb,
                                wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, fused_topk, poll_every, seqs, lengths,
                                steps_run, err_flag, stream);
}

size_t capnet_lstm_beam_decode_constrained_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk) {
  return lstm_beam_decode_ws_bytes(nlayers, n, k, H, V, max_steps, fused_topk, true);
}

int capnet_lstm_beam_decode_constrained(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps,
                                        long long start_token, long long end_token, const float* first_inputs, const float* emb,
                                        const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                        const float* state0, void* workspace, float* slab, size_t slab_floats, int fused_topk,
                                        int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                        capnet_stream_t stream, int no_repeat_ngram, int min_words, const int* banned,
                                        int n_banned, const int* forced, int n_forced) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned, forced, n_forced};
  return lstm_beam_decode_entry("lstm_beam_decode_constrained", cell, nlayers, n, k, E, H, V, max_steps, start_token, end_token,
                                first_inputs, emb, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, fused_topk, poll_every,
                                seqs, lengths, steps_run, err_flag, stream, &con);
}

size_t capnet_lstm_beam_decode_groups_ws_bytes(int nlayers, int groups, int n, int k, int H, int V, int max_steps,
                                               int fused_topk) {
  return lstm_beam_decode_groups_ws_bytes(nlayers, groups, n, k, H, V, max_steps, fused_topk);
}

// n below: the sentences of one group; the checks are capnet_lstm_beam_decode's at groups x n sentences
static int lstm_beam_decode_groups_entry(const char* who, int cell, int nlayers, int groups, int n, int k, int E, int H, int V,
                                         int max_steps, long long start_token, long long end_token, const float* const* emb,
                                         const float* const* wcat, const float* const* beff, const float* const* Cw,
                                         const float* const* Cb, const float* state0, void* workspace, float* slab,
                                         size_t slab_floats, int fused_topk, int poll_every, long long* seqs, int* lengths,
                                         int* steps_run, int* err_flag, capnet_stream_t stream,
                                         const BeamConstraints* con = nullptr) {
  if (int rc = stack_decode_check(who, cell, nlayers, groups, n, k, E, H, V, max_steps, start_token, poll_every,
                                  fused_topk, groups, emb, wcat, beff, Cw, state0, workspace, slab, slab_floats, seqs, lengths,
                                  err_flag))
    return rc;
  CAPNET_REQUIRE((long)groups * n * k < (1L << 24), "%s: n k too large", who);
  for (int g = 0; g < groups; ++g)
    CAPNET_REQUIRE(aligned16(emb[g]), "%s: emb and Cw must be 16-B aligned (group %d)", who, g);
  if (con)
    if (int rc = lstm_constraints_check(who, *con, fused_topk)) return rc;
  return lstm_beam_decode_groups(cell, nlayers, groups, n, k, E, H, V, max_steps, start_token, end_token, emb, wcat, beff, Cw, Cb,
                                 state0, workspace, slab, slab_floats, fused_topk, poll_every, seqs, lengths, steps_run, err_flag,
                                 S(stream), con);
}

int capnet_lstm_beam_decode_groups(int cell, int nlayers, int groups, int n, int k, int E, int H, int V, int max_steps,
                                   long long start_token, long long end_token, const float* const* emb,
                                   const float* const* wcat, const float* const* beff, const float* const* Cw,
                                   const float* const* Cb, const float* state0, void* workspace, float* slab,
                                   size_t slab_floats, int fused_topk, int poll_every, long long* seqs, int* lengths,
                                   int* steps_run, int* err_flag, capnet_stream_t stream) {
  return lstm_beam_decode_groups_entry("lstm_beam_decode", cell, nlayers, groups, n, k, E, H, V, max_steps, start_token, end_token, emb,
                                       wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, fused_topk, poll_every, seqs,
                                       lengths, steps_run, err_flag, stream);
}

size_t capnet_lstm_beam_decode_groups_constrained_ws_bytes(int nlayers, int groups, int n, int k, int H, int V, int max_steps,
                                                           int fused_topk) {
  return lstm_beam_decode_groups_ws_bytes(nlayers, groups, n, k, H, V, max_steps, fused_topk, true);
}

int capnet_lstm_beam_decode_groups_constrained(int cell, int nlayers, int groups, int n, int k, int E, int H, int V, int max_steps,
                                               long long start_token, long long end_token, const float* const* emb,
                                               const float* const* wcat, const float* const* beff, const float* const* Cw,
                                               const float* const* Cb, const float* state0, void* workspace, float* slab,
                                               size_t slab_floats, int fused_topk, int poll_every, long long* seqs,
                                               int* lengths, int* steps_run, int* err_flag, capnet_stream_t stream,
                                               int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                                               const int* forced, int n_forced) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned, forced, n_forced};
  return lstm_beam_decode_groups_entry("lstm_beam_decode_groups_constrained", cell, nlayers, groups, n, k, E, H, V, max_steps,
                                       start_token, end_token, emb, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats,
                                       fused_topk, poll_every, seqs, lengths, steps_run, err_flag, stream, &con);
}

int capnet_att_decode_supported(int E, int C, int H, int A, int P, int k, int nlayers) {
  return att_decode_supported(E, C, H, A, P, k, nlayers) ? 1 : 0;
}
size_t capnet_att_decode_step_ws_bytes(int n, int k, int P, int A, int C, int E) { return att_decode_step_ws_bytes(n, k, P, A, C, E); }

// what capnet_att_decode_step and capnet_att_beam_decode check alike
static int att_decode_check(const char* who, int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V,
                            const float* att1, const float* feat, const float* emb, const float* wz, const float* bz,
                            const float* w_full, const float* b_full, const float* const* wcat, const float* const* beff,
                            const void* workspace, const float* slab, size_t slab_floats, const int* err_flag, int groups = 1) {
  CAPNET_REQUIRE(groups >= 1 && groups <= 8, "%s: groups %d (1..8)", who, groups);
  const int n_images = n;
  n = n >= 1 && n < (1 << 24) ? groups * n : 0;   // the beam groups
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "%s: unknown cell %d", who, cell);
  CAPNET_REQUIRE(nlayers >= 1 && nlayers <= 8, "%s: layers %d (1..8)", who, nlayers);
  CAPNET_REQUIRE(n >= 1 && V >= 1, "%s: n %d, V %d", who, n_images, V);
  CAPNET_REQUIRE(k >= 1 && k <= 16 && k <= V, "%s: k=%d (1 <= k <= 16, k <= V = %d)", who, k, V);
  CAPNET_REQUIRE(att_decode_supported(E, C, H, A, P, k, nlayers), "%s: unsupported E=%d C=%d H=%d A=%d P=%d", who, E, C, H, A, P);
  CAPNET_REQUIRE((long)n * k * V < (1L << 31) && (long)n * P * C < (1L << 40), "%s: n k too large", who);
  CAPNET_REQUIRE(att1 && feat && emb && wz && bz && w_full && b_full && wcat && beff && workspace && slab && err_flag,
                 "%s: null argument", who);
  CAPNET_REQUIRE(aligned16(att1) && aligned16(feat) && aligned16(emb) && aligned16(wz) && aligned16(w_full) &&
                     aligned16(workspace) && aligned16(slab), "%s: att1, feat, emb, wz, w_full, workspace and slab must be 16-B aligned", who);
  // (wz and w_full of group g lie (A + C) H and A floats on: multiples of 16 bytes, A % 4 == 0 and H % 4 == 0)
  const size_t need = (size_t)n * k * (size_t)(V > A + C ? V : A + C);
  CAPNET_REQUIRE(slab_floats >= need, "%s: the slab holds %zu floats, one [n k][max(V, A + C)] block is %zu", who, slab_floats, need);
  return layer_weights_check(who, nlayers, wcat, beff);
}

int capnet_att_decode_step(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, const float* att1,
                           const float* feat, const long long* tokens, const float* emb, const float* wz, const float* bz,
                           const float* w_full, const float* b_full, const float* const* wcat, const float* const* beff,
                           const float* state_in, const long long* parent_rows, float* state_out, float* h_top,
                           void* workspace, float* slab, size_t slab_floats, int* err_flag, capnet_stream_t stream) {
  return capnet_att_decode_step_groups(cell, nlayers, 1, n, k, P, A, C, E, H, V, att1, feat, tokens, emb, wz, bz, w_full, b_full,
                                       wcat, beff, state_in, parent_rows, state_out, h_top, workspace, slab, slab_floats, err_flag,
                                       stream);
}

// capnet_att_decode_step_groups and capnet_att_decode_step_alphas (with_alphas: the maps are required)
static int att_decode_step_entry(int cell, int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                 const float* att1, const float* feat, const long long* tokens, const float* emb,
                                 const float* wz, const float* bz, const float* w_full, const float* b_full,
                                 const float* const* wcat, const float* const* beff, const float* state_in,
                                 const long long* parent_rows, float* state_out, float* h_top, void* workspace, float* slab,
                                 size_t slab_floats, int* err_flag, capnet_stream_t stream, bool with_alphas, float* alphas) {
  if (int rc = att_decode_check("att_decode_step", cell, nlayers, n, k, P, A, C, E, H, V, att1, feat, emb, wz, bz, w_full, b_full,
                                wcat, beff, workspace, slab, slab_floats, err_flag, groups))
    return rc;
  CAPNET_REQUIRE(tokens && state_in && state_out && h_top, "att_decode_step: null argument");
  CAPNET_REQUIRE(state_in != state_out, "att_decode_step: state_in and state_out must differ");
  CAPNET_REQUIRE(aligned16(state_in) && aligned16(state_out), "att_decode_step: state alignment (16-B aligned)");
  CAPNET_REQUIRE(!with_alphas || alphas, "att_decode_step: null argument (alphas is required)");
  CAPNET_REQUIRE((size_t)alphas % 4 == 0, "att_decode_step: alphas alignment");
  return att_decode_step(cell, nlayers, n, k, P, A, C, E, H, V, att1, feat, tokens, emb, wz, bz, w_full, b_full, wcat, beff,
                         state_in, parent_rows, state_out, h_top, workspace, slab, slab_floats, err_flag, S(stream), groups, alphas);
}

int capnet_att_decode_step_groups(int cell, int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                  const float* att1, const float* feat, const long long* tokens, const float* emb,
                                  const float* wz, const float* bz, const float* w_full, const float* b_full,
                                  const float* const* wcat, const float* const* beff, const float* state_in,
                                  const long long* parent_rows, float* state_out, float* h_top, void* workspace, float* slab,
                                  size_t slab_floats, int* err_flag, capnet_stream_t stream) {
  return att_decode_step_entry(cell, nlayers, groups, n, k, P, A, C, E, H, V, att1, feat, tokens, emb, wz, bz, w_full, b_full, wcat,
                               beff, state_in, parent_rows, state_out, h_top, workspace, slab, slab_floats, err_flag, stream, false,
                               nullptr);
}

int capnet_att_decode_step_alphas(int cell, int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                  const float* att1, const float* feat, const long long* tokens, const float* emb,
                                  const float* wz, const float* bz, const float* w_full, const float* b_full,
                                  const float* const* wcat, const float* const* beff, const float* state_in,
                                  const long long* parent_rows, float* state_out, float* h_top, void* workspace, float* slab,
                                  size_t slab_floats, int* err_flag, capnet_stream_t stream, float* alphas) {
  return att_decode_step_entry(cell, nlayers, groups, n, k, P, A, C, E, H, V, att1, feat, tokens, emb, wz, bz, w_full, b_full, wcat,
                               beff, state_in, parent_rows, state_out, h_top, workspace, slab, slab_floats, err_flag, stream, true,
                               alphas);
}

size_t capnet_att_beam_decode_ws_bytes(int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps) {
  return att_beam_decode_ws_bytes(nlayers, n, k, P, A, C, E, H, V, max_steps);
}

int capnet_att_beam_decode(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                           long long start_token, long long end_token, const float* att1, const float* feat, const float* emb,
                           const float* wz, const float* bz, const float* w_full, const float* b_full,
                           const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                           const float* state0, void* workspace, float* slab, size_t slab_floats, int poll_every,
                           long long* seqs, int* lengths, int* steps_run, int* err_flag, capnet_stream_t stream) {
  return capnet_att_beam_decode_groups(cell, nlayers, 1, n, k, P, A, C, E, H, V, max_steps, start_token, end_token, att1, feat, emb,
                                       wz, bz, w_full, b_full, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every,
                                       seqs, lengths, steps_run, err_flag, stream);
}

// capnet_att_beam_decode_groups and capnet_att_beam_decode_alphas (with_alphas: the maps are required)
static int att_beam_decode_entry(int cell, int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                 int max_steps, long long start_token, long long end_token, const float* att1,
                                 const float* feat, const float* emb, const float* wz, const float* bz, const float* w_full,
                                 const float* b_full, const float* const* wcat, const float* const* beff, const float* Cw,
                                 const float* Cb, const float* state0, void* workspace, float* slab, size_t slab_floats,
                                 int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                 capnet_stream_t stream, bool with_alphas, float* alphas,
                                 const BeamConstraints* con = nullptr, const BeamTeams* teams = nullptr) {
  if (int rc = att_decode_check("att_beam_decode", cell, nlayers, n, k, P, A, C, E, H, V, att1, feat, emb, wz, bz, w_full, b_full,
                                wcat, beff, workspace, slab, slab_floats, err_flag, groups))
    return rc;
  CAPNET_REQUIRE(max_steps >= 1 && poll_every >= 0, "att_beam_decode: max_steps %d, poll_every %d", max_steps, poll_every);
  CAPNET_REQUIRE((long)groups * n * k * (max_steps + 2) < (1L << 28), "att_beam_decode: n k too large");
  CAPNET_REQUIRE(start_token >= 0 && start_token <= 0x7fffffffLL, "att_beam_decode: start_token %lld", start_token);
  CAPNET_REQUIRE(Cw && state0 && seqs && lengths, "att_beam_decode: null argument (state0 is required)");
  CAPNET_REQUIRE(aligned16(Cw) && aligned16(state0), "att_beam_decode: Cw and state0 must be 16-B aligned");
  CAPNET_REQUIRE((size_t)seqs % 8 == 0 && (size_t)lengths % 4 == 0, "att_beam_decode: seqs / lengths alignment");
  CAPNET_REQUIRE(!with_alphas || alphas, "att_beam_decode: null argument (alphas is required)");
  CAPNET_REQUIRE((size_t)alphas % 4 == 0, "att_beam_decode: alphas alignment");
  if (con)
    if (int rc = beam_constraints_check("att_beam_decode", *con)) return rc;
  if (teams)
    if (int rc = decode_teams_check("att_beam_decode_diverse", groups * n, k, *teams, max_steps)) return rc;
  return att_beam_decode(cell, nlayers, n, k, P, A, C, E, H, V, max_steps, start_token, end_token, att1, feat, emb, wz, bz, w_full,
                         b_full, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths, steps_run,
                         err_flag, S(stream), groups, alphas, con, teams);
}

int capnet_att_beam_decode_diverse(int cell, int nlayers, int n, int k, int teams, float strength, int P, int A, int C, int E, int H,
                                   int V, int max_steps, long long start_token, long long end_token, const float* att1,
                                   const float* feat, const float* emb, const float* wz, const float* bz, const float* w_full,
                                   const float* b_full, const float* const* wcat, const float* const* beff, const float* Cw,
                                   const float* Cb, const float* state0, void* workspace, float* slab, size_t slab_floats,
                                   int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                   capnet_stream_t stream, float* alphas, int no_repeat_ngram, int min_words, const int* banned,
                                   int n_banned) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned};
  const BeamTeams dv{teams, strength, nullptr};
  return att_beam_decode_entry(cell, nlayers, 1, n, k, P, A, C, E, H, V, max_steps, start_token, end_token, att1, feat, emb, wz, bz,
                               w_full, b_full, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths,
                               steps_run, err_flag, stream, false, alphas, &con, &dv);
}

int capnet_att_beam_decode_forced(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                                  long long start_token, long long end_token, const float* att1, const float* feat,
                                  const float* emb, const float* wz, const float* bz, const float* w_full, const float* b_full,
                                  const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                  const float* state0, void* workspace, float* slab, size_t slab_floats, int poll_every,
                                  long long* seqs, int* lengths, int* steps_run, int* err_flag, capnet_stream_t stream,
                                  float* alphas, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                                  const int* forced, int n_forced) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned, forced, n_forced};
  if (int rc = beam_forced_check("att_beam_decode_forced", con)) return rc;
  return att_beam_decode_entry(cell, nlayers, 1, n, k, P, A, C, E, H, V, max_steps, start_token, end_token, att1, feat, emb, wz, bz,
                               w_full, b_full, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths,
                               steps_run, err_flag, stream, false, alphas, &con);
}

int capnet_att_beam_decode_rules(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                                 long long start_token, long long end_token, const float* att1, const float* feat,
                                 const float* emb, const float* wz, const float* bz, const float* w_full, const float* b_full,
                                 const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                 const float* state0, void* workspace, float* slab, size_t slab_floats, int poll_every,
                                 long long* seqs, int* lengths, int* steps_run, int* err_flag, capnet_stream_t stream,
                                 float* alphas, const int* rules) {
  if (int rc = beam_rules_check("att_beam_decode_rules", rules)) return rc;
  BeamConstraints con{0, 0, nullptr, 0};
  con.rules = rules;
  return att_beam_decode_entry(cell, nlayers, 1, n, k, P, A, C, E, H, V, max_steps, start_token, end_token, att1, feat, emb, wz, bz,
                               w_full, b_full, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths,
                               steps_run, err_flag, stream, false, alphas, &con);
}

int capnet_att_beam_decode_groups(int cell, int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                  int max_steps, long long start_token, long long end_token, const float* att1,
                                  const float* feat, const float* emb, const float* wz, const float* bz, const float* w_full,
                                  const float* b_full, const float* const* wcat, const float* const* beff, const float* Cw,
                                  const float* Cb, const float* state0, void* workspace, float* slab, size_t slab_floats,
                                  int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                  capnet_stream_t stream) {
  return att_beam_decode_entry(cell, nlayers, groups, n, k, P, A, C, E, H, V, max_steps, start_token, end_token, att1, feat, emb, wz,
                               bz, w_full, b_full, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs,
                               lengths, steps_run, err_flag, stream, false, nullptr);
}

// the three size queries of the attention sampler: 0 for arguments the entries refuse
static size_t att_sample_ws_query(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k, bool nucleus,
                                  bool excl) {
  if (nlayers < 1 || nlayers > 8 || H < 1 || V < 1 || top_k < 0 || top_k > 16 || top_k > V) return 0;
  return att_sample_decode_ws_bytes(nlayers, n, m, P, A, C, E, H, V, top_k, nucleus, excl);
}
size_t capnet_att_sample_decode_ws_bytes(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k) {
  return att_sample_ws_query(nlayers, n, m, P, A, C, E, H, V, top_k, false, false);
}
size_t capnet_att_sample_decode_nucleus_ws_bytes(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k) {
  return att_sample_ws_query(nlayers, n, m, P, A, C, E, H, V, top_k, true, false);
}
size_t capnet_att_sample_decode_excl_ws_bytes(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k,
                                              float top_p) {
  if (!(top_p > 0.f && top_p <= 1.f)) return 0;
  return att_sample_ws_query(nlayers, n, m, P, A, C, E, H, V, top_k, top_p < 1.f, true);
}

// every capnet_att_sample_decode* entry; top_p_one and ex as sample_decode_entry's (the start tokens are required anyway)
static int att_sample_decode_entry(const char* who, int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V,
                                   int steps, const long long* start_tokens, const float* att1, const float* feat,
                                   const float* emb, const float* wz, const float* bz, const float* w_full, const float* b_full,
                                   const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                   const float* state0, float temperature, int top_k, float top_p, bool top_p_one,
                                   unsigned long long seed, void* workspace, float* slab, size_t slab_floats, long long* ids,
                                   float* logp, float* state_out, int* err_flag, capnet_stream_t stream, unsigned greedy_stride,
                                   const SampleExcl* ex = nullptr) {
  if (int rc = greedy_stride_check(who, n * m, greedy_stride, m)) return rc;
  if (ex)
    if (int rc = sample_excl_check(who, *ex)) return rc;
  if (int rc = att_decode_check(who, cell, nlayers, n, m, P, A, C, E, H, V, att1, feat, emb, wz, bz, w_full, b_full, wcat, beff,
                                workspace, slab, slab_floats, err_flag))
    return rc;
  float inv_T = 0.f;
  if (int rc = top_p_check(who, top_p, top_p_one)) return rc;
  CAPNET_REQUIRE(steps >= 1 && steps <= 65535, "%s: steps %d (1..65535)", who, steps);
  if (int rc = sample_check(who, n * m, V, temperature, 0, 0, &inv_T)) return rc;
  CAPNET_REQUIRE(top_k >= 0 && top_k <= 16 && top_k <= V, "%s: top_k=%d (0 = off, 1 .. 16, <= V = %d)", who, top_k, V);
  CAPNET_REQUIRE(vocab_sample_supported(H), "%s: unsupported H=%d", who, H);
  CAPNET_REQUIRE(start_tokens && Cw && state0 && ids && logp, "%s: null argument (state0 is required)", who);
  CAPNET_REQUIRE(aligned16(Cw) && aligned16(state0) && (!state_out || aligned16(state_out)),
                 "%s: Cw and the states must be 16-B aligned", who);
  CAPNET_REQUIRE((size_t)start_tokens % 8 == 0 && (size_t)ids % 8 == 0 && (size_t)logp % 4 == 0, "%s: ids / logp alignment", who);
  return att_sample_decode(cell, nlayers, n, m, P, A, C, E, H, V, steps, start_tokens, att1, feat, emb, wz, bz, w_full, b_full, wcat,
                           beff, Cw, Cb, state0, SampleOpts{inv_T, top_k, top_p, seed, greedy_stride, ex}, workspace, slab,
                           slab_floats, ids, logp, state_out, err_flag, S(stream));
}
int capnet_att_sample_decode(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int steps,
                             const long long* start_tokens, const float* att1, const float* feat, const float* emb,
                             const float* wz, const float* bz, const float* w_full, const float* b_full,
                             const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                             const float* state0, float temperature, int top_k, unsigned long long seed, void* workspace,
                             float* slab, size_t slab_floats, long long* ids, float* logp, float* state_out, int* err_flag,
                             capnet_stream_t stream) {
  return att_sample_decode_entry("att_sample_decode", cell, nlayers, n, m, P, A, C, E, H, V, steps, start_tokens, att1, feat, emb, wz,
                                 bz, w_full, b_full, wcat, beff, Cw, Cb, state0, temperature, top_k, 1.f, true, seed, workspace, slab,
                                 slab_floats, ids, logp, state_out, err_flag, stream, 0);
}
int capnet_att_sample_decode_greedy(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int steps,
                                    const long long* start_tokens, const float* att1, const float* feat, const float* emb,
                                    const float* wz, const float* bz, const float* w_full, const float* b_full,
                                    const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                    const float* state0, float temperature, int top_k, unsigned long long seed,
                                    void* workspace, float* slab, size_t slab_floats, long long* ids, float* logp,
                                    float* state_out, int* err_flag, unsigned greedy_stride, capnet_stream_t stream) {
  return att_sample_decode_entry("att_sample_decode", cell, nlayers, n, m, P, A, C, E, H, V, steps, start_tokens, att1, feat, emb, wz,
                                 bz, w_full, b_full, wcat, beff, Cw, Cb, state0, temperature, top_k, 1.f, true, seed, workspace, slab,
                                 slab_floats, ids, logp, state_out, err_flag, stream, greedy_stride);
}
int capnet_att_sample_decode_nucleus(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V,
                                     int steps, const long long* start_tokens, const float* att1, const float* feat,
                                     const float* emb, const float* wz, const float* bz, const float* w_full,
                                     const float* b_full, const float* const* wcat, const float* const* beff,
                                     const float* Cw, const float* Cb, const float* state0, float temperature, int top_k,
                                     float top_p, unsigned long long seed, void* workspace, float* slab, size_t slab_floats,
                                     long long* ids, float* logp, float* state_out, int* err_flag, capnet_stream_t stream) {
  return att_sample_decode_entry("att_sample_decode_nucleus", cell, nlayers, n, m, P, A, C, E, H, V, steps, start_tokens, att1, feat,
                                 emb, wz, bz, w_full, b_full, wcat, beff, Cw, Cb, state0, temperature, top_k, top_p, false, seed,
                                 workspace, slab, slab_floats, ids, logp, state_out, err_flag, stream, 0);
}
int capnet_att_sample_decode_nucleus_greedy(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V,
                                            int steps, const long long* start_tokens, const float* att1, const float* feat,
                                            const float* emb, const float* wz, const float* bz, const float* w_full,
                                            const float* b_full, const float* const* wcat, const float* const* beff,
                                            const float* Cw, const float* Cb, const float* state0, float temperature,
                                            int top_k, float top_p, unsigned long long seed, void* workspace, float* slab,
                                            size_t slab_floats, long long* ids, float* logp, float* state_out, int* err_flag,
                                            unsigned greedy_stride, capnet_stream_t stream) {
  return att_sample_decode_entry("att_sample_decode_nucleus", cell, nlayers, n, m, P, A, C, E, H, V, steps, start_tokens, att1, feat,
                                 emb, wz, bz, w_full, b_full, wcat, beff, Cw, Cb, state0, temperature, top_k, top_p, false, seed,
                                 workspace, slab, slab_floats, ids, logp, state_out, err_flag, stream, greedy_stride);
}
int capnet_att_sample_decode_excl(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int steps,
                                  const long long* start_tokens, const float* att1, const float* feat, const float* emb,
                                  const float* wz, const float* bz, const float* w_full, const float* b_full,
                                  const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                  const float* state0, float temperature, int top_k, float top_p, unsigned long long seed,
                                  void* workspace, float* slab, size_t slab_floats, long long* ids, float* logp,
                                  float* state_out, int* err_flag, unsigned greedy_stride, long long end_token,
                                  int no_repeat_ngram, int min_words, const int* banned, int n_banned, capnet_stream_t stream) {
  const SampleExcl ex{end_token, no_repeat_ngram, min_words, banned, n_banned, nullptr};
  return att_sample_decode_entry("att_sample_decode_excl", cell, nlayers, n, m, P, A, C, E, H, V, steps, start_tokens, att1, feat, emb,
                                 wz, bz, w_full, b_full, wcat, beff, Cw, Cb, state0, temperature, top_k, top_p, true, seed, workspace,
                                 slab, slab_floats, ids, logp, state_out, err_flag, stream, greedy_stride, &ex);
}

size_t capnet_att_beam_decode_alphas_ws_bytes(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                              int max_steps) {
  return att_beam_decode_alphas_ws_bytes(nlayers, groups, n, k, P, A, C, E, H, V, max_steps);
}

int capnet_att_beam_decode_alphas(int cell, int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                  int max_steps, long long start_token, long long end_token, const float* att1,
                                  const float* feat, const float* emb, const float* wz, const float* bz, const float* w_full,
                                  const float* b_full, const float* const* wcat, const float* const* beff, const float* Cw,
                                  const float* Cb, const float* state0, void* workspace, float* slab, size_t slab_floats,
                                  int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                  capnet_stream_t stream, float* alphas) {
  return att_beam_decode_entry(cell, nlayers, groups, n, k, P, A, C, E, H, V, max_steps, start_token, end_token, att1, feat, emb, wz,
                               bz, w_full, b_full, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs,
                               lengths, steps_run, err_flag, stream, true, alphas);
}

int capnet_att_beam_decode_constrained(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                                       long long start_token, long long end_token, const float* att1, const float* feat,
                                       const float* emb, const float* wz, const float* bz, const float* w_full,
                                       const float* b_full, const float* const* wcat, const float* const* beff, const float* Cw,
                                       const float* Cb, const float* state0, void* workspace, float* slab, size_t slab_floats,
                                       int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                       capnet_stream_t stream, int no_repeat_ngram, int min_words, const int* banned,
                                       int n_banned) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned};
  return att_beam_decode_entry(cell, nlayers, 1, n, k, P, A, C, E, H, V, max_steps, start_token, end_token, att1, feat, emb, wz, bz,
                               w_full, b_full, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths,
                               steps_run, err_flag, stream, false, nullptr, &con);
}

int capnet_att_beam_decode_alphas_constrained(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V,
                                              int max_steps, long long start_token, long long end_token,
                                              const float* att1, const float* feat, const float* emb, const float* wz,
                                              const float* bz, const float* w_full, const float* b_full,
                                              const float* const* wcat, const float* const* beff, const float* Cw,
                                              const float* Cb, const float* state0, void* workspace, float* slab,
                                              size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run,
                                              int* err_flag, capnet_stream_t stream, float* alphas, int no_repeat_ngram,
                                              int min_words, const int* banned, int n_banned) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned};
  return att_beam_decode_entry(cell, nlayers, 1, n, k, P, A, C, E, H, V, max_steps, start_token, end_token, att1, feat, emb, wz, bz,
                               w_full, b_full, wcat, beff, Cw, Cb, state0, workspace, slab, slab_floats, poll_every, seqs, lengths,
                               steps_run, err_flag, stream, true, alphas, &con);
}

int capnet_lstm_pointwise_bwd(const float* gates, const float* c, const float* c_prev, const float* dh, float* dc_io,
                              float* dpre, int b, int H, int cell, capnet_stream_t stream) {
  CAPNET_REQUIRE(gates && c && dh && dc_io && dpre && b >= 0 && H > 0, "lstm_pointwise_bwd: bad argument");
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "lstm_pointwise_bwd: unknown cell %d", cell);
  const bool f = cell == kCellFactored;
  // (no separate recurrent dh: the caller's dh is the whole gradient of h; dc_io: in dL/dc, out dL/dc_prev)
  return lstm_pointwise_bwd(gates, 4L * H, c, c_prev, dh, nullptr, dc_io, dpre, 4L * H, b, b, H, 0, 1, f ? 2 : 3, f ? 3 : 2,
                            f ? 0 : 1, S(stream), 0, 0);
}
size_t capnet_lstm_wfrag_floats(int H) { return lstm_wfrag_floats(H); }
int capnet_lstm_pack_wfrag(const float* w_cat, float* w_frag, int H, int cell, capnet_stream_t stream) {
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "lstm_pack_wfrag: unknown cell %d", cell);
  return cell == kCellFactored ? lstm_pack_wfrag(w_cat, w_frag, H, 0, 1, 2, 3, S(stream))
                               : lstm_pack_wfrag(w_cat, w_frag, H, 0, 1, 3, 2, S(stream));
}
int capnet_lstm_step_fused(const float* h_prev, const float* w_cat, float* gates, long ldg,
                           const float* c_prev, float* c_out, float* h_out, int b, int H, int cell,
                           capnet_stream_t stream) {
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "lstm_step_fused: unknown cell %d", cell);
  if (cell == kCellFactored)
    return lstm_step_fused(h_prev, w_cat, gates, ldg, c_prev, c_out, h_out, b, H, 0, 1, 2, 3, 0, S(stream));
  return lstm_step_fused(h_prev, w_cat, gates, ldg, c_prev, c_out, h_out, b, H, 0, 1, 3, 2, 1, S(stream));
}
int capnet_lstm_step_fused_stamped(const float* h_prev, const float* w_frag, float* gates, long ldg,
                                   const float* c_prev, float* c_out, float* h_out, int b, int H,
                                   unsigned long long* stamps, capnet_stream_t stream) {
  return lstm_step_fused(h_prev, w_frag, gates, ldg, c_prev, c_out, h_out, b, H, 0, 1, 2, 3, 0,
                         S(stream), stamps);
}
int capnet_lstm_step_fused_supported(int b, int H) { return lstm_step_fused_supported(b, H) ? 1 : 0; }

int capnet_lstm_step_fused_route(int b, int H, int* detail) {
  StepFusedRoute r;
  if (!lstm_step_fused_route(b, H, &r)) return 0;
  if (detail) detail[0] = r.ngw, detail[1] = r.mt, detail[2] = r.halves, detail[3] = r.xcd_map;
  return 1;
}

int capnet_stacked_decode_route(int E, int H, int xvec, int* detail) {
  DecodeRoute r;
  // stacked_decode_supported(1, H): H is one of the step kernels' hidden sizes, as every entry above the layer requires
  if (E < 1 || E > (1 << 20) || !stacked_decode_supported(1, H) || !stacked_decode_route((E + 15) / 16 * 16, H, xvec, &r)) return 0;
  if (detail) detail[0] = r.nj, detail[1] = r.tm;
  return r.wide ? 2 : 1;
}

int capnet_lstm_upper_step(const float* xin, const float* h_prev, const float* c_prev, const float* w_eff, const float* w_rec,
                           const float* b_eff, float* x_out, float* gates, float* c_out, float* h_out, int b, int H, int r0,
                           float p, unsigned long long seed, int layer, int use_dropout, int cell, capnet_stream_t stream) {
  return lstm_upper_step(xin, h_prev, c_prev, w_eff, w_rec, b_eff, x_out, gates, c_out, h_out, b, H, r0, p, seed, layer,
                         use_dropout, S(stream), cell);
}

int capnet_lstm_persist_supported(int b, int H) { return lstm_persist_supported(b, H) ? 1 : 0; }
int capnet_lstm_persist_set_mode(int mode) { return lstm_persist_set_mode(mode); }
size_t capnet_lstm_persist_w_floats(void) { return lstm_persist_w_floats(); }
size_t capnet_lstm_persist_ctl_ints(void) { return lstm_persist_ctl_ints(); }
int capnet_lstm_persist_pack(const float* w_cat, float* w_img, int cell, capnet_stream_t stream) {
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "lstm_persist_pack: unknown cell %d", cell);
  return cell == kCellFactored ? lstm_persist_pack(w_cat, w_img, 0, 1, 2, 3, S(stream))
                               : lstm_persist_pack(w_cat, w_img, 0, 1, 3, 2, S(stream));
}
int capnet_lstm_persist_run(const float* w_img, float* gates, float* cell_states, float* hiddens,
                            const int* batch_sizes, int t0, int t1, int H, int cell, int segment,
                            int* ctl, int* err_flag, unsigned long long* stamps,
                            capnet_stream_t stream) {
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "lstm_persist_run: unknown cell %d", cell);
  CAPNET_REQUIRE(batch_sizes && t1 > 0 && t1 <= kMaxSteps, "lstm_persist_run: bad steps");
  int off[kMaxSteps + 1];
  off[0] = 0;
  for (int t = 0; t < t1; ++t) off[t + 1] = off[t] + batch_sizes[t];
  const bool f = cell == kCellFactored;
  return lstm_persist_run(w_img, gates, cell_states, hiddens, off, batch_sizes, t0, t1, H, 0, 1,
                          f ? 2 : 3, f ? 3 : 2, f ? 0 : 1, segment, ctl, err_flag, S(stream), stamps);
}

size_t capnet_seq_saved_floats(const int* dims) { return seq_saved_floats(to_dims(dims)); }
size_t capnet_seq_saved_ints(const int* dims) { return seq_saved_ints(to_dims(dims)); }
size_t capnet_seq_saved_cell_offset(const int* dims) { return seq_saved_cell_offset(to_dims(dims)); }
size_t capnet_seq_fwd_scratch_floats(const int* dims) { return seq_fwd_scratch_floats(to_dims(dims)); }
size_t capnet_seq_bwd_scratch_floats(const int* dims) { return seq_bwd_scratch_floats(to_dims(dims)); }

int capnet_seq_forward_stacked(const int* dims, int nlayers, const int* batch_sizes, const unsigned char* tf_mask,
                               const long long* captions, const float* features, const float* emb,
                               const float* const* weights, const float* Cw, const float* Cb, float dropout_p,
                               unsigned long long seed, int training, float* const* saved, int* const* saved_i,
                               float* scratch, float* const* hiddens, int* err_flag, capnet_stream_t stream) {
  CAPNET_REQUIRE(dims && weights && nlayers >= 1 && nlayers <= 8, "seq_forward_stacked: null dims / weights or layers %d", nlayers);
  const SeqDims d = to_dims(dims);
  CAPNET_REQUIRE(d.cell == kCellFactored || d.cell == kCellLSTM, "seq_forward_stacked: unknown cell %d", d.cell);
  SeqWeights w[8];
  for (int l = 0; l < nlayers; ++l) {
    for (int i = 0; i < 32; ++i)
      CAPNET_REQUIRE(!weight_used(d.cell, i) || weights[32 * l + i], "seq_forward_stacked: weight %d of layer %d is null", i, l);
    to_weights(weights + 32 * l, w[l]);
  }
  return seq_forward_stacked(d, nlayers, batch_sizes, tf_mask, captions, features, emb, w, Cw, Cb, dropout_p, seed, training,
                             saved, saved_i, scratch, hiddens, err_flag, S(stream));
}

int capnet_seq_backward_stacked(const int* dims, int nlayers, const int* batch_sizes, const float* d_hiddens,
                                const float* const* hiddens, const float* const* saved, const int* const* saved_i,
                                float* scratch, float* const* dh_work, float* const* grads, float dropout_p,
                                unsigned long long seed, int training, capnet_stream_t stream) {
  CAPNET_REQUIRE(dims && grads && nlayers >= 1 && nlayers <= 8, "seq_backward_stacked: null dims / grads or layers %d", nlayers);
  SeqGrads g[8];
  for (int l = 0; l < nlayers; ++l) to_grads(grads + 9 * l, g[l]);
  return seq_backward_stacked(to_dims(dims), nlayers, batch_sizes, d_hiddens, hiddens, saved, saved_i, scratch, dh_work, g,
                              dropout_p, seed, training, S(stream));
}

// the single-layer entries: the stacked ones at one layer
int capnet_seq_forward(const int* dims, const int* batch_sizes, const unsigned char* tf_mask,
                       const long long* captions, const float* features, const float* emb,
                       const float* const* weights, const float* Cw, const float* Cb,
                       float dropout_p, unsigned long long seed, int training, float* saved,
                       int* saved_i, float* scratch, float* hiddens, int* err_flag,
                       capnet_stream_t stream) {
  return capnet_seq_forward_stacked(dims, 1, batch_sizes, tf_mask, captions, features, emb, weights, Cw, Cb, dropout_p, seed,
                                    training, &saved, &saved_i, scratch, &hiddens, err_flag, stream);
}

int capnet_seq_backward(const int* dims, const int* batch_sizes, const float* d_hiddens,
                        const float* hiddens, const float* saved, const int* saved_i,
                        float* scratch, float* const* grads, float dropout_p,
                        unsigned long long seed, int training, capnet_stream_t stream) {
  return capnet_seq_backward_stacked(dims, 1, batch_sizes, d_hiddens, &hiddens, &saved, &saved_i, scratch, nullptr, grads,
                                     dropout_p, seed, training, stream);
}

int capnet_att_set_chain_mode(int mode) { return att_set_chain_mode(mode); }
size_t capnet_att_saved_floats(const int* dims) { return att_saved_floats(to_adims(dims)); }
size_t capnet_att_saved_ints(const int* dims) { return att_saved_ints(to_adims(dims)); }
size_t capnet_att_fwd_scratch_floats(const int* dims) { return att_fwd_scratch_floats(to_adims(dims)); }
size_t capnet_att_bwd_scratch_floats(const int* dims) { return att_bwd_scratch_floats(to_adims(dims)); }

int capnet_beam_topk_batched(const float* logits, long ld, int V, const float* prev_scores, const int* meta, int n,
                             float* top_scores, long long* top_index, capnet_stream_t stream) {
  // (no option given: the plain kernel, which only reads the logits)
  return beam_topk_batched("beam_topk_batched", const_cast<float*>(logits), ld, V, prev_scores, meta, n, nullptr, 0, nullptr, nullptr,
                           nullptr, 0, 0, top_scores, top_index, S(stream));
}
int capnet_beam_topk(const float* logits, long ld, int rows, int V, const float* prev_scores, int k,
                     float* top_scores, long long* top_index, capnet_stream_t stream) {
  return beam_topk(logits, ld, rows, V, prev_scores, k, top_scores, top_index, S(stream));
}
int capnet_beam_topk_banned(float* logits, long ld, int rows, int V, const float* prev_scores, int k, const int* bans, int cap,
                            float* top_scores, long long* top_index, capnet_stream_t stream) {
  return beam_topk_banned(logits, ld, rows, V, prev_scores, k, bans, cap, top_scores, top_index, S(stream));
}
int capnet_beam_topk_batched_banned(float* logits, long ld, int V, const float* prev_scores, const int* meta, int n,
                                    const int* bans, int cap, float* top_scores, long long* top_index, capnet_stream_t stream) {
  CAPNET_REQUIRE(bans, "beam_topk_batched_banned: bad argument");
  return beam_topk_batched("beam_topk_batched_banned", logits, ld, V, prev_scores, meta, n, bans, cap, nullptr, nullptr, nullptr, 0,
                           0, top_scores, top_index, S(stream));
}
size_t capnet_beam_state_bytes(int n, int k, int max_steps) { return beam_state_bytes(n, k, max_steps); }
int capnet_beam_init(void* beam, int n, int k, int max_steps, long long start_token, long long* prev_words,
                     capnet_stream_t stream) {
  return beam_init(beam, n, k, max_steps, start_token, prev_words, S(stream));
}
int capnet_beam_advance(void* beam, const float* logits, long ld, int V, int n, int k, int max_steps, int step,
                        long long end_token, long long* next_words, long long* parent_rows, capnet_stream_t stream) {
  // (no option given: the plain kernel, which only reads the logits)
  return beam_advance("beam_advance", beam, const_cast<float*>(logits), ld, V, n, k, max_steps, step, end_token, nullptr, nullptr,
                      next_words, parent_rows, nullptr, S(stream));
}
int capnet_beam_advance_topk(void* beam, const float* values, const int* index, const float* lse, int V, int n, int k,
                             int max_steps, int step, long long end_token, long long* next_words, long long* parent_rows,
                             capnet_stream_t stream) {
  return beam_advance_topk(beam, values, index, lse, V, n, k, max_steps, step, end_token, next_words, parent_rows, S(stream));
}
int capnet_beam_finish(const void* beam, int n, int k, int max_steps, long long end_token, long long* seqs, int* lengths,
                       capnet_stream_t stream) {
  return beam_finish(beam, n, k, max_steps, end_token, seqs, lengths, S(stream));
}
size_t capnet_beam_trace_bytes(int n, int k, int max_steps) { return beam_trace_bytes(n, k, max_steps); }
int capnet_beam_advance_traced(void* beam, void* trace, const float* logits, long ld, int V, int n, int k, int max_steps,
                               int step, long long end_token, long long* next_words, long long* parent_rows,
                               capnet_stream_t stream) {
  CAPNET_REQUIRE(trace != nullptr, "beam_advance_traced: null trace");
  CAPNET_REQUIRE((size_t)beam % 4 == 0 && (size_t)trace % 4 == 0, "beam_advance_traced: the state and the trace must be 4-byte aligned");
  return beam_advance("beam_advance_traced", beam, const_cast<float*>(logits), ld, V, n, k, max_steps, step, end_token, nullptr,
                      nullptr, next_words, parent_rows, trace, S(stream));
}
int capnet_beam_advance_constrained(void* beam, float* logits, long ld, int V, int n, int k, int max_steps, int step,
                                    long long end_token, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                                    long long* next_words, long long* parent_rows, capnet_stream_t stream) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned};
  return beam_advance("beam_advance_constrained", beam, logits, ld, V, n, k, max_steps, step, end_token, &con, nullptr, next_words,
                      parent_rows, nullptr, S(stream));
}
int capnet_beam_advance_constrained_traced(void* beam, void* trace, float* logits, long ld, int V, int n, int k, int max_steps,
                                           int step, long long end_token, int no_repeat_ngram, int min_words, const int* banned,
                                           int n_banned, long long* next_words, long long* parent_rows, capnet_stream_t stream) {
  CAPNET_REQUIRE(trace != nullptr, "beam_advance_constrained_traced: null trace");
  CAPNET_REQUIRE((size_t)beam % 4 == 0 && (size_t)trace % 4 == 0,
                 "beam_advance_constrained_traced: the state and the trace must be 4-byte aligned");
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned};
  return beam_advance("beam_advance_constrained_traced", beam, logits, ld, V, n, k, max_steps, step, end_token, &con, nullptr,
                      next_words, parent_rows, trace, S(stream));
}
int capnet_beam_advance_diverse(void* beam, void* trace, float* logits, long ld, int V, int n, int k, int teams, float strength,
                                int max_steps, int step, long long end_token, int no_repeat_ngram, int min_words,
                                const int* banned, int n_banned, long long* next_words, long long* parent_rows,
                                capnet_stream_t stream) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned};
  const BeamTeams dv{teams, strength, nullptr};
  return beam_advance("beam_advance_diverse", beam, logits, ld, V, n, k, max_steps, step, end_token, &con, &dv, next_words,
                      parent_rows, trace, S(stream));
}
int capnet_beam_topk_batched_diverse(float* logits, long ld, int V, const float* prev_scores, const int* meta, int n, int teams,
                                     float strength, const int* bans, int cap, float* top_scores, long long* top_index,
                                     capnet_stream_t stream) {
  const BeamTeams dv{teams, strength, nullptr};
  return beam_topk_batched("beam_topk_batched_diverse", logits, ld, V, prev_scores, meta, n, bans, cap, &dv, nullptr, nullptr, 0, 0,
                           top_scores, top_index, S(stream));
}
int capnet_beam_advance_forced(void* beam, void* trace, float* logits, long ld, int V, int n, int k, int max_steps, int step,
                               long long end_token, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                               const int* forced, int n_forced, long long* next_words, long long* parent_rows,
                               capnet_stream_t stream) {
  const BeamConstraints con{no_repeat_ngram, min_words, banned, n_banned, forced, n_forced};
  if (int rc = beam_forced_check("beam_advance_forced", con)) return rc;   // (n_forced == 0 would be the constrained step)
  return beam_advance("beam_advance_forced", beam, logits, ld, V, n, k, max_steps, step, end_token, &con, nullptr, next_words,
                      parent_rows, trace, S(stream));
}
int capnet_beam_topk_batched_forced(float* logits, long ld, int V, const float* prev_scores, const int* meta, int n,
                                    const int* bans, int cap, const int* met, const int* forced, int n_forced,
                                    long long end_token, float* top_scores, long long* top_index, capnet_stream_t stream) {
  if (int rc = beam_forced_check("beam_topk_batched_forced", BeamConstraints{0, 0, nullptr, 0, forced, n_forced})) return rc;
  return beam_topk_batched("beam_topk_batched_forced", logits, ld, V, prev_scores, meta, n, bans, cap, nullptr, met, forced, n_forced,
                           end_token, top_scores, top_index, S(stream));
}
int capnet_beam_advance_rules(void* beam, void* trace, float* logits, long ld, int V, int n, int k, int max_steps, int step,
                              long long end_token, const int* rules, long long* next_words, long long* parent_rows,
                              capnet_stream_t stream) {
  if (int rc = beam_rules_check("beam_advance_rules", rules)) return rc;   // (NULL would be the plain step)
  BeamConstraints con{0, 0, nullptr, 0};
  con.rules = rules;
  return beam_advance("beam_advance_rules", beam, logits, ld, V, n, k, max_steps, step, end_token, &con, nullptr, next_words,
                      parent_rows, trace, S(stream));
}
int capnet_beam_topk_batched_rules(float* logits, long ld, int V, const float* prev_scores, const int* meta, int n,
                                   const int* bans, int cap, const int* met, const int* rules, long long end_token,
                                   float* top_scores, long long* top_index, capnet_stream_t stream) {
  if (int rc = beam_rules_check("beam_topk_batched_rules", rules)) return rc;
  return beam_topk_batched("beam_topk_batched_rules", logits, ld, V, prev_scores, meta, n, bans, cap, nullptr, met, nullptr, 0,
                           end_token, top_scores, top_index, S(stream), rules);
}
int capnet_beam_finish_traced(const void* beam, const void* trace, int n, int k, int max_steps, long long end_token,
                              long long* seqs, int* lengths, int* rows, capnet_stream_t stream) {
  CAPNET_REQUIRE(trace && rows, "beam_finish_traced: null trace or rows");
  CAPNET_REQUIRE((size_t)beam % 4 == 0 && (size_t)trace % 4 == 0 && (size_t)rows % 4 == 0,
                 "beam_finish_traced: the state, the trace and the rows must be 4-byte aligned");
  return beam_finish(beam, n, k, max_steps, end_token, seqs, lengths, S(stream), trace, rows);
}
int capnet_beam_nbest(const void* beam, int n, int k, int max_steps, float length_penalty, long long* seqs, int* lengths,
                      float* scores, int* counts, capnet_stream_t stream) {
  return beam_nbest(beam, n, k, max_steps, length_penalty, seqs, lengths, scores, counts, S(stream));
}
int capnet_beam_nbest_traced(const void* beam, const void* trace, int n, int k, int max_steps, float length_penalty,
                             long long* seqs, int* lengths, float* scores, int* counts, int* rows, capnet_stream_t stream) {
  CAPNET_REQUIRE(trace && rows, "beam_nbest_traced: null trace or rows");
  CAPNET_REQUIRE((size_t)beam % 4 == 0 && (size_t)trace % 4 == 0 && (size_t)rows % 4 == 0,
                 "beam_nbest_traced: the state, the trace and the rows must be 4-byte aligned");
  return beam_nbest(beam, n, k, max_steps, length_penalty, seqs, lengths, scores, counts, S(stream), trace, rows);
}
size_t capnet_beam_decode_ws_beam_offset(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk, int groups) {
  return beam_decode_ws_beam_offset(nlayers, n, k, H, V, max_steps, fused_topk, groups);
}
size_t capnet_att_beam_decode_alphas_ws_trace_offset(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H,
                                                     int V, int max_steps) {
  return att_beam_decode_alphas_ws_trace_offset(nlayers, groups, n, k, P, A, C, E, H, V, max_steps);
}
size_t capnet_att_beam_decode_alphas_ws_hist_offset(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H,
                                                    int V, int max_steps) {
  return att_beam_decode_alphas_ws_hist_offset(nlayers, groups, n, k, P, A, C, E, H, V, max_steps);
}
int capnet_alpha_gather(const float* hist, const int* rows, int captions, int nk, int max_steps, int P, float* alphas,
                        capnet_stream_t stream) {
  return alpha_gather(hist, rows, captions, nk, max_steps, P, alphas, S(stream));
}
int capnet_beam_live(const void* beam, int n, int k, int max_steps, const int** live_total, const int** live,
                     const float** scores) {
  return beam_live(beam, n, k, max_steps, live_total, live, scores);
}
int capnet_att_step_fwd(const float* att1, const float* feat, const float* att2, float* gate_io,
                        long ldz, const float* w_full, const float* b_full, int rows, int P, int A,
                        int C, float* alpha_out, float* alphas_bt, int steps, int t, float* awe_out,
                        float* xa_out, long ldx, float* scores_ws, capnet_stream_t stream) {
  CAPNET_REQUIRE(steps > 0 && t >= 0 && t < steps, "att_step_fwd: t=%d steps=%d", t, steps);
  return att_step_fwd(att1, feat, att2, gate_io, ldz, w_full, b_full, rows, P, A, C, alpha_out,
                      alphas_bt, steps, t, awe_out, xa_out, ldx, scores_ws, S(stream));
}
size_t capnet_att_stacked_saved_floats(const int* dims, int layer) { return att_stacked_saved_floats(to_adims(dims), layer); }
size_t capnet_att_stacked_saved_ints(const int* dims, int layer) { return att_stacked_saved_ints(to_adims(dims), layer); }
size_t capnet_att_stacked_fwd_scratch_floats(const int* dims, int nlayers) {
  return att_stacked_fwd_scratch_floats(to_adims(dims), nlayers);
}
size_t capnet_att_stacked_bwd_scratch_floats(const int* dims, int nlayers) {
  return att_stacked_bwd_scratch_floats(to_adims(dims), nlayers);
}

int capnet_att_seq_forward_stacked(const int* dims, int nlayers, const int* batch_sizes, const unsigned char* tf_mask,
                                   const long long* captions, const float* features, const float* emb,
                                   const float* const* weights, const float* Cw, const float* Cb, float dropout_p,
                                   unsigned long long seed, int training, float* const* saved, int* const* saved_i,
                                   float* scratch, float* const* hiddens, float* alphas, int* err_flag,
                                   capnet_stream_t stream) {
  CAPNET_REQUIRE(dims && weights && nlayers >= 1 && nlayers <= 8, "att_seq_forward_stacked: null dims / weights or layers %d",
                 nlayers);
  AttWeights w0;
  int rc = to_aweights(weights, &w0, dims[11]);
  if (rc) return rc;
  SeqWeights wu[8];
  UpperInit iu[8];
  for (int l = 1; l < nlayers; ++l) {
    const float* const* p = weights + 44 + 36 * (l - 1);
    for (int i = 0; i < 36; ++i)
      CAPNET_REQUIRE(p[i] || (i < 32 && !weight_used(dims[11], i)), "att_seq_forward_stacked: weight %d of layer %d is null",
                     i, l);
    to_weights(p, wu[l - 1]);
    iu[l - 1] = UpperInit{p[32], p[33], p[34], p[35]};
  }
  return att_seq_forward_stacked(to_adims(dims), nlayers, batch_sizes, tf_mask, captions, features, emb, w0, wu, iu, Cw, Cb,
                                 dropout_p, seed, training, saved, saved_i, scratch, hiddens, alphas, err_flag, S(stream));
}

int capnet_att_seq_backward_stacked(const int* dims, int nlayers, const int* batch_sizes, const float* d_hiddens,
                                    const float* d_alphas, const float* const* hiddens, const float* features,
                                    const float* const* weights, const float* const* saved, const int* const* saved_i,
                                    float* scratch, float* const* dh_work, float* const* grads, float dropout_p,
                                    unsigned long long seed, int training, capnet_stream_t stream) {
  CAPNET_REQUIRE(dims && weights && grads && nlayers >= 1 && nlayers <= 8,
                 "att_seq_backward_stacked: null dims / weights / grads or layers %d", nlayers);
  AttWeights w0;
  int rc = to_aweights(weights, &w0, dims[11]);
  if (rc) return rc;
  AttGrads g;
  to_agrads(grads, g);
  SeqGrads gu[8];
  UpperInitGrads giu[8];
  for (int l = 1; l < nlayers; ++l) {
    float* const* q = grads + 16 + 11 * (l - 1);
    for (int i = 0; i < 11; ++i)
      CAPNET_REQUIRE(q[i] || (i >= 1 && i <= 4 && dims[11] != kCellFactored),
                     "att_seq_backward_stacked: gradient %d of layer %d is null", i, l);
    to_grads(q, gu[l - 1]);
    gu[l - 1].dEmb = gu[l - 1].dFeat = nullptr;       // (q[7..10]: init_h{l} / init_c{l}; no embedding, no features)
    giu[l - 1] = UpperInitGrads{q[7], q[8], q[9], q[10]};
  }
  return att_seq_backward_stacked(to_adims(dims), nlayers, batch_sizes, d_hiddens, d_alphas, hiddens, features, w0, saved,
                                  saved_i, scratch, dh_work, g, gu, giu, dropout_p, seed, training, S(stream));
}

// the single-layer entries: the stacked ones at one layer
int capnet_att_seq_forward(const int* dims, const int* batch_sizes, const unsigned char* tf_mask,
                           const long long* captions, const float* features, const float* emb,
                           const float* const* weights, const float* Cw, const float* Cb,
                           float dropout_p, unsigned long long seed, int training, float* saved,
                           int* saved_i, float* scratch, float* hiddens, float* alphas,
                           int* err_flag, capnet_stream_t stream) {
  return capnet_att_seq_forward_stacked(dims, 1, batch_sizes, tf_mask, captions, features, emb, weights, Cw, Cb, dropout_p,
                                        seed, training, &saved, &saved_i, scratch, &hiddens, alphas, err_flag, stream);
}

int capnet_att_seq_backward(const int* dims, const int* batch_sizes, const float* d_hiddens,
                            const float* d_alphas, const float* hiddens, const float* features,
                            const float* const* weights, const float* saved, const int* saved_i,
                            float* scratch, float* const* grads, float dropout_p,
                            unsigned long long seed, int training, capnet_stream_t stream) {
  return capnet_att_seq_backward_stacked(dims, 1, batch_sizes, d_hiddens, d_alphas, &hiddens, features, weights, &saved,
                                         &saved_i, scratch, nullptr, grads, dropout_p, seed, training, stream);
}

int capnet_xent_fwd(const float* logits, long ld, int N, int V, const long long* targets,
                    float* lse, float* row_loss, float* loss, int* err_flag,
                    capnet_stream_t stream) {
  return xent_fwd(logits, ld, N, V, targets, lse, row_loss, loss, err_flag, S(stream));
}
int capnet_resize_u8(const unsigned char* src, int Hs, int Ws, unsigned char* tmp, unsigned char* dst,
                     int Ho, int Wo, const int* bounds_h, const int* coef_h, int kmax_h,
                     const int* bounds_v, const int* coef_v, int kmax_v, capnet_stream_t stream) {
  return resize_u8(src, Hs, Ws, tmp, dst, Ho, Wo, bounds_h, coef_h, kmax_h, bounds_v, coef_v, kmax_v,
                   S(stream));
}
int capnet_crop_flip_normalize(const unsigned char* src, int B, int Hs, int Ws, const int* params,
                               float* dst, int Hc, int Wc, const float* mean, const float* stdv,
                               capnet_stream_t stream) {
  return crop_flip_normalize(src, B, Hs, Ws, params, dst, Hc, Wc, mean, stdv, S(stream));
}
int capnet_topk_correct(const float* logits, long ld, int N, int V, const long long* targets, int k,
                        int* count, int* err_flag, capnet_stream_t stream) {
  return topk_correct(logits, ld, N, V, targets, k, count, err_flag, S(stream));
}
int capnet_xent_bwd(const float* logits, long ld, int N, int V, const long long* targets,
                    const float* lse, const float* grad_out, float* dlogits, long ldd,
                    capnet_stream_t stream) {
  return xent_bwd(logits, ld, N, V, targets, lse, grad_out, dlogits, ldd, S(stream));
}
int capnet_att_loss_fwd(const float* nll, const float* alphas, int B, int steps, int P, float alpha_c,
                        float* colsum, float* out, capnet_stream_t stream) {
  return att_loss_fwd(nll, alphas, B, steps, P, alpha_c, colsum, out, S(stream));
}
int capnet_att_loss_bwd(const float* gout, const float* colsum, int B, int steps, int P, float alpha_c,
                        float* dalphas, capnet_stream_t stream) {
  return att_loss_bwd(gout, colsum, B, steps, P, alpha_c, dalphas, S(stream));
}
int capnet_policy_xent_fwd(const float* logits, long ld, int N, int V, const long long* targets,
                           const float* advantages, int B, const int* batch_sizes, int steps, float* lse,
                           float* row_logp, float* caption_logp, float* loss, int* err_flag, capnet_stream_t stream) {
  return policy_xent_fwd(logits, ld, N, V, targets, advantages, B, batch_sizes, steps, lse, row_logp, caption_logp, loss,
                         err_flag, S(stream));
}
int capnet_policy_xent_bwd(const float* logits, long ld, int N, int V, const long long* targets, const float* lse,
                           const float* advantages, int B, const int* batch_sizes, int steps, const float* grad_out,
                           float* dlogits, long ldd, capnet_stream_t stream) {
  return policy_xent_bwd(logits, ld, N, V, targets, lse, advantages, B, batch_sizes, steps, grad_out, dlogits, ldd,
                         S(stream));
}

int capnet_bleu_rows(const long long* ids, long ld, int rows, int steps, long long start_token, long long end_token,
                     int per_image, const int* refs, const int* ref_len, int images, int R, int Lr, const double* weights,
                     int smooth, float* reward, int* stats, capnet_stream_t stream) {
  CAPNET_REQUIRE((size_t)ids % 8 == 0 && (size_t)refs % 4 == 0 && (size_t)ref_len % 4 == 0 && (size_t)reward % 4 == 0 &&
                     (size_t)stats % 4 == 0,
                 "bleu_rows: alignment");
  return bleu_rows(ids, ld, rows, steps, start_token, end_token, per_image, refs, ref_len, images, R, Lr, weights, smooth, reward,
                   stats, S(stream));
}
int capnet_cider_rows(const long long* ids, long ld, int rows, int steps, long long start_token, long long end_token,
                      int per_image, const int* refs, const int* ref_len, const double* ref_norm, int images, int R, int Lr,
                      const int* const* keys, const double* const* idf, const int* counts, double log_n, double sigma,
                      float* reward, double* parts, int* stats, capnet_stream_t stream) {
  CAPNET_REQUIRE(keys && idf && counts, "cider_rows: null argument");
  bool aligned = (size_t)ids % 8 == 0 && (size_t)refs % 4 == 0 && (size_t)ref_len % 4 == 0 && (size_t)ref_norm % 8 == 0 &&
                 (size_t)reward % 4 == 0 && (size_t)parts % 8 == 0 && (size_t)stats % 4 == 0;
  for (int n = 0; n < 4; ++n) aligned = aligned && (size_t)keys[n] % 4 == 0 && (size_t)idf[n] % 8 == 0;
  CAPNET_REQUIRE(aligned, "cider_rows: alignment");
  return cider_rows(ids, ld, rows, steps, start_token, end_token, per_image, refs, ref_len, ref_norm, images, R, Lr, keys, idf,
                    counts, log_n, sigma, reward, parts, stats, S(stream));
}

int capnet_clamp_adam(int n, float* const* params, float* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, const long* numel, const int* step, float lr,
                      float beta1, float beta2, float eps, float clip, int write_grad,
                      const int* skip_flag, capnet_stream_t stream) {
  return clamp_adam(n, params, grads, exp_avg, exp_avg_sq, numel, step, lr, beta1, beta2, eps, clip,
                    write_grad, skip_flag, S(stream));
}

int capnet_trunk_set_timing(capnet_trunk_t* t, int enable) {
  return trunk_set_timing(reinterpret_cast<Trunk*>(t), enable);
}
int capnet_trunk_time_next_pass(capnet_trunk_t* t) { return trunk_time_next_pass(reinterpret_cast<Trunk*>(t)); }
int capnet_trunk_collect_timing(capnet_trunk_t* t, double* conv_ms, long* conv_launches,
                                double* conv_flops) {
  return trunk_collect_timing(reinterpret_cast<Trunk*>(t), conv_ms, conv_launches, conv_flops);
}

int capnet_packed_targets(const long long* captions, int T, int steps, const int* batch_sizes,
                          long long* out, capnet_stream_t stream) {
  CAPNET_REQUIRE(batch_sizes && steps > 0 && steps <= kMaxSteps, "packed_targets: steps %d", steps);
  SeqMeta m;
  m.steps = steps; m.has_features = 0; m.off[0] = 0;
  for (int t = 0; t < steps; ++t) {
    CAPNET_REQUIRE(batch_sizes[t] > 0, "packed_targets: batch_sizes[%d]", t);
    m.off[t + 1] = m.off[t] + batch_sizes[t];
    m.tf[t] = 1;
  }
  m.N = m.off[steps];
  return packed_targets(m, captions, T, out, S(stream));
}

int capnet_pack_tensors(int n, float* const* tensors, const long* numel, float* flat,
                        int direction, float scale, capnet_stream_t stream) {
  return pack_tensors(n, tensors, numel, flat, direction, scale, S(stream));
}

size_t capnet_fused_block_weight_words(int C, int MID, int role) { return fused_block_weight_words(C, MID, role); }
int capnet_fused_block_pack(const float* w, unsigned* img, int C, int MID, int role, capnet_stream_t stream) {
  return fused_block_pack(w, img, C, MID, role, S(stream));
}
size_t capnet_fused_block_stats_floats(long M, int MID) { return fused_block_stats_floats(M, MID); }
int capnet_fused_block_stats(const float* y2, const float* s2, const float* t2, const unsigned* w3img, long M, int MID,
                             int in_exp, const float* gamma, const float* beta, float* running_mean, float* running_var,
                             float momentum, float eps, float* scale, float* shift, float* work, int* err_flag,
                             capnet_stream_t stream) {
  return fused_block_stats(y2, s2, t2, w3img, M, MID, in_exp, gamma, beta, running_mean, running_var, momentum, eps, scale,
                           shift, nullptr, nullptr, work, err_flag, S(stream));
}
int capnet_fused_block_tiles(long M, int MID) { return fused_block_tiles(M, MID); }
int capnet_fused_block_forward(const float* y2, const float* s2, const float* t2, const unsigned* w3img, const float* s3,
                               const float* t3, const float* res, const float* sd, const float* td, float* out,
                               const unsigned* w1img, float* y1, float* part_sum, float* part_sq, long M, int MID, int e3,
                               int e1, int* err_flag, capnet_stream_t stream) {
  return fused_block_forward(y2, s2, t2, w3img, s3, t3, res, sd, td, out, w1img, y1, part_sum, part_sq, M, MID, e3, e1,
                             err_flag, S(stream));
}

int capnet_comm_unique_id(void* id128) { return comm_unique_id(id128); }
int capnet_comm_create(const void* id128, int rank, int world, capnet_comm_t** out) {
  return comm_create(id128, rank, world, reinterpret_cast<Comm**>(out));
}
int capnet_comm_destroy(capnet_comm_t* comm) { return comm_destroy(reinterpret_cast<Comm*>(comm)); }
int capnet_allreduce_grads(capnet_comm_t* comm, float* flat, long count, capnet_stream_t stream) {
  return allreduce_grads(reinterpret_cast<Comm*>(comm), flat, count, S(stream));
}

int capnet_err_word_exchange(int* err_flag, float* slot, int direction, capnet_stream_t stream) {
  return err_word_exchange(err_flag, slot, direction, S(stream));
}

int capnet_count_skipped(const int* err_flag, int* counter, capnet_stream_t stream) {
  return count_skipped(err_flag, counter, S(stream));
}

int capnet_clamp(float* x, long n, float lo, float hi, capnet_stream_t stream) {
  return clamp_inplace(x, n, lo, hi, S(stream));
}

}  // extern "C"
