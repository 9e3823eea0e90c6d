// Internal C++ entry points of libcapnet_hip (one per kernel family). The extern "C"
// boundary in capi.cpp forwards to these; nothing here allocates or synchronises.
#pragma once
#include <hip/hip_runtime.h>

namespace capnet {

// gemm_f32.hip
int sgemm(bool ta, bool tb, int M, int N, int K, const float* A, long lda, const float* B,
          long ldb, float* C, long ldc, const float* bias, int accumulate, int batch, long sA,
          long sB, long sC, long sBias, int force_tile, hipStream_t stream);

// gemm_b3.hip: the same product on the bf16 matrix cores, three bf16 pieces per fp32 operand and six products per multiply
// (fp32-grade, fp32's range); sgemm takes it by itself for large products
bool sgemm_b3_eligible(bool ta, bool tb, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                       const float* C, long ldc, const float* bias, int batch, long sA, long sB, long sC, long sBias);
int sgemm_b3(bool ta, bool tb, int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
             const float* bias, int accumulate, int batch, long sA, long sB, long sC, long sBias, hipStream_t stream,
             float* ws = nullptr, size_t ws_floats = 0);

// Which kernel a product is given (CAPNET_ROUTE_* of capnet.h). The two plan functions are host code: they make every
// choice of sgemm / sgemm_splitk_batched -- the launch code consumes the plan -- and look at pointers for null and
// alignment only.
enum Route : int {
  kRouteNone = 0,            // an empty product: nothing is launched
  kRouteGeneric64 = 1, kRouteGeneric128 = 2, kRouteGeneric6432 = 3,   // gemm_f32_kernel's k-loop at that tile
  kRouteNtDma = 4, kRouteB3 = 5, kRouteRows16 = 6, kRouteSkinny64 = 7, kRouteSkinny128 = 8,
  kRouteKloopSplitk = 9,     // gemm_f32_kernel over K slabs + reduce_slabs
  kRouteB3Splitk = 10,       // gemm_b3_kernel over K slabs + reduce_slabs
  kRouteFellThrough = 64,    // sgemm_splitk_batched handed the product to sgemm, whose route is SplitkPlan::inner
};
struct SgemmPlan {
  int route;
  bool vec;                  // the generic kernel's loader form (16-B loads); true for nt_dma and b3
  int tiles_m, tiles_n;
};
struct SplitkPlan {
  int route;
  bool vec;                  // k-loop split-K: the loader form; the other split-K kernels load 16 B
  int splits;                // slabs of K
  int chunk;                 // rows16: 256-k chunks per workgroup (sub); skinny: kc; k-loop / b3 split-K: k per slab
  int tiles;                 // output tiles (rows16: 64-column tiles of one member)
  SgemmPlan inner;           // kRouteFellThrough
};
int sgemm_plan(bool ta, bool tb, int M, int N, int K, const float* A, long lda, const float* B, long ldb, const float* C,
               long ldc, const float* bias, int accumulate, int batch, long sA, long sB, long sC, long sBias,
               int force_tile, SgemmPlan* p);
int sgemm_splitk_plan(bool ta, bool tb, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                      const float* C, long ldc, const float* bias, int accumulate, int batch, long sA, long sB, long sC,
                      long sBias, const float* ws, size_t ws_floats, const int* counters, size_t n_counters,
                      bool allow_rows16, SplitkPlan* p);
// gemm_b3.hip's own cut of K (splits = 1 without a workspace) and its 128 x 128 tile count
void sgemm_b3_plan(int M, int N, int K, int batch, const float* ws, size_t ws_floats, int* splits, int* steps_per_split,
                   int* tiles);

// counters (optional): n_counters ints, zero before the first use and left zero by every call -- one per 64-column
// output tile and batch member; with them, products of M <= 16 rows are ONE launch (gemm_rows16_kernel: the
// workgroup that arrives last at a tile sums the K-chunk partials)
constexpr size_t kSplitKCounters = 1024;
int sgemm_splitk(bool ta, bool tb, int M, int N, int K, const float* A, long lda, const float* B,
                 long ldb, float* C, long ldc, const float* bias, int accumulate, float* ws,
                 size_t ws_floats, hipStream_t stream, int* counters = nullptr, size_t n_counters = 0);
int sgemm_splitk_slabs(bool tb, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                       float* ws, size_t ws_floats, int* n_slabs, hipStream_t stream);
int sgemm_rows16_slabs(bool tb, int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* ws,
                       size_t ws_floats, int* n_slabs, hipStream_t stream);
int sgemm_splitk_batched(bool ta, bool tb, int M, int N, int K, const float* A, long lda,
                         const float* B, long ldb, float* C, long ldc, const float* bias,
                         int accumulate, int batch, long sA, long sB, long sC, long sBias, float* ws,
                         size_t ws_floats, hipStream_t stream, int* counters = nullptr, size_t n_counters = 0);

// conv_f32.hip
int conv2d_fwd(const float* x, long sxb, long sxh, long sxw, long sxc, const float* w_packed,
               int Kw, float* y, const float* in_scale, const float* in_shift, int relu_in,
               float* part_sum, float* part_sq, int Bn, int H, int W, int Cin, int Cout, int KH,
               int KW, int stride, int pad, int tile, hipStream_t stream);
int conv_auto_tile(int M, int Cout);
// conv_f32_v2.hip (weights packed K-major [Kw][Cout])
bool conv_v2_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int Bn, int Cin,
                      int Cout, const float* in_scale, const float* in_shift);
int conv2d_fwd_v2(const float* x, long sxb, long sxh, long sxw, const float* wk, int Kw, float* y,
                  const float* in_scale, const float* in_shift, int relu_in, float* part_sum,
                  float* part_sq, int Bn, int H, int W, int Cin, int Cout, int KH, int KW,
                  int stride, int pad, int tile, float* slabs, hipStream_t stream,
                  const float* out_scale = nullptr, const float* out_shift = nullptr,
                  const float* res = nullptr, int relu_out = 0);
size_t conv_v2_slab_floats(int M, int Cout, int Kw, int tile);
int conv_v2_auto_tile(int M, int Cout, int Kw);
void conv_v2_plan(int M, int Cout, int Kw, int tile, int* out);
int conv_tiles_m(int M, int tile);
// gemm_dma.hip: C = A . B^T with both operands K-contiguous, LDS-DMA staging (1x1 convs, vocabulary projection)
bool sgemm_nt_dma_eligible(int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                           const float* C, long ldc);
int sgemm_nt_dma(int M, int N, int K, const float* A, long lda, const float* B, float* C,
                 const float* bias, hipStream_t stream);
bool conv1x1_dma_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int Bn, int H, int W,
                          int Cin, int Cout, int stride);
int conv1x1_tiles_m(long M);
int conv1x1_fwd_dma(const float* x, long sxb, long sxh, long sxw, const float* w_oi, float* y,
                    float* part_sum, float* part_sq, int Bn, int H, int W, int Cin, int Cout, int stride,
                    hipStream_t stream, const float* out_scale = nullptr, const float* out_shift = nullptr,
                    const float* res = nullptr, int relu_out = 0);

// conv_f16x3.hip: 1x1 convolution as three f16 MFMA products of 2-way split, power-of-two scaled fp32 operands
// (fp32-grade results; the default for Cin % 64 == 0)
bool conv1x1_f16x3_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int Bn, int H, int W,
                            int Cin, int Cout, int stride, const float* in_scale, const float* in_shift);
int conv1x1_f16x3_bn(long M, int Cout);
// ... and the 3x3 (pad 1) convolutions as an implicit GEMM over (tap, channel) in the same kernel: k = 1 or 3
bool conv_f16x3_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int Bn, int H, int W, int Cin,
                         int Cout, int k, int stride, int pad, const float* in_scale, const float* in_shift);
size_t conv_f16x3_weight_words(int Cin, int Cout, int k);
// first step of every split-f16 weight pack (conv_f16x3_pack, fused_block_pack, conv_stem_f16x3_pack): zeroes the image
// header (split_f16.h) and leaves the bits of max |w| over the n weights in its word 1 for the layout kernel that follows
int f16x3_pack_header(const float* w, unsigned* img, long n, hipStream_t stream);
int conv_f16x3_pack(const float* w_oihw, unsigned* img, int Cout, int Cin, int k, int bn, hipStream_t stream);
int conv_fwd_f16x3(const float* x, long sxb, long sxh, long sxw, const unsigned* wimg, int bn, float* y,
                   const float* in_scale, const float* in_shift, int relu_in, float* part_sum, float* part_sq, int Bn,
                   int H, int W, int Cin, int Cout, int k, int stride, int pad, hipStream_t stream,
                   const float* out_scale = nullptr, const float* out_shift = nullptr, const float* res = nullptr,
                   int relu_out = 0, int in_exp = 0, int* err = nullptr);
// (in_exp, here and below: the input is multiplied by 2^in_exp on its way into the f16 planes -- folded into the
//  BatchNorm's scale / shift where there is one -- and the accumulators by 2^-in_exp: exact, and what keeps the split
//  operands inside f16's range whatever the scale of the tensor; chosen per tensor by the trunk)
// The stem (7x7 stride 2 pad 3, 3 -> 64 channels, NCHW image in, NHWC out) on the same split-f16 arithmetic
// (conv_stem.hip); statistics partials: one row per workgroup
bool conv_stem_f16x3_eligible(const float* x, long sxb, long sxc, long sxh, long sxw, int Bn, int H, int W, int Cin,
                              int Cout, int k, int stride, int pad);
size_t conv_stem_f16x3_weight_words();
int conv_stem_f16x3_part_rows(int Bn, int H, int W);
int conv_stem_f16x3_pack(const float* w_oihw, unsigned* img, hipStream_t stream);
int conv_stem_fwd_f16x3(const float* x, long sxb, long sxc, long sxh, const unsigned* wimg, float* y, float* part_sum,
                        float* part_sq, int Bn, int H, int W, hipStream_t stream, int in_exp = 0, int* err = nullptr);
// ... and the stride-1 3x3 ones with the tile's input patch resident in LDS (conv3x3_patch.hip): same weight image,
// tile width and statistics rows as conv_fwd_f16x3; dense NHWC input
bool conv3x3_patch_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int Bn, int H, int W, int Cin,
                            int Cout, int k, int stride, int pad, const float* in_scale, const float* in_shift);
int conv3x3_fwd_patch(const float* x, const unsigned* wimg, int bn, float* y, const float* in_scale, const float* in_shift,
                      int relu_in, float* part_sum, float* part_sq, int Bn, int H, int W, int Cin, int Cout,
                      hipStream_t stream, bool shared_chip = false, int in_exp = 0, int* err = nullptr);
// Stride-1 1x1 convolutions with Cin = 64 / 128 / 256 (conv3 of stages 1-3) with the A operand resident in registers
// (conv1x1_areg.hip): dense [M][Cin] input, same weight image, tile width and statistics rows as conv_fwd_f16x3
bool conv1x1_areg_eligible(const float* x, long M, int Cin, int Cout, int bn, const float* in_scale, const float* in_shift);
int conv1x1_fwd_areg(const float* x, const unsigned* wimg, int bn, float* y, const float* in_scale, const float* in_shift,
                     int relu_in, float* part_sum, float* part_sq, long M, int Cin, int Cout, int in_exp, hipStream_t stream,
                     int* err = nullptr);
// A bottleneck block's tail (bn_add_relu) fused into the next block's stride-1 1x1 conv1 (conv3x3_patch.hip)
bool conv1x1_tail_eligible(const float* y3, const float* res, long M, int Cin, int Cout);
int conv1x1_fwd_tail(const float* y3, const float* s1, const float* t1, const float* res, const float* s2, const float* t2,
                     float* tail_out, const unsigned* wimg, int bn, float* y, float* part_sum, float* part_sq, long M,
                     int Cin, int Cout, hipStream_t stream, int in_exp = 0, int* err = nullptr);
size_t conv1x1_f16x3_weight_words(int Cin, int Cout);
int conv1x1_f16x3_pack(const float* w, unsigned* img, int Cout, int Cin, int bn, hipStream_t stream);
int conv1x1_fwd_f16x3(const float* x, long sxb, long sxh, long sxw, const unsigned* wimg, int bn, float* y,
                      const float* in_scale, const float* in_shift, int relu_in, float* part_sum,
                      float* part_sq, int Bn, int H, int W, int Cin, int Cout, int stride,
                      hipStream_t stream, const float* out_scale = nullptr, const float* out_shift = nullptr,
                      const float* res = nullptr, int relu_out = 0);

// bn_pool.hip
int bn_finalize(const float* part_sum, const float* part_sq, int tiles, int C, long count,
                const float* gamma, const float* beta, float* running_mean, float* running_var,
                float momentum, float eps, float* scale, float* shift, hipStream_t stream,
                float* batch_mean = nullptr, float* batch_var = nullptr, int* err = nullptr);
int bn_eval_scale_shift(const float* gamma, const float* beta, const float* rm, const float* rv,
                        float eps, int C, float* scale, float* shift, hipStream_t stream);
int bn_running_update_multi(int n, const float* const* mean, const float* const* var, float* const* rm,
                            float* const* rv, const int* C, float momentum, hipStream_t stream);
int bn_eval_multi(int n, const float* const* gamma, const float* const* beta, const float* const* rm,
                  const float* const* rv, const int* C, float* const* scale, float* const* shift,
                  float eps, hipStream_t stream);
int bn_add_relu(const float* y, const float* s1, const float* t1, const float* res,
                const float* s2, const float* t2, float* out, long rows, int C,
                hipStream_t stream);
int bn_relu_maxpool(const float* y, const float* scale, const float* shift, float* out, int Bn,
                    int H, int W, int C, hipStream_t stream);
int global_avgpool(const float* x, float* out, int Bn, int HW, int C, hipStream_t stream, int* err = nullptr);
int adaptive_pool_replicate(const float* x, float* out, int Bn, int S, int OUT, int C,
                            hipStream_t stream);
int pack_conv_weight_kmajor(const float* w_oihw, float* out, int Cout, int Cin, int KH, int KW,
                            int Kw, hipStream_t stream);
int pack_conv_weight(const float* w_oihw, float* out, int Cout, int Cin, int KH, int KW, int Kw,
                     hipStream_t stream);

// trunk.cpp
struct Trunk;
int trunk_create(int B, int H, int W, Trunk** out);
void trunk_destroy(Trunk* t);
size_t trunk_workspace_bytes(const Trunk* t);
int trunk_num_convs(const Trunk* t);
int trunk_final_side(const Trunk* t);
int trunk_conv_shape(const Trunk* t, int i, int* cout, int* cin, int* k, int* stride, int* kw);
int trunk_conv_kmajor(const Trunk* t, int i);
int trunk_conv_tile_n(const Trunk* t, int i);
double trunk_flops(const Trunk* t);
double trunk_conv_flops(const Trunk* t, int i);
int trunk_set_timing(Trunk* t, int enable);
int trunk_time_next_pass(Trunk* t);
int trunk_collect_timing(Trunk* t, double* conv_ms, long* conv_launches, double* conv_flops);
int trunk_set_tail_balance(Trunk* t, int on);
int trunk_update_running(Trunk* t, const float* workspace, float* const* bn_rmean, float* const* bn_rvar,
                         float momentum, hipStream_t stream);
int trunk_forward(Trunk* t, const float* images_nchw, const float* const* w_packed,
                  const float* const* bn_gamma, const float* const* bn_beta,
                  float* const* bn_rmean, float* const* bn_rvar, int train, float momentum,
                  float eps, float* workspace, float* out_pooled, float* out_map,
                  const int* in_exps, int* err_flag, hipStream_t stream);

// seq_kernels.hip
constexpr int kMaxSteps = 128;
struct SeqMeta {
  int N, steps, has_features;
  int off[kMaxSteps + 1];
  unsigned char tf[kMaxSteps];
};
int build_rows(const SeqMeta& m, int* row_sample, int* row_col, int* row_token, int* prev_row,
               hipStream_t stream);
int gather_inputs(const long long* captions, int T, const float* features, const float* emb, int E,
                  int V, const int* row_sample, const int* row_col, int* row_token, float* X,
                  long ldx, int r0, int r1, float p, unsigned long long seed, int use_dropout,
                  int dynamic, int* err_flag, hipStream_t stream);
int embedding_fwd(const long long* idx, int n, const float* emb, int E, int V, float* out,
                  int* err_flag, hipStream_t stream);
int packed_targets(const SeqMeta& m, const long long* captions, int T, long long* out,
                   hipStream_t stream);
// dst[i] = src[i] (+ src2[i] where given), up to 40 items in one launch
struct CopyTable {
  static constexpr int kMax = 40;
  const float* src[kMax];
  const float* src2[kMax];
  float* dst[kMax];
  size_t n[kMax];
  int count = 0;
  void add(float* d, const float* a, size_t len, const float* b = nullptr) {
    if (count < kMax) { src[count] = a; src2[count] = b; dst[count] = d; n[count] = len; }
    ++count;      // (an overflow is caught by multi_copy)
  }
};
int multi_copy(const CopyTable& t, hipStream_t stream);
// (slabs: n_slabs partial products [k][b][4H] still to be added to `pre`, in slab order -- sgemm_rows16_slabs)
int lstm_pointwise_fwd(float* pre, long ldp, const float* c_prev, float* c_out, float* h_out, int b,
                       int H, int gi, int gf, int go, int gg, int tanh_out, hipStream_t stream,
                       const float* slabs = nullptr, int n_slabs = 0);
int lstm_pointwise_bwd(const float* gates, long ldg, const float* c, const float* c_prev,
                       const float* dH, const float* dh_rec, float* dc_io, float* dpre, long ldq,
                       int b, int b_next, int H, int gi, int gf, int go, int gg, int tanh_out,
                       hipStream_t stream, int dh_slabs = 0, long dh_slab_stride = 0);
int gather_prev_rows(const float* src, const int* idx, const float* first, const int* sample,
                     float* out, int rows, int C, hipStream_t stream);
int argmax_rows(const float* x, int rows, int ld, int V, int* out, hipStream_t stream);
// ---- beam_search.hip: the selection step of beam search
int beam_topk(const float* logits, long ld, int rows, int V, const float* prev, int k,
              float* out_scores, long long* out_index, hipStream_t stream);
// (bans int32 [rows][1 + cap] on the device, per logits row its count and that many words)
int beam_topk_banned(float* logits, long ld, int rows, int V, const float* prev, int k, const int* bans, int cap,
                     float* out_scores, long long* out_index, hipStream_t stream);
// beam search with device-side bookkeeping (fixed slots: image i's beams at rows i k .. i k + k - 1 throughout)
size_t beam_state_bytes(int n, int k, int max_steps);
int beam_init(void* beam, int n, int k, int max_steps, long long start_token, long long* prev_words, hipStream_t stream);
// constrained search: what a step must not select -- no g-gram twice in a hypothesis (0: off, at most 4), no
// <end> at steps 1 .. min_words, none of the n_banned (<= 32) words of the DEVICE array banned. The excluded words are
// overwritten with -inf in the logits block AFTER the rows' log-sum-exp: the block is modified, the scores are not.
struct BeamConstraints {
  int no_repeat_ngram, min_words;
  const int* banned;
  int n_banned;
  // forced words: n_forced (<= 4) distinct ids of the DEVICE array forced that every completed hypothesis must
  // contain; 0: none. <end> is excluded on a row that lacks a forced id, and the `live` candidates are dealt out of a pool (the
  // plain selection, every row's missing forced ids, every row's best word) across banks by met count, F, F - 1 .. 0, F ..;
  // the scores are the plain ones.
  const int* forced = nullptr;
  int n_forced = 0;
  // per-image rules: a DEVICE int32 table [n][kBeamRuleWords], row i the rule of image i -- word 0
  // no_repeat_ngram, 1 min_words, 2 n_banned, 3 n_forced, 4 .. 35 banned, 36 .. 39 forced; a row of zeros: no rule. Set: the
  // fields above are not read, and every workgroup takes its own row, each count clamped to its range as it is read.
  const int* rules = nullptr;
};
constexpr int kBeamRuleWords = 40;
// diverse search: n images x k beams as `teams` teams of k / teams. Team g of an image selects after teams
// 0 .. g - 1 by score - strength * (candidates they chose at this step with the same word); the scores written are
// unpenalised. (beam: the one-call searches' -- the block that holds the state of n teams searches of k / teams beams)
struct BeamTeams {
  int teams;
  float strength;
  void* beam;
};
int beam_constraints_check(const char* who, const BeamConstraints& c);
int beam_forced_check(const char* who, const BeamConstraints& c);                  // (refuses n_forced == 0)
int beam_rules_check(const char* who, const int* rules);                          // (non-null, 16-byte aligned)
int beam_teams_check(const char* who, int k, int teams, float strength);          // (the only check of either range)
// One step on the device state, and the same selection in the host loops' form. con / bans, teams, forced ids and trace are
// each nullable (0), and WHICH are given chooses the kernel: con->rules without teams -> the per-image kernel, which takes
// each image's branch from its row (rules in the host loops' form: met is required, bans optional, forced / n_forced
// unread); teams -> diverse (its constraints and ban lists optional); else forced ids -> forced; else con / bans -> constrained; else plain, which leaves the logits block as it is (every
// other kernel modifies it). With teams, beam and trace are those of n teams searches of k / teams beams and meta is
// [n teams][3] per (image, team). who: the caller's name, in front of every message.
int beam_advance(const char* who, void* beam, float* logits, long ld, int V, int n, int k, int max_steps, int step,
                 long long end_token, const BeamConstraints* con, const BeamTeams* teams, long long* next_words,
                 long long* parent_rows, void* trace, hipStream_t stream);
// (met int32 per logits row, bit f: forced[f] is among the row's words)
int beam_topk_batched(const char* who, float* logits, long ld, int V, const float* prev, const int* meta, int n, const int* bans,
                      int cap, const BeamTeams* teams, const int* met, const int* forced, int n_forced, long long end_token,
                      float* out_scores, long long* out_index, hipStream_t stream, const int* rules = nullptr);
// (trace, optional, beam_trace_bytes: the row history of every hypothesis beside the state -- rows[2][n][k][L] |
// done_rows[n][k][L] int32, entry e = the slot whose step-e attention preceded word e; beam_finish then also writes the
// winner's rows [n][max_steps] as decoder-step rows i k + slot, -1 past length - 1)
size_t beam_trace_bytes(int n, int k, int max_steps);
// (beam_advance on a step's k best logits per row and the rows' log-sum-exp, vocab_topk's outputs, instead of its logits)
int beam_advance_topk(void* beam, const float* values, const int* index, const float* lse, int V, int n, int k, int max_steps,
                      int step, long long end_token, long long* next_words, long long* parent_rows, hipStream_t stream);
int beam_finish(const void* beam, int n, int k, int max_steps, long long end_token, long long* seqs, int* lengths,
                hipStream_t stream, const void* trace = nullptr, int* rows = nullptr);
// every completed hypothesis of every image, best first by done_score / (done_len - 1)^length_penalty (penalty 0: by
// done_score itself), ties to the earlier completion: seqs [n][k][max_steps + 2], lengths / scores [n][k], counts [n]; with
// the trace, rows [n][k][max_steps] as beam_finish's, per hypothesis. The state is only read.
int beam_nbest(const void* beam, int n, int k, int max_steps, float length_penalty, long long* seqs, int* lengths,
               float* scores, int* counts, hipStream_t stream, const void* trace = nullptr, int* rows = nullptr);
int beam_live(const void* beam, int n, int k, int max_steps, const int** live_total, const int** live, const float** scores);
// (the [n k] hypotheses step `step` reads: rows of max_steps + 2 int32, `step` tokens each, <start> first)
int beam_tokens(const void* beam, int n, int k, int max_steps, int step, const int** tokens);
// ---- seq_kernels.hip again
int gather_rows(const float* src, const int* idx, float* out, int rows, int C, hipStream_t stream);
int colsum(const float* x, long ld, int rows, int C, float* out, int accumulate, hipStream_t stream,
           float* ws = nullptr, size_t ws_floats = 0);
// out[m][n] = sum_k slab[k][m][n] (+ bias[n]) (+ out[m][n]), fixed order (gemm_f32.hip)
int reduce_slabs(const float* slab, int count, int M, int N, float* out, long ldc, const float* bias,
                 int accumulate, hipStream_t stream);
// dst[r][e] = src[r][e] * mask(seed, layer, r, e) / keep for rows [r0, r1) of width C (the dropout between stacked layers;
// use_dropout 0: a copy). The same call maps a gradient back through the mask.
int rows_dropout(const float* src, float* dst, int r0, int r1, int C, float p, unsigned long long seed, int layer,
                 int use_dropout, hipStream_t stream);
int scatter_input_grad(const float* dX, long ldx, int N, int E, const int* row_sample, const int* row_col,
                       const int* row_token, float* dEmb, float* dFeat, int V, float p,
                       unsigned long long seed, int use_dropout, hipStream_t stream, int* tables, size_t table_ints);

// lstm_step.hip
bool lstm_step_fused_supported(int b, int H);
// the instance and grid lstm_step_fused launches at (b, H): k groups per wave (H padded to 64 ngw), 16-row tiles per
// workgroup, row halves, and whether workgroup ids are dealt XCD-major (H / 4 unit groups a multiple of 8). Host only.
struct StepFusedRoute { int ngw, mt, halves, xcd_map; };
bool lstm_step_fused_route(int b, int H, StepFusedRoute* r);   // false: lstm_step_fused refuses (b, H)
size_t lstm_wfrag_floats(int H);
int lstm_pack_wfrag(const float* Wcat, float* Wfrag, int H, int gi, int gf, int go, int gg,
                    hipStream_t stream);
int lstm_step_fused(const float* hprev, const float* Wfrag, float* G, long ldg, const float* cprev,
                    float* c_out, float* h_out, int b, int H, int gi, int gf, int go, int gg,
                    int tanh_out, hipStream_t stream, unsigned long long* stamps = nullptr);

// lstm_upper_step.hip: one step of a stacked layer above the first (<= 16 rows): dropout of the layer below's rows, the
// collapsed chain and the recurrent product as one product, the gates -- one launch. cell: 0 = the factored cell (Weff =
// the collapsed chain), 1 = nn.LSTMCell (Weff = weight_ih, gate blocks i, f, g, o, h = o tanh(c))
bool lstm_upper_step_supported(int b, int H);
int lstm_upper_step(const float* xin, const float* hprev, const float* cprev, const float* Weff, const float* Wrec,
                    const float* beff, float* x_out, float* G, float* c_out, float* h_out, int b, int H, int r0, float p,
                    unsigned long long seed, int layer, int use_dropout, hipStream_t stream, int cell = 0);

// lstm_decode_step.hip: one inference step of every layer of a stacked LSTM (beam search), one launch per layer, any
// number of rows: [x | h] . [Weff | W]^T + beff and the gates (blocks i, f, o, c~); layer 0 gathers its embedding rows by
// token id. cell 0: the factored cell, h = o c; cell 1: nn.LSTMCell, h = o tanh(c). parent_rows (int64 [rows], optional): row
// r reads its previous h and c at row parent_rows[r] of state_in (a beam search's re-ordering, read in place)
bool stacked_decode_supported(int E, int H);
int stacked_decode_step(int cell, int nlayers, int rows, int E, int H, int V, const long long* tokens, const float* x,
                        const float* const* wcat, const float* const* beff, const float* state_in, float* state_out,
                        float* h_top, int* err_flag, hipStream_t stream, const long long* parent_rows = nullptr, int groups = 1,
                        const float* const* tables = nullptr);
// (groups: `rows` = groups x rows per group, group-major; wcat[l] [groups][4H][kin + H], beff[l] [groups][4H]; tables:
// `groups` host-side pointers, group g gathers its token rows from tables[g] [V][E] instead of x -- no table is copied)
// the same kernels' family for layer 0 of an attention decoder, kin + H up to 4096 (x rows of E % 4 == 0 columns, 16-B aligned)
bool stacked_decode_wide_supported(int E, int H);
// the kernel a layer of kin (a multiple of 16) input columns runs on: lstm_decode_step_kernel<nj, tm> or, wide,
// lstm_decode_step_wide_kernel<nj> (two 16-row tiles per pass); xvec: its x rows take 16-B loads. Host only.
struct DecodeRoute { int wide, nj, tm; };
bool stacked_decode_route(int kin, int H, int xvec, DecodeRoute* r);   // false: the layer is refused (K too large)
// One beam step of an attention decoder without the projection: z = h_prev . [decoder_att; f_beta]^T + bz (sgemm_splitk on
// `slab`), att_beam_step_fwd, layer 0 on xa = [embedding | gated context] (wide or narrow by shape), the upper layers.
// ws: att_decode_step_ws_bytes (z | xa | escore)
bool att_decode_supported(int E, int C, int H, int A, int P, int k, int nlayers);
size_t att_decode_step_ws_bytes(int n, int k, int P, int A, int C, int E);
int att_decode_step(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, const float* att1,
                    const float* feat, const long long* tokens, const float* emb, const float* wz, const float* bz,
                    const float* wf, const float* bf, const float* const* wcat, const float* const* beff,
                    const float* state_in, const long long* parent_rows, float* state_out, float* h_top, void* ws, float* slab,
                    size_t slab_floats, int* err_flag, hipStream_t stream, int groups = 1, float* alphas = nullptr);
// (alphas [groups n k][P], optional: the step's attention maps, att_beam_step_fwd's alpha_out)
// (groups: groups x n beam groups of k rows, group-major; att1 [groups n][P][A], feat [n][P][C], wz / bz / wf / bf and the
// layers' weights with a leading groups dimension; ws: att_decode_step_ws_bytes at groups x n)

// vocab_argmax.hip: tok[r] = first argmax_v (h[r] . W[v] + b[v]) in one launch, no logits in memory (ws: vocab_argmax_ws_bytes,
// its first 16 bytes zero before the first use)
bool vocab_argmax_supported(int H);
size_t vocab_argmax_ws_bytes(int rows, int V);
int vocab_argmax(const float* h, const float* w, const float* b, int rows, int H, int V, void* ws, long long* tok,
                 long long* ids, long ld_ids, hipStream_t stream);
// weight groups: rows = groups x rpg, group-major; group g's rows are projected on w[g] / b[g] (host-side pointer tables,
// b or any b[g] may be null) in the same launch, one arrival counter per group (ws: vocab_argmax_groups_ws_bytes, its first
// 16 groups bytes zero before the first use)
size_t vocab_argmax_groups_ws_bytes(int groups, int rpg, int V);
int vocab_argmax_groups(const float* h, const float* const* w, const float* const* b, int groups, int rpg, int H, int V,
                        void* ws, long long* tok, long long* ids, long ld_ids, hipStream_t stream);
// decode_loops.hip: capnet.seq2seq's greedy `sample` as one chain of launches (per step the decode step and vocab_argmax)
size_t lstm_greedy_decode_ws_bytes(int nlayers, int rows, int H, int V);
size_t lstm_greedy_decode_groups_ws_bytes(int nlayers, int groups, int rpg, int H, int V);
int lstm_greedy_decode_groups(int nlayers, int groups, int rpg, int E, int H, int V, int steps, const float* features,
                              const long long* start_tokens, const float* const* emb, const float* const* wcat,
                              const float* const* beff, const float* const* Cw, const float* const* Cb, const float* state0,
                              void* ws, long long* ids, float* state_out, int* err_flag, hipStream_t s);
// (the greedy loop of `groups` decoders at once: emb / Cw / Cb one pointer per group, wcat[l] / beff[l] with a leading
// groups dimension, rows group-major; features only with one group)
int lstm_greedy_decode(int nlayers, int rows, int E, int H, int V, int steps, const float* features,
                       const long long* start_tokens, const float* emb, const float* const* wcat,
                       const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* ws,
                       long long* ids, float* state_out, int* err_flag, hipStream_t s);
// decode_loops.hip: the beam search of a plain stack as one chain of launches: per step the gathered decode step, the
// vocabulary projection (sgemm_splitk on the caller's slab) and beam_advance; poll_every > 0 reads live_total after every
// such step
size_t beam_decode_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps);
int beam_decode(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                long long end_token, const float* emb, const float* const* wcat, const float* const* beff, const float* Cw,
                const float* Cb, const float* state0, void* ws, float* slab, size_t slab_floats, int poll_every,
                long long* seqs, int* lengths, int* steps_run, int* err_flag, hipStream_t s, int groups = 1,
                const BeamConstraints* con = nullptr, const BeamTeams* teams = nullptr);
// (teams, here and in att_beam_decode: the diverse search -- every step's selection is beam_advance's diverse form on a state of
// n teams searches of k / teams beams, which lies BEHIND the workspace described here (beam_state_bytes(n teams, k / teams,
// max_steps) more bytes; teams->beam is ignored); seqs / lengths then hold n teams winners, one per (image, team))
// (groups: the search over groups x n beam groups, group g on its own weights; ws, seqs, lengths at groups x n)
// (con, here and in att_beam_decode: the constrained search -- every step's selection is beam_advance's constrained form, or
// its forced form where con->n_forced > 0 and there are no teams)
// vocab_topk.hip: per row the k best of h[r] . W[v] + b[v] (logit descending, index ascending; fewer pickable entries: the
// tail is (-inf, -1)) and log sum_v exp, one launch, no logits in memory (ws: vocab_topk_ws_bytes, its first 16 bytes zero
// before the first use)
bool vocab_topk_supported(int H, int k, int V);
size_t vocab_topk_ws_bytes(int rows, int k, int V);
// (mask: sample_exclude.hip's exclusion mask [rows][ceil(V / 32)] or null -- a set bit is not pickable, lse is then over the
// allowed entries; null: the kernel without the mask, bit for bit. select_only (the constrained beam search's): a
// set bit leaves the k best alone -- lse stays the log-sum-exp over EVERY entry, the unmasked launch's bit for bit)
int vocab_topk(const float* h, const float* w, const float* b, int rows, int H, int V, int k, void* ws, float* values,
               int* index, float* lse, hipStream_t stream, const unsigned* mask = nullptr, bool select_only = false);
// weight groups, as vocab_argmax_groups: rows = groups x rpg, group-major; group g's rows on w[g] / b[g] (host-side pointer
// tables, b or any b[g] may be null) in the same launch, one arrival counter and one block of partials per group (ws:
// vocab_topk_groups_ws_bytes, its first 16 groups bytes zero before the first use); outputs [groups rpg][k] / [groups rpg]
size_t vocab_topk_groups_ws_bytes(int groups, int rpg, int k, int V);
int vocab_topk_groups(const float* h, const float* const* w, const float* const* b, int groups, int rpg, int H, int V, int k,
                      void* ws, float* values, int* index, float* lse, hipStream_t stream, const unsigned* mask = nullptr,
                      bool select_only = false);
// vocab_sample.hip: per row a draw from softmax((h[r] . W + b) inv_T) by Gumbel-max on sample_rng.h's stream keyed (seed,
// step, row0 + r, v), one launch, no logits in memory: tok[r] / ids[r ld] the token, logp[r ld] its log-probability (each
// optional; ws: vocab_sample_ws_bytes, its first 16 bytes zero before the first use). sample_pick: the same draw among
// vocab_topk's k candidates (logp renormalised over them); sample_rows: from a logits block in memory. greedy_stride (here,
// in vocab_nucleus.hip and in the sampling loops): sample_key.h's vs_row_key -- g > 0: every g-th row is a greedy row (the
// argmax, no noise) and the drawn rows keep the noise rows of the decode without them; 0: off
bool vocab_sample_supported(int H);
float sample_uniform_host(unsigned long long seed, unsigned step, unsigned row, unsigned v);
size_t vocab_sample_ws_bytes(int rows, int V);
int vocab_sample(const float* h, const float* w, const float* b, int rows, int H, int V, float inv_T, unsigned long long seed,
                 unsigned step, unsigned row0, void* ws, long long* tok, long long* ids, float* logp, long ld,
                 hipStream_t stream, unsigned greedy_stride = 0, const unsigned* mask = nullptr);   // (mask: as vocab_topk's)
int sample_pick(const float* values, const int* index, int rows, int k, int V, float inv_T, unsigned long long seed,
                unsigned step, unsigned row0, long long* tok, long long* ids, float* logp, long ld, hipStream_t stream,
                unsigned greedy_stride = 0);
int sample_rows(const float* logits, int rows, long ld_logits, int V, float inv_T, unsigned long long seed, unsigned step,
                unsigned row0, long long* tok, long long* ids, float* logp, long ld, hipStream_t stream, unsigned greedy_stride = 0);
// sample_exclude.hip: what a sampled row may not draw (capnet.beam.banned_words on [start, the row's words so far], the same
// rule as BeamConstraints' without forced words), as a bit mask [rows][sample_mask_words(V)]: bit v & 31 of word v >> 5 set =
// word v excluded on that launch row. `mask` is left null by the callers of the loops: sample_loop places it behind their workspace
struct SampleExcl {
  long long end_token;
  int no_repeat_ngram, min_words;
  const int* banned;   // device array
  int n_banned;
  unsigned* mask;
};
static inline int sample_mask_words(int V) { return (V + 31) / 32; }
size_t sample_mask_bytes(int rows, int V);           // 16-B aligned
int sample_excl_check(const char* who, const SampleExcl& c);
// the mask of stream step t: ids[r ld + 0 .. t - 1] the row's words so far, start_tokens[r] its <start> (null: none)
int sample_exclusion_mask(const long long* ids, long ld, const long long* start_tokens, int rows, int t, int V,
                          const SampleExcl& c, unsigned* mask, hipStream_t stream);
// the same mask of the [n k] rows of a device beam search at step `step` (1-based), from the hypotheses in its state (c's
// forced words are not the mask's: a forced search selects from logits)
int beam_exclusion_mask(const void* beam, int n, int k, int max_steps, int step, int V, long long end_token,
                        const BeamConstraints& c, unsigned* mask, hipStream_t stream);
// -inf at the mask's set bits of logits [rows][ld]
int mask_logits(float* logits, int rows, long ld, int V, const unsigned* mask, hipStream_t stream);
// vocab_nucleus.hip: nucleus (top-p) sampling, 0 < top_p < 1: sample_rows' / sample_pick's draw among the smallest set of
// best entries whose probability reaches top_p, logp renormalised over that set. nucleus_rows: one workgroup per row finds the
// set's edge by an exact search (any V up to 2^24); nucleus_pick: among vocab_topk's k candidates (top_k first, then top_p)
int nucleus_rows(const float* logits, int rows, long ld_logits, int V, float inv_T, float top_p, unsigned long long seed,
                 unsigned step, unsigned row0, long long* tok, long long* ids, float* logp, long ld, hipStream_t stream,
                 unsigned greedy_stride = 0);
int nucleus_pick(const float* values, const int* index, int rows, int k, int V, float inv_T, float top_p, unsigned long long seed,
                 unsigned step, unsigned row0, long long* tok, long long* ids, float* logp, long ld, hipStream_t stream,
                 unsigned greedy_stride = 0);
// decode_loops.hip: lstm_greedy_decode's loop with the draw in place of the argmax. The draw by its options: top_p == 1 and
// top_k == 0: vocab_sample; top_k > 0: vocab_topk + sample_pick (top_p < 1: + nucleus_pick); top_p < 1 without top_k: the
// projection into a logits block of the workspace (sgemm_splitk on the caller's slab, else unused) + nucleus_rows. ex (top_p <=
// 1; its mask left null): per step sample_exclusion_mask into the mask behind the loop's own workspace, then the step's draw on
// it -- vocab_sample / vocab_topk with the mask, or mask_logits on the logits block in front of nucleus_rows
struct SampleOpts {
  float inv_T;
  int top_k;             // 0: off
  float top_p;           // 1: off
  unsigned long long seed;
  unsigned greedy_stride;
  const SampleExcl* ex;  // null: none
};
// ws: the loop's own bytes (nucleus: with the logits block where top_k == 0); excl: 16-B aligned, then sample_mask_bytes
size_t sample_decode_ws_bytes(int nlayers, int rows, int H, int V, int top_k, bool nucleus, bool excl);
int sample_decode(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                  const long long* start_tokens, const float* emb, const float* const* wcat, const float* const* beff,
                  const float* Cw, const float* Cb, const float* state0, const SampleOpts& o, void* ws, float* slab,
                  size_t slab_floats, long long* ids, float* logp, float* state_out, int* err_flag, hipStream_t s);
// the same for an attention decoder: n images x m samples each on att_decode_step (k = m, every row its own parent)
size_t att_sample_decode_ws_bytes(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k, bool nucleus,
                                  bool excl);
int att_sample_decode(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int steps,
                      const long long* start_tokens, const float* att1, const float* feat, const float* emb, const float* wz,
                      const float* bz, const float* wf, const float* bf, const float* const* wcat, const float* const* beff,
                      const float* Cw, const float* Cb, const float* state0, const SampleOpts& o, void* ws, float* slab,
                      size_t slab_floats, long long* ids, float* logp, float* state_out, int* err_flag, hipStream_t s);
// decode_loops.hip: beam_decode's loop from a given state (one weight group), step 1 on first_inputs [n k][E] when set;
// fused_topk: a step's projection and selection as vocab_topk + beam_advance_topk (no logits block in ws, slab unused), else
// beam_decode's. con: the constrained search -- unfused, beam_advance's constrained or forced form; fused (no
// forced words), beam_exclusion_mask into a mask BEHIND the workspace's other parts (constrained = true in the size query:
// sample_mask_bytes(n k, V) more, fused only) and vocab_topk's select-only instance in front of the unchanged beam_advance_topk
size_t lstm_beam_decode_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk, bool constrained = false);
int lstm_beam_decode(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                     long long end_token, const float* first_inputs, const float* emb, const float* const* wcat,
                     const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* ws, float* slab,
                     size_t slab_floats, int fused_topk, int poll_every, long long* seqs, int* lengths, int* steps_run,
                     int* err_flag, hipStream_t s, const BeamConstraints* con = nullptr);
// the same loop over groups x n sentences, group-major, group g on emb[g] / wcat[l] + g 4H (kin + H) / beff[l] + g 4H / Cw[g] /
// Cb[g] (host-side pointer tables; Cb or any Cb[g] may be null): per step the gathered decode step on per-group tables,
// then vocab_topk_groups + beam_advance_topk, or one sgemm_splitk per group into its row block of the logits + beam_advance
size_t lstm_beam_decode_groups_ws_bytes(int nlayers, int groups, int n, int k, int H, int V, int max_steps, int fused_topk,
                                        bool constrained = false);
int lstm_beam_decode_groups(int cell, int nlayers, int groups, int n, int k, int E, int H, int V, int max_steps,
                            long long start_token, long long end_token, const float* const* emb, const float* const* wcat,
                            const float* const* beff, const float* const* Cw, const float* const* Cb, const float* state0,
                            void* ws, float* slab, size_t slab_floats, int fused_topk, int poll_every, long long* seqs,
                            int* lengths, int* steps_run, int* err_flag, hipStream_t s, const BeamConstraints* con = nullptr);
// beam_decode's loop around att_decode_step (att1 = encoder_att(feat), once per call, is the caller's; state0 is required)
size_t att_beam_decode_ws_bytes(int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps);
int att_beam_decode(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                    long long start_token, long long end_token, const float* att1, const float* feat, const float* emb,
                    const float* wz, const float* bz, const float* wf, const float* bf, const float* const* wcat,
                    const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* ws, float* slab,
                    size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                    hipStream_t s, int groups = 1, float* alphas = nullptr, const BeamConstraints* con = nullptr,
                    const BeamTeams* teams = nullptr);
// alphas [groups n][max_steps][P], optional (ws: att_beam_decode_alphas_ws_bytes): row e - 1 of a caption is the softmax over
// the pixels that preceded its word e, rows past its length - 1 are zero. ws then continues: the row trace | the winners'
// rows | the history [max_steps][groups n k][P] of every step's maps
size_t att_beam_decode_alphas_ws_bytes(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                       int max_steps);
// where a one-call search leaves what capnet_beam_nbest reads, as byte offsets into its workspace (0: a refused shape).
// The beam state of beam_decode_layout (n: the sentences of one group; the attention searches share the unfused layout);
// the trace and the history of att_beam_decode's maps.
size_t beam_decode_ws_beam_offset(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk, int groups);
size_t att_beam_decode_alphas_ws_trace_offset(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                              int max_steps);
size_t att_beam_decode_alphas_ws_hist_offset(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                             int max_steps);
// alpha_gather_kernel on its own: alphas [captions][max_steps][P] = hist[e][rows[caption][e]], zeros for a row outside [0, nk)
int alpha_gather(const float* hist, const int* rows, int captions, int nk, int max_steps, int P, float* alphas, hipStream_t s);

// lstm_persist.hip: a run of teacher-forced steps [t0, t1) in one launch (H = 512, b <= 128)
bool lstm_persist_supported(int b, int H);
size_t lstm_persist_w_floats();
size_t lstm_persist_ctl_ints();
int lstm_persist_pack(const float* Wcat, float* Wp, int gi, int gf, int go, int gg, hipStream_t stream);
int lstm_persist_run(const float* Wp, float* G, float* Cst, float* hiddens, const int* off,
                     const int* batch_sizes, int t0, int t1, int H, int gi, int gf, int go, int gg,
                     int tanh_out, int seg, int* ctl, int* err_flag, hipStream_t stream,
                     unsigned long long* stamps);

// att_kernels.hip
int att_step_fwd(const float* att1, const float* feat, const float* att2, float* gate_io, long ldz,
                 const float* wf, const float* bf, int rows, int P, int A, int C,
                 float* alpha_out, float* alphas_bt, int steps, int t, float* awe_out,
                 float* xa_out, long ldx, float* escore, hipStream_t stream);
// the k beams of an image on one read of its maps: att1 [n][P][A], feat [n][P][C], row r of image r / k; att2 and the gate
// from z [n k][A + C] at row parent_rows[r] (null: r), read only; xa [n k][E + C] = [emb[tokens[r]] | gated context]
bool att_beam_step_supported(int E, int C, int A, int P, int k);
int att_beam_step_fwd(const float* att1, const float* feat, const float* z, const long long* parent_rows, const float* wf,
                      const float* bf, const long long* tokens, const float* emb, int V, int E, int n, int k, int P, int A,
                      int C, float* escore, float* xa, int* err_flag, hipStream_t stream, int n_img = 0,
                      float* alpha_out = nullptr);
// (n_img > 0, n = G n_img beam groups of G weight groups: group q reads att1 at q, feat [n_img][P][C] at q % n_img and
// full_att wf [G][A], bf [G] at q / n_img; alpha_out [n k][P], optional: every row's softmax over the pixels, stored by
// the image's first channel block -- the arithmetic is the same with it and without)
int att_step_bwd(const float* att1, const float* feat, const float* att2, long ldz2,
                 const float* gate, long ldzg, const float* awe, const float* alpha,
                 const float* wf, float* dxa, long ldx, const float* dalphas_bt, int steps,
                 int t, int rows, int P, int A, int C, float* dalpha_part, float* dgate_out,
                 float* datt2, long ldz, float* de_out, float* dwf_rows, float* dbf_rows,
                 hipStream_t stream, const float* dxa_slabs = nullptr, int n_slabs = 0, int emb_cols = 0);
int att_datt1(const float* att1, const float* att2_rows, long ldz2, const float* de_rows,
              const float* wf, const int* off, int steps, int B, int P, int A, float* datt1,
              hipStream_t stream);

// image_ops.hip
int resize_u8(const unsigned char* src, int Hs, int Ws, unsigned char* tmp, unsigned char* dst, int Ho,
              int Wo, const int* bounds_h, const int* coef_h, int kmax_h, const int* bounds_v,
              const int* coef_v, int kmax_v, hipStream_t stream);
int crop_flip_normalize(const unsigned char* src, int B, int Hs, int Ws, const int* params, float* dst,
                        int Hc, int Wc, const float* mean, const float* stdv, hipStream_t stream);

// loss_optim.hip
int xent_fwd(const float* logits, long ld, int N, int V, const long long* targets, float* lse,
             float* row_loss, float* loss, int* err_flag, hipStream_t stream);
int topk_correct(const float* logits, long ld, int N, int V, const long long* targets, int k,
                 int* count, int* err_flag, hipStream_t stream);
int xent_bwd(const float* logits, long ld, int N, int V, const long long* targets,
             const float* lse, const float* gout, float* dlogits, long ldd, hipStream_t stream);
int att_loss_fwd(const float* nll, const float* alphas, int B, int steps, int P, float alpha_c,
                 float* colsum, float* out, hipStream_t stream);
int att_loss_bwd(const float* gout, const float* colsum, int B, int steps, int P, float alpha_c,
                 float* dalphas, hipStream_t stream);
// policy_loss.hip
int policy_xent_fwd(const float* logits, long ld, int N, int V, const long long* targets, const float* adv, int B,
                    const int* batch_sizes, int steps, float* lse, float* row_logp, float* caption_logp, float* loss,
                    int* err_flag, hipStream_t stream);
int policy_xent_bwd(const float* logits, long ld, int N, int V, const long long* targets, const float* lse,
                    const float* adv, int B, const int* batch_sizes, int steps, const float* gout, float* dlogits,
                    long ldd, hipStream_t stream);
// caption_reward.hip: sentence BLEU of decoded rows. Limits: a hypothesis of at most kBleuMaxSteps + 1 words, at most
// kBleuMaxRefs reference slots per image and kBleuRefWords padded reference words per image (slots x padded length)
constexpr int kBleuMaxSteps = 128, kBleuMaxRefs = 16, kBleuRefWords = 4096;
int bleu_rows(const long long* ids, long ld, int rows, int steps, long long start_token, long long end_token, int per_image,
              const int* refs, const int* ref_len, int images, int R, int Lr, const double* weights, int smooth, float* reward,
              int* stats, hipStream_t stream);
// CIDEr-D of decoded rows under the same limits; keys / idf / counts: HOST arrays of four (device pointers, sizes), one per order
int cider_rows(const long long* ids, long ld, int rows, int steps, long long start_token, long long end_token, int per_image,
               const int* refs, const int* ref_len, const double* ref_norm, int images, int R, int Lr, const int* const* keys,
               const double* const* idf, const int* counts, double log_n, double sigma, float* reward, double* parts, int* stats,
               hipStream_t stream);
int lstm_persist_set_mode(int mode);
int clamp_adam(int n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
               float* const* exp_avg_sq, const long* numel, const int* step, float lr, float b1,
               float b2, float eps, float clip, int write_grad, const int* skip_flag, hipStream_t stream);
// fused_block.hip: conv3 + BatchNorm3 + residual + ReLU + the next conv1 without y3 (statistics from the Gram matrix of conv3's input)
bool fused_block_shape_ok(long M, int MID);
size_t fused_block_weight_words(int C, int MID, int role);
int fused_block_pack(const float* w, unsigned* img, int C, int MID, int role, hipStream_t stream);
size_t fused_block_stats_floats(long M, int K);
int fused_block_stats(const float* y2, const float* s2, const float* t2, const unsigned* w3img, long M, int MID, int in_exp,
                      const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                      float* scale, float* shift, float* batch_mean, float* batch_var, float* work, int* err, hipStream_t stream);
int fused_block_tiles(long M, int MID);
int fused_block_forward(const float* y2, const float* s2, const float* t2, const unsigned* w3img, const float* s3, const float* t3,
                        const float* res, const float* sd, const float* td, float* out, const unsigned* w1img, float* y1,
                        float* part_sum, float* part_sq, long M, int MID, int e3, int e1, int* err, hipStream_t stream);
struct Comm;
int comm_unique_id(void* id128);
int comm_create(const void* id128, int rank, int world, Comm** out);
int comm_destroy(Comm* c);
int allreduce_grads(Comm* c, float* flat, long count, hipStream_t stream);
int err_word_exchange(int* err_flag, float* slot, int dir, hipStream_t stream);
int count_skipped(const int* err_flag, int* counter, hipStream_t stream);
int pack_tensors(int n_tensors, float* const* tensors, const long* numel, float* flat, int dir,
                 float scale, hipStream_t stream);
int clamp_inplace(float* x, long n, float lo, float hi, hipStream_t stream);
int bn1d_fwd(const float* x, int B, int C, const float* gamma, const float* beta, float* rmean,
             float* rvar, int train, float momentum, float eps, float* y, float* save_mean,
             float* save_invstd, hipStream_t stream);
int bn1d_bwd(const float* dy, const float* x, int B, int C, const float* gamma,
             const float* save_mean, const float* save_invstd, float* dx, float* dgamma,
             float* dbeta, hipStream_t stream);

// decoder_seq.cpp
constexpr int kCellFactored = 0;  // DecoderFactoredLSTM (stylenet/model.py)
constexpr int kCellLSTM = 1;      // nn.LSTMCell (nic/model.py)
constexpr int kSeqInputDropoutOnly = 2;   // bit of seq_forward_stacked's / seq_backward_stacked's `training`: no dropout
                                          // between the layers (torch.nn.LSTM without dropout=), embeddings only
struct SeqDims {
  int B, T, steps, N, E, F, H, V, has_features, cell;
};
// Factored: Vw/Vb/Sw/Sb/Uw/Ub/Ww/Wb per gate (i, f, o, c). LSTM cell: Vw[0] = weight_ih,
// Vb[0] = bias_ih, Ww[0] = weight_hh, Wb[0] = bias_hh (gate order i, f, g, o).
struct SeqWeights {
  const float* Vw[4]; const float* Vb[4];
  const float* Sw[4]; const float* Sb[4];
  const float* Uw[4]; const float* Ub[4];
  const float* Ww[4]; const float* Wb[4];
};
// packed gradients: dVcat [4F][E] (or weight_ih [4H][E]), dbV [4F], dScat [4][F][F], dbS [4F],
// dUcat [4][H][F], dbUW [4H] (= grad of U bias = grad of W bias; LSTM: of both biases),
// dWcat [4H][H], dEmb [V][E], dFeat [B][E] or null
struct SeqGrads {
  float* dVcat; float* dbV; float* dScat; float* dbS; float* dUcat; float* dbUW; float* dWcat;
  float* dEmb; float* dFeat;
};
size_t seq_saved_floats(const SeqDims& d);
size_t seq_saved_ints(const SeqDims& d);
size_t seq_fwd_scratch_floats(const SeqDims& d);
size_t seq_bwd_scratch_floats(const SeqDims& d);
size_t seq_saved_cell_offset(const SeqDims& d);   // floats from the start of a layer's `saved` to its cell states [N][H]
SeqDims seq_upper_dims(const SeqDims& d0);
int seq_forward_stacked(const SeqDims& d0, int nlayers, const int* batch_sizes, const unsigned char* tf_mask,
                        const long long* captions, const float* features, const float* emb, const SeqWeights* w,
                        const float* Cw, const float* Cb, float dropout_p, unsigned long long seed, int training,
                        float* const* saved, int* const* saved_i, float* scratch, float* const* hiddens, int* err_flag,
                        hipStream_t s);
int seq_backward_stacked(const SeqDims& d0, int nlayers, const int* batch_sizes, const float* dH_top,
                         const float* const* hiddens, const float* const* saved, const int* const* saved_i, float* scratch,
                         float* const* dH_work, const SeqGrads* g, float dropout_p, unsigned long long seed, int training,
                         hipStream_t s);

// decoder_att_seq.cpp -- DecoderFactoredLSTMAtt (stylenet/model_att.py:73-305)
struct AttDims {
  int B, T, steps, N, E, F, H, V, A, P, C;
  int cell;  // kCellFactored: DecoderFactoredLSTMAtt; kCellLSTM: nic DecoderRNNAtt (nn.LSTMCell)
};
struct AttWeights {
  const float* Vw[4]; const float* Vb[4];   // V_g: [F][E+C]
  const float* Sw[4]; const float* Sb[4];   // mode-selected S_g
  const float* Uw[4]; const float* Ub[4];
  const float* Ww[4]; const float* Wb[4];
  const float* init_h_w; const float* init_h_b; const float* init_c_w; const float* init_c_b;
  const float* enc_att_w; const float* enc_att_b;   // [A][C]   (mode-selected attention module)
  const float* dec_att_w; const float* dec_att_b;   // [A][H]
  const float* full_att_w; const float* full_att_b; // [1][A], [1]
  const float* f_beta_w; const float* f_beta_b;     // [C][H]
};
// dWz [4H+A+C][H] = [dW_i; dW_f; dW_o; dW_c; d decoder_att; d f_beta]; dbz likewise
// (dbz[0:4H] is the gradient of both the U and the W biases)
struct AttGrads {
  float* dVcat; float* dbV; float* dScat; float* dbS; float* dUcat; float* dWz; float* dbz;
  float* dWe; float* dbe; float* dwf; float* dbf; float* dWih; float* dbih; float* dWic;
  float* dbic; float* dEmb;
};
int att_set_chain_mode(int mode);      // the factored input product as one matrix per call: 0 by shape, 1 always, -1 never
size_t att_saved_floats(const AttDims& d);
size_t att_saved_ints(const AttDims& d);
size_t att_fwd_scratch_floats(const AttDims& d);
size_t att_bwd_scratch_floats(const AttDims& d);
int att_seq_backward(const AttDims& d, const int* bs, const float* dH, const float* dalphas_bt,
                     const float* hiddens, const float* feat, const AttWeights& w,
                     const float* saved, const int* saved_i, float* scratch, const AttGrads& g,
                     float dropout_p, unsigned long long seed, int training, hipStream_t s);

// the attention decoder of 1 to 8 layers (one: DecoderFactoredLSTMAtt / DecoderRNNAtt, either cell; more: capnet.stacked_att,
// factored cells only): layer 0 is the attention cell (att_fwd_begin / att_fwd_step), layers l > 0 the factored cell on
// dropout(h^{l-1}_t) with initial state init_h{l} / init_c{l} of the mean feature. hiddens[0]: [N][H]; hiddens[l > 0]:
// [B + N][H], rows 0..B-1 the initial state. Upper weights: SeqWeights + init_h{l} w, b, init_c{l} w, b.
struct UpperInit { const float* init_h_w; const float* init_h_b; const float* init_c_w; const float* init_c_b; };
struct UpperInitGrads { float* dWih; float* dbih; float* dWic; float* dbic; };
size_t att_stacked_saved_floats(const AttDims& d, int layer);
size_t att_stacked_saved_ints(const AttDims& d, int layer);
size_t att_stacked_fwd_scratch_floats(const AttDims& d, int nlayers);
size_t att_stacked_bwd_scratch_floats(const AttDims& d, int nlayers);
int att_seq_forward_stacked(const AttDims& d, int nlayers, const int* bs, const unsigned char* tf, const long long* captions,
                            const float* feat, const float* emb, const AttWeights& w0, const SeqWeights* wu,
                            const UpperInit* iu, const float* Cw, const float* Cb, float dropout_p, unsigned long long seed,
                            int training, float* const* saved, int* const* saved_i, float* scratch, float* const* hiddens,
                            float* alphas_bt, int* err_flag, hipStream_t s);
int att_seq_backward_stacked(const AttDims& d, int nlayers, const int* bs, const float* dH_top, const float* dalphas_bt,
                             const float* const* hiddens, const float* feat, const AttWeights& w0,
                             const float* const* saved, const int* const* saved_i, float* scratch, float* const* dH_work,
                             const AttGrads& g0, const SeqGrads* gu, const UpperInitGrads* giu, float dropout_p,
                             unsigned long long seed, int training, hipStream_t s);

}  // namespace capnet
