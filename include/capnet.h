/* capnet.h -- C ABI of libcapnet_hip.so: the MI355X (gfx950) training-step kernels of the
 * StyleNet / NIC captioning path.
 *
 * The reference (deryrahman/image-caption-emotion-indonesia) has no native/FFI layer: its
 * boundary is the Python class surface of stylenet/model.py, nic/model.py and the loops in
 * stylenet/train_multitask.py. Each entry point below names the torch call(s) of the
 * reference it replaces (file:line under /root/reference). The Python mirror of those classes
 * binds these symbols through ctypes.
 *
 * Conventions
 *   - every function returns 0 on success, a negative status otherwise;
 *     capnet_last_error() returns the message of the calling thread's last failure;
 *   - all `float*` / `long long*` / `int*` data pointers are CALLER-OWNED DEVICE pointers
 *     (tensor.data_ptr()); arrays documented as "host" are ordinary host memory;
 *   - `stream` is a hipStream_t; nothing here allocates device memory, synchronises the
 *     stream or touches the default stream, so every call can be captured in a hipGraph;
 *   - arithmetic is fp32 with fp32 accumulation (v_mfma_f32_32x32x2_f32 == fmaf chain).
 */
#ifndef CAPNET_H_
#define CAPNET_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* capnet_stream_t; /* hipStream_t */
typedef struct capnet_trunk capnet_trunk_t;

#define CAPNET_OK 0
#define CAPNET_ERR_INVALID_ARG (-1)
#define CAPNET_ERR_HIP (-2)

const char* capnet_last_error(void);
int capnet_abi_version(void);

/* ---- dense projections --------------------------------------------------------------
 * C[M x N] (+)= op(A) . op(B) + bias[N], row-major, `batch` independent problems at the given
 * element strides. transA=0: A is [M][K]; 1: [K][M]. transB=0: B is [K][N]; 1: [N][K].
 * Replaces every nn.Linear forward and autograd matmul of the decoders and the encoder head:
 * stylenet/model.py:119-150 (V/S/U/W gates), :189-194 (C), :19,26 (encoder.linear);
 * nic/model.py:52,77,105-113. force_tile: 0 = auto; 64, 128 or 6432 (64 x 64 tile, 32-deep k slices) keep the product
 * on the generic k-loop kernel at that tile. */
int capnet_sgemm(int transA, int transB, int M, int N, int K, const float* A, long lda,
                 const float* B, long ldb, float* C, long ldc, const float* bias, int accumulate,
                 int batch, long strideA, long strideB, long strideC, long strideBias,
                 int force_tile, capnet_stream_t stream);
/* The same product on the bf16 matrix cores: each fp32 operand cut into three bf16 pieces (exactly), six piece products
 * per multiply accumulated in fp32 -- fp32-grade results over fp32's whole exponent range, no prescale (csrc/gemm_b3.hip).
 * capnet_sgemm takes this path by itself for large products (CAPNET_NO_B3=1 in the environment keeps everything on the f32
 * MFMA). Eligible: 16-B aligned operands, leading dimensions and batch strides multiples of 4, K % 4 == 0 when an operand
 * is K-contiguous, M % 4 == 0 / N % 4 == 0 when A / B is stored with that dimension contiguous. ws (optional, batch 1):
 * ws_floats floats for split-K partials -- products of few 128 x 128 tiles and a long K are cut over the chip. */
int capnet_sgemm_b3(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                    float* C, long ldc, const float* bias, int accumulate, int batch, long strideA, long strideB,
                    long strideC, long strideBias, float* ws, size_t ws_floats, capnet_stream_t stream);
int capnet_sgemm_b3_eligible(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                             const float* C, long ldc, const float* bias, int batch, long strideA, long strideB,
                             long strideC, long strideBias);

/* The same product for the per-time-step shapes of the decoders (M <= 128 rows, A not transposed):
 * K is cut into chunks, one workgroup per (64x64 tile, chunk) loads its chunk in one round trip and
 * writes a partial tile to `workspace` (workspace_floats >= ceil(K/64)*M*N for the finest split);
 * the partials are summed in a fixed order. Falls back to capnet_sgemm's kernel when the shape
 * does not qualify. Replaces the per-step nn.Linear calls of stylenet/model.py:147-150,189 and
 * model_att.py:59-60,283. */
int capnet_sgemm_splitk(int transA, int transB, int M, int N, int K, const float* A, long lda,
                        const float* B, long ldb, float* C, long ldc, const float* bias,
                        int accumulate, float* workspace, size_t workspace_floats,
                        capnet_stream_t stream);

/* The same, with tile counters: `counters` = n_counters ints (>= ceil(N/64)), zero before the first call and left
 * zero by every call. With them a product of M <= 16 rows (the time step of a 12-image batch, decoding) is ONE
 * launch: a workgroup per (16 rows x 64 columns, 256-k chunk), and the workgroup that arrives last at a tile's
 * counter sums the chunk partials in chunk order (csrc/gemm_f32.hip, gemm_rows16_kernel). Other shapes: as
 * capnet_sgemm_splitk. Calls that share `counters` or `workspace` must be ordered on one stream. */
int capnet_sgemm_splitk_fused(int transA, int transB, int M, int N, int K, const float* A, long lda,
                              const float* B, long ldb, float* C, long ldc, const float* bias,
                              int accumulate, float* workspace, size_t workspace_floats, int* counters,
                              size_t n_counters, capnet_stream_t stream);

/* out[c] (+)= sum_r x[r][c]  -- bias gradients (autograd of nn.Linear bias). */
int capnet_colsum(const float* x, long ld, int rows, int C, float* out, int accumulate,
                  capnet_stream_t stream);

/* capnet_colsum with a workspace: inputs of more than 4096 rows are cut into row chunks (at most 32, workspace_floats >=
 * chunks * C) whose partial sums capnet_reduce_slabs' kernel adds in chunk order. workspace NULL: capnet_colsum. */
int capnet_colsum_ws(const float* x, long ld, int rows, int C, float* out, int accumulate, float* workspace,
                     size_t workspace_floats, capnet_stream_t stream);

/* out[m][n] = (((0 + slab[0][m][n]) + slab[1][m][n]) + ...) + bias[n], then + out[m][n] when accumulating: the fixed-order
 * fp32 sum of `count` dense [M][N] partials that closes every split-K product. out has leading dimension ldc. */
int capnet_reduce_slabs(const float* slab, int count, int M, int N, float* out, long ldc, const float* bias,
                        int accumulate, capnet_stream_t stream);

/* capnet_sgemm_splitk_fused over `batch` members (the four gates of the factored chain). The split-K kernels take the
 * batch when the members' outputs are adjacent column blocks of C (strideC == N; bias concatenated, strideBias == N;
 * strideA, strideB multiples of 4; batch <= 64); any other batch goes to capnet_sgemm's kernels. counters (optional):
 * >= ceil(N/64) * batch ints. */
int capnet_sgemm_splitk_batched(int transA, int transB, int M, int N, int K, const float* A, long lda,
                                const float* B, long ldb, float* C, long ldc, const float* bias, int accumulate,
                                int batch, long strideA, long strideB, long strideC, long strideBias,
                                float* workspace, size_t workspace_floats, int* counters, size_t n_counters,
                                capnet_stream_t stream);

/* The K-chunk partial products only, A [M][K] not transposed: workspace[k][M][N] for k < *n_slabs, left for the consumer
 * to sum in slab order (capnet_reduce_slabs, or a kernel that folds the sum in). *n_slabs = 0 and an untouched workspace
 * when the shape does not qualify: _splitk_slabs is the M <= 128 kernel of capnet_sgemm_splitk, _rows16_slabs the
 * M <= 16 kernel of capnet_sgemm_splitk_fused without its in-launch hand-off. */
int capnet_sgemm_splitk_slabs(int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                              float* workspace, size_t workspace_floats, int* n_slabs, capnet_stream_t stream);
int capnet_sgemm_rows16_slabs(int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                              float* workspace, size_t workspace_floats, int* n_slabs, capnet_stream_t stream);

/* Which kernel capnet_sgemm / capnet_sgemm_splitk_batched gives a product: the dispatchers' own plan functions, run
 * without launching anything (no device is needed; pointers are looked at for null and 16-B alignment only). Returns a
 * CAPNET_ROUTE_* code, or a negative status where the call itself would be refused. detail (optional, 4 ints):
 *   [0] loader form: 1 = 16-B vector loads, 0 = guarded scalar loads (odd leading dimension or stride, misaligned base)
 *   [1] splits: slabs K is cut into (1: none)
 *   [2] rows16: 256-k chunks per workgroup (sub); skinny: kc; k-loop / b3 split-K: k per slab (kchunk); else 0
 *   [3] output tiles: 64 x 64 or 128 x 128 tiles of one batch member for the generic kernel, the k-loop split-K and b3;
 *       64-column tiles of one member for rows16; 64 x 64 tiles of all members for skinny; ceil(M/128) * (N/64) for nt_dma
 * tests/gemm_cases.py lists one product per branch with the route it must take. */
#define CAPNET_ROUTE_NONE 0             /* empty product: nothing launched */
#define CAPNET_ROUTE_GENERIC_64 1       /* gemm_f32_kernel, the k-loop, 64 x 64 tile, BK 16 */
#define CAPNET_ROUTE_GENERIC_128 2      /* ... 128 x 128 tile */
#define CAPNET_ROUTE_GENERIC_6432 3     /* ... 64 x 64 tile, BK 32 (force_tile 6432 only) */
#define CAPNET_ROUTE_NT_DMA 4           /* nt_dma_kernel (gemm_dma.hip) */
#define CAPNET_ROUTE_B3 5               /* gemm_b3_kernel (gemm_b3.hip) */
#define CAPNET_ROUTE_ROWS16 6           /* gemm_rows16_kernel: M <= 16, one launch */
#define CAPNET_ROUTE_SKINNY_64 7        /* gemm_skinny_kernel, kc = 64, + the slab reducer */
#define CAPNET_ROUTE_SKINNY_128 8       /* ... kc = 128 */
#define CAPNET_ROUTE_KLOOP_SPLITK 9     /* gemm_f32_kernel over K slabs + the slab reducer */
#define CAPNET_ROUTE_B3_SPLITK 10       /* gemm_b3_kernel over K slabs + the slab reducer */
#define CAPNET_ROUTE_FELL_THROUGH 64    /* flag: the split-K entry handed the product to capnet_sgemm; the low bits are
                                           the route capnet_sgemm takes, `detail` is capnet_sgemm_route's */
int capnet_sgemm_route(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                       const float* C, long ldc, const float* bias, int accumulate, int batch, long strideA,
                       long strideB, long strideC, long strideBias, int force_tile, int* detail);
int capnet_sgemm_splitk_route(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B,
                              long ldb, const float* C, long ldc, const float* bias, int accumulate, int batch,
                              long strideA, long strideB, long strideC, long strideBias, const float* workspace,
                              size_t workspace_floats, const int* counters, size_t n_counters, int* detail);

/* out[row] = index of the first maximum of x[row][0:V]  -- `output.max(1)` at
 * stylenet/model.py:190, nic/model.py:109. */
int capnet_argmax_rows(const float* x, int rows, int ld, int V, int* out, capnet_stream_t stream);

/* One beam-search expansion of `sample()` (stylenet/model.py:229-249, model_att.py:362-384,
 * nic/model.py sample): scores[r][v] = prev_scores[r] + log_softmax(logits[r])[v]; returns the k
 * best entries of the flattened [rows*V] scores, best first (ties: lower flat index):
 * top_scores[k], top_index[k] (flat index = r*V + v; the caller splits it with // and %).
 * rows, k <= 16. The reference passes rows = 1 on the first step (all beams identical). */
int capnet_beam_topk(const float* logits, long ld, int rows, int V, const float* prev_scores, int k,
                     float* top_scores, long long* top_index, capnet_stream_t stream);
/* The same expansion for n images in one launch (the test-set evaluator, stylenet/evaluator.py:63-120, decodes every image
 * of a batch with sample(); here all of them advance together): meta is a DEVICE array [n][3] = (first row of the image's
 * beams in logits / prev_scores, rows that compete, k); outputs [n][16], flat indices local to the image. Images whose
 * k is 0 (every beam finished) are skipped. rows, k <= 16. */
int capnet_beam_topk_batched(const float* logits, long ld, int V, const float* prev_scores, const int* meta, int n,
                             float* top_scores, long long* top_index, capnet_stream_t stream);

/* Beam search whose bookkeeping stays on the device (capnet.beam.beam_search_device): what capnet.beam's loops do on the
 * host after every capnet_beam_topk_batched -- which beam survives, the sequences, the completed list -- done by the
 * workgroup that selected. Image i owns rows i k .. i k + k - 1 of the decoder step for the WHOLE search; its live beams
 * are its first live[i] slots in top-k rank order, dead slots still take the step (their logits are never read).
 * `beam`: capnet_beam_state_bytes(n, k, max_steps) bytes of caller-owned device memory, 4-byte aligned; max_steps is the
 * number of capnet_beam_advance calls the search may make (max_seq_length + 1 for the decoders). 1 <= k <= 16, k <= V.
 *   init:    every beam live with score 0 and the sequence [start_token]; prev_words[n k] = start_token.
 *   advance: step = 1, 2, ... in order, on the logits [n k][ld] of that step. The selection is capnet_beam_topk_batched's
 *            (row 0 alone at step 1). A selected <end> completes its beam (appended to the image's completed list, by step
 *            then rank); any other word w of parent slot p survives into the image's next free slot s:
 *            next_words[i k + s] = w, parent_rows[i k + s] = i k + p. Dead slots get end_token and their own row, so both
 *            arrays are fully written by every call and the caller re-indexes its state by parent_rows.
 *   finish:  per image the first maximum of the completed scores in completion order (the reference's
 *            list.index(max(...))), [end_token] if nothing completed: seqs[n][max_steps + 2] (padded with 0), lengths[n].
 *   live:    (host arithmetic only) device pointers into `beam`: live_total (the number of live beams of all images; zero
 *            means every later advance is a no-op), live[n], scores[n k]. Any of the three may be NULL. */
size_t capnet_beam_state_bytes(int n, int k, int max_steps);
int capnet_beam_init(void* beam, int n, int k, int max_steps, long long start_token, long long* prev_words,
                     capnet_stream_t stream);
int capnet_beam_advance(void* beam, const float* logits, long ld, int V, int n, int k, int max_steps, int step,
                        long long end_token, long long* next_words, long long* parent_rows, capnet_stream_t stream);
int capnet_beam_finish(const void* beam, int n, int k, int max_steps, long long end_token, long long* seqs, int* lengths,
                       capnet_stream_t stream);
/* capnet_beam_advance on a step's CANDIDATES instead of its logits (capnet_vocab_topk's outputs): values f32 [n k][k] and
 * index int32 [n k][k], per row its k best logits and their vocabulary entries, best first, index -1 where a row had
 * fewer; lse f32 [n k], the rows' log-sum-exp. Image i takes its live[i] best of scores[row] - lse[row] + values[row][j]
 * over its live rows (row 0 alone at step 1) and j < k, ties to the lower flat index row_in_image V + index[row][j]; from
 * there on it is capnet_beam_advance (one device function serves both). fp32 addition is monotone, so a row's members of
 * the image's top-live are among that row's top-live logits: the selection is capnet_beam_advance's on the same logits
 * whenever no two candidate scores tie after rounding. A padded candidate is never chosen and never used as an address;
 * an image that is offered fewer candidates than it has live beams keeps that many beams. 1 <= k <= 16, k <= V. */
int capnet_beam_advance_topk(void* beam, const float* values, const int* index, const float* lse, int V, int n, int k,
                             int max_steps, int step, long long end_token, long long* next_words, long long* parent_rows,
                             capnet_stream_t stream);
int capnet_beam_live(const void* beam, int n, int k, int max_steps, const int** live_total, const int** live,
                     const float** scores);

/* ---- ResNet-152 trunk -------------------------------------------------------------------
 * torchvision resnet152 children[:-1] (pooled [B][2048]) or [:-2] (NHWC map [B][S][S][2048]),
 * as run under torch.no_grad() by EncoderCNN.forward: stylenet/model.py:15-18,23-25,
 * stylenet/model_att.py:15-18,23-24, nic/model.py:14-17,22-24. train != 0 reproduces
 * encoder.train() (stylenet/train_multitask.py:367): batch statistics + running-stat update
 * (momentum 0.1, eps 1e-5); train == 0 uses the running statistics.
 * Convolution i (torchvision parameter order, 155 of them) takes its weights PACKED as
 * [Cout][KH][KW][Cin] rows padded to `row_stride` floats (capnet_pack_conv_weight). */
int capnet_trunk_create(int batch, int height, int width, capnet_trunk_t** out);
void capnet_trunk_destroy(capnet_trunk_t* t);
size_t capnet_trunk_workspace_bytes(const capnet_trunk_t* t);
int capnet_trunk_num_convs(const capnet_trunk_t* t);
int capnet_trunk_final_side(const capnet_trunk_t* t);
double capnet_trunk_flops(const capnet_trunk_t* t); /* 2*MACs of all convolutions, this batch */
double capnet_trunk_conv_flops(const capnet_trunk_t* t, int i); /* 2*MACs of convolution i (direct sum) */
int capnet_trunk_conv_shape(const capnet_trunk_t* t, int i, int* cout, int* cin, int* ksize,
                            int* stride, int* row_stride);
/* w_packed / bn_* : HOST arrays of num_convs DEVICE pointers. out_pooled and/or out_map may
 * be NULL (at least one must be given).
 * input_exponents: NULL, or a HOST array of num_convs ints e[i]: convolution i's input tensor is multiplied by 2^e[i] on
 * its way into the f16 planes of the split-f16 kernels (folded into the preceding BatchNorm's scale / shift where there
 * is one; exact; undone in the epilogue). What gives the split operands the domain of fp32: the caller derives e[i] from
 * the BatchNorm parameters so that the tensor's largest possible value sits just below f16's 65 504
 * (capnet.model._TrunkRunner._input_exponents).
 * err_flag: NULL, or the device error word: bit 3 (value 8) is set when a convolution's output statistics (train mode)
 * or the pooled features (inference) are not finite -- an activation beyond the range the exponents allow for, or a
 * genuine fp32 overflow; never silently inf. */
int capnet_trunk_forward(const capnet_trunk_t* t, const float* images_nchw,
                         const float* const* w_packed, const float* const* bn_weight,
                         const float* const* bn_bias, float* const* bn_running_mean,
                         float* const* bn_running_var, int train, float momentum, float eps,
                         void* workspace, float* out_pooled, float* out_map,
                         const int* input_exponents, int* err_flag, capnet_stream_t stream);

/* train == 2 in capnet_trunk_forward: batch statistics as for train == 1, but the running
 * statistics are NOT touched; the pass leaves every BatchNorm's batch mean / unbiased variance in
 * the workspace and this call applies them (same arithmetic, momentum as given). Lets two passes
 * be in flight on different streams (different workspaces) while the running statistics are still
 * updated in pass order: the caller orders these calls with stream events
 * (capnet.train.TrunkPipeline). */
/* Tail balancing of the convolutions (tiles past the last full round of 256 CUs are cut into K
 * slices summed by a fix-up launch): on by default; pays for a single pass, costs when several
 * passes share the chip (capnet.train.TrunkPipeline turns it off). Applies to later forwards. */
int capnet_trunk_set_tail_balance(const capnet_trunk_t* t, int on);

int capnet_trunk_update_running(const capnet_trunk_t* t, const void* workspace,
                                float* const* bn_running_mean, float* const* bn_running_var,
                                float momentum, capnet_stream_t stream);
/* Per-convolution hipEvent timing for bench.py's roofline: while enabled, every conv kernel
 * launched by capnet_trunk_forward is bracketed by two events on the launch stream;
 * collect synchronises on them and returns the totals since the previous collect. enable = N > 1:
 * only every N-th pass is bracketed (an event pair is a bubble in its stream). */
int capnet_trunk_set_timing(capnet_trunk_t* t, int enable);
/* Brackets the NEXT capnet_trunk_forward only, whatever capnet_trunk_set_timing says: for a caller that replays most passes
 * from hipGraphs (events cannot ride in a replayed graph) and launches every N-th one directly. */
int capnet_trunk_time_next_pass(capnet_trunk_t* t);
int capnet_trunk_collect_timing(capnet_trunk_t* t, double* conv_ms, long* conv_launches,
                                double* conv_flops);
/* Weight image convolution i expects: 0 = rows [Cout][row_stride] (capnet_pack_conv_weight),
 * 1 = K-major [row_stride][Cout] (capnet_pack_conv_weight_kmajor; streamed to LDS by LDS-DMA) -- the f32-MFMA kernels,
 * which take every convolution when the trunk is created with CAPNET_NO_H3=1 in the environment and otherwise those the
 * split-f16 kernels do not (none in ResNet-152),
 * 5 = the split-f16 image of a 1x1 or 3x3 convolution (capnet_conv_f16x3_pack with tile width
 * capnet_trunk_conv_tile_n(t, i)),
 * 6 = the split-f16 image of the stem (capnet_conv_stem_f16x3_pack; unless CAPNET_NO_STEM_H3=1). */
int capnet_trunk_conv_kmajor(const capnet_trunk_t* t, int i);
int capnet_trunk_conv_tile_n(const capnet_trunk_t* t, int i);
int capnet_pack_conv_weight_kmajor(const float* w_oihw, float* out, int Cout, int Cin, int KH,
                                   int KW, int k_rows, capnet_stream_t stream);
/* OIHW (torch Conv2d.weight) -> packed rows */
int capnet_pack_conv_weight(const float* w_oihw, float* out, int Cout, int Cin, int KH, int KW,
                            int row_stride, capnet_stream_t stream);
/* nn.AdaptiveAvgPool2d(out_side) on an NHWC map whose side divides out_side (7 -> 14 is a
 * 2x replication): stylenet/model_att.py:19-20,26-28. */
int capnet_adaptive_pool_replicate(const float* x, float* out, int B, int side, int out_side,
                                   int C, capnet_stream_t stream);

/* single building blocks of the trunk, exported for the parity tests */
int capnet_conv2d_fwd(const float* x, long sxb, long sxh, long sxw, long sxc,
                      const float* w_packed, int row_stride, float* y, const float* in_scale,
                      const float* in_shift, int relu_in, float* part_sum, float* part_sq, int B,
                      int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                      int tile, capnet_stream_t stream);
/* C[M][N] = A[M][K] . B[N][K]^T + bias[N] with both operands staged by LDS-DMA (csrc/gemm_dma.hip):
 * the vocabulary projection logits = hiddens . C^T + b (stylenet/model.py:193-194) and every
 * nn.Linear forward whose shape is eligible (N % 64 == 0, K % 32 == 0, B and C dense, 16-B aligned). */
int capnet_sgemm_nt_dma_eligible(int M, int N, int K, const float* A, long lda, const float* B,
                                 long ldb, const float* C, long ldc);
int capnet_sgemm_nt_dma(int M, int N, int K, const float* A, long lda, const float* B, float* C,
                        const float* bias, capnet_stream_t stream);
/* 1x1 convolution (any stride) on an NHWC input, weights in their OIHW = [Cout][Cin] layout, same
 * kernel: the conv1 / conv3 / downsample convolutions of the bottlenecks (torchvision resnet152 via
 * stylenet/model.py:15-18,24). Cin % 32 == 0, Cout % 64 == 0. Either raw output +
 * capnet_conv1x1_tiles_m(M) rows of part_sum / part_sq (train-mode BatchNorm statistics of each
 * 128-row tile), or, with out_scale / out_shift, y = act(conv * out_scale[n] + out_shift[n] + res). */
int capnet_conv1x1_tiles_m(long M);
int capnet_conv1x1_fwd_dma(const float* x, long sxb, long sxh, long sxw, const float* w_oi, float* y,
                           float* part_sum, float* part_sq, int B, int H, int W, int Cin, int Cout,
                           int stride, const float* out_scale, const float* out_shift, const float* res,
                           int relu_out, capnet_stream_t stream);

/* 1x1 convolution with fp32-grade results from three f16 MFMA products per multiply (csrc/conv_f16x3.hip):
 * both operands scaled by a power of two and split into two f16 pieces (activations by 2^4, weights by a
 * per-tensor 2^ew kept in the image's header), fp32 accumulation, the accumulators scaled back exactly;
 * rms error against fp64 at or below the f32-MFMA kernels' for |x| < 4094. Needs Cin % 64 == 0,
 * Cout % 64 == 0 and, with a folded input (in_scale), Cin <= 512. in_scale / in_shift / relu_in: BatchNorm + ReLU of the
 * producer applied on load; out_scale / out_shift / res / relu_out: folded inference epilogue (then no statistics);
 * statistics rows: capnet_conv1x1_tiles_m(M). Weights: capnet_conv1x1_f16x3_pack for tile width bn = capnet_conv1x1_f16x3_bn(M, Cout). */
/* The same convolution for a dense [M][Cin] input with Cin = 64 / 128 / 256 (conv3 of the bottlenecks of stages 1-3) with
 * the A operand resident in registers (csrc/conv1x1_areg.hip): every 128 rows are folded and split once for all output
 * columns. Same weight image (capnet_conv1x1_f16x3_pack, tile width bn), statistics rows capnet_conv1x1_tiles_m(M).
 * in_exp: the input is scaled by 2^in_exp on its way into the f16 planes and the result scaled back (exact). */
int capnet_conv1x1_fwd_areg(const float* x, const unsigned* image, int bn, float* y, const float* in_scale,
                            const float* in_shift, int relu_in, float* part_sum, float* part_sq, long M, int Cin, int Cout,
                            int in_exp, capnet_stream_t stream);
size_t capnet_conv1x1_f16x3_weight_words(int Cin, int Cout);
int capnet_conv1x1_f16x3_bn(long M, int Cout);
int capnet_conv1x1_f16x3_pack(const float* w_oi, unsigned* image, int Cout, int Cin, int bn,
                              capnet_stream_t stream);
int capnet_conv1x1_fwd_f16x3(const float* x, long sxb, long sxh, long sxw, const unsigned* image, int bn,
                             float* y, const float* in_scale, const float* in_shift, int relu_in,
                             float* part_sum, float* part_sq, int B, int H, int W, int Cin, int Cout,
                             int stride, const float* out_scale, const float* out_shift,
                             const float* res, int relu_out, capnet_stream_t stream);

/* The same kernel as an implicit GEMM over (tap, channel): k = 1 (pad 0) or k = 3 (pad 1), any stride. Weights:
 * capnet_conv_f16x3_pack of the OIHW tensor (capnet_conv_f16x3_weight_words(Cin, Cout, k) words) for tile width
 * bn = capnet_conv1x1_f16x3_bn(M, Cout); statistics rows capnet_conv1x1_tiles_m(M), M = B * OH * OW. */
size_t capnet_conv_f16x3_weight_words(int Cin, int Cout, int k);
int capnet_conv_f16x3_pack(const float* w_oihw, unsigned* image, int Cout, int Cin, int k, int bn,
                           capnet_stream_t stream);
int capnet_conv2d_fwd_f16x3(const float* x, long sxb, long sxh, long sxw, const unsigned* image, int bn, float* y,
                            const float* in_scale, const float* in_shift, int relu_in, float* part_sum,
                            float* part_sq, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                            const float* out_scale, const float* out_shift, const float* res, int relu_out,
                            capnet_stream_t stream);

/* The stride-1 3x3 convolutions with the tile's input patch staged once in LDS instead of once per tap
 * (csrc/conv3x3_patch.hip; torchvision Bottleneck.conv2, /root/reference/stylenet/model.py:14-33): dense NHWC x
 * [B][H][W][Cin], Cin % 32 == 0, Cout % bn == 0, W <= 56; weight image, bn and statistics rows exactly as
 * capnet_conv2d_fwd_f16x3 with k = 3. shared_chip != 0: other kernels run beside this one (several trunk passes in
 * flight) -- the <= 128-VGPR wave arrangement is used whatever the tile count; 0: launches of at most one tile per CU
 * split K between wave pairs (faster alone). Results differ between the two at rounding level only. */
int capnet_conv3x3_fwd_patch(const float* x, const unsigned* image, int bn, float* y, const float* in_scale,
                             const float* in_shift, int relu_in, float* part_sum, float* part_sq, int B, int H, int W,
                             int Cin, int Cout, int shared_chip, capnet_stream_t stream);

/* A bottleneck block's tail fused into the next block's first convolution (csrc/conv3x3_patch.hip). One launch computes
 *   tail_out [M][Cin] = relu(y3 * s1 + t1 + res (* s2 + t2))     -- torchvision Bottleneck.forward's `out += identity;
 *                                                                    relu(out)` behind bn3 (and the downsample's BatchNorm)
 *   y [M][Cout]       = tail_out . w^T                            -- the next block's conv1 (1x1, stride 1)
 * as /root/reference/stylenet/model.py:33 runs them through resnet152. s2 / t2 null: res is added as it is. Cin / 32 a
 * power of two; weight image (capnet_conv_f16x3_pack, k = 1), bn and statistics rows as capnet_conv2d_fwd_f16x3.
 * tail_out has exactly the values capnet_bn_add_relu would have written. */
int capnet_conv1x1_fwd_tail(const float* y3, const float* s1, const float* t1, const float* res, const float* s2,
                            const float* t2, float* tail_out, const unsigned* image, int bn, float* y, float* part_sum,
                            float* part_sq, long M, int Cin, int Cout, capnet_stream_t stream);
/* The three entry points above with the input's power-of-two prescale: the input tensor is multiplied by 2^in_exp on its
 * way into the f16 planes (folded into in_scale / in_shift where given; the tail written by capnet_conv1x1_fwd_tail
 * stays unscaled) and the accumulators by 2^-in_exp -- exact. With in_exp chosen so that max |input| 2^in_exp lies in
 * [2^14, 2^15) the result has fp32-grade RELATIVE accuracy whatever the scale of the tensor; without it (in_exp = 0)
 * inputs beyond 65 504 overflow the f16 pieces and inputs far below 1 lose their residuals to f16's subnormals.
 * capnet_trunk_forward applies it per tensor (input_exponents). */
int capnet_conv2d_fwd_f16x3_scaled(const float* x, long sxb, long sxh, long sxw, const unsigned* image, int bn, float* y,
                                   const float* in_scale, const float* in_shift, int relu_in, float* part_sum,
                                   float* part_sq, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                   int in_exp, capnet_stream_t stream);
int capnet_conv3x3_fwd_patch_scaled(const float* x, const unsigned* image, int bn, float* y, const float* in_scale,
                                    const float* in_shift, int relu_in, float* part_sum, float* part_sq, int B, int H,
                                    int W, int Cin, int Cout, int shared_chip, int in_exp, capnet_stream_t stream);
int capnet_conv1x1_fwd_tail_scaled(const float* y3, const float* s1, const float* t1, const float* res, const float* s2,
                                   const float* t2, float* tail_out, const unsigned* image, int bn, float* y,
                                   float* part_sum, float* part_sq, long M, int Cin, int Cout, int in_exp,
                                   capnet_stream_t stream);

/* The stem on the same arithmetic (csrc/conv_stem.hip): 7x7, stride 2, pad 3, 3 -> 64 channels; x is the NCHW image
 * (strides in floats, unit stride along W, W % 4 == 0, 16-B aligned rows), y is NHWC [B][OH][OW][64]. Replaces
 * torchvision resnet152.conv1 as run by /root/reference/stylenet/model.py:14-24,33. Weights: capnet_conv_stem_f16x3_pack
 * of the OIHW tensor [64][3][7][7] into capnet_conv_stem_f16x3_weight_words() words. part_sum / part_sq (or both
 * null): [capnet_conv_stem_f16x3_part_rows(B, H, W)][64], one row per workgroup, for capnet_bn_finalize. */
size_t capnet_conv_stem_f16x3_weight_words(void);
int capnet_conv_stem_f16x3_part_rows(int B, int H, int W);
int capnet_conv_stem_f16x3_pack(const float* w_oihw, unsigned* image, capnet_stream_t stream);
int capnet_conv_stem_fwd_f16x3(const float* x, long sxb, long sxc, long sxh, const unsigned* image, float* y,
                               float* part_sum, float* part_sq, int B, int H, int W, capnet_stream_t stream);

/* the low-VALU kernel used for every trunk convolution with Cin % 16 == 0 and Cout % 64 == 0:
 * NHWC channel-contiguous input, K-major weights, k_rows == KH*KW*Cin */
int capnet_conv2d_fwd_kmajor(const float* x, long sxb, long sxh, long sxw, const float* w_kmajor,
                             int k_rows, float* y, const float* in_scale, const float* in_shift,
                             int relu_in, float* part_sum, float* part_sq, int B, int H, int W,
                             int Cin, int Cout, int KH, int KW, int stride, int pad, int tile,
                             float* slabs, capnet_stream_t stream);
/* `slabs` (may be NULL = no tail balancing): scratch of capnet_conv_kmajor_slab_floats floats.
 * When the tile count is not a multiple of the 256 CUs, the tiles past the last full round are
 * cut into K-slices (fp32 partial slabs, summed in a fixed order by a fix-up launch) so that
 * every CU ends at the same time. */
size_t capnet_conv_kmajor_slab_floats(int M, int Cout, int k_rows, int tile);
/* the launch plan of that call: out5 = {tile, tiles, whole tiles, K-slices per tail tile,
 * k-tiles per slice} (diagnostics / tests) */
void capnet_conv_kmajor_plan(int M, int Cout, int k_rows, int tile, int* out5);
/* rows of the part_sum / part_sq arrays that call writes (tile = 0: its own choice) */
int capnet_conv_kmajor_tiles_m(int M, int Cout, int k_rows, int tile);
int capnet_conv_tiles_m(int M, int Cout, int tile);
/* The convolution kernels' eligibility predicates as their launchers and the trunk apply them: 1 = the kernel takes this
 * operand (address, strides in floats, shape), 0 = it refuses. Host code, no device; the pointers are only looked at. */
int capnet_conv_v2_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int B, int Cin, int Cout,
                            const float* in_scale, const float* in_shift);
int capnet_conv1x1_dma_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int B, int H, int W, int Cin,
                                int Cout, int stride);
int capnet_conv_f16x3_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int B, int H, int W, int Cin,
                               int Cout, int k, int stride, int pad, const float* in_scale, const float* in_shift);
int capnet_conv3x3_patch_eligible(const float* x, long sxb, long sxh, long sxw, long sxc, int B, int H, int W, int Cin,
                                  int Cout, int k, int stride, int pad, const float* in_scale, const float* in_shift);
int capnet_conv1x1_areg_eligible(const float* x, long M, int Cin, int Cout, int bn, const float* in_scale,
                                 const float* in_shift);
int capnet_conv1x1_tail_eligible(const float* y3, const float* res, long M, int Cin, int Cout);
int capnet_conv_stem_f16x3_eligible(const float* x, long sxb, long sxc, long sxh, long sxw, int B, int H, int W, int Cin,
                                    int Cout, int k, int stride, int pad);
int capnet_bn_finalize(const float* part_sum, const float* part_sq, int tiles, int C, long count,
                       const float* gamma, const float* beta, float* running_mean,
                       float* running_var, float momentum, float eps, float* scale, float* shift,
                       capnet_stream_t stream);
int capnet_bn_add_relu(const float* y, const float* s1, const float* t1, const float* res,
                       const float* s2, const float* t2, float* out, long rows, int C,
                       capnet_stream_t stream);
int capnet_bn_relu_maxpool(const float* y, const float* scale, const float* shift, float* out,
                           int B, int H, int W, int C, capnet_stream_t stream);
int capnet_global_avgpool(const float* x, float* out, int B, int HW, int C,
                          capnet_stream_t stream);

/* ---- encoder head: nn.BatchNorm1d(embed, momentum=0.01) -- stylenet/model.py:20,26 ------- */
int capnet_bn1d_fwd(const float* x, int B, int C, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int train, float momentum, float eps,
                    float* y, float* save_mean, float* save_invstd, capnet_stream_t stream);
int capnet_bn1d_bwd(const float* dy, const float* x, int B, int C, const float* gamma,
                    const float* save_mean, const float* save_invstd, float* dx, float* dgamma,
                    float* dbeta, capnet_stream_t stream);

/* ---- caption decoders: whole-sequence forward / BPTT ------------------------------------
 * dims (host int[10]) = {B, T, steps, N, E, F, H, V, has_features, cell}
 *   B batch, T caption columns, steps = max(lengths), N = sum(lengths) packed rows,
 *   E embed, F factored (ignored for cell 1), H hidden, V vocab,
 *   cell 0 = DecoderFactoredLSTM.forward  (stylenet/model.py:157-196, forward_step :115-155)
 *   cell 1 = DecoderRNN.forward           (nic/model.py:81-115, nn.LSTMCell :52,77)
 * batch_sizes (host int[steps]) = pack_padded_sequence(...).batch_sizes; tf_mask (host
 * uint8[steps]) = the per-step `random.random() < teacher_forcing_ratio` draws (model.py:181).
 * weights (host array of 32 device pointers):
 *   cell 0: [0..3]=V_{i,f,o,c}.weight [F][E]  [4..7]=V bias  [8..11]=S_g.weight (mode-selected)
 *           [12..15]=S bias  [16..19]=U_g.weight [H][F]  [20..23]=U bias
 *           [24..27]=W_g.weight [H][H]  [28..31]=W bias
 *   cell 1: [0]=lstm.weight_ih [4H][E]  [4]=lstm.bias_ih  [24]=lstm.weight_hh  [28]=lstm.bias_hh
 * emb = B.weight / embed.weight [V][E]; Cw/Cb = output projection (only read on free-running
 * steps, for the argmax feedback). hiddens [N][H] is the packed `torch.cat(hiddens, 0)`.
 * saved / saved_i / scratch: caller-provided device buffers of the sizes queried below; saved
 * buffers must reach the matching backward call untouched. err_flag: device int, set non-zero
 * when a token id is out of range (the caller checks it when it next synchronises).
 * capnet_seq_forward / _backward are capnet_seq_forward_stacked / _backward_stacked at nlayers = 1. */
size_t capnet_seq_saved_floats(const int* dims);
size_t capnet_seq_saved_ints(const int* dims);
/* Floats from the start of a layer's `saved` buffer to its cell states c [N][H] in packed row order (the final c of the
 * rows alive at the last step is the tail; the final h is the tail of the layer's hiddens). Read-only for the caller. */
size_t capnet_seq_saved_cell_offset(const int* dims);
size_t capnet_seq_fwd_scratch_floats(const int* dims);
size_t capnet_seq_bwd_scratch_floats(const int* dims);
int capnet_seq_forward(const int* dims, const int* batch_sizes, const unsigned char* tf_mask,
                       const long long* captions, const float* features, const float* emb,
                       const float* const* weights, const float* Cw, const float* Cb,
                       float dropout_p, unsigned long long seed, int training, float* saved,
                       int* saved_i, float* scratch, float* hiddens, int* err_flag,
                       capnet_stream_t stream);
/* grads (host array of 9 device pointers, all written, not accumulated):
 *   [0] dV  [4F][E] (cell 1: d weight_ih [4H][E])   [1] dV bias [4F]      (cell 1: unused)
 *   [2] dS  [4][F][F] (mode-selected S)              [3] dS bias [4F]
 *   [4] dU  [4][H][F]                                [5] dbias [4H] (U bias = W bias; cell 1:
 *                                                        bias_ih = bias_hh)
 *   [6] dW  [4H][H] (cell 1: d weight_hh)            [7] d emb [V][E]   [8] d features [B][E]|NULL
 * Gate order inside the packed blocks: cell 0 i,f,o,c ; cell 1 i,f,g,o (nn.LSTMCell). */
int capnet_seq_backward(const int* dims, const int* batch_sizes, const float* d_hiddens,
                        const float* hiddens, const float* saved, const int* saved_i,
                        float* scratch, float* const* grads, float dropout_p,
                        unsigned long long seed, int training, capnet_stream_t stream);

/* 1 to 8 layers: at nlayers = 1 either cell (capnet_seq_forward / _backward); more are stacked FactoredLSTM layers
 * (cell 0 only; BASELINE configs[3] / [4]: "2-layer", "3-layer"). PERF-ONLY, PARITY UNPINNED: the reference
 * advertises lstm_layers 1, 2, 3 (README.md:24) but its decoders ignore num_layers (stylenet/model.py:37); the semantics
 * are SURVEY App. A-1's, modelled on the only stacking in the tree (seq2seq/model.py:45-49): layer l > 0 is the same
 * factored cell on dropout(hidden of layer l - 1) at the same step (V: Linear(H -> F)), the top layer's hidden feeds C.
 * dims = capnet_seq_forward's of layer 0; the layers above have E = H and no features (sizes: capnet_seq_saved_floats
 * etc. with those dims). weights: nlayers x 32 pointers in capnet_seq_forward's order; saved / saved_i / hiddens: one
 * buffer per layer (the top layer's hiddens [N][H] are the output); scratch as capnet_seq_forward's.
 * Backward: d_hiddens of the top layer in; grads: nlayers x 9 pointers in capnet_seq_backward's order (dEmb / dFeat of
 * layer 0 only); dh_work: nlayers - 1 buffers [N][H]; scratch: the largest capnet_seq_bwd_scratch_floats of the layers.
 * `training` is a bit set in both calls: 0 = inference, 1 = training (dropout p on the token embeddings and between
 * the layers), 3 = training with dropout on the token embeddings ONLY and none between the layers -- torch.nn.LSTM
 * built without dropout=, the one stacking the reference has (capnet.seq2seq; seq2seq/model.py:46-49, 140-143), where
 * cell 1 at nlayers > 1 is reference-pinned. Forward and backward of one step must get the same value. */
int capnet_seq_forward_stacked(const int* dims, int nlayers, const int* batch_sizes, const unsigned char* tf_mask,
                               const long long* captions, const float* features, const float* emb,
                               const float* const* weights, const float* Cw, const float* Cb, float dropout_p,
                               unsigned long long seed, int training, float* const* saved, int* const* saved_i,
                               float* scratch, float* const* hiddens, int* err_flag, capnet_stream_t stream);
int capnet_seq_backward_stacked(const int* dims, int nlayers, const int* batch_sizes, const float* d_hiddens,
                                const float* const* hiddens, const float* const* saved, const int* const* saved_i,
                                float* scratch, float* const* dh_work, float* const* grads, float dropout_p,
                                unsigned long long seed, int training, capnet_stream_t stream);

/* ---- attention decoders: DecoderFactoredLSTMAtt.forward (stylenet/model_att.py:238-305) and
 * DecoderRNNAtt.forward (nic/model_att.py:152-202) ----
 * dims (host int[12]) = {B, T, steps, N, E, F, H, V, A, P, C, cell}: A attention size, P pixels
 * (14*14), C feature size (2048; must be a multiple of 512); cell 0 = factored LSTM, cell 1 =
 * nn.LSTMCell(E+C, H) (F ignored, pass 4; weights[0]/[4] = weight_ih [4H][E+C] / bias_ih,
 * weights[24]/[28] = weight_hh / bias_hh, the other V/S/U/W slots NULL; grads[0] = d weight_ih,
 * grads[5]/[6] first 4H rows = d weight_hh / d bias_ih = d bias_hh, grads[1..4] may be NULL). captions are the reference's
 * captions[:, :-1] (T columns), batch_sizes / tf_mask as for capnet_seq_forward, features the
 * NHWC map [B][P][C] of the attention encoder (no gradient: the trunk is frozen).
 * weights (host array of 44 device pointers): [0..31] V/S/U/W weights and biases per gate as in
 * capnet_seq_forward (V_g is [F][E+C]); [32,33] init_h w,b  [34,35] init_c  [36,37] the selected
 * attention module's encoder_att  [38,39] decoder_att  [40,41] full_att  [42,43] f_beta.
 * Outputs: hiddens [N][H]; alphas [B][steps][P] (zero where a sequence has ended, :261,296).
 * encoder_att(features) is computed once per call, not once per step (:59,279).
 * capnet_att_seq_forward / _backward are capnet_att_seq_forward_stacked / _backward_stacked at nlayers = 1. */
/* Process-wide choice for the factored cell's input product U_g (S_g (V_g x + bV_g) + bS_g) (stylenet/model_att.py:196-236)
 * inside capnet_att_seq_forward/backward: 0 = by shape (batches of at most 16 rows run it as ONE product per step against
 * U_g S_g V_g, formed once per call, and form the intermediate rows for all steps at once in the backward: the steps of
 * such a batch are chains of dependent launches, six of them this product's), 1 = always, -1 = never (three products per
 * step each way). Returns the previous choice. Set it between calls, not between a forward and its backward. */
int capnet_att_set_chain_mode(int mode);
size_t capnet_att_saved_floats(const int* dims);
size_t capnet_att_saved_ints(const int* dims);
size_t capnet_att_fwd_scratch_floats(const int* dims);
size_t capnet_att_bwd_scratch_floats(const int* dims);
/* One attention step for `rows` rows (Attention.forward, stylenet/model_att.py:51-70, plus the
 * f_beta gate of :283-284), as used per time step inside capnet_att_seq_forward and per decode
 * step by sample() (model_att.py:352-357). att1 [rows][P][A] = encoder_att(features) (hoisted),
 * feat [rows][P][C], att2 (ld ldz) = decoder_att(h), gate_io (ld ldz): f_beta(h) in, sigmoid out;
 * w_full [A], b_full [1]. Outputs: alpha_out [rows][P]; alphas_bt[(row*steps + t)*P + p] (the
 * user-visible alphas tensor); awe_out [rows][C] (ungated context); xa_out (ld ldx) = gate*awe.
 * scores_ws: scratch [rows][P] (the scores before the softmax). */
int capnet_att_step_fwd(const float* att1, const float* feat, const float* att2, float* gate_io,
                        long ldz, const float* w_full, const float* b_full, int rows, int P, int A,
                        int C, float* alpha_out, float* alphas_bt, int steps, int t, float* awe_out,
                        float* xa_out, long ldx, float* scores_ws, capnet_stream_t stream);

int capnet_att_seq_forward(const int* dims, const int* batch_sizes, const unsigned char* tf_mask,
                           const long long* captions, const float* features, const float* emb,
                           const float* const* weights, const float* Cw, const float* Cb,
                           float dropout_p, unsigned long long seed, int training, float* saved,
                           int* saved_i, float* scratch, float* hiddens, float* alphas,
                           int* err_flag, capnet_stream_t stream);
/* grads (host array of 16 device pointers, all written): [0] dV [4F][E+C]  [1] dV bias [4F]
 * [2] dS [4][F][F]  [3] dS bias  [4] dU [4][H][F]
 * [5] dWz [4H+A+C][H] = [dW_i; dW_f; dW_o; dW_c; d decoder_att.weight; d f_beta.weight]
 * [6] dbz [4H+A+C] (first 4H: U and W biases)  [7] d encoder_att.weight [A][C]  [8] its bias
 * [9] d full_att.weight [A]  [10] d full_att.bias [1]  [11] d init_h.weight [H][C]  [12] bias
 * [13] d init_c.weight  [14] bias  [15] d emb [V][E].  d_alphas may be NULL. */
int capnet_att_seq_backward(const int* dims, const int* batch_sizes, const float* d_hiddens,
                            const float* d_alphas, const float* hiddens, const float* features,
                            const float* const* weights, const float* saved, const int* saved_i,
                            float* scratch, float* const* grads, float dropout_p,
                            unsigned long long seed, int training, capnet_stream_t stream);

/* The attention decoder of 1 to 8 layers: at nlayers = 1 either cell (capnet_att_seq_forward / _backward); more layers are
 * capnet.stacked_att.StackedFactoredLSTMAtt (cell 0 only; PERF-ONLY, PARITY UNPINNED: the reference ignores
 * num_layers). Layer 0 is capnet_att_seq_forward's cell; layer l > 0 is the factored cell on
 * dropout_l(h^{l-1}_t) (the mask capnet_rows_dropout draws for layer l, training only) with initial state
 * init_h{l} / init_c{l}(mean over pixels); only the top layer feeds C (the argmax of free-running steps).
 * dims: as capnet_att_seq_forward. saved[l] / saved_i[l]: capnet_att_stacked_saved_floats / _ints(dims, l) each;
 * hiddens[0]: [N][H]; hiddens[l > 0]: [B + N][H] (rows 0..B-1 the layer's initial state, then the packed rows).
 * weights: layer 0's 44 tensors of capnet_att_seq_forward, then per layer l > 0 36: the 32 of capnet_seq_forward (V w x4
 * ([F][H]), V b x4, S w x4, S b x4, U w x4, U b x4, W w x4, W b x4), init_h{l} w [H][C], b, init_c{l} w, b.
 * A lone step of an upper layer with <= 16 rows is one launch (the fused upper step) unless the environment has
 * CAPNET_NO_FUSED_UPPER_STEP=1 at the call. */
size_t capnet_att_stacked_saved_floats(const int* dims, int layer);
size_t capnet_att_stacked_saved_ints(const int* dims, int layer);
size_t capnet_att_stacked_fwd_scratch_floats(const int* dims, int nlayers);
size_t capnet_att_stacked_bwd_scratch_floats(const int* dims, int nlayers);
int capnet_att_seq_forward_stacked(const int* dims, int nlayers, const int* batch_sizes, const unsigned char* tf_mask,
                                   const long long* captions, const float* features, const float* emb,
                                   const float* const* weights, const float* Cw, const float* Cb, float dropout_p,
                                   unsigned long long seed, int training, float* const* saved, int* const* saved_i,
                                   float* scratch, float* const* hiddens, float* alphas, int* err_flag,
                                   capnet_stream_t stream);
/* grads: layer 0's 16 buffers of capnet_att_seq_backward, then per layer l > 0 eleven: d V [4F][H], d bV [4F],
 * d S [4][F][F], d bS [4F], d U [4][H][F], d bUW [4H] (of both the U and the W bias), d W [4H][H], d init_h{l} w [H][C],
 * b [H], d init_c{l} w, b. d_hiddens: the top layer's packed rows [N][H]; dh_work: nlayers - 1 buffers [N][H]. */
int capnet_att_seq_backward_stacked(const int* dims, int nlayers, const int* batch_sizes, const float* d_hiddens,
                                    const float* d_alphas, const float* const* hiddens, const float* features,
                                    const float* const* weights, const float* const* saved, const int* const* saved_i,
                                    float* scratch, float* const* dh_work, float* const* grads, float dropout_p,
                                    unsigned long long seed, int training, capnet_stream_t stream);

/* Single-step pieces used by forward_step() / sample() (no autograd):
 *   out[r] = emb[idx[r]]                      -- self.B(k_prev_words), stylenet/model.py:221
 *   gate pointwise on pre-activations [b][4H] (in place: overwritten by the activated gates),
 *   cell 0: blocks i,f,o,c~ and h = o*c (model.py:147-153); cell 1: i,f,g,o and h = o*tanh(c). */
int capnet_embedding_fwd(const long long* idx, int n, const float* emb, int E, int V, float* out,
                         int* err_flag, capnet_stream_t stream);
int capnet_lstm_pointwise_fwd(float* pre, const float* c_prev, float* c_out, float* h_out, int b,
                              int H, int cell, capnet_stream_t stream);
/* ... and its backward (the cell of capnet.stacked's layers): gates = the ACTIVATED gates the forward left in `pre`,
 * c / c_prev the new / previous cell state (c_prev NULL = zeros), dh = dL/dh; dc_io: in dL/dc, out dL/dc_prev;
 * dpre [b][4H] = dL/d pre-activations. */
int capnet_lstm_pointwise_bwd(const float* gates, const float* c, const float* c_prev, const float* dh, float* dc_io,
                              float* dpre, int b, int H, int cell, capnet_stream_t stream);

/* One beam-search step of capnet.stacked.StackedFactoredLSTM (inference: no dropout), every layer, one launch per layer
 * on `stream`; no host synchronisation, no allocation. Layer l computes, for `rows` rows,
 *   gates = [x | h_prev] . wcat[l]^T + beff[l];  i, f, o = sigmoid, c~ = tanh;  c = f c_prev + i c~;  h = o c
 * with wcat[l] [4H][kin_l + H] = [U_g S_g V_g (zero columns up to kin_l) | W_g] in gate blocks i, f, o, c~ and
 * beff[l] [4H] = U_g (S_g bV_g + bS_g) + bU_g + bW_g (the chain folded on the host; stylenet/model.py:115-155 at
 * inference). kin_0 = E rounded up to a multiple of 16, kin_l = H above. Layer 0's x: with `tokens` (int64 [rows]),
 * row tokens[r] of the table x [V][E] (an id outside [0, V) sets bit 0 of *err_flag and reads row 0); without, x is the
 * inputs [rows][E]. Layer l > 0's x is layer l-1's new h.
 * state_in / state_out: [rows][2 nlayers][H] (slot 2l = h of layer l, 2l+1 = c), distinct, 16-B aligned;
 * h_top [rows][H] receives the top layer's h once more. wcat / beff: HOST arrays of nlayers device pointers.
 * H in {64, 128, 256, 512, 1024}, kin_0 + H <= 2048, 1 <= nlayers <= 8. */
int capnet_stacked_decode_step(int nlayers, int rows, int E, int H, int V, const long long* tokens, const float* x,
                               const float* const* wcat, const float* const* beff, const float* state_in,
                               float* state_out, float* h_top, int* err_flag, capnet_stream_t stream);

/* capnet_stacked_decode_step for either cell: cell 0 = the factored cell (exactly capnet_stacked_decode_step), cell 1 =
 * nn.LSTMCell (capnet.nic_stacked: StackedDecoderRNN, the upper layers of StackedDecoderRNNAtt), whose h = o tanh(c):
 * wcat[l] = [weight_ih (zero columns up to kin_l) | weight_hh] and beff[l] = bias_ih + bias_hh, with torch's gate
 * blocks i, f, g, o reordered to i, f, o, c~ = g on the host. Same shapes, bounds and checks otherwise. */
int capnet_stacked_decode_step_cell(int cell, int nlayers, int rows, int E, int H, int V, const long long* tokens,
                                    const float* x, const float* const* wcat, const float* const* beff,
                                    const float* state_in, float* state_out, float* h_top, int* err_flag,
                                    capnet_stream_t stream);

/* capnet_stacked_decode_step_cell reading the previous state through a beam search's parent rows: with parent_rows (int64
 * [rows], device), row r's h_prev and c_prev of every layer are those of row parent_rows[r] of state_in -- the result of
 * the step on state_in.index_select(0, parent_rows), bit for bit, without that copy. x, tokens, state_out and h_top stay
 * indexed by the row itself; parents may repeat (state_in != state_out). A parent outside [0, rows) sets bit 0 of *err_flag
 * and the row reads itself; parent_rows needs err_flag. parent_rows NULL: exactly capnet_stacked_decode_step_cell. */
int capnet_stacked_decode_step_gather(int cell, int nlayers, int rows, int E, int H, int V, const long long* tokens,
                                      const float* x, const float* const* wcat, const float* const* beff,
                                      const float* state_in, const long long* parent_rows, float* state_out, float* h_top,
                                      int* err_flag, capnet_stream_t stream);

/* capnet_stacked_decode_step_gather for `groups` weight groups in the same launches (every style of a factored decoder at
 * once): rows = groups x rows_per_group, group-major -- group g owns rows g rows_per_group .. (g + 1) rows_per_group - 1
 * -- and its rows run on ITS weights: wcat[l] is [groups][4H][kin_l + H] and beff[l] [groups][4H], one device buffer per
 * layer. The grid of a layer's launch is (H / 4, groups); a 16-row tile never reaches into the next group. Row r of group
 * g is, bit for bit, the row of capnet_stacked_decode_step_gather on group g's rows and weights alone. tokens, x,
 * parent_rows, state_in, state_out and h_top cover all the rows; a parent is checked against [0, rows), not against its
 * group. 1 <= groups <= 8; groups = 1 is exactly capnet_stacked_decode_step_gather. Same shapes and checks otherwise. */
int capnet_stacked_decode_step_groups(int cell, int nlayers, int groups, int rows_per_group, int E, int H, int V,
                                      const long long* tokens, const float* x, const float* const* wcat,
                                      const float* const* beff, const float* state_in, const long long* parent_rows,
                                      float* state_out, float* h_top, int* err_flag, capnet_stream_t stream);

/* capnet_stacked_decode_step_groups with one layer-0 table PER GROUP (capnet.seq2seq: every emotion's DecoderRNN owns its
 * embedding): tables is a HOST array of `groups` device pointers, tables[g] [V][E], and row r of group g reads
 * tables[g][tokens[r]] -- the kernel receives the pointers by value and picks its group's by the workgroup's group index;
 * no table is copied or stacked. tokens is required (there are no input rows); V is the same for every group. Row r of
 * group g is, bit for bit, the row of capnet_stacked_decode_step_gather on group g's rows, weights and table alone. A
 * token id outside [0, V) sets bit 0 of *err_flag and reads row 0 of its group's table. E + H (E rounded up to 16) <= 2048,
 * the narrow kernel. Every tables[g] non-NULL. Same shapes and checks otherwise. */
int capnet_stacked_decode_step_tables(int cell, int nlayers, int groups, int rows_per_group, int E, int H, int V,
                                      const long long* tokens, const float* const* tables, const float* const* wcat,
                                      const float* const* beff, const float* state_in, const long long* parent_rows,
                                      float* state_out, float* h_top, int* err_flag, capnet_stream_t stream);

/* tokens[r] = the FIRST argmax over v of h[r] . w[v] + b[v], r < rows: the vocabulary projection (nn.Linear: w [V][H],
 * b [V] or NULL) and the row argmax in one launch, fp32 throughout, the logits never stored. A -inf or NaN logit is never
 * picked and a row with nothing to pick yields 0, as capnet_argmax_rows. rows >= 1, V >= 1, H in {64, 128, 256, 512,
 * 1024}; h [rows][H], w and the workspace 16-B aligned. workspace: capnet_vocab_argmax_ws_bytes(rows, V) bytes of device
 * memory whose first 16 bytes are ZERO before the first use (they hold the arrival counter of the in-launch reduction;
 * every launch leaves them zero, so back-to-back calls on one stream may share a workspace; calls on different streams
 * may not). tokens: int64 [rows]. */
size_t capnet_vocab_argmax_ws_bytes(int rows, int V);
int capnet_vocab_argmax(const float* h, const float* w, const float* b, int rows, int H, int V, void* workspace,
                        long long* tokens, capnet_stream_t stream);

/* capnet_vocab_argmax for `groups` projections in one launch: rows = groups x rows_per_group, group-major, and group g's
 * rows are projected on w[g] [V][H] / b[g] [V] (w, b: HOST arrays of `groups` device pointers; b or any b[g] may be NULL;
 * every w[g] 16-B aligned; V the same for all groups). The grid is (ceil(V / 32), groups); each group has its own arrival
 * counter and its own block of partials, so no group waits on another, and tokens of group g are, bit for bit, those of
 * capnet_vocab_argmax on group g's rows and projection alone. workspace: capnet_vocab_argmax_groups_ws_bytes(groups,
 * rows_per_group, V) bytes whose first 16 groups bytes are ZERO before the first use (and are left zero). 1 <= groups <=
 * 8; groups = 1 is exactly capnet_vocab_argmax (the same grid, the same workspace layout). */
size_t capnet_vocab_argmax_groups_ws_bytes(int groups, int rows_per_group, int V);
int capnet_vocab_argmax_groups(const float* h, const float* const* w, const float* const* b, int groups, int rows_per_group,
                               int H, int V, void* workspace, long long* tokens, capnet_stream_t stream);

/* Greedy decoding of a stacked nn.LSTM + nn.Linear for a fixed number of steps (capnet.seq2seq: EncoderRNN.sample /
 * DecoderRNN.sample, seq2seq/model.py:100-122, 193-217; no end token, no dropout), the whole loop on `stream` with no
 * host synchronisation, no allocation and nothing read back: per step one launch per layer of
 * capnet_stacked_decode_step_cell's LSTM cell and one capnet_vocab_argmax launch, whose token the next step's layer 0
 * gathers its embedding row by. The first step's input is features [rows][E] (the encoder) or emb[start_tokens[r]]
 * (int64 [rows]; the decoders): exactly one of the two is non-NULL. emb [V][E]; wcat / beff: HOST arrays of nlayers device
 * pointers packed as for capnet_stacked_decode_step_cell with cell 1; Cw [V][H] / Cb [V] (or NULL) the projection.
 * state0: the initial [rows][2 nlayers][H] state (slot 2l = h of layer l, 2l+1 = c) or NULL for zeros; state_out receives
 * the state after the last step in the same layout (it may be state0). ids: int64 [rows][steps].
 * workspace: capnet_lstm_greedy_decode_ws_bytes(nlayers, rows, H, V) bytes, 16-B aligned, contents irrelevant.
 * A token id outside [0, V) (only start_tokens can hold one) sets bit 0 of *err_flag and reads row 0.
 * Shapes: those of capnet_stacked_decode_step_cell. */
size_t capnet_lstm_greedy_decode_ws_bytes(int nlayers, int rows, int H, int V);
int capnet_lstm_greedy_decode(int nlayers, int rows, int E, int H, int V, int steps, const float* features,
                              const long long* start_tokens, const float* emb, const float* const* wcat,
                              const float* const* beff, const float* Cw, const float* Cb, const float* state0,
                              void* workspace, long long* ids, float* state_out, int* err_flag, capnet_stream_t stream);

/* capnet_lstm_greedy_decode for `groups` decoders at once (capnet.seq2seq.Seq2Seq.sample_styles: every emotion's
 * DecoderRNN from the encoder's final state): rows = groups x rows_per_group, group-major, and group g decodes on ITS
 * embedding emb[g] [V][E], LSTM weights and projection Cw[g] [V][H] / Cb[g] [V] -- per step one launch per layer of
 * capnet_stacked_decode_step_tables and one capnet_vocab_argmax_groups launch, so the launches of one decoder serve all.
 * emb, Cw, Cb: HOST arrays of `groups` device pointers (Cb itself may be NULL: no bias); nothing is stacked or copied. wcat[l]
 * [groups][4H][kin_l + H] and beff[l] [groups][4H], one device buffer per layer, as capnet_stacked_decode_step_groups. The
 * first input is emb[g][start_tokens[r]] (int64 [rows], required; features are not an input: the encoder is one group and
 * keeps capnet_lstm_greedy_decode). state0 [rows][2 nlayers][H] or NULL for zeros; ids int64 [rows][steps], group-major;
 * state_out as capnet_lstm_greedy_decode. Row r of group g is, bit for bit, the row of capnet_lstm_greedy_decode on group
 * g's rows and parameters alone. workspace: capnet_lstm_greedy_decode_groups_ws_bytes(nlayers, groups, rows_per_group, H,
 * V) bytes, 16-B aligned, contents irrelevant. Refused before any launch: groups outside 1..8, rows_per_group < 1, steps <
 * 1, layers outside 1..8, unsupported E / H, a NULL or misaligned pointer, a NULL entry of any table. */
size_t capnet_lstm_greedy_decode_groups_ws_bytes(int nlayers, int groups, int rows_per_group, int H, int V);
int capnet_lstm_greedy_decode_groups(int nlayers, int groups, int rows_per_group, int E, int H, int V, int steps,
                                     const long long* start_tokens, const float* const* emb, const float* const* wcat,
                                     const float* const* beff, const float* const* Cw, const float* const* Cb,
                                     const float* state0, void* workspace, long long* ids, float* state_out, int* err_flag,
                                     capnet_stream_t stream);

/* The whole beam search of a plain LSTM stack (capnet.beam.beam_search_device's loop for StackedFactoredLSTM /
 * StackedDecoderRNN / DecoderFactoredLSTM / DecoderRNN) in one call: n images x k fixed slots, rows i k .. i k + k - 1 are
 * image i's. Per step s = 1 .. max_steps, on `stream`: capnet_stacked_decode_step_gather on the previous step's words and
 * parent rows (no parents at s = 1), logits [n k][V] = h_top . Cw^T + Cb by capnet_sgemm_splitk's entry on `slab` (the
 * kernel choice and the logits of that call with that slab), capnet_beam_advance. Then capnet_beam_finish into seqs
 * int64 [n][max_steps + 2] and lengths int32 [n] (caller-owned device memory, 8- / 4-byte aligned).
 * cell, wcat, beff (HOST arrays of nlayers device pointers), emb [V][E]: as capnet_stacked_decode_step_cell; Cw [V][H],
 * Cb [V] or NULL. state0: the initial [n k][2 nlayers][H] state, NULL for zeros. max_steps = max_seq_length + 1 for the
 * decoders. workspace: capnet_beam_decode_ws_bytes(...) bytes of device memory, 16-B aligned, contents irrelevant (the two
 * state buffers, h_top, the logits, two word buffers, the parent rows and the capnet_beam_state_bytes block, each part
 * rounded up to 16 bytes; 0 for shapes outside 1 <= k <= 16, 1 <= nlayers <= 8). slab: at least n k V floats, 16-B aligned.
 * The call allocates nothing. poll_every = 0: no host synchronisation and nothing read. poll_every = m > 0: after every
 * m-th step short of the last, one blocking 4-byte read of the count of live beams; the loop stops at zero (same result).
 * *steps_run (host, may be NULL): the steps issued. A token id outside [0, V) (start_token) sets bit 0 of *err_flag.
 * Every bad argument is refused before any launch. */
size_t capnet_beam_decode_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps);
int capnet_beam_decode(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                       long long end_token, const float* emb, const float* const* wcat, const float* const* beff,
                       const float* Cw, const float* Cb, const float* state0, void* workspace, float* slab,
                       size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                       capnet_stream_t stream);

/* capnet_beam_decode over groups x n beam groups, beam group q = g n + i (weight group g, image i) at rows q k .. q k + k -
 * 1 and on group g's weights (capnet_stacked_decode_step_groups with rows_per_group = n k: wcat[l] [groups][4H][kin_l + H],
 * beff[l] [groups][4H]). emb, Cw, Cb and the beam bookkeeping are shared: the vocabulary projection is one product over all
 * groups n k rows, so its kernel choice -- and the last bit of a logit -- may differ from a search of one group alone.
 * workspace: capnet_beam_decode_ws_bytes(nlayers, groups n, ...); slab: at least groups n k V floats; seqs int64
 * [groups n][max_steps + 2], lengths int32 [groups n]; state0 [groups n k][2 nlayers][H] or NULL. 1 <= groups <= 8; groups =
 * 1 is exactly capnet_beam_decode. Every bad argument is refused before any launch. */
int capnet_beam_decode_groups(int cell, int nlayers, int groups, int n, int k, int E, int H, int V, int max_steps,
                              long long start_token, long long end_token, const float* emb, const float* const* wcat,
                              const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* workspace,
                              float* slab, size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run,
                              int* err_flag, capnet_stream_t stream);

/* The vocabulary projection of a beam step without its logits: for every row r < rows, over logit[v] = h[r] . w[v] + b[v]
 * (nn.Linear: w [V][H], b [V] or NULL), in ONE launch, fp32 throughout:
 *   index[r][0..k)  the k best entries by (logit descending, index ascending)       int32 [rows][k]
 *   values[r][j]    their logits                                                    f32 [rows][k]
 *   lse[r]          log(sum_v exp(logit[v]))                                        f32 [rows]
 * A NaN or -inf logit is never picked and does not enter the sum; a row with fewer than k pickable entries pads its tail
 * with (-inf, -1). A workgroup owns 32 entries and all rows and emits, per row, its maximum m_w, s_w = sum expf(logit -
 * m_w) and its k best; the workgroup that arrives last at the arrival counter merges them in a fixed order (M = max m_w,
 * lse = M + logf(sum s_w expf(m_w - M))), so the result does not depend on which workgroup that is. No workgroup waits on
 * another. 1 <= k <= 16, k <= V, rows >= 1, H in {64, 128, 256, 512, 1024}; h, w and the workspace 16-B aligned.
 * workspace: capnet_vocab_topk_ws_bytes(rows, k, V) bytes (0 outside the limits) of device memory whose first 16 bytes are
 * ZERO before the first use (the arrival counter; every launch leaves them zero, so back-to-back calls on one stream may
 * share a workspace; calls on different streams may not). Bad arguments are refused before any launch. */
size_t capnet_vocab_topk_ws_bytes(int rows, int k, int V);
int capnet_vocab_topk(const float* h, const float* w, const float* b, int rows, int H, int V, int k, void* workspace,
                      float* values, int* index, float* lse, capnet_stream_t stream);

/* ---- sampled decoding: temperature and top-k sampling (csrc/vocab_sample.hip, csrc/sample_rng.h) ----
 * The random stream, on the HOST (no GPU): u(seed, step, row, v) = (2 b + 1) / 2^24, b the top 23 bits of the finalized
 * hash of seed + 0x9E3779B97F4A7C15 (((step << 48) | (row << 24) | v) + 1): an odd multiple of 2^-24, strictly inside
 * (0, 1), exact in fp32. step <= 65535, row < 2^24, v < 2^24. The kernels below draw
 *   token = argmax_v (logit_v / T - logf(-logf(u(seed, step, row0 + r, v)))),   ties to the lower v
 * a draw from softmax(logit / T) (Gumbel-max), so a caller can reproduce every draw from the logits alone. */
float capnet_sample_uniform(unsigned long long seed, unsigned step, unsigned row, unsigned v);

/* tokens[r] (int64) = a draw from softmax((h[r] . w + b) / temperature), logp[r] = its log-probability under that
 * distribution, in ONE launch, the logits never in memory (capnet_vocab_argmax's mapping; noise in the epilogue). h [rows][H],
 * w [V][H], b [V] or NULL; H in {64, 128, 256, 512, 1024}; rows < 2^24, V <= 2^24; temperature finite and > 0. A NaN or -inf
 * logit is never drawn and adds nothing to the normaliser; a row with nothing to draw yields token 0 and logp = -inf.
 * row0: the stream row of row 0 (rows split over launches draw what one launch draws). workspace:
 * capnet_vocab_sample_ws_bytes(rows, V) bytes, 16-B aligned, whose first 16 bytes are ZERO before the first use and are
 * left zero (back-to-back calls on one stream may share it). Deterministic: the same bits whichever workgroup merges. */
size_t capnet_vocab_sample_ws_bytes(int rows, int V);
int capnet_vocab_sample(const float* h, const float* w, const float* b, int rows, int H, int V, float temperature,
                        unsigned long long seed, unsigned step, unsigned row0, void* workspace, long long* tokens, float* logp,
                        capnet_stream_t stream);

/* Top-k sampling on capnet_vocab_topk's outputs: the same draw among the k candidates values / index [rows][k] (1 <= k <= 16),
 * the noise keyed by the candidate's vocabulary index (V bounds it), logp renormalised over the k candidates. Padding
 * slots (-inf, -1) are never drawn; a row of padding yields token 0 and logp = -inf. */
int capnet_sample_pick(const float* values, const int* index, int rows, int k, int V, float temperature, unsigned long long seed,
                       unsigned step, unsigned row0, long long* tokens, float* logp, capnet_stream_t stream);

/* The same draw as capnet_vocab_sample from logits [rows][ld] in memory (ld >= V), one workgroup per row: any H, any V. */
int capnet_sample_rows(const float* logits, int rows, long ld, int V, float temperature, unsigned long long seed, unsigned step,
                       unsigned row0, long long* tokens, float* logp, capnet_stream_t stream);

/* `steps` sampled decode steps of a plain stack in ONE C call: capnet_lstm_greedy_decode's loop with the cell kind passed to
 * capnet_stacked_decode_step_cell and, in place of the argmax, capnet_vocab_sample at stream step t (top_k == 0) or
 * capnet_vocab_topk + capnet_sample_pick (1 <= top_k <= 16). The first input is first_inputs [rows][E] or
 * emb[start_tokens] (exactly one of them); state0 [rows][2 nlayers][H] or NULL for zeros. ids int64 [rows][steps], logp
 * float [rows][steps]; state_out [rows][2 nlayers][H] or NULL. No end token is looked at: all `steps` (<= 65535) steps run
 * and the caller truncates. workspace: capnet_sample_decode_ws_bytes(nlayers, rows, H, V, top_k) bytes (0: unsupported),
 * 16-B aligned, contents irrelevant. */
size_t capnet_sample_decode_ws_bytes(int nlayers, int rows, int H, int V, int top_k);
int capnet_sample_decode(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                         const long long* start_tokens, const float* emb, const float* const* wcat, const float* const* beff,
                         const float* Cw, const float* Cb, const float* state0, float temperature, int top_k,
                         unsigned long long seed, void* workspace, long long* ids, float* logp, float* state_out, int* err_flag,
                         capnet_stream_t stream);

/* The same for an attention decoder: n images x m samples each (row i m + j = sample j of image i; 1 <= m <= 16), the step
 * capnet_att_decode_step with k = m and every row continuing from itself, so an image's maps are read once per step for all
 * its samples; operands as capnet_att_beam_decode (state0 [n m][2 nlayers][H] is required; start_tokens int64 [n m]).
 * workspace: capnet_att_sample_decode_ws_bytes(...) bytes (0: unsupported), 16-B aligned; slab: the split-K slab. */
size_t capnet_att_sample_decode_ws_bytes(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k);
int capnet_att_sample_decode(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int steps,
                             const long long* start_tokens, const float* att1, const float* feat, const float* emb,
                             const float* wz, const float* bz, const float* w_full, const float* b_full,
                             const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                             const float* state0, float temperature, int top_k, unsigned long long seed, void* workspace,
                             float* slab, size_t slab_floats, long long* ids, float* logp, float* state_out, int* err_flag,
                             capnet_stream_t stream);

/* ---- nucleus (top-p) sampling (csrc/vocab_nucleus.hip) ----
 * The draw of capnet_sample_rows among the NUCLEUS of the row: with s_v = fl32(logit_v / T), the pickable entries (not NaN,
 * not -inf, v < V) ordered by s descending, then v ascending, and p = softmax(s) over them,
 *   before(v) = the sum of p_u over the entries strictly better than v,   N = { v : before(v) < top_p }
 * -- the smallest set of best entries whose probability reaches top_p, always holding the best one -- and
 *   token = argmax over N of (s_v - logf(-logf(u(seed, step, row0 + r, v)))),   logp = s_token - log sum_{v in N} exp(s_v),
 * the log-probability under the distribution sampled from. 0 < top_p <= 1; top_p == 1 is "off": capnet_sample_rows itself
 * (not a nucleus with p = 1, which would drop the tail once the fp32 mass rounds to 1). logits [rows][ld], ld >= V, any V up
 * to 2^24; one workgroup per row finds the edge of N by an exact search over the integer images of s with the index breaking
 * ties, every sum a fixed tree: the same bits at every call, whatever the order of the entries' arrival. */
int capnet_nucleus_rows(const float* logits, int rows, long ld, int V, float temperature, float top_p, unsigned long long seed,
                        unsigned step, unsigned row0, long long* tokens, float* logp, capnet_stream_t stream);

/* top_k, then top_p: the same rule among capnet_vocab_topk's k candidates values / index [rows][k] (1 <= k <= 16), p and logp
 * renormalised over the k, then over the kept ones. The order of the list does not matter. top_p == 1: capnet_sample_pick. */
int capnet_nucleus_pick(const float* values, const int* index, int rows, int k, int V, float temperature, float top_p,
                        unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp,
                        capnet_stream_t stream);

/* capnet_sample_decode with the nucleus draw, 0 < top_p < 1 (top_p == 1 is capnet_sample_decode's): per step the projection
 * into a logits block of the workspace (capnet_sgemm_splitk's product on `slab`, the split-K slab; it may be NULL when
 * top_k > 0) + capnet_nucleus_rows, or capnet_vocab_topk + capnet_nucleus_pick (1 <= top_k <= 16). Every other operand as
 * capnet_sample_decode; workspace: capnet_sample_decode_nucleus_ws_bytes(nlayers, rows, H, V, top_k) bytes (0: unsupported). */
size_t capnet_sample_decode_nucleus_ws_bytes(int nlayers, int rows, int H, int V, int top_k);
int capnet_sample_decode_nucleus(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                                 const long long* start_tokens, const float* emb, const float* const* wcat,
                                 const float* const* beff, const float* Cw, const float* Cb, const float* state0,
                                 float temperature, int top_k, float top_p, unsigned long long seed, void* workspace, float* slab,
                                 size_t slab_floats, long long* ids, float* logp, float* state_out, int* err_flag,
                                 capnet_stream_t stream);

/* The same for an attention decoder: capnet_att_sample_decode with the nucleus draw, 0 < top_p < 1. */
size_t capnet_att_sample_decode_nucleus_ws_bytes(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k);
int capnet_att_sample_decode_nucleus(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int steps,
                                     const long long* start_tokens, const float* att1, const float* feat, const float* emb,
                                     const float* wz, const float* bz, const float* w_full, const float* b_full,
                                     const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                     const float* state0, float temperature, int top_k, float top_p, unsigned long long seed,
                                     void* workspace, float* slab, size_t slab_floats, long long* ids, float* logp,
                                     float* state_out, int* err_flag, capnet_stream_t stream);

/* The sampling entries with greedy rows: each capnet_X_greedy is capnet_X with one more argument, greedy_stride, in front of
 * the stream; with greedy_stride 0 it is capnet_X, bit for bit. greedy_stride g >= 1: the rows (for the stand-alone draws
 * the PHYSICAL rows row0 + r) come in groups of g, an image's: row i g + j, j < g - 1, is sample j of image i and draws
 * with the noise row i (g - 1) + j -- the row it has in the same call without greedy rows and g - 1 rows per image, so its
 * tokens and log-probabilities are those of that call; row i g + g - 1 is the image's GREEDY row: its key is the scaled
 * logit itself, so its token is argmax_v logit_v (ties to the lower index), whatever the temperature, top_k or top_p (the
 * best word is in every truncation), and its logp is taken under the same distribution as a drawn row's. The loops
 * require rows % g == 0; the attention loops g == m (the decode step then runs m rows per image on one read of the maps,
 * m <= 16). The self-critical baseline of capnet.train.self_critical_step: one more row per image, not a second search. */
int capnet_vocab_sample_greedy(const float* h, const float* w, const float* b, int rows, int H, int V, float temperature,
                               unsigned long long seed, unsigned step, unsigned row0, void* workspace, long long* tokens,
                               float* logp, unsigned greedy_stride, capnet_stream_t stream);
int capnet_sample_pick_greedy(const float* values, const int* index, int rows, int k, int V, float temperature,
                              unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp,
                              unsigned greedy_stride, capnet_stream_t stream);
int capnet_sample_rows_greedy(const float* logits, int rows, long ld, int V, float temperature, unsigned long long seed,
                              unsigned step, unsigned row0, long long* tokens, float* logp, unsigned greedy_stride,
                              capnet_stream_t stream);
int capnet_sample_decode_greedy(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                                const long long* start_tokens, const float* emb, const float* const* wcat,
                                const float* const* beff, const float* Cw, const float* Cb, const float* state0,
                                float temperature, int top_k, unsigned long long seed, void* workspace, long long* ids,
                                float* logp, float* state_out, int* err_flag, unsigned greedy_stride,
                                capnet_stream_t stream);
int capnet_nucleus_rows_greedy(const float* logits, int rows, long ld, int V, float temperature, float top_p,
                               unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp,
                               unsigned greedy_stride, capnet_stream_t stream);
int capnet_nucleus_pick_greedy(const float* values, const int* index, int rows, int k, int V, float temperature, float top_p,
                               unsigned long long seed, unsigned step, unsigned row0, long long* tokens, float* logp,
                               unsigned greedy_stride, capnet_stream_t stream);
int capnet_sample_decode_nucleus_greedy(int cell, int nlayers, int rows, int E, int H, int V, int steps,
                                        const float* first_inputs, const long long* start_tokens, const float* emb,
                                        const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                        const float* state0, float temperature, int top_k, float top_p,
                                        unsigned long long seed, void* workspace, float* slab, size_t slab_floats,
                                        long long* ids, float* logp, float* state_out, int* err_flag, unsigned greedy_stride,
                                        capnet_stream_t stream);
int capnet_att_sample_decode_greedy(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int steps,
                                    const long long* start_tokens, const float* att1, const float* feat, const float* emb,
                                    const float* wz, const float* bz, const float* w_full, const float* b_full,
                                    const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                    const float* state0, float temperature, int top_k, unsigned long long seed,
                                    void* workspace, float* slab, size_t slab_floats, long long* ids, float* logp,
                                    float* state_out, int* err_flag, unsigned greedy_stride, capnet_stream_t stream);
int capnet_att_sample_decode_nucleus_greedy(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V,
                                            int steps, const long long* start_tokens, const float* att1, const float* feat,
                                            const float* emb, const float* wz, const float* bz, const float* w_full,
                                            const float* b_full, const float* const* wcat, const float* const* beff,
                                            const float* Cw, const float* Cb, const float* state0, float temperature,
                                            int top_k, float top_p, unsigned long long seed, void* workspace, float* slab,
                                            size_t slab_floats, long long* ids, float* logp, float* state_out, int* err_flag,
                                            unsigned greedy_stride, capnet_stream_t stream);

/* Sampled decoding with exclusions (csrc/sample_exclude.hip): words a row may not draw at a step -- no repeated n-gram, a
 * minimum length, banned words; the rule of capnet_beam_advance_constrained, its four trailing arguments in the same order
 * (no_repeat_ngram 0..4, min_words >= 0, banned: a DEVICE int32 array of n_banned <= 32 word ids, 4-byte aligned). Unlike in
 * the beam search an excluded word is treated as a -inf logit is: never drawn, never a top-k candidate, never in the
 * nucleus, and it adds nothing to any sum, so logp is that of the distribution renormalised over the allowed words.
 * The mask: unsigned [rows][W], W = ceil(V / 32); bit v & 31 of word v >> 5 of row r set = word v is excluded on launch row r.
 *
 * capnet_sample_exclusion_mask: the mask of stream step t (0-based, 0 <= t <= steps) of a decode whose ids are
 * [rows] x ld int64 (ld >= steps; words 0 .. t - 1 of a row are read; ids may be NULL at t = 0): row r is the hypothesis
 * [start_tokens[r], ids[r][0] .. ids[r][t - 1]] at step t + 1 (start_tokens NULL: the words alone), the tokens as drawn
 * whether or not the row has emitted end_token. Excluded: every banned word; end_token while t + 1 <= min_words; with g =
 * no_repeat_ngram >= 1 and at least g tokens, every word that would complete a g-gram the hypothesis already contains
 * (<start> counts; a context seen several times excludes several words). Every word of the mask is written.
 * capnet_mask_logits: -inf at the mask's set bits of logits [rows][ld] (ld >= V), for the draws that read logits from memory
 * (capnet_sample_rows, capnet_nucleus_rows, a top-k in front of capnet_sample_pick / capnet_nucleus_pick).
 * capnet_vocab_sample_masked: capnet_vocab_sample_greedy (greedy_stride 0: capnet_vocab_sample) under a mask, which is required.
 * A row with every word excluded gives token 0 and logp -inf.
 * capnet_vocab_topk_masked: capnet_vocab_topk under a mask: the k best of the ALLOWED entries, and lse is the log-sum-exp
 * over the allowed entries only.
 * All refuse bad arguments on the host before any launch (the offending name in capnet_last_error()). */
int capnet_sample_exclusion_mask(const long long* ids, long ld, int steps, const long long* start_tokens, int rows, int t, int V,
                                 long long end_token, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                                 unsigned* mask, capnet_stream_t stream);
int capnet_mask_logits(float* logits, int rows, long ld, int V, const unsigned* mask, capnet_stream_t stream);
int capnet_vocab_sample_masked(const float* h, const float* w, const float* b, int rows, int H, int V, float temperature,
                               unsigned long long seed, unsigned step, unsigned row0, const unsigned* mask, void* workspace,
                               long long* tokens, float* logp, unsigned greedy_stride, capnet_stream_t stream);
int capnet_vocab_topk_masked(const float* h, const float* w, const float* b, int rows, int H, int V, int k, const unsigned* mask,
                             void* workspace, float* values, int* index, float* lse, capnet_stream_t stream);

/* The sampling loops under exclusions, ONE pair that takes everything: capnet_sample_decode[_nucleus][_greedy] (top_p == 1:
 * the plain draws; greedy_stride 0: no greedy rows) with one more launch per step, capnet_sample_exclusion_mask on the
 * caller's ids and start_tokens (required), and the step's draw under that mask; the decode step is untouched. slab is needed
 * only where top_p < 1 and top_k == 0. workspace: capnet_[att_]sample_decode_excl_ws_bytes (the loop's own bytes, then the
 * mask: rows W 4 bytes, 16-B aligned; 0: unsupported). The other arguments are those of the entries they extend. */
size_t capnet_sample_decode_excl_ws_bytes(int nlayers, int rows, int H, int V, int top_k, float top_p);
int capnet_sample_decode_excl(int cell, int nlayers, int rows, int E, int H, int V, int steps, const float* first_inputs,
                              const long long* start_tokens, const float* emb, const float* const* wcat,
                              const float* const* beff, const float* Cw, const float* Cb, const float* state0, float temperature,
                              int top_k, float top_p, unsigned long long seed, void* workspace, float* slab, size_t slab_floats,
                              long long* ids, float* logp, float* state_out, int* err_flag, unsigned greedy_stride,
                              long long end_token, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                              capnet_stream_t stream);
size_t capnet_att_sample_decode_excl_ws_bytes(int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int top_k,
                                              float top_p);
int capnet_att_sample_decode_excl(int cell, int nlayers, int n, int m, int P, int A, int C, int E, int H, int V, int steps,
                                  const long long* start_tokens, const float* att1, const float* feat, const float* emb,
                                  const float* wz, const float* bz, const float* w_full, const float* b_full,
                                  const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                  const float* state0, float temperature, int top_k, float top_p, unsigned long long seed,
                                  void* workspace, float* slab, size_t slab_floats, long long* ids, float* logp,
                                  float* state_out, int* err_flag, unsigned greedy_stride, long long end_token,
                                  int no_repeat_ngram, int min_words, const int* banned, int n_banned, capnet_stream_t stream);

/* capnet_vocab_topk for `groups` projections in one launch: rows = groups x rows_per_group, group-major, and group g's rows
 * are projected on w[g] [V][H] / b[g] [V] (w, b: HOST arrays of `groups` device pointers; b or any b[g] may be NULL; every
 * w[g] 16-B aligned; V the same for all groups). The grid is (ceil(V / 32), groups); each group has its own arrival counter
 * and its own block of partials, and its last arriver merges its rows only, so no group waits on another, and values, index
 * and lse of group g ([groups rows_per_group][k], [groups rows_per_group][k], [groups rows_per_group], group-major) are, bit
 * for bit, those of capnet_vocab_topk on group g's rows and projection alone. workspace:
 * capnet_vocab_topk_groups_ws_bytes(groups, rows_per_group, k, V) bytes (0 outside 1 <= groups <= 8 or capnet_vocab_topk's
 * limits) whose first 16 groups bytes are ZERO before the first use (and are left zero). groups = 1 is exactly
 * capnet_vocab_topk (the same grid, the same workspace layout). */
size_t capnet_vocab_topk_groups_ws_bytes(int groups, int rows_per_group, int k, int V);
int capnet_vocab_topk_groups(const float* h, const float* const* w, const float* const* b, int groups, int rows_per_group,
                             int H, int V, int k, void* workspace, float* values, int* index, float* lse,
                             capnet_stream_t stream);

/* capnet_beam_decode's loop for a stack that starts from a GIVEN state and, optionally, from given first inputs
 * (capnet.seq2seq: DecoderRNN.sample_beam from the encoder's state, EncoderRNN.sample_beam from the feature column), one
 * weight group. first_inputs non-NULL ([n k][E], 16-B aligned): step 1 feeds those rows to layer 0 instead of
 * emb[start_token]; start_token then only seeds the sequences.
 * fused_topk = 1: a step is the gathered decode step (one launch per layer), capnet_vocab_topk on h_top and
 * capnet_beam_advance_topk; the workspace has no logits block and slab may be NULL. fused_topk = 0: a step is
 * capnet_beam_decode's (capnet_sgemm_splitk's entry on `slab`, at least n k V floats, then capnet_beam_advance).
 * workspace: capnet_lstm_beam_decode_ws_bytes(...) bytes, 16-B aligned, contents irrelevant (the two state buffers, h_top,
 * the logits or, fused, values | index | lse | capnet_vocab_topk's workspace, two word buffers, the parent rows and the
 * beam state; 0 outside the limits). Everything else -- cell, wcat, beff, emb, Cw, Cb, state0, seqs, lengths,
 * poll_every, *steps_run, the error word -- as capnet_beam_decode. The call allocates nothing; every bad argument is
 * refused before any launch. */
size_t capnet_lstm_beam_decode_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk);
int capnet_lstm_beam_decode(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                            long long end_token, const float* first_inputs, const float* emb, const float* const* wcat,
                            const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* workspace,
                            float* slab, size_t slab_floats, int fused_topk, int poll_every, long long* seqs, int* lengths,
                            int* steps_run, int* err_flag, capnet_stream_t stream);

/* capnet_lstm_beam_decode for `groups` decoders at once (capnet.seq2seq.Seq2Seq.sample_beam_styles: every emotion's
 * DecoderRNN from the encoder's final state): the search runs over groups x n sentences, sentence q = g n + i (group g,
 * sentence i) at rows q k .. q k + k - 1, and group g decodes on ITS embedding emb[g] [V][E], LSTM weights and projection
 * Cw[g] [V][H] / Cb[g] [V]. Per step: one launch per layer of capnet_stacked_decode_step_tables with the parent rows (a (H /
 * 4, groups) grid), then, fused_topk = 1, ONE capnet_vocab_topk_groups launch and one capnet_beam_advance_topk over all
 * groups n sentences; fused_topk = 0, one capnet_sgemm_splitk per group into that group's row block of the logits (same
 * stream, the one slab) and one capnet_beam_advance. emb, Cw, Cb: HOST arrays of `groups` device pointers, every emb[g] and
 * Cw[g] non-NULL and 16-B aligned (Cb itself or any Cb[g] may be NULL: no bias); nothing is stacked or copied. wcat[l]
 * [groups][4H][kin_l + H] and beff[l] [groups][4H], one device buffer per layer, as capnet_stacked_decode_step_groups. There
 * are no first_inputs: the emotion decoders never take a feature column. state0 [groups n k][2 nlayers][H] or NULL; seqs
 * int64 [groups n][max_steps + 2], lengths int32 [groups n]; slab (unfused) at least groups n k V floats. workspace:
 * capnet_lstm_beam_decode_groups_ws_bytes(...) bytes (0 outside 1 <= groups <= 8 or capnet_lstm_beam_decode's limits at
 * groups n sentences), 16-B aligned, contents irrelevant. The lists of group g are those of capnet_lstm_beam_decode on group
 * g's sentences and parameters alone; groups = 1 returns capnet_lstm_beam_decode's lists (without first_inputs). Everything
 * else as capnet_lstm_beam_decode; every bad argument is refused before any launch. */
size_t capnet_lstm_beam_decode_groups_ws_bytes(int nlayers, int groups, int n, int k, int H, int V, int max_steps,
                                               int fused_topk);
int capnet_lstm_beam_decode_groups(int cell, int nlayers, int groups, int n, int k, int E, int H, int V, int max_steps,
                                   long long start_token, long long end_token, const float* const* emb,
                                   const float* const* wcat, const float* const* beff, const float* const* Cw,
                                   const float* const* Cb, const float* state0, void* workspace, float* slab,
                                   size_t slab_floats, int fused_topk, int poll_every, long long* seqs, int* lengths,
                                   int* steps_run, int* err_flag, capnet_stream_t stream);

/* capnet.seq2seq's beam searches under constraints (capnet.beam.Constraints; the rule and the trailing arguments of
 * capnet_beam_decode_forced: no_repeat_ngram 0..4, min_words >= 0, banned a DEVICE int32 array of n_banned <= 32 ids, forced a
 * DEVICE int32 array of n_forced <= 4 ids, n_forced = 0: none). An excluded word leaves a step's SELECTION only: it stays
 * in the row's log-sum-exp, so a caption's score is the model's own summed log-probability, on either step.
 *
 * capnet_beam_exclusion_mask: what each of the n k rows of a device beam search (the state of capnet_beam_init /
 * capnet_beam_advance*, n images x k slots, max_steps) may not select at step `step` (1-based, <= max_steps), as the bit mask
 * of capnet_sample_exclusion_mask: unsigned [n k][ceil(V / 32)], every word written. Row r is the hypothesis in slot r % k of
 * image r / k as step `step` reads it -- `step` tokens, <start> first, the tokens capnet_beam_advance_constrained derives its
 * exclusions from -- under capnet.beam.banned_words (forced words are not part of it). The rows of dead slots get a mask
 * nobody reads; a token outside [0, V) is never an address. One launch, the kernel of capnet_sample_exclusion_mask.
 * capnet_vocab_topk_select: capnet_vocab_topk under a SELECTION mask: an entry whose bit is set is not ranked and never a
 * candidate (a row with fewer than k allowed entries ends in (-inf, -1)), while lse is the log-sum-exp over every finite
 * entry -- bit for bit capnet_vocab_topk's; values and index are bit for bit capnet_vocab_topk_masked's.
 * capnet_vocab_topk_groups_masked: capnet_vocab_topk_groups under a mask [groups rows_per_group][ceil(V / 32)] indexed by the
 * launch's row; select_only = 1: capnet_vocab_topk_select's meaning, 0: capnet_vocab_topk_masked's. Group g's outputs are bit
 * for bit those of the single launch on its rows, projection and mask rows.
 * capnet_lstm_beam_decode_constrained / capnet_lstm_beam_decode_groups_constrained: capnet_lstm_beam_decode[_groups] whose every
 * step selects under the constraints. fused_topk = 0: capnet_beam_advance_constrained (n_forced > 0: capnet_beam_advance_forced)
 * on the logits block. fused_topk = 1 (n_forced must be 0): the decode step, capnet_beam_exclusion_mask,
 * capnet_vocab_topk_select (groups: capnet_vocab_topk_groups_masked, select_only = 1) and the unchanged
 * capnet_beam_advance_topk -- one more small launch per step. workspace: the *_constrained_ws_bytes functions: the
 * unconstrained layout and, fused, the mask behind it (n k ceil(V / 32) 4 bytes rounded up to 16), so
 * capnet_beam_decode_ws_beam_offset still tells where the state lies. Every bad argument is refused before any launch. */
int capnet_beam_exclusion_mask(const void* beam, int n, int k, int max_steps, int step, int V, long long end_token,
                               int no_repeat_ngram, int min_words, const int* banned, int n_banned, unsigned* mask,
                               capnet_stream_t stream);
int capnet_vocab_topk_select(const float* h, const float* w, const float* b, int rows, int H, int V, int k, const unsigned* mask,
                             void* workspace, float* values, int* index, float* lse, capnet_stream_t stream);
int capnet_vocab_topk_groups_masked(const float* h, const float* const* w, const float* const* b, int groups, int rows_per_group,
                                    int H, int V, int k, const unsigned* mask, int select_only, void* workspace, float* values,
                                    int* index, float* lse, capnet_stream_t stream);
size_t capnet_lstm_beam_decode_constrained_ws_bytes(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk);
int capnet_lstm_beam_decode_constrained(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps,
                                        long long start_token, long long end_token, const float* first_inputs, const float* emb,
                                        const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                        const float* state0, void* workspace, float* slab, size_t slab_floats, int fused_topk,
                                        int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                        capnet_stream_t stream, int no_repeat_ngram, int min_words, const int* banned,
                                        int n_banned, const int* forced, int n_forced);
size_t capnet_lstm_beam_decode_groups_constrained_ws_bytes(int nlayers, int groups, int n, int k, int H, int V, int max_steps,
                                                           int fused_topk);
int capnet_lstm_beam_decode_groups_constrained(int cell, int nlayers, int groups, int n, int k, int E, int H, int V, int max_steps,
                                               long long start_token, long long end_token, const float* const* emb,
                                               const float* const* wcat, const float* const* beff, const float* const* Cw,
                                               const float* const* Cb, const float* state0, void* workspace, float* slab,
                                               size_t slab_floats, int fused_topk, int poll_every, long long* seqs,
                                               int* lengths, int* steps_run, int* err_flag, capnet_stream_t stream,
                                               int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                                               const int* forced, int n_forced);

/* One beam step of an attention decoder (DecoderFactoredLSTMAtt / DecoderRNNAtt and their stacked forms) without the
 * vocabulary projection, for n images x k fixed slots (row r belongs to image r / k), on `stream`, in this order:
 *   1. z [n k][A + C] = h_prev . wz^T + bz, wz = [decoder_att; f_beta] stacked ([A + C][H]), h_prev = layer 0's h of every
 *      row of state_in, NOT gathered, by capnet_sgemm_splitk's entry on `slab`;
 *   2. two attention launches that handle the k beams of an image together on ONE read of its maps: att1 [n][P][A]
 *      (= encoder_att(feat), the caller's) and feat [n][P][C] are per image, never per row; att2 and the gate
 *      pre-activation of row r are z's row parent_rows[r] (z is only read: no sigmoid is written back); the second launch
 *      writes xa [n k][E + C] = [emb[tokens[r]] | sigmoid(gate) * context];
 *   3. layer 0 of capnet_stacked_decode_step_gather's kernel family on the dense xa rows (E + C rounded up to 16, plus H,
 *      may reach 4096: above 2048 the wide kernel of the family), h and c read at row parent_rows[r];
 *   4. layers 1 .. nlayers - 1, plain H -> H cells on the layer below, as capnet_stacked_decode_step_gather.
 * cell / wcat / beff (HOST arrays of nlayers device pointers) as capnet_stacked_decode_step_cell, wcat[0] [4H][kin + H] with
 * kin = E + C rounded up to 16. state_in / state_out [n k][2 nlayers][H], different buffers; h_top [n k][H].
 * parent_rows: int64 [n k] or NULL (every row its own parent); one outside [0, n k) sets bit 0 of *err_flag and the row reads
 * itself. A token id outside [0, V) sets bit 0 of *err_flag and reads row 0 of emb [V][E].
 * workspace: capnet_att_decode_step_ws_bytes(n, k, P, A, C, E) bytes, 16-B aligned: z, then xa, then the raw scores
 * [n k][P rounded up to 4]. slab: at least n k max(V, A + C) floats, 16-B aligned.
 * Shapes (capnet_att_decode_supported): A % 4 == 0, C % 512 == 0, 1 <= P <= 4096, E % 4 == 0, 1 <= k <= 16, H in {64, 128,
 * 256, 512, 1024}, round16(E + C) + H <= 4096, 1 <= nlayers <= 8. Every bad argument is refused before any launch. */
int capnet_att_decode_supported(int E, int C, int H, int A, int P, int k, int nlayers);
size_t capnet_att_decode_step_ws_bytes(int n, int k, int P, int A, int C, int E);
int capnet_att_decode_step(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, const float* att1,
                           const float* feat, const long long* tokens, const float* emb, const float* wz, const float* bz,
                           const float* w_full, const float* b_full, const float* const* wcat, const float* const* beff,
                           const float* state_in, const long long* parent_rows, float* state_out, float* h_top,
                           void* workspace, float* slab, size_t slab_floats, int* err_flag, capnet_stream_t stream);

/* capnet_att_decode_step for `groups` weight groups on the same n images (every style at once): groups x n beam groups,
 * beam group q = g n + i at rows q k .. q k + k - 1. att1 is [groups n][P][A] (each group has its own encoder_att), feat
 * stays [n][P][C] (beam group q reads image q % n: the map is not copied per group), wz [groups][A + C][H], bz
 * [groups][A + C], w_full [groups][A], b_full [groups], wcat[l] [groups][4H][kin_l + H], beff[l] [groups][4H]. z is one
 * capnet_sgemm_splitk product per group on the group's n k rows -- the call a step of that group alone makes, so z, xa,
 * the state and h_top of group g's rows equal capnet_att_decode_step's on that group bit for bit. tokens, parent_rows, the
 * states and h_top cover all groups n k rows; a parent is checked against all of them. workspace:
 * capnet_att_decode_step_ws_bytes(groups n, ...); slab: at least groups n k max(V, A + C) floats. 1 <= groups <= 8;
 * groups = 1 is exactly capnet_att_decode_step. */
int capnet_att_decode_step_groups(int cell, int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                  const float* att1, const float* feat, const long long* tokens, const float* emb,
                                  const float* wz, const float* bz, const float* w_full, const float* b_full,
                                  const float* const* wcat, const float* const* beff, const float* state_in,
                                  const long long* parent_rows, float* state_out, float* h_top, void* workspace, float* slab,
                                  size_t slab_floats, int* err_flag, capnet_stream_t stream);

/* The whole beam search of an attention decoder in one call: capnet_beam_decode's loop with capnet_att_decode_step as the
 * step. Per step s = 1 .. max_steps: the attention step on the previous step's words and parent rows (no parents at
 * s = 1), logits = h_top . Cw^T + Cb by capnet_sgemm_splitk's entry on `slab`, capnet_beam_advance; then
 * capnet_beam_finish into seqs int64 [n][max_steps + 2] and lengths int32 [n]. state0 [n k][2 nlayers][H] is required (the
 * attention decoders start at init_h / init_c of the mean feature). workspace: capnet_att_beam_decode_ws_bytes(...) bytes,
 * 16-B aligned (capnet_beam_decode's parts, then capnet_att_decode_step's block; 0 for shapes outside the limits). The call
 * allocates nothing and issues plain launches; poll_every and *steps_run as capnet_beam_decode. Every bad argument is
 * refused before any launch. */
size_t capnet_att_beam_decode_ws_bytes(int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps);
int capnet_att_beam_decode(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                           long long start_token, long long end_token, const float* att1, const float* feat, const float* emb,
                           const float* wz, const float* bz, const float* w_full, const float* b_full,
                           const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                           const float* state0, void* workspace, float* slab, size_t slab_floats, int poll_every,
                           long long* seqs, int* lengths, int* steps_run, int* err_flag, capnet_stream_t stream);

/* capnet_att_beam_decode with capnet_att_decode_step_groups as the step: the searches of `groups` weight groups over the
 * same n images in one loop (operands as that step's). The vocabulary projection is one product over all groups n k rows
 * (Cw is shared), as in capnet_beam_decode_groups. workspace: capnet_att_beam_decode_ws_bytes(nlayers, groups n, ...); seqs
 * int64 [groups n][max_steps + 2], lengths int32 [groups n]; state0 [groups n k][2 nlayers][H] is required. 1 <= groups <= 8;
 * groups = 1 is exactly capnet_att_beam_decode. Every bad argument is refused before any launch. */
int capnet_att_beam_decode_groups(int cell, int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                  int max_steps, long long start_token, long long end_token, const float* att1,
                                  const float* feat, const float* emb, const float* wz, const float* bz, const float* w_full,
                                  const float* b_full, const float* const* wcat, const float* const* beff, const float* Cw,
                                  const float* Cb, const float* state0, void* workspace, float* slab, size_t slab_floats,
                                  int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                  capnet_stream_t stream);

/* The attention maps of the one-call search: for a caption [start, w_1 .. w_m], row e - 1 of its maps is the softmax over
 * the P pixels that the decoder computed at step e, from the layer-0 hidden state reached on start, w_1 .. w_{e-1}.
 *
 * The row trace. Beams change slots at every step, so the search remembers, per hypothesis, the slot it occupied at
 * every step: `trace`, capnet_beam_trace_bytes(n, k, max_steps) bytes of caller-owned device memory BESIDE the beam
 * state (the state's layout and capnet_beam_state_bytes do not change), 4-byte aligned, in the sequences' own shape:
 * rows int32 [2][n][k][max_steps + 2] (the two buffers swap as the state's sequences do) | done_rows [n][k][max_steps + 2].
 * Entry e (1 <= e <= step) is the slot, within the image, whose step-e attention preceded word e; entry 0 is -1. It
 * needs no initialisation: step 1 reads nothing of it.
 *   capnet_beam_advance_traced: capnet_beam_advance (same selection, same state, same next_words / parent_rows) whose
 *     copy of a survivor's or a completion's tokens also copies its parent's row history and appends the parent's slot.
 *   capnet_beam_finish_traced: capnet_beam_finish, and rows int32 [n][max_steps]: entry e - 1 is the winner's row at step e
 *     as a row of the decoder step, i k + slot; -1 past length - 1, everywhere where nothing completed, and for a
 *     recorded slot outside [0, k) -- a recorded row is never used as an address unchecked.
 * 0 bytes / an error for n < 1, k outside 1..16, max_steps < 1, a null or misaligned pointer. */
size_t capnet_beam_trace_bytes(int n, int k, int max_steps);
int capnet_beam_advance_traced(void* beam, void* trace, const float* logits, long ld, int V, int n, int k, int max_steps,
                               int step, long long end_token, long long* next_words, long long* parent_rows,
                               capnet_stream_t stream);
int capnet_beam_finish_traced(const void* beam, const void* trace, int n, int k, int max_steps, long long end_token,
                              long long* seqs, int* lengths, int* rows, capnet_stream_t stream);

/* capnet_att_decode_step_groups with its maps out: alphas f32 [groups n k][P] (required, 4-byte aligned), row r = the
 * softmax over the pixels of row r's scores, stored by the context kernel's first channel block of the image from the
 * values it multiplies the map with. The state, h_top and the workspace's contents are those of the call without it,
 * bit for bit. */
int capnet_att_decode_step_alphas(int cell, int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                  const float* att1, const float* feat, const long long* tokens, const float* emb,
                                  const float* wz, const float* bz, const float* w_full, const float* b_full,
                                  const float* const* wcat, const float* const* beff, const float* state_in,
                                  const long long* parent_rows, float* state_out, float* h_top, void* workspace, float* slab,
                                  size_t slab_floats, int* err_flag, capnet_stream_t stream, float* alphas);

/* capnet_att_beam_decode_groups that also returns the winners' maps: alphas f32 [groups n][max_steps][P] (required,
 * 4-byte aligned); a caption of `length` tokens has length - 1 rows, the rest are zero ([<end>] alone: all zero). Step e
 * writes every row's map into slice e - 1 of a history [max_steps][groups n k][P], the advance records rows
 * (capnet_beam_advance_traced), and after capnet_beam_finish_traced one launch, a workgroup per (caption, step), gathers
 * history[e - 1][rows[e - 1]]. Sequences and lengths are capnet_att_beam_decode_groups' own. workspace:
 * capnet_att_beam_decode_alphas_ws_bytes(...) = capnet_att_beam_decode_ws_bytes(nlayers, groups n, ...) + the trace
 * (capnet_beam_trace_bytes(groups n, k, max_steps)) + the rows (groups n max_steps int32) + the history (max_steps groups
 * n k P floats), each part rounded up to 16 bytes; 0 for the shapes capnet_att_beam_decode_ws_bytes refuses and groups
 * outside 1..8. poll_every and *steps_run as before (steps that were not issued leave their slices unread). Every bad
 * argument is refused before any launch. */
size_t capnet_att_beam_decode_alphas_ws_bytes(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                              int max_steps);
int capnet_att_beam_decode_alphas(int cell, int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H, int V,
                                  int max_steps, long long start_token, long long end_token, const float* att1,
                                  const float* feat, const float* emb, const float* wz, const float* bz, const float* w_full,
                                  const float* b_full, const float* const* wcat, const float* const* beff, const float* Cw,
                                  const float* Cb, const float* state0, void* workspace, float* slab, size_t slab_floats,
                                  int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                  capnet_stream_t stream, float* alphas);

/* N-best: every completed hypothesis of every image, best first, read out of a beam state after its search (any search:
 * the step-by-step calls above, or a one-call search through the offsets below). One launch, one wave per image; the
 * state is only read, so capnet_beam_finish gives the same before and after.
 *   key      done_score / (done_len - 1)^length_penalty; done_len - 1 is the number of generated words, <end> included.
 *            length_penalty == 0: done_score itself, no division and no powf -- entry 0 is then capnet_beam_finish's winner
 *            bit for bit. Ties go to the earlier completion. length_penalty must be finite.
 *   seqs     int64 [n][k][max_steps + 2], zero past each length (8-byte aligned)
 *   lengths  int32 [n][k]; scores f32 [n][k]: the raw summed log-probability whatever the penalty; counts int32 [n]: the
 *            completed hypotheses of the image, <= k. Entries at and past counts[i] are zeros with length 0; an image with
 *            nothing completed has count 0 (capnet_beam_finish's [<end>] is NOT among the entries).
 *   capnet_beam_nbest_traced: also rows int32 [n][k][max_steps], capnet_beam_finish_traced's rule per hypothesis (i k + slot,
 *            -1 past length - 1, past the count, and for a recorded slot outside [0, k)). Its checks are
 *            capnet_beam_finish_traced's.
 * An error for n < 1, k outside 1..16, max_steps < 1, a null or misaligned pointer. */
int capnet_beam_nbest(const void* beam, int n, int k, int max_steps, float length_penalty, long long* seqs, int* lengths,
                      float* scores, int* counts, capnet_stream_t stream);
int capnet_beam_nbest_traced(const void* beam, const void* trace, int n, int k, int max_steps, float length_penalty,
                             long long* seqs, int* lengths, float* scores, int* counts, int* rows, capnet_stream_t stream);

/* Where the one-call searches leave their beam state, trace and map history in the caller's workspace, as byte offsets:
 * the n-best of such a search is capnet_beam_nbest on workspace + offset after the search returned (same stream).
 *   capnet_beam_decode_ws_beam_offset: the beam state of capnet_beam_decode[_groups] / capnet_lstm_beam_decode[_groups]
 *     (n: the sentences of ONE group, the state holds groups n images; fused_topk as the search's) and, with fused_topk 0
 *     and groups 1 at n = all beam groups, of capnet_att_beam_decode[_groups / _alphas]. 0 where
 *     capnet_lstm_beam_decode_groups_ws_bytes of the same arguments is 0.
 *   capnet_att_beam_decode_alphas_ws_trace_offset / _hist_offset: the trace (capnet_beam_trace_bytes(groups n, ...)) and
 *     the history f32 [max_steps][groups n k][P] of capnet_att_beam_decode_alphas. 0 where its _ws_bytes is 0. */
size_t capnet_beam_decode_ws_beam_offset(int nlayers, int n, int k, int H, int V, int max_steps, int fused_topk, int groups);
size_t capnet_att_beam_decode_alphas_ws_trace_offset(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H,
                                                     int V, int max_steps);
size_t capnet_att_beam_decode_alphas_ws_hist_offset(int nlayers, int groups, int n, int k, int P, int A, int C, int E, int H,
                                                    int V, int max_steps);

/* The gather of capnet_att_beam_decode_alphas on its own: alphas f32 [captions][max_steps][P], row (c, e) =
 * hist[e][rows[c][e]] of a history f32 [max_steps][nk][P]; rows int32 [captions][max_steps], a row outside [0, nk) gives
 * zeros. With captions = n k and capnet_beam_nbest_traced's rows: every hypothesis's maps in one launch. max_steps <=
 * 65535; pointers 4-byte aligned. */
int capnet_alpha_gather(const float* hist, const int* rows, int captions, int nk, int max_steps, int P, float* alphas,
                        capnet_stream_t stream);

/* One recurrent step in one launch (used inside capnet_seq_forward for t > 0):
 *   gates[b][4H] (in: U(S(V x)) + biases, ld ldg) += h_prev[b][H] . W[4H][H]^T (W given as the
 *   capnet_lstm_pack_wfrag image), then the gate
 *   non-linearities, c = f*c_prev + i*g, h = o*c (cell 0) / o*tanh(c) (cell 1); gates are
 *   overwritten by the activated values. Each wave keeps its slice of w_cat in registers for
 *   the launch. 1 <= b <= 64, H any multiple of 16 in 16..512 (capnet_lstm_step_fused_supported):
 *   H is padded with zero weights to 64, 128, 256 or 512 inside the fragment image. h_prev and
 *   w_frag 16-byte aligned; gates, c_prev, c_out, h_out dense rows of 4-byte alignment, ldg >= 4H. */
size_t capnet_lstm_wfrag_floats(int H);
/* w_cat [4H][H] (gate blocks in the cell's storage order) -> the fragment-major image the step
 * kernel streams with fully coalesced 1-KB reads (one per 4 MFMA k-steps and wave) */
int capnet_lstm_pack_wfrag(const float* w_cat, float* w_frag, int H, int cell,
                           capnet_stream_t stream);
int capnet_lstm_step_fused(const float* h_prev, const float* w_frag, float* gates, long ldg,
                           const float* c_prev, float* c_out, float* h_out, int b, int H, int cell,
                           capnet_stream_t stream);
/* diagnostic variant (cell 0): also writes 5 s_memtime readings per workgroup to `stamps`
 * ([H/8][5] uint64: start, operands staged, MFMAs done, K-reduced, end) */
int capnet_lstm_step_fused_stamped(const float* h_prev, const float* w_frag, float* gates, long ldg,
                                   const float* c_prev, float* c_out, float* h_out, int b, int H,
                                   unsigned long long* stamps, capnet_stream_t stream);
int capnet_lstm_step_fused_supported(int b, int H);
/* Host only, nothing launched: the instance capnet_lstm_step_fused runs at (b, H). Returns 0 where the call refuses the
 * shape, else 1 with detail[4] (optional) = { k groups per wave (1, 2, 4, 8: H padded to 64 times that), 16-row tiles per
 * workgroup (1: b <= 16, else 2), row halves (2: b > 32), 1 where workgroup ids are dealt XCD-major (H / 4 a multiple
 * of 8) else 0 }. */
int capnet_lstm_step_fused_route(int b, int H, int* detail);
/* Host only: the kernel a decode-step layer of E input columns (rounded up to 16) and hidden size H runs on, xvec = its
 * input rows take 16-byte loads (E % 4 == 0, aligned rows). 0: refused (K = round16(E) + H above 2048 without xvec, above
 * 4096, or an H outside {64, 128, 256, 512, 1024}); 1: the narrow kernel, 2: the wide one. detail[2] (optional) = { k
 * groups per wave of the instance (narrow 2, 4, 6, 8, 12, 16; wide 12, 16 per half), 16-row tiles per pass }. */
int capnet_stacked_decode_route(int E, int H, int xvec, int* detail);

/* One training step of a stacked layer above the first on at most 16 rows, in one launch (the step capnet_att_seq_forward
 * runs for its upper layers): x_out = dropout(xin) (use_dropout: the mask of (seed, row r0 + r, layer), scaled by 1 / (1 - p);
 * else a copy), pre = [x_out | h_prev] . [w_eff | w_rec]^T + b_eff, gates [b][4H] = the activated gates in the cell's block
 * order (cell 0: i, f, o, c~; cell 1: i, f, g, o), c_out = f c_prev + i g, h_out = o c_out (cell 0) or o tanh(c_out).
 * xin, h_prev, c_prev, x_out, c_out, h_out [b][H] dense; w_eff, w_rec [4H][H]; b_eff [4H]. 1 <= b <= 16, H in {64, 128, 256,
 * 512, 1024}; xin, h_prev, w_eff, w_rec 16-byte aligned. */
int capnet_lstm_upper_step(const float* xin, const float* h_prev, const float* c_prev, const float* w_eff, const float* w_rec,
                           const float* b_eff, float* x_out, float* gates, float* c_out, float* h_out, int b, int H, int r0,
                           float p, unsigned long long seed, int layer, int use_dropout, int cell, capnet_stream_t stream);

/* Persistent sequence kernel: steps [t0, t1) of the recurrence in ONE launch, the recurrent
 * weights register-resident for the launch (north star: "the LSTM step as a persistent
 * wavefront-resident kernel"; the loop it replaces: stylenet/model.py:180-191 for teacher-forced
 * steps, cell :147-153 / nic/model.py:77). H = 512, b <= 128, a device with >= 256 CUs
 * (capnet_lstm_persist_supported; CAPNET_NO_PERSISTENT_LSTM=1 disables it).
 *   w_img        capnet_lstm_persist_pack image of w_cat [4H][H]     (capnet_lstm_persist_w_floats; the weights as two f16
 *                pieces each, scaled by 2^10, in MFMA operand order: fp32-grade products for |w| < 32)
 *   gates        [N][4H] packed time-major: in = pre-activations without the recurrent term,
 *                out = activated gates (blocks in the cell's order)
 *   cell_states  [N][H] out (row block of step t0-1 is read when t0 > 0)
 *   hiddens      [N][H] out (row block of step t0-1 is read when t0 > 0); also the medium through
 *                which the workgroups hand h_t to each other
 *   batch_sizes  [t1] non-increasing rows per step (host array)
 *   ctl          capnet_lstm_persist_ctl_ints() ints, zeroed once before the first segment of a
 *                forward pass; segment = 1, 2, ... numbers the launches that share it
 *   err_flag     bit 5 (value 32) is set if the weight image holds a value beyond f16's range (a recurrent weight with
 *                |w| >= 64: capnet_lstm_persist_pack marks the image, the results are not finite);
 *                bit 2 (value 4) is set if a bounded wait expired (the results are then invalid; capnet_clamp_adam
 *                given the same word skips its update)
 *   stamps       NULL, or ([t1-t0][256][8] + [256][2]) uint64 s_memtime readings (diagnostic instantiation) */
int capnet_lstm_persist_supported(int b, int H);
/* Process-wide mode of the persistent path; returns the previous mode, mode < 0 only queries. Bit 0: off (one launch
 * per step everywhere; the initial value when CAPNET_NO_PERSISTENT_LSTM=1 is in the environment). Bits 1 and 2 force
 * the two rare paths for tests: the cross-XCD (write-through) hand-off, and a handshake time-out (every workgroup
 * leaves, err_flag |= 4). */
int capnet_lstm_persist_set_mode(int mode);
size_t capnet_lstm_persist_w_floats(void);
size_t capnet_lstm_persist_ctl_ints(void);
int capnet_lstm_persist_pack(const float* w_cat, float* w_img, int cell, capnet_stream_t stream);
int capnet_lstm_persist_run(const float* w_img, float* gates, float* cell_states, float* hiddens,
                            const int* batch_sizes, int t0, int t1, int H, int cell, int segment,
                            int* ctl, int* err_flag, unsigned long long* stamps,
                            capnet_stream_t stream);

/* ---- loss: nn.CrossEntropyLoss() (mean) -- stylenet/train_multitask.py:134,383 ----------
 * logits [N][V] with leading dimension ld >= V, dlogits likewise with ldd >= V (a smaller one is refused). A target
 * outside [0, V) sets bit 1 (value 2) of err_flag, beside whatever bits the word already holds. */
int capnet_xent_fwd(const float* logits, long ld, int N, int V, const long long* targets,
                    float* lse, float* row_loss, float* loss, int* err_flag,
                    capnet_stream_t stream);
int capnet_xent_bwd(const float* logits, long ld, int N, int V, const long long* targets,
                    const float* lse, const float* grad_out, float* dlogits, long ldd,
                    capnet_stream_t stream);
/* Loss of the attention loops (stylenet/train_multitask_att.py:409-411):
 *   out = nll + alpha_c * ((1 - sum_t alphas[b][t][p])^2).mean()     alphas [B][steps][P]
 * colsum [B*P] receives sum_t alphas for the backward call, which writes
 *   dalphas[b][t][p] = gout * alpha_c * 2 (colsum[b][p] - 1) / (B P). */
int capnet_att_loss_fwd(const float* nll, const float* alphas, int B, int steps, int P, float alpha_c,
                        float* colsum, float* out, capnet_stream_t stream);
int capnet_att_loss_bwd(const float* gout, const float* colsum, int B, int steps, int P, float alpha_c,
                        float* dalphas, capnet_stream_t stream);
/* Policy-gradient loss over a packed batch of B sampled captions (self-critical sequence training):
 *   loss = -(1/N) sum_i advantages[cap(i)] * (logits[i][targets[i]] - lse[i])
 * logits [N][V] (leading dimension ld), targets [N] in pack_padded_sequence order; batch_sizes (host int[steps], steps
 * <= 128, batch_sizes[0] == B) as for capnet_seq_forward: in the step whose first row is off_t, cap(i) = i - off_t.
 * advantages [B] (device) in the batch's sorted order. The forward call writes lse [N], row_logp [N] (the log-probability
 * of every target), caption_logp [B] (a caption's rows summed in step order) and the scalar loss; a target outside [0, V)
 * raises bit 1 of err_flag, as in capnet_xent_fwd. The backward call writes
 *   dlogits[i][:] = (softmax_i - onehot_i) * grad_out[0] * advantages[cap(i)] / N;
 * a row whose advantage is exactly 0 is written as zeros without its logits being read. With every advantage 1.0f both
 * calls give capnet_xent_fwd's loss and capnet_xent_bwd's dlogits bit for bit. */
int capnet_policy_xent_fwd(const float* logits, long ld, int N, int V, const long long* targets,
                           const float* advantages, int B, const int* batch_sizes, int steps, float* lse,
                           float* row_logp, float* caption_logp, float* loss, int* err_flag, capnet_stream_t stream);
int capnet_policy_xent_bwd(const float* logits, long ld, int N, int V, const long long* targets, const float* lse,
                           const float* advantages, int B, const int* batch_sizes, int steps, const float* grad_out,
                           float* dlogits, long ldd, capnet_stream_t stream);
/* The reward of decoded captions: sentence BLEU of every row of a sampled decode against the references of its image.
 * ids int64 [rows][ld] as the sampling loops write them, `steps` columns (1 .. 128, ld >= steps). The hypothesis of a row
 * is [start_token] + its ids through the first end_token inclusive (none: all `steps` columns); columns behind the first
 * end_token do not enter the result. Row r belongs to image r / per_image (rows <= images * per_image).
 * refs int32 [images][R][Lr], zero padded, ref_len int32 [images][R] (device): reference slot (i, j) holds ref_len[i][j]
 * words, taken as they are; a length of 0 is an absent slot (skipped), a length outside [0, Lr] is clamped into it.
 * Limits: R <= 16 and R * Lr <= 4096. weights: four doubles on the HOST; smooth 0 or 1.
 *   num_n = sum over the distinct n-grams of the hypothesis of min(its count there, the MAXIMUM over the references of its
 *           count in a reference),  den_n = max(1, L - n + 1),  L the hypothesis' words
 *   closest = the reference length nearest to L, ties to the shorter;  bp = 1 if L > closest else exp(1 - closest / L)
 *   reward = bp * exp(sum_n weights[n] log(num_n / den_n)), 0 where L is 0 or any num_n is 0 (whatever its weight)
 *   smooth 1 (Lin & Och 2004, add one): (num_n + 1) / (den_n + 1) in place of num_n / den_n for n >= 2; then the reward
 *   is 0 only where num_1 is 0.
 * reward float32 [rows]: formed in fp64 and rounded once. stats int32 [rows][10]: num_1..4, den_1..4, L, closest (0 where
 * the image has no reference). One workgroup per row; integer sums only, so the result does not depend on any order. */
int capnet_bleu_rows(const long long* ids, long ld, int rows, int steps, long long start_token, long long end_token,
                     int per_image, const int* refs, const int* ref_len, int images, int R, int Lr, const double* weights,
                     int smooth, float* reward, int* stats, capnet_stream_t stream);
/* CIDEr-D (Vedantam et al. 2015, as the COCO caption tools' cider_scorer forms it) of every row of a sampled decode against
 * the references of its image. ids / steps / start_token / end_token / per_image / refs / ref_len / images / R / Lr, the
 * hypothesis of a row and the limits: as capnet_bleu_rows. The corpus enters as four sorted tables, one per order n = 1..4:
 * keys[n-1] int32 [counts[n-1]][n] (device) in strictly ascending lexicographic order and idf[n-1] float64 [counts[n-1]]
 * (device), the value ln N - ln max(1, df) the host computed for that n-gram; keys, idf and counts themselves are HOST
 * arrays of four. counts[n-1] >= 0; a table pointer may be null only where its count is 0. log_n = ln N is the idf of an
 * n-gram no table holds. ref_norm float64 [images][R][4] (device): norm_n of every reference slot, computed by the host.
 *   v_s(g) = (count of g in s) * idf(g);  norm_n(s) = sqrt(sum over the n-grams g of s of v_s(g)^2)
 *   sim_n(r) = sum over the distinct n-grams g of the hypothesis of min(v_h(g), v_r(g)) * v_r(g), divided by
 *              norm_n(h) * norm_n(r) where both are non-zero, times exp(-(L - ref_len)^2 / (2 sigma^2)),  sigma > 0
 *   part_n = the mean of sim_n over the slots of non-zero length;  reward = 2.5 * (part_1 + part_2 + part_3 + part_4)
 * reward float32 [rows] (formed in fp64, rounded once), parts float64 [rows][4], stats int32 [rows][9]: L, the number of
 * distinct n-grams of the hypothesis for n = 1..4, and how many of them the table of order n holds. Every n-gram is looked
 * up by binary search over whole keys; all sums are fp64 in a fixed order, without atomics: the same input gives the same
 * bits. One workgroup per row. */
int capnet_cider_rows(const long long* ids, long ld, int rows, int steps, long long start_token, long long end_token,
                      int per_image, const int* refs, const int* ref_len, const double* ref_norm, int images, int R, int Lr,
                      const int* const* keys, const double* const* idf, const int* counts, double log_n, double sigma,
                      float* reward, double* parts, int* stats, capnet_stream_t stream);

/* ---- input pipeline (stylenet/train_multitask.py:62-69: Resize((336,336)) -> RandomCrop(224) ->
 * RandomHorizontalFlip -> ToTensor -> Normalize) on uint8 HWC device images ----------------------
 * capnet_resize_u8: Pillow's two-pass antialiased resample (what torchvision 0.2.2's Resize calls).
 * src [Hs][Ws][3], tmp [Hs][Wo][3] scratch, dst [Ho][Wo][3]. bounds_* (device int [out][2] =
 * {first tap, tap count}) and coef_* (device int [out][kmax], 22-bit fixed point) are the filter
 * tables of the horizontal / vertical pass, built on the host as Pillow's precompute_coeffs does
 * (capnet.data.resample_tables); the result is bit-identical to PIL.Image.resize(BILINEAR).
 * capnet_crop_flip_normalize: src [B][Hs][Ws][3] uint8, params (device int [B][3] = {top, left,
 * flip}), mean/std host float[3]; dst [B][3][Hc][Wc] fp32 = (u8/255 - mean)/std. */
int capnet_resize_u8(const unsigned char* src, int Hs, int Ws, unsigned char* tmp, unsigned char* dst,
                     int Ho, int Wo, const int* bounds_h, const int* coef_h, int kmax_h,
                     const int* bounds_v, const int* coef_v, int kmax_v, capnet_stream_t stream);
int capnet_crop_flip_normalize(const unsigned char* src, int B, int Hs, int Ws, const int* params,
                               float* dst, int Hc, int Wc, const float* mean, const float* stdv,
                               capnet_stream_t stream);

/* count[0] = number of rows whose target is among the k largest logits of its row -- the numerator
 * of utils.accuracy(scores, targets, k) (stylenet/utils.py:127-140; top-5 in val_factual,
 * train_multitask.py:306). Ties are ranked lower index first. count is overwritten. */
int capnet_topk_correct(const float* logits, long ld, int N, int V, const long long* targets, int k,
                        int* count, int* err_flag, capnet_stream_t stream);

/* ---- optimiser: utils.clip_gradient (element-wise clamp, stylenet/utils.py:51-60) fused with
 * torch.optim.Adam.step (stylenet/train_multitask.py:166-167,389; no weight decay, no amsgrad).
 * Host arrays of n device pointers / sizes / per-tensor step counts (>= 1, already
 * incremented). clip <= 0 disables the clamp; write_grad != 0 also stores the clamped grad. The clamp is
 * torch.clamp's: a NaN gradient stays NaN, and so do the moments and the parameter it reaches.
 * skip_flag: NULL, or the device error word the step's kernels were given (err_flag): while it is non-zero
 * the launch leaves parameters, moments and gradients untouched -- a step whose inputs were invalid (token id or
 * target out of range, an expired wait of the persistent LSTM kernel) is dropped, not applied. */
int capnet_clamp_adam(int n, float* const* params, float* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, const long* numel, const int* step, float lr,
                      float beta1, float beta2, float eps, float clip, int write_grad,
                      const int* skip_flag, capnet_stream_t stream);

/* targets = pack_padded_sequence(captions, lengths, batch_first=True)[0]
 * (stylenet/train_multitask.py:377-379); batch_sizes is a host array. out: [sum(batch_sizes)]. */
int capnet_packed_targets(const long long* captions, int T, int steps, const int* batch_sizes,
                          long long* out, capnet_stream_t stream);

/* Data-parallel plumbing (no reference counterpart: the reference is single-device): gather
 * n gradient tensors into one flat buffer (direction 0) for ONE RCCL all-reduce, and scatter
 * it back multiplied by `scale` (direction 1). Host arrays of device pointers / sizes. */
int capnet_pack_tensors(int n, float* const* tensors, const long* numel, float* flat,
                        int direction, float scale, capnet_stream_t stream);

/* ---- a bottleneck's conv3 + bn3 + residual + ReLU + the next block's conv1 without ever forming y3 (csrc/fused_block.hip).
 * Replaces, between two blocks of one stage of torchvision's resnet152 (Bottleneck.forward, called from
 * stylenet/model.py:15-18,24): `out = relu(bn3(conv3(relu(bn2(y2)))) + identity)` of block b and `y1 = conv1(out)` of
 * block b + 1. MID = conv3's input channels (64 / 128 / 256), C = 4 MID its output channels; all tensors NHWC fp32
 * flattened to [M = B H W][channels].
 *   capnet_fused_block_pack        role 0: conv3's weights [C][MID] -> its image (+ an fp32 copy, read by the statistics);
 *                                  role 1: the next conv1's weights [MID][C] -> its image. Sizes: .._weight_words.
 *   capnet_fused_block_stats       train mode: (scale, shift) of bn3 -- and its running statistics, momentum as torch --
 *                                  from the second moments of conv3's INPUT: sum_m y3[m,c]^2 = w_c^T (a2^T a2) w_c with
 *                                  a2 = relu(y2 s2 + t2). `work`: .._stats_floats(M, MID) floats, 16-B aligned.
 *   capnet_fused_block_forward     writes out [M][C] and y1 [M][MID]; part_sum / part_sq [.._tiles(M, MID)][MID]: per-tile
 *                                  column sums of y1 for capnet_bn_finalize (null: inference). res = the block's input
 *                                  (sd = td = null) or its downsample branch's raw output with that BatchNorm's (sd, td).
 *   e3 / e1: power-of-two prescales of conv3's and conv1's inputs in the f16 planes (capnet_trunk_forward's exponents). */
size_t capnet_fused_block_weight_words(int C, int MID, int role);
int capnet_fused_block_pack(const float* w, unsigned* img, int C, int MID, int role, capnet_stream_t stream);
size_t capnet_fused_block_stats_floats(long M, int MID);
int capnet_fused_block_stats(const float* y2, const float* s2, const float* t2, const unsigned* w3img, long M, int MID,
                             int in_exp, const float* gamma, const float* beta, float* running_mean, float* running_var,
                             float momentum, float eps, float* scale, float* shift, float* work, int* err_flag,
                             capnet_stream_t stream);
int capnet_fused_block_tiles(long M, int MID);
int capnet_fused_block_forward(const float* y2, const float* s2, const float* t2, const unsigned* w3img, const float* s3,
                               const float* t3, const float* res, const float* sd, const float* td, float* out,
                               const unsigned* w1img, float* y1, float* part_sum, float* part_sq, long M, int MID, int e3,
                               int e1, int* err_flag, capnet_stream_t stream);

/* Data-parallel plumbing, the collective (no reference counterpart -- the reference is single-device): an
 * RCCL communicator behind an opaque handle and the step's ONE collective, an in-place SUM all-reduce of the flat fp32
 * gradient buffer, enqueued on the caller's stream (the side stream of capnet.parallel: it overlaps the next trunk
 * passes). One process per GPU. capnet_comm_unique_id fills 128 bytes on ONE rank; the caller hands them to every rank
 * by its own means (capnet.parallel: torch.distributed's store); capnet_comm_create is collective over the `world`
 * ranks and binds the communicator to the calling process's current HIP device. librccl is resolved at run time (an
 * RCCL already mapped into the process first, then /opt/rocm/lib): a single-GPU host never loads it. */
typedef struct capnet_comm capnet_comm_t;
int capnet_comm_unique_id(void* id128);
int capnet_comm_create(const void* id128, int rank, int world, capnet_comm_t** out);
int capnet_comm_destroy(capnet_comm_t* comm);
int capnet_allreduce_grads(capnet_comm_t* comm, float* flat, long count, capnet_stream_t stream);

/* Data-parallel plumbing, the error word: capnet_clamp_adam drops a step while the LOCAL device error word is set, and
 * every rank has to take that decision alike. direction 0: *slot = (word != 0) -- the slot is one extra float behind the
 * flat gradient buffer, so it is summed by the same all-reduce; direction 1: if the sum is positive and the local word is
 * clear, set it to 16 ("another rank dropped this step"). No reference counterpart. */
int capnet_err_word_exchange(int* err_flag, float* slot, int direction, capnet_stream_t stream);

/* *counter += 1 while *err_flag != 0. capnet.optim.Adam launches it once per step() in front of capnet_clamp_adam and
 * takes the dropped steps out of its host-side step counts (torch.optim.Adam's bias correction, train_multitask.py:389)
 * when check_device_errors() reports them. */
int capnet_count_skipped(const int* err_flag, int* counter, capnet_stream_t stream);

/* x[i] = min(max(x[i], lo), hi) as torch.clamp has it, a NaN staying NaN: utils.clip_gradient alone
 * (stylenet/utils.py:57-60). */
int capnet_clamp(float* x, long n, float lo, float hi, capnet_stream_t stream);

/* ---- Constrained beam search (capnet.beam.Constraints; no reference counterpart: the reference patches its
 * captions after the search) ----
 * What a step must not select. At step s (1-based) a live hypothesis is tokens = [start, w_1 .. w_{s-1}]; the candidate
 * (hypothesis, word v) is excluded if v is one of banned[0 .. n_banned) (a DEVICE int32 array, n_banned <= 32; may be NULL
 * when n_banned is 0), or v == end_token and s <= min_words, or g = no_repeat_ngram (0: off, at most 4) is >= 1, s >= g and
 * appending v would complete a g-gram the hypothesis already holds, <start> included (g = 1: no word twice).
 * Exclusion comes AFTER the log-softmax: every row's log-sum-exp is taken over the whole, unmodified row, then the excluded
 * entries of the logits block are overwritten with -inf and the selection runs as ever (row 0 alone at step 1, ties to the
 * lower flat index). A survivor's score is still the model's own summed log-probability; nothing is renormalised. THE
 * LOGITS BLOCK IS MODIFIED (hence neither const nor restrict): it is the step's scratch on every route. The caller
 * guarantees k finite candidates per step: V - n_banned - 1 - max_steps >= k.
 *   capnet_beam_advance_constrained: capnet_beam_advance with the exclusions derived by the selecting workgroup from the
 *     image's own sequences in the beam state (the host never sees them): one thread per (competing row, start position)
 *     and g - 1 compares each. Everything else -- state, next_words, parent_rows, completion order -- as capnet_beam_advance. */
int capnet_beam_advance_constrained(void* beam, float* logits, long ld, int V, int n, int k, int max_steps, int step,
                                    long long end_token, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                                    long long* next_words, long long* parent_rows, capnet_stream_t stream);
/* capnet_beam_advance_traced under the same constraints: the row trace is recorded as there. */
int capnet_beam_advance_constrained_traced(void* beam, void* trace, float* logits, long ld, int V, int n, int k, int max_steps,
                                           int step, long long end_token, int no_repeat_ngram, int min_words, const int* banned,
                                           int n_banned, long long* next_words, long long* parent_rows, capnet_stream_t stream);
/* capnet_beam_topk with a ban list per row, for the host loops, which hold the sequences themselves
 * (capnet.beam.banned_words): bans is a DEVICE int32 array [rows][1 + cap], per row of the logits its count (<= cap) and
 * that many words; 1 <= cap <= 65536. The same removal after the log-sum-exp, in the same device function; the logits
 * block is modified. */
int capnet_beam_topk_banned(float* logits, long ld, int rows, int V, const float* prev_scores, int k, const int* bans, int cap,
                            float* top_scores, long long* top_index, capnet_stream_t stream);
/* capnet_beam_topk_batched with ban lists: bans [all rows of the logits][1 + cap], row r of the array for row r of the
 * logits (image i's lists start at row meta[3 i]). The logits block is modified. */
int capnet_beam_topk_batched_banned(float* logits, long ld, int V, const float* prev_scores, const int* meta, int n,
                                    const int* bans, int cap, float* top_scores, long long* top_index, capnet_stream_t stream);
/* capnet_beam_decode (one weight group) whose every step selects with capnet_beam_advance_constrained: arguments, workspace
 * (capnet_beam_decode_ws_bytes) and results as there, the constraints behind the stream. Always the stored-logits step. */
int capnet_beam_decode_constrained(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                                   long long end_token, const float* emb, const float* const* wcat, const float* const* beff,
                                   const float* Cw, const float* Cb, const float* state0, void* workspace, float* slab,
                                   size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run,
                                   int* err_flag, capnet_stream_t stream, int no_repeat_ngram, int min_words, const int* banned,
                                   int n_banned);
/* capnet_att_beam_decode under constraints: arguments, workspace (capnet_att_beam_decode_ws_bytes) and results as there. */
int capnet_att_beam_decode_constrained(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                                       long long start_token, long long end_token, const float* att1, const float* feat,
                                       const float* emb, const float* wz, const float* bz, const float* w_full,
                                       const float* b_full, const float* const* wcat, const float* const* beff, const float* Cw,
                                       const float* Cb, const float* state0, void* workspace, float* slab, size_t slab_floats,
                                       int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                       capnet_stream_t stream, int no_repeat_ngram, int min_words, const int* banned,
                                       int n_banned);
/* capnet_att_beam_decode_alphas under constraints, one weight group (no `groups` argument, as
 * capnet_att_beam_decode_constrained has none): the maps are recorded and gathered as there (workspace:
 * capnet_att_beam_decode_alphas_ws_bytes with groups = 1); the constraints follow alphas. */
int capnet_att_beam_decode_alphas_constrained(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V,
                                              int max_steps, long long start_token, long long end_token,
                                              const float* att1, const float* feat, const float* emb, const float* wz,
                                              const float* bz, const float* w_full, const float* b_full,
                                              const float* const* wcat, const float* const* beff, const float* Cw,
                                              const float* Cb, const float* state0, void* workspace, float* slab,
                                              size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run,
                                              int* err_flag, capnet_stream_t stream, float* alphas, int no_repeat_ngram,
                                              int min_words, const int* banned, int n_banned);

/* ---- Diverse beam search (capnet.beam.Diversity; Vijayakumar et al. 2016; no reference counterpart) ----
 * Image i's k beams are `teams` = D teams of kt = k / D (D divides k; "teams", because `groups` already means weight
 * groups); team g holds slots g kt .. g kt + kt - 1 of the image's k rows. Each team is a beam search of its own with
 * capnet_beam_advance's bookkeeping (step 1: its first row alone; <end> retires a beam; its live beams are its first slots
 * in rank order), so the state of a diverse search over n images IS the state of n D plain searches of kt beams:
 * capnet_beam_state_bytes / _init / _finish / _nbest / _live and the trace are called with (n D, kt), state-image i D + g
 * being team g of image i. At each step the teams of an image select in order; team g takes its live best candidates
 * (row, word v) by
 *     key = score - strength * c_g(v),
 * score = the running score + the row's log-softmax (what capnet_beam_advance ranks), c_g(v) = the number of candidates
 * selected at THIS step by teams 0 .. g - 1 of the same image whose word is v. <end> is counted like any word (the published
 * rule). A team with no live beam selects nothing and counts nothing. Ties go to the lower flat index within the team. The
 * penalty shapes the selection only: the score carried forward and reported is (prev - lse) + logit, unpenalised. With
 * constraints (zeros: none; banned may then be NULL) the exclusions apply first, per row from that row's own hypothesis,
 * then the penalty. strength: finite, >= 0; at 0 every team is exactly its plain search. THE LOGITS BLOCK IS MODIFIED.
 *   capnet_beam_advance_diverse: one workgroup per image walks its teams; logits [n k][ld], next_words / parent_rows [n k]
 *     (parent rows are global rows). trace: NULL, or the row trace of (n D, kt) as capnet_beam_advance_traced records it. */
int capnet_beam_advance_diverse(void* beam, void* trace, float* logits, long ld, int V, int n, int k, int teams, float strength,
                                int max_steps, int step, long long end_token, int no_repeat_ngram, int min_words,
                                const int* banned, int n_banned, long long* next_words, long long* parent_rows,
                                capnet_stream_t stream);
/* The host loops' form: capnet_beam_topk_batched over n images x `teams` teams. meta is a DEVICE int32 array [n teams][3]
 * = (first row, rows that compete, live) per (image, team), rows compacted as for capnet_beam_topk_batched; flat indices
 * are local to the team (row within the team * V + word); outputs [n teams][16], the first `live` entries of a row set.
 * bans: NULL, or capnet_beam_topk_batched_banned's lists, a row per logits row. */
int capnet_beam_topk_batched_diverse(float* logits, long ld, int V, const float* prev_scores, const int* meta, int n, int teams,
                                     float strength, const int* bans, int cap, float* top_scores, long long* top_index,
                                     capnet_stream_t stream);
/* capnet_beam_decode (one weight group) as a diverse search: the decode step runs on n images of k rows as ever, every
 * step's selection is capnet_beam_advance_diverse, and the beam state is that of n teams searches of k / teams beams.
 * WORKSPACE: capnet_beam_decode_ws_bytes(nlayers, n, k, H, V, max_steps) bytes laid out as there, FOLLOWED BY
 * capnet_beam_state_bytes(n teams, k / teams, max_steps) bytes, which hold that state when the call returns (for
 * capnet_beam_nbest with (n teams, k / teams), which yields the scores too). seqs [n teams][max_steps + 2] and lengths
 * [n teams]: capnet_beam_finish's winner per (image, team), state-image i teams + g being team g of image i. The
 * constraints follow the stream, zeros meaning none. Always the stored-logits step. */
int capnet_beam_decode_diverse(int cell, int nlayers, int n, int k, int teams, float strength, int E, int H, int V, int max_steps,
                               long long start_token, long long end_token, const float* emb, const float* const* wcat,
                               const float* const* beff, const float* Cw, const float* Cb, const float* state0, void* workspace,
                               float* slab, size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run,
                               int* err_flag, capnet_stream_t stream, int no_repeat_ngram, int min_words, const int* banned,
                               int n_banned);
/* capnet_att_beam_decode (one weight group) as a diverse search; an image's maps are still read once for all its k beams.
 * alphas: NULL, or [n teams][max_steps][P] for the maps of every (image, team)'s winner, recorded as
 * capnet_att_beam_decode_alphas records them. WORKSPACE: capnet_att_beam_decode_ws_bytes(...) bytes (alphas NULL) or
 * capnet_att_beam_decode_alphas_ws_bytes(..., groups = 1, ...) bytes (the trace and the history at its offsets: the trace
 * is that of (n teams, k / teams)), FOLLOWED BY capnet_beam_state_bytes(n teams, k / teams, max_steps) bytes rounded up
 * to 16 -- the state, as above -- and, with alphas, 4 n teams max_steps more bytes (the winners' rows). */
int capnet_att_beam_decode_diverse(int cell, int nlayers, int n, int k, int teams, float strength, int P, int A, int C, int E, int H,
                                   int V, int max_steps, long long start_token, long long end_token, const float* att1,
                                   const float* feat, const float* emb, const float* wz, const float* bz, const float* w_full,
                                   const float* b_full, const float* const* wcat, const float* const* beff, const float* Cw,
                                   const float* Cb, const float* state0, void* workspace, float* slab, size_t slab_floats,
                                   int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                                   capnet_stream_t stream, float* alphas, int no_repeat_ngram, int min_words, const int* banned,
                                   int n_banned);

/* ---- Forced words (capnet.beam.Constraints(forced=...); Post & Vilar 2018, dynamic beam allocation; no
 * reference counterpart) ----
 * forced: a DEVICE int32 array of n_forced (1 .. 4) distinct word ids, none of them end_token, that every completed
 * hypothesis must contain. At step s a live hypothesis is [start, w_1 .. w_{s-1}]; its met mask has bit f set where
 * forced[f] is among w_1 .. (<start> does not count). The met count of a candidate (row r, word v) is the popcount of
 * (r's mask | the bits of the forced ids that equal v): its BANK, 0 .. F.
 *   Exclusions: the constraint arguments' (zeros: none; banned may then be NULL), after the rows' log-sum-exp as ever, and
 *   <end> on every row whose mask is not full.
 *   Pool, for an image that selects `live` candidates from `rows` competing rows: (1) the `live` best non-excluded candidates
 *   by score -- capnet_beam_advance's selection; (2) for every competing row r and every forced id not in r's mask and not
 *   excluded on r, the candidate (r, that id); (3) every competing row's best non-excluded word. A flat index is in the pool
 *   once. Scores are (prev - lse) + logit, formed as capnet_beam_advance forms them; nothing is renormalised.
 *   Allocation: within a bank by score descending, ties to the lower flat index; the banks are visited F, F - 1 .. 0, F ..,
 *   a visit takes the bank's best untaken candidate if it has one, until `live` are taken. The order of taking is the
 *   output order: the survivors' slots and the completion order of the hypotheses that end at this step.
 * Everything behind the selection is capnet_beam_advance's. THE LOGITS BLOCK IS MODIFIED.
 *   capnet_beam_advance_forced: one workgroup per image; trace: NULL, or the row trace as capnet_beam_advance_traced
 *     records it. */
int capnet_beam_advance_forced(void* beam, void* trace, float* logits, long ld, int V, int n, int k, int max_steps, int step,
                               long long end_token, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                               const int* forced, int n_forced, long long* next_words, long long* parent_rows,
                               capnet_stream_t stream);
/* The host loops' form: capnet_beam_topk_batched (meta [n][3] = (first row, rows that compete, live), outputs [n][16]) with
 * bans NULL or capnet_beam_topk_batched_banned's lists, a row per logits row -- the caller's lists hold <end> for a row
 * that lacks a forced id or not, the kernel excludes it either way -- and met, a DEVICE int32 per logits row: the row's
 * mask. Where the pool holds fewer than `live` candidates the remaining entries are -inf / -1. */
int capnet_beam_topk_batched_forced(float* logits, long ld, int V, const float* prev_scores, const int* meta, int n,
                                    const int* bans, int cap, const int* met, const int* forced, int n_forced,
                                    long long end_token, float* top_scores, long long* top_index, capnet_stream_t stream);
/* capnet_beam_decode_constrained with every step's selection capnet_beam_advance_forced; workspace and results as there. */
int capnet_beam_decode_forced(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                              long long end_token, const float* emb, const float* const* wcat, const float* const* beff,
                              const float* Cw, const float* Cb, const float* state0, void* workspace, float* slab,
                              size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                              capnet_stream_t stream, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                              const int* forced, int n_forced);
/* capnet_att_beam_decode_constrained (alphas NULL; workspace capnet_att_beam_decode_ws_bytes) or
 * capnet_att_beam_decode_alphas_constrained (alphas [n][max_steps][P]; workspace capnet_att_beam_decode_alphas_ws_bytes with
 * groups = 1) with every step's selection capnet_beam_advance_forced, the trace passed through. */
int capnet_att_beam_decode_forced(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                                  long long start_token, long long end_token, const float* att1, const float* feat,
                                  const float* emb, const float* wz, const float* bz, const float* w_full, const float* b_full,
                                  const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                  const float* state0, void* workspace, float* slab, size_t slab_floats, int poll_every,
                                  long long* seqs, int* lengths, int* steps_run, int* err_flag, capnet_stream_t stream,
                                  float* alphas, int no_repeat_ngram, int min_words, const int* banned, int n_banned,
                                  const int* forced, int n_forced);

/* ---- Per-image rules (capnet.beam.PerImage; no reference counterpart) ----
 * Every image of a batched search under a rule of its own: the constraint and forced-word arguments above as ONE DEVICE
 * table, rules int32 [n][CAPNET_BEAM_RULE_WORDS], row i the rule of image i (160 bytes a row, the table 16-byte aligned):
 *   word 0        no_repeat_ngram (0 .. 4)
 *   word 1        min_words (>= 0)
 *   word 2        n_banned (0 .. 32)
 *   word 3        n_forced (0 .. 4)
 *   words 4..35   banned: the first n_banned are read
 *   words 36..39  forced: the first n_forced are read
 * A row of zeros is no rule: that image's search is capnet_beam_advance's. The host cannot read the table, so the kernels
 * clamp each of the four counts to the range above as they read it: whatever the table holds, nothing outside the row is
 * indexed, and a word id outside [0, V) is never an address (as everywhere above). What the ids must satisfy for the search
 * to keep k candidates is the caller's to check (capnet.beam.PerImage.check). The entries refuse a NULL or misaligned
 * rules on the host.
 *   capnet_beam_advance_rules: capnet_beam_advance_forced's arguments with rules in place of the six constraint arguments.
 *     One workgroup per image, as there; it reads its row once and takes, as a whole, the forced selection (n_forced > 0),
 *     else the constrained one (any other count non-zero), else the plain one -- the selections of the entries above, on the
 *     row's values. trace: NULL, or the row trace. THE LOGITS BLOCK IS MODIFIED. */
#define CAPNET_BEAM_RULE_WORDS 40
int capnet_beam_advance_rules(void* beam, void* trace, float* logits, long ld, int V, int n, int k, int max_steps, int step,
                              long long end_token, const int* rules, long long* next_words, long long* parent_rows,
                              capnet_stream_t stream);
/* The host loops' form: capnet_beam_topk_batched_forced with the forced ids and their count read per image from rules
 * (row i for meta row i); bans (NULL, or a list per logits row) and met (required, a mask per logits row) are built by the
 * caller from each row's own image's rule. An image with n_forced == 0 takes capnet_beam_topk_batched_banned's selection
 * on its rows (capnet_beam_topk_batched's where bans is NULL). */
int capnet_beam_topk_batched_rules(float* logits, long ld, int V, const float* prev_scores, const int* meta, int n,
                                   const int* bans, int cap, const int* met, const int* rules, long long end_token,
                                   float* top_scores, long long* top_index, capnet_stream_t stream);
/* capnet_beam_decode_forced with rules [n][CAPNET_BEAM_RULE_WORDS] in place of its six constraint arguments: every step
 * selects with capnet_beam_advance_rules; workspace and results as there. */
int capnet_beam_decode_rules(int cell, int nlayers, int n, int k, int E, int H, int V, int max_steps, long long start_token,
                             long long end_token, const float* emb, const float* const* wcat, const float* const* beff,
                             const float* Cw, const float* Cb, const float* state0, void* workspace, float* slab,
                             size_t slab_floats, int poll_every, long long* seqs, int* lengths, int* steps_run, int* err_flag,
                             capnet_stream_t stream, const int* rules);
/* capnet_att_beam_decode_forced likewise: alphas NULL or [n][max_steps][P] with the workspaces named there, the trace
 * passed through to capnet_beam_advance_rules. */
int capnet_att_beam_decode_rules(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, int max_steps,
                                 long long start_token, long long end_token, const float* att1, const float* feat,
                                 const float* emb, const float* wz, const float* bz, const float* w_full, const float* b_full,
                                 const float* const* wcat, const float* const* beff, const float* Cw, const float* Cb,
                                 const float* state0, void* workspace, float* slab, size_t slab_floats, int poll_every,
                                 long long* seqs, int* lengths, int* steps_run, int* err_flag, capnet_stream_t stream,
                                 float* alphas, const int* rules);

#ifdef __cplusplus
}
#endif
#endif /* CAPNET_H_ */
