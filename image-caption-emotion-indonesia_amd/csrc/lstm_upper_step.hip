// One step of a stacked factored-LSTM layer above the first for at most 16 rows, in ONE launch (capnet.stacked_att):
//   x      = dropout_l(h^{l-1}_t)                               (the mask rows_dropout draws for layer l)
//   gates  = [x | h^l_{t-1}] . [Weff | W]^T + beff              Weff_g = U_g S_g V_g, beff_g = U_g (S_g bV_g + bS_g) + bU_g + bW_g
//   i, f, o = sigmoid, c~ = tanh;  c = f c_{t-1} + i c~;  h = o c      (stylenet/model.py:147-153)
// Composed, the same step is rows_dropout, three chain products and the fused recurrent step: five dependent launches of
// 8-12 us each at a dozen rows, whatever they compute (NOTEBOOK 4l).
// Mapping: a workgroup owns 4 hidden units = 16 gate columns (one N tile of the 16-row product, step_core.h) and all rows
// (one 16-row M tile); its 8 waves split K = 2H into eighths (waves 0-3 the dropped-out input, 4-7 the recurrent state). A
// lane reads 16 B of its row and 16 B of its column's weight row per 16-wide k group straight from global memory, and all
// of a wave's loads are in flight before its first MFMA. The eight K-partial tiles are summed through LDS; the epilogue
// applies the gates and writes what BPTT reads: activated gates, c, h and the dropped-out input row.
// The nn.LSTMCell instance (CELL = kCellLSTM, capnet.nic_stacked) takes Weff = weight_ih, W = weight_hh and
// beff = bias_ih + bias_hh as they are, gate blocks i, f, g, o: only the epilogue differs -- gate roles 0, 1, 3, 2,
// h = o tanh(c), and the activated gates stored where the LSTM cell's BPTT reads them (gate_order(kCellLSTM)).
#include "common.h"
#include "dropout_mask.h"
#include "kernels.h"
#include "step_core.h"

namespace capnet {

constexpr int kUpperRows = 16;
constexpr int kUpperWaves = 8;

template <int NJ, int CELL>  // 16-wide k groups per wave: H = 64 NJ; kCellFactored or kCellLSTM
__global__ __launch_bounds__(512) void lstm_upper_step_kernel(
    const float* __restrict__ xin, const float* __restrict__ hprev, const float* __restrict__ cprev,
    const float* __restrict__ Weff, const float* __restrict__ Wrec, const float* __restrict__ beff,
    float* __restrict__ x_out, float* __restrict__ G, float* __restrict__ c_out, float* __restrict__ h_out, int b, int H,
    int r0, float p, unsigned long long seed, int layer, int use_dropout) {
  __shared__ float red[kUpperWaves][kUpperRows][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int u0 = blockIdx.x * 4;
  const float inv_keep = p < 1.f ? 1.f / (1.f - p) : 0.f;
  const int row = clamp_row(li, b);
  // this wave's eighth of K: waves 0-3 read the input half, 4-7 the recurrent half
  const bool rec = wave >= kUpperWaves / 2;
  const int k0 = (wave & 3) * (H / 4);                 // offset inside the half
  const float* arow = (rec ? hprev : xin) + (long)row * H + k0 + 4 * lq;
  const int n = li, grow = (n >> 2) * H + u0 + (n & 3);   // gate role n >> 2 (i, f, o, c~), unit u0 + (n & 3)
  const float* wrow = (rec ? Wrec : Weff) + (long)grow * H + k0 + 4 * lq;
  f32x4 av[NJ], wv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    av[j] = *reinterpret_cast<const f32x4*>(arow + 16 * j);
    wv[j] = *reinterpret_cast<const f32x4*>(wrow + 16 * j);
  }
  // epilogue operands, requested before the products: thread -> (row er, unit eu)
  const int er = tid >> 2, eu = tid & 3;
  const bool evalid = tid < 4 * kUpperRows && er < b;
  const int erow = clamp_row(er, b);
  float pre[4], cp = 0.f;
  if (tid < 4 * kUpperRows) {
#pragma unroll
    for (int g = 0; g < 4; ++g) pre[g] = beff[g * H + u0 + eu];
    cp = cprev[(long)erow * H + u0 + eu];
  }
  if (use_dropout && !rec) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) av[j][e] *= dropout_scale(seed, r0 + row, 0x40000000 + layer, k0 + 16 * j + 4 * lq + e, p, inv_keep);
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = mfma_chain<NJ>(av, wv, acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][4 * lq + r][li] = acc[r];
  // the dropped-out input row for BPTT: this workgroup's 4 columns of every row
  if (tid < 4 * kUpperRows && er < b) {
    const int k = u0 + eu;
    float v = xin[(long)er * H + k];
    if (use_dropout) v *= dropout_scale(seed, r0 + er, 0x40000000 + layer, k, p, inv_keep);
    x_out[(long)er * H + k] = v;
  }
  __syncthreads();
  if (evalid) {
#pragma unroll
    for (int g = 0; g < 4; ++g) pre[g] = sum_partials<kUpperWaves>(red, er, g * 4 + eu, pre[g]);
    constexpr int GO = CELL == kCellLSTM ? 3 : 2, GG = CELL == kCellLSTM ? 2 : 3;   // blocks of o and c~ (g)
    float i, f, og, gt, c;
    lstm_cell(pre[0], pre[1], pre[GO], pre[GG], cp, i, f, og, gt, c);
    const long gr = (long)er * 4 * H + u0 + eu;
    G[gr] = i;
    G[gr + H] = f;
    G[gr + GO * H] = og;
    G[gr + GG * H] = gt;
    c_out[(long)er * H + u0 + eu] = c;
    h_out[(long)er * H + u0 + eu] = lstm_cell_h(og, c, CELL == kCellLSTM);
  }
}

bool lstm_upper_step_supported(int b, int H) {
  return b >= 1 && b <= kUpperRows && step_hidden_supported(H);
}

int lstm_upper_step(const float* xin, const float* hprev, const float* cprev, const float* Weff, const float* Wrec,
                    const float* beff, float* x_out, float* G, float* c_out, float* h_out, int b, int H, int r0, float p,
                    unsigned long long seed, int layer, int use_dropout, hipStream_t stream, int cell) {
  CAPNET_REQUIRE(xin && hprev && cprev && Weff && Wrec && beff && x_out && G && c_out && h_out,
                 "lstm_upper_step: null argument");
  CAPNET_REQUIRE(cell == kCellFactored || cell == kCellLSTM, "lstm_upper_step: unknown cell %d", cell);
  CAPNET_REQUIRE(lstm_upper_step_supported(b, H), "lstm_upper_step: unsupported b=%d H=%d", b, H);
  CAPNET_REQUIRE(aligned16(xin) && aligned16(hprev) && aligned16(Weff) && aligned16(Wrec),
                 "lstm_upper_step: alignment");
  dispatch_nj(H, [&](auto nj) {
    const auto kern = cell == kCellLSTM ? lstm_upper_step_kernel<nj, kCellLSTM> : lstm_upper_step_kernel<nj, kCellFactored>;
    hipLaunchKernelGGL(kern, dim3(H / 4), dim3(64 * kUpperWaves), 0, stream, xin, hprev, cprev, Weff, Wrec, beff, x_out, G,
                       c_out, h_out, b, H, r0, p, seed, layer, use_dropout);
  });
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
