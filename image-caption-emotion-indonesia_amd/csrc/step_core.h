// What the per-time-step kernels share (lstm_step.hip, lstm_upper_step.hip, lstm_decode_step.hip, vocab_core.h, the
// gate kernel of seq_kernels.hip): the 16-row product on v_mfma_f32_16x16x4_f32, the LSTM cell, the supported hidden sizes.
// The 16-row product: a workgroup owns a 16-column N tile (4 hidden units x 4 gate roles, or 16 vocabulary entries) and
// walks the rows 16 at a time; its waves split K and each holds a K-partial 16x16 tile.
//   operands: lane l feeds row (A) / column (B) l & 15 with the four floats k = 16 j + 4 (l >> 4) + e, e = 0..3, of the
//             16-wide k group j: ONE 16-B load per operand and k group serves the MFMA steps (j, e). Any k <-> (j, lane
//             quarter, e) bijection is a valid reduction order as long as both operands use it, so row-major activations
//             and row-major weights need no fragment image. Rows beyond the last are a clamped copy, never stored.
//   result:   D[row 4 (l >> 4) + r][column l & 15] = acc[r], stored into red[wave][row][17] (17: a column's four row
//             quarters land in different banks); after a barrier the thread of (row, column) adds the waves' partials.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace capnet {

typedef float f32x4 __attribute__((ext_vector_type(4)));
__host__ __device__ __forceinline__ int clamp_row(int r, int n) { return r < n ? r : n - 1; }

// acc + A . B over NJ k groups of one row tile
template <int NJ>
__device__ __forceinline__ f32x4 mfma_chain(const f32x4 (&av)[NJ], const f32x4 (&wv)[NJ], f32x4 acc) {
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j][e], wv[j][e], acc, 0, 0, 0);
  return acc;
}
// init + the WAVES partials of (row, col), added in wave order 0 .. WAVES - 1
template <int WAVES, int ROWS>
__device__ __forceinline__ float sum_partials(const float (*red)[ROWS][17], int row, int col, float init) {
  float s = init;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) s += red[w][row][col];
  return s;
}

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// The LSTM cell on the pre-activations of the four roles (input, forget, output, candidate), whatever column block a
// kernel keeps them in: c = f c' + i g; h = o c (DecoderFactoredLSTM, stylenet/model.py:147-153) or, tanh_out, h = o tanh(c)
// (nn.LSTMCell, nic/model.py:77). lstm_cell_h is called where a kernel stores h, behind its stores of the gates and c.
// lstm_pointwise_fwd_kernel (seq_kernels.hip) has lstm_cell's lines written out: change the cell in both places.
__device__ __forceinline__ void lstm_cell(float pi, float pf, float po, float pg, float cp, float& i, float& f, float& o,
                                          float& g, float& c) {
  i = sigm(pi), f = sigm(pf), o = sigm(po), g = tanhf(pg);
  c = f * cp + i * g;
}
__device__ __forceinline__ float lstm_cell_h(float o, float c, int tanh_out) { return tanh_out ? o * tanhf(c) : o * c; }

// Kernels whose waves hold NJ = H / 64 = 1, 2, 4, 8 or 16 k groups each: dispatch_nj calls f(nj_t<NJ>{}) for a supported H
constexpr bool step_hidden_supported(int H) { return H == 64 || H == 128 || H == 256 || H == 512 || H == 1024; }
template <int N> using nj_t = std::integral_constant<int, N>;
template <class F>
static inline void dispatch_nj(int H, F&& f) {
  switch (H) {
    case 64: f(nj_t<1>{}); break;
    case 128: f(nj_t<2>{}); break;
    case 256: f(nj_t<4>{}); break;
    case 512: f(nj_t<8>{}); break;
    default: f(nj_t<16>{}); break;
  }
}

}  // namespace capnet
