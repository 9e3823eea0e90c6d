// One inference step of one factored-LSTM layer of capnet.stacked.StackedFactoredLSTM, for any number of rows, in ONE
// launch (beam-search decoding: k rows per image, n k rows per batched decode step):
//   gates = [x | h_prev] . [Weff | W]^T + beff      Weff_g = U_g S_g V_g, beff_g = U_g (S_g bV_g + bS_g) + bU_g + bW_g
//   i, f, o = sigmoid, c~ = tanh;  c = f c_prev + i c~;  h = o c      (no tanh on c, stylenet/model.py:147-153)
// Inference has no dropout between V, S and U, so the chain folds into one H x in matrix per gate (the host folds it once
// per decode, capnet.stacked). Layer 0's x is a row of the embedding table picked by token id (or a given input row),
// layer l > 0's x is h of layer l-1 at the same step, which the previous launch of the same call has just written.
//
// Mapping: a workgroup owns 4 hidden units = 16 gate columns (one N tile of the 16-row product, step_core.h) and ALL rows. Its 8
// waves split K = kin + H (kin = in rounded up to the 16-wide k group; the weights carry zero columns there) into eight
// contiguous ranges of k groups. Each lane loads its column's weights for its range once (NJ f32x4 registers: the
// layer's weights cross HBM once per launch) and keeps them while the workgroup walks the rows 16 TM at a time: per pass a
// lane reads 16 B of x or h_prev per k group for each of TM 16-row tiles, runs the tiles' MFMA chains interleaved (TM = 2;
// TM = 1 at 16 groups per wave, where two tiles' operands and the weights would not fit in 256 VGPRs),
// and the eight K-partial tiles are summed through LDS by the epilogue, which applies the gates and writes c, h (and the
// top layer's h once more, densely, for the vocabulary projection). Plain vector loads and stores only.
// GATHER (beam search: capnet_stacked_decode_step_gather, capnet_beam_decode): a row's h_prev and c_prev are those of row
// parent[row] of state_in -- the re-ordering of the beams read in place instead of copied first. Only the two state reads
// move: x, the token ids and every store stay on the row itself, and state_in != state_out makes repeated parents safe.
// The nn.LSTMCell instance (TANH_OUT, capnet.nic_stacked) takes wcat = [weight_ih, zero columns up to kin | weight_hh]
// and beff = bias_ih + bias_hh with the host's gate blocks reordered from torch's i, f, g, o to i, f, o, c~ = g: the
// LSTM cell has no chain to fold, and only the epilogue differs, h = o tanh(c).
// Weight groups (every style at once: capnet_stacked_decode_step_groups, capnet_beam_decode_groups): the grid is (H / 4,
// G), rows are group-major, and workgroup (., g) walks only rows [g rpg, (g + 1) rpg) on the weights w + g 4H (kin + H)
// and b + g 4H. A 16-row tile never reaches into the next group (the row clamp and the store mask end at the group);
// parents are checked against all the rows. G = 1 is the kernel as it was.
// Per-group layer-0 tables (every emotion of capnet.seq2seq at once: capnet_stacked_decode_step_tables,
// capnet_lstm_greedy_decode_groups): workgroup (., g) gathers its token rows from xg[g], one table pointer per group held
// by value in the argument struct and picked by blockIdx.y -- a scalar load from the kernel arguments, no copy of a table
// and nothing per lane. Every other caller puts its one table (or its input rows) into all the slots.
// Layer 0 of an attention decoder reads [embedding | gated context], E + C columns: above kDecMaxK it runs on
// lstm_decode_step_wide_kernel (below; K up to 4096, a wave's range in two halves), and att_decode_step at the end of
// this file is the attention decoders' beam step around it (z, the beam-aware attention kernels of att_kernels.hip, the layers).
#include "common.h"
#include "kernels.h"
#include "step_core.h"

namespace capnet {

constexpr int kDecWaves = 8;
constexpr int kDecMaxK = 2048;       // kin + H <= 8 waves x 16 groups x 16 (lstm_decode_step_wide_kernel: kDecWideMaxK)
constexpr int kDecMaxGroups = 8;     // weight groups of one launch (capnet_*_groups)

struct DecodeLayerArgs {
  const long long* tok;  // layer 0 with token ids: x row = x + tok[r] * ldx (else x + r * ldx)
  const float* x;
  long ldx;
  int xn;                // valid columns of an x row (E or H); columns [xn, kin) read as zero
  int xvec;              // x rows 16-B aligned and xn % 4 == 0: f32x4 loads
  int V;                 // token ids must lie in [0, V)
  int* err;              // bit 0 is raised (atomicOr: the word's other bits stay) on an out-of-range id (the row then reads token 0)
  const float* hprev;    // [rows] x stride lds_in
  const float* cprev;
  long lds_in;
  float* h_out;
  float* c_out;
  long lds_out;
  float* h_top;          // optional dense [rows, H] copy of h
  const float* w;        // [4H, kin + H] = [Weff | W], gate blocks i, f, o, c~
  const float* b;        // [4H]
  int kin, rows, H;
  const long long* parent;  // GATHER: int64 [rows], hprev / cprev are read at row parent[r] (outside [0, rows): err, row r)
  int rpg;               // rows per weight group: workgroup (., g) walks rows [g rpg, (g + 1) rpg) on w + g wgs, b + g 4H
  long wgs;              // floats between two groups' weights, 4H (kin + H)
  const float* xg[kDecMaxGroups];   // lstm_decode_step_kernel: group g's x (`x` itself unless the groups own their tables)
};

// the row whose previous state row `row` reads
template <bool GATHER>
__device__ __forceinline__ long state_row(const DecodeLayerArgs& a, int row) {
  if constexpr (GATHER) {
    const long long p = a.parent[row];
    const bool ok = p >= 0 && p < a.rows;
    if (!ok && a.err) atomicOr(a.err, 1);
    return ok ? (long)p : (long)row;
  } else {
    return row;
  }
}

// k groups per wave (at most), 16-row tiles per pass; h = o tanh(c); the previous state through a.parent
template <int NJ, int TM, bool TANH_OUT, bool GATHER>
__global__ __launch_bounds__(512) void lstm_decode_step_kernel(DecodeLayerArgs a) {
  constexpr int kPass = 16 * TM;
  __shared__ float red[kDecWaves][kPass][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int H = a.H, u0 = blockIdx.x * 4;
  const int K = a.kin + H, KG = K >> 4, inG = a.kin >> 4;
  const int g0 = wave * KG / kDecWaves, ng = (wave + 1) * KG / kDecWaves - g0;   // this wave's groups [g0, g0 + ng)
  // B operand: column li = gate role li >> 2 (i, f, o, c~), unit u0 + (li & 3)
  const int grp = blockIdx.y, rbeg = grp * a.rpg, rend = rbeg + a.rpg;   // this group's rows; one group: [0, rows)
  const float* wrow = a.w + grp * a.wgs + (long)((li >> 2) * H + u0 + (li & 3)) * K + 4 * lq;
  const float* xbase = a.xg[grp];
  f32x4 wv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    wv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (j < ng) wv[j] = *reinterpret_cast<const f32x4*>(wrow + 16 * (g0 + j));
  }
  // epilogue thread: (row er of the pass, unit eu); threads 0 .. 64 TM - 1
  const int er = tid >> 2, eu = tid & 3;
  const bool ethread = tid < 4 * kPass;
  float bias[4] = {0.f, 0.f, 0.f, 0.f};
  if (ethread) {
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = a.b[(grp * 4 + g) * H + u0 + eu];
  }
  for (int r0 = rbeg; r0 < rend; r0 += kPass) {
    f32x4 av[TM][NJ];
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      const int row = clamp_row(r0 + 16 * m + li, rend);
      long xr = row;
      if (a.tok) {
        const long long t = a.tok[row];
        const bool ok = t >= 0 && t < a.V;
        if (!ok && a.err) atomicOr(a.err, 1);
        xr = ok ? (long)t : 0;
      }
      const float* xrow = xbase + xr * a.ldx;
      const float* hrow = a.hprev + state_row<GATHER>(a, row) * a.lds_in;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int g = g0 + j, k = 16 * g + 4 * lq;
        if (j < ng) {
          if (g >= inG) {
            v = *reinterpret_cast<const f32x4*>(hrow + (k - a.kin));
          } else if (a.xvec) {
            if (k < a.xn) v = *reinterpret_cast<const f32x4*>(xrow + k);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = k + e < a.xn ? xrow[k + e] : 0.f;
          }
        }
        av[m][j] = v;
      }
    }
    const int erow = r0 + er;
    const bool estore = ethread && erow < rend;
    const float cp = estore ? a.cprev[state_row<GATHER>(a, erow) * a.lds_in + u0 + eu] : 0.f;
    f32x4 acc[TM];
#pragma unroll
    for (int m = 0; m < TM; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (j < ng) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int m = 0; m < TM; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][j][e], wv[j][e], acc[m], 0, 0, 0);
      }
    }
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][16 * m + 4 * lq + r][li] = acc[m][r];
    __syncthreads();
    if (estore) {
      float pre[4], i, f, og, gt, c;
#pragma unroll
      for (int g = 0; g < 4; ++g) pre[g] = sum_partials<kDecWaves>(red, er, g * 4 + eu, bias[g]);
      lstm_cell(pre[0], pre[1], pre[2], pre[3], cp, i, f, og, gt, c);
      const float h = lstm_cell_h(og, c, TANH_OUT);
      a.c_out[(long)erow * a.lds_out + u0 + eu] = c;
      a.h_out[(long)erow * a.lds_out + u0 + eu] = h;
      if (a.h_top) a.h_top[(long)erow * H + u0 + eu] = h;
    }
    __syncthreads();   // red is rewritten by the next pass
  }
}

// K = kin + H above kDecMaxK, up to kDecWideMaxK (layer 0 of an attention decoder: x = [embedding | gated context], E + C
// columns): a wave's range is up to 2 NJ k groups, walked in two halves of at most NJ. Per pass of 32 rows and per half a
// lane loads the half's weights (NJ f32x4) and, tile by tile, the activations of the pass's two 16-row tiles (NJ f32x4 at a
// time); the two accumulators are carried across the halves. So up to 32 rows the weights cross HBM once per launch, as
// above; past 32 rows every further pass reads them again (from L2: a workgroup's slice is 16 columns x K). Both halves'
// weights resident (2 NJ f32x4) beside one half's activations did not fit in 256 VGPRs. x rows must take f32x4 loads.
constexpr int kDecWideMaxK = 4096;   // 8 waves x 2 halves x 16 groups x 16

template <int NJ, bool TANH_OUT, bool GATHER>
__global__ __launch_bounds__(512) void lstm_decode_step_wide_kernel(DecodeLayerArgs a) {
  __shared__ float red[kDecWaves][32][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int H = a.H, u0 = blockIdx.x * 4;
  const int K = a.kin + H, KG = K >> 4, inG = a.kin >> 4;
  const int g0 = wave * KG / kDecWaves, ng = (wave + 1) * KG / kDecWaves - g0;   // this wave's groups [g0, g0 + ng), ng <= 2 NJ
  const int grp = blockIdx.y, rbeg = grp * a.rpg, rend = rbeg + a.rpg;   // this group's rows; one group: [0, rows)
  const float* wrow = a.w + grp * a.wgs + (long)((li >> 2) * H + u0 + (li & 3)) * K + 4 * lq;
  const int er = tid >> 2, eu = tid & 3;
  const bool ethread = tid < 128;
  float bias[4] = {0.f, 0.f, 0.f, 0.f};
  if (ethread) {
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = a.b[(grp * 4 + g) * H + u0 + eu];
  }
  for (int r0 = rbeg; r0 < rend; r0 += 32) {
    const int tiles = r0 + 16 < rend ? 2 : 1;
    const float* xrow[2];
    const float* hrow[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int row = clamp_row(r0 + 16 * m + li, rend);
      long xr = row;
      if (a.tok) {
        const long long t = a.tok[row];
        const bool ok = t >= 0 && t < a.V;
        if (!ok && a.err) atomicOr(a.err, 1);
        xr = ok ? (long)t : 0;
      }
      xrow[m] = a.x + xr * a.ldx;
      hrow[m] = a.hprev + state_row<GATHER>(a, row) * a.lds_in;
    }
    const int erow = r0 + er;
    const bool estore = ethread && erow < rend;
    const float cp = estore ? a.cprev[state_row<GATHER>(a, erow) * a.lds_in + u0 + eu] : 0.f;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 1
    for (int hf = 0; hf < 2; ++hf) {
      const int j0 = hf * NJ;
      f32x4 wv[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        wv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j0 + j < ng) wv[j] = *reinterpret_cast<const f32x4*>(wrow + 16 * (g0 + j0 + j));
      }
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        if (m < tiles) {
          f32x4 av[NJ];
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int g = g0 + j0 + j, k = 16 * g + 4 * lq;
            if (j0 + j < ng) {
              if (g >= inG) v = *reinterpret_cast<const f32x4*>(hrow[m] + (k - a.kin));
              else if (k < a.xn) v = *reinterpret_cast<const f32x4*>(xrow[m] + k);
            }
            av[j] = v;
          }
          acc[m] = mfma_chain<NJ>(av, wv, acc[m]);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][16 * m + 4 * lq + r][li] = acc[m][r];
    __syncthreads();
    if (estore) {
      float pre[4], i, f, og, gt, c;
#pragma unroll
      for (int g = 0; g < 4; ++g) pre[g] = sum_partials<kDecWaves>(red, er, g * 4 + eu, bias[g]);
      lstm_cell(pre[0], pre[1], pre[2], pre[3], cp, i, f, og, gt, c);
      const float h = lstm_cell_h(og, c, TANH_OUT);
      a.c_out[(long)erow * a.lds_out + u0 + eu] = c;
      a.h_out[(long)erow * a.lds_out + u0 + eu] = h;
      if (a.h_top) a.h_top[(long)erow * H + u0 + eu] = h;
    }
    __syncthreads();   // red is rewritten by the next pass
  }
}

static int round16(int v) { return (v + 15) / 16 * 16; }

bool stacked_decode_supported(int E, int H) {
  return E >= 1 && step_hidden_supported(H) && round16(E) + H <= kDecMaxK;
}

bool stacked_decode_wide_supported(int E, int H) {
  return E >= 4 && E % 4 == 0 && step_hidden_supported(H) && round16(E) + H <= kDecWideMaxK;
}

constexpr int dec_tm(int nj) { return nj <= 12 ? 2 : 1; }   // 16-row tiles per pass of lstm_decode_step_kernel<nj>

// Host only: the instance launch_decode_layer gives a layer of kin (a multiple of 16) input columns, or false where
// decode_layer refuses the shape (capnet_stacked_decode_route reports it). The wide kernel always walks two tiles.
bool stacked_decode_route(int kin, int H, int xvec, DecodeRoute* r) {
  const int K = kin + H;
  if (!(K <= kDecMaxK || (xvec && K <= kDecWideMaxK))) return false;
  const int per_wave = (K / 16 + kDecWaves - 1) / kDecWaves;
  r->wide = per_wave > 16;
  r->nj = per_wave <= 2 ? 2 : per_wave <= 4 ? 4 : per_wave <= 6 ? 6 : per_wave <= 8 ? 8 : per_wave <= 12 ? 12 : per_wave <= 16 ? 16
          : per_wave <= 24 ? 12 : 16;
  r->tm = r->wide ? 2 : dec_tm(r->nj);
  return true;
}

template <int NJ, bool TANH_OUT, bool GATHER>
static void launch_decode(const DecodeLayerArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL((lstm_decode_step_kernel<NJ, dec_tm(NJ), TANH_OUT, GATHER>), dim3(a.H / 4, a.rows / a.rpg), dim3(64 * kDecWaves), 0,
                     stream, a);
}

template <bool TANH_OUT, bool GATHER>
static int launch_decode_layer(const DecodeLayerArgs& a, hipStream_t stream) {
  DecodeRoute r;
  CAPNET_REQUIRE(stacked_decode_route(a.kin, a.H, a.xvec, &r), "decode step: K = %d + %d", a.kin, a.H);
  if (r.wide) {
    if (r.nj == 12) hipLaunchKernelGGL((lstm_decode_step_wide_kernel<12, TANH_OUT, GATHER>), dim3(a.H / 4, a.rows / a.rpg), dim3(64 * kDecWaves), 0, stream, a);
    else hipLaunchKernelGGL((lstm_decode_step_wide_kernel<16, TANH_OUT, GATHER>), dim3(a.H / 4, a.rows / a.rpg), dim3(64 * kDecWaves), 0, stream, a);
  } else {
    switch (r.nj) {
      case 2: launch_decode<2, TANH_OUT, GATHER>(a, stream); break;
      case 4: launch_decode<4, TANH_OUT, GATHER>(a, stream); break;
      case 6: launch_decode<6, TANH_OUT, GATHER>(a, stream); break;
      case 8: launch_decode<8, TANH_OUT, GATHER>(a, stream); break;
      case 12: launch_decode<12, TANH_OUT, GATHER>(a, stream); break;
      default: launch_decode<16, TANH_OUT, GATHER>(a, stream); break;
    }
  }
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

// layer l of the stack on x rows of xn valid columns at stride ldx (token ids: rows of the table x)
static int decode_layer(int cell, int l, int nlayers, int rows, int H, int V, const long long* tokens, const float* x, long ldx,
                        int xn, const float* w, const float* b, const float* state_in, float* state_out, float* h_top,
                        int* err_flag, hipStream_t stream, const long long* parent_rows, int groups,
                        const float* const* tables = nullptr) {
  const long lds = 2L * nlayers * H;
  DecodeLayerArgs a;
  CAPNET_REQUIRE(groups >= 1 && groups <= kDecMaxGroups && rows % groups == 0, "decode step: %d rows in %d groups", rows, groups);
  CAPNET_REQUIRE(!tables || tokens, "decode step: per-group tables are read by token id");
  a.tok = tokens;
  a.x = tables ? tables[0] : x;
  a.ldx = ldx;
  a.xn = xn;
  a.xvec = xn % 4 == 0 && ldx % 4 == 0;
  for (int g = 0; g < kDecMaxGroups; ++g) {
    a.xg[g] = tables && g < groups ? tables[g] : a.x;
    a.xvec = a.xvec && aligned16(a.xg[g]);
  }
  a.kin = round16(xn);
  a.V = V;
  a.err = err_flag;
  a.hprev = state_in + (long)(2 * l) * H;
  a.cprev = state_in + (long)(2 * l + 1) * H;
  a.lds_in = lds;
  a.h_out = state_out + (long)(2 * l) * H;
  a.c_out = state_out + (long)(2 * l + 1) * H;
  a.lds_out = lds;
  a.h_top = l == nlayers - 1 ? h_top : nullptr;
  a.w = w;
  a.b = b;
  a.rows = rows;
  a.H = H;
  a.parent = parent_rows;
  a.rpg = rows / groups;
  a.wgs = 4L * H * (a.kin + H);
  CAPNET_REQUIRE(a.kin + H <= kDecMaxK || (a.xvec && a.kin + H <= kDecWideMaxK), "decode step: K = %d + %d", a.kin, H);
  CAPNET_REQUIRE(!tables || a.kin + H <= kDecMaxK, "decode step: per-group tables need K = %d + %d <= %d", a.kin, H, kDecMaxK);
  if (parent_rows) return cell == kCellLSTM ? launch_decode_layer<true, true>(a, stream) : launch_decode_layer<false, true>(a, stream);
  return cell == kCellLSTM ? launch_decode_layer<true, false>(a, stream) : launch_decode_layer<false, false>(a, stream);
}

int stacked_decode_step(int cell, int nlayers, int rows, int E, int H, int V, const long long* tokens, const float* x,
                        const float* const* wcat, const float* const* beff, const float* state_in, float* state_out,
                        float* h_top, int* err_flag, hipStream_t stream, const long long* parent_rows, int groups,
                        const float* const* tables) {
  const long lds = 2L * nlayers * H;
  for (int l = 0; l < nlayers; ++l) {
    const int rc = l == 0 ? decode_layer(cell, 0, nlayers, rows, H, V, tokens, x, E, E, wcat[0], beff[0], state_in, state_out,
                                         h_top, err_flag, stream, parent_rows, groups, tables)
                          : decode_layer(cell, l, nlayers, rows, H, V, nullptr, state_out + (long)(2 * l - 2) * H, lds, H, wcat[l],
                                         beff[l], state_in, state_out, h_top, err_flag, stream, parent_rows, groups);
    if (rc != kOk) return rc;
  }
  return kOk;
}

// ---- one beam step of an attention decoder ---------------------------------------------------------------------------
// ws (floats): z [n k][A + C] | xa [n k][E + C] | escore [n k][P rounded up to 4]; every part a multiple of 16 bytes
bool att_decode_supported(int E, int C, int H, int A, int P, int k, int nlayers) {
  return nlayers >= 1 && nlayers <= 8 && att_beam_step_supported(E, C, A, P, k) && stacked_decode_wide_supported(E + C, H);
}

size_t att_decode_step_ws_bytes(int n, int k, int P, int A, int C, int E) {
  if (n < 1 || !att_beam_step_supported(E, C, A, P, k)) return 0;
  return (size_t)n * k * ((size_t)A + 2 * (size_t)C + E + (P + 3) / 4 * 4) * sizeof(float);
}

int att_decode_step(int cell, int nlayers, int n, int k, int P, int A, int C, int E, int H, int V, const float* att1,
                    const float* feat, const long long* tokens, const float* emb, const float* wz, const float* bz,
                    const float* wf, const float* bf, const float* const* wcat, const float* const* beff,
                    const float* state_in, const long long* parent_rows, float* state_out, float* h_top, void* ws, float* slab,
                    size_t slab_floats, int* err_flag, hipStream_t stream, int groups, float* alphas) {
  const int gk = n * k, nk = groups * gk;     // rows of one weight group (n images), rows in all
  const long lds = 2L * nlayers * H;
  float* z = reinterpret_cast<float*>(ws);
  float* xa = z + (size_t)nk * (A + C);
  float* escore = xa + (size_t)nk * (E + C);
  // z of every row from its OWN previous h (layer 0's, slot 0 of state_in); the kernels read it at the parent's row.
  // One product per weight group on the group's rows: the call a search of that group alone makes
  int rc = kOk;
  for (int g = 0; g < groups && rc == kOk; ++g)
    rc = sgemm_splitk(false, true, gk, A + C, H, state_in + (long)g * gk * lds, lds, wz + (long)g * (A + C) * H, H,
                      z + (long)g * gk * (A + C), A + C, bz + (long)g * (A + C), 0, slab, slab_floats, stream);
  if (rc == kOk) rc = att_beam_step_fwd(att1, feat, z, parent_rows, wf, bf, tokens, emb, V, E, groups * n, k, P, A, C, escore, xa,
                                        err_flag, stream, n, alphas);
  if (rc == kOk) rc = decode_layer(cell, 0, nlayers, nk, H, V, nullptr, xa, E + C, E + C, wcat[0], beff[0], state_in, state_out,
                                   h_top, err_flag, stream, parent_rows, groups);
  for (int l = 1; l < nlayers && rc == kOk; ++l)
    rc = decode_layer(cell, l, nlayers, nk, H, V, nullptr, state_out + (long)(2 * l - 2) * H, lds, H, wcat[l], beff[l], state_in,
                      state_out, h_top, err_flag, stream, parent_rows, groups);
  return rc;
}

}  // namespace capnet
