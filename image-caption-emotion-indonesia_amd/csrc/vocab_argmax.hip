// Greedy decoding of capnet.seq2seq (seq2seq/model.py:100-122, 193-217): the vocabulary projection and its argmax in ONE
// launch, without the logits ever reaching memory (the whole `sample` loop around it: decode_loops.hip).
//   tok[r] = first argmax_v (h[r] . W[v] + b[v])        h [rows][H], W [V][H] (nn.Linear), b [V]
//
// The mapping, the weight groups and the hand-off are vocab_core.h's. Per row, 32 threads reduce (value, index) with a
// strict comparison, ties to the lower index, and the workgroup writes one packed (value, index) word. The group's last
// arriver reduces the workgroups' words per row -- the winner does not depend on who was last, the comparison is a total
// order on (value, index) -- and writes the int64 token where the next step's layer-0 launch gathers its embedding row
// (and into the ids matrix). NaN and -inf logits are never picked (strict `>` against -inf, as argmax_rows_kernel); a row
// with nothing to pick yields 0.
#include "common.h"
#include "kernels.h"
#include "vocab_core.h"

namespace capnet {

struct VocabArgmaxArgs {
  const float* h;            // [rows][H], group-major
  unsigned long long* part;  // [groups][workgroups][rpg]: (value bits << 32) | index
  int* counter;              // group g's at counter + 4 g; zero before the first use, zero again when the launch ends
  long long* tok;            // optional [rows]
  long long* ids;            // optional: ids[r * ld_ids]
  long ld_ids;
  int rpg, H, V;             // rows per group: workgroup (., g) owns rows [g rpg, (g + 1) rpg)
  VocabGroups g;
};

template <int NJ, int TM>
__global__ __launch_bounds__(512) void vocab_argmax_kernel(VocabArgmaxArgs a) {
  const int rows = a.rpg, grp = blockIdx.y;
  const long rbeg = (long)grp * rows;                                    // the group's rows, numbered from 0 below
  unsigned long long* gpart = a.part + (long)grp * gridDim.x * rows;     // the group's block, [workgroups][rpg]
  unsigned long long* part = gpart + (long)blockIdx.x * rows;
  vocab_front<NJ, TM>(a.h + rbeg * a.H, rows, a.g.w[grp], a.g.b[grp], a.H, a.V, [&](int row, bool valid, float v) {
    const int ec = threadIdx.x & 31, ecol = blockIdx.x * kVocCols + ec;   // the thread's entry
    float best = -INFINITY;
    int bi = kVocNone;
    if (ecol < a.V && v > best) { best = v; bi = ecol; }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {                    // the row's 32 threads are one half of a wave
      const float ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (vocab_better(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if (ec == 0 && valid) vocab_store(part + row, vocab_pack(best, (unsigned)bi));
  });
  if (!arrive_last(a.counter + 4 * grp, gridDim.x)) return;
  // the group's last arriver: a wave per row of the group, the workgroups' partials across its lanes
  const int nwg = gridDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int row = wave; row < rows; row += kVocWaves) {
    float best = -INFINITY;
    int bi = kVocNone;
    for (int p0 = 0; p0 < nwg; p0 += 64 * 4) {
      unsigned long long u[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) u[q] = vocab_load(gpart + (long)min(p0 + 64 * q + lane, nwg - 1) * rows + row);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = vocab_hi(u[q]);
        const int i = (int)vocab_lo(u[q]);
        if (p0 + 64 * q + lane < nwg && vocab_better(v, i, best, bi)) { best = v; bi = i; }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (vocab_better(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) {
      const long long t = bi == kVocNone ? 0 : bi;
      if (a.tok) a.tok[rbeg + row] = t;
      if (a.ids) a.ids[(rbeg + row) * a.ld_ids] = t;
    }
  }
  vocab_rearm(a.counter + 4 * grp);
}

bool vocab_argmax_supported(int H) { return step_hidden_supported(H); }

// workspace: per group 16 bytes whose first int is the group's counter, then one 8-byte partial per group, workgroup and row
size_t vocab_argmax_groups_ws_bytes(int groups, int rpg, int V) {
  return 16 * (size_t)groups + (size_t)groups * vocab_workgroups(V) * rpg * 8;
}
size_t vocab_argmax_ws_bytes(int rows, int V) { return vocab_argmax_groups_ws_bytes(1, rows, V); }

int vocab_argmax(const float* h, const float* w, const float* b, int rows, int H, int V, void* ws, long long* tok,
                 long long* ids, long ld_ids, hipStream_t stream) {
  return vocab_argmax_groups(h, &w, b ? &b : nullptr, 1, rows, H, V, ws, tok, ids, ld_ids, stream);
}

int vocab_argmax_groups(const float* h, const float* const* w, const float* const* b, int groups, int rpg, int H, int V,
                        void* ws, long long* tok, long long* ids, long ld_ids, hipStream_t stream) {
  CAPNET_REQUIRE(groups >= 1 && groups <= kVocMaxGroups && rpg >= 1, "vocab_argmax: %d groups of %d rows", groups, rpg);
  VocabArgmaxArgs a;
  a.h = h;
  vocab_fill_groups(a.g, w, b, groups);
  a.counter = reinterpret_cast<int*>(ws);
  a.part = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ws) + 16 * (size_t)groups);
  a.tok = tok; a.ids = ids; a.ld_ids = ld_ids;
  a.rpg = rpg; a.H = H; a.V = V;
  const dim3 grid(vocab_workgroups(V), groups), block(64 * kVocWaves);
  dispatch_nj(H, [&](auto nj) {   // two row tiles per pass where their operands fit beside the weights
    hipLaunchKernelGGL((vocab_argmax_kernel<nj, nj <= 8 ? 2 : 1>), grid, block, 0, stream, a);
  });
  CAPNET_LAUNCH_CHECK();
  return kOk;
}

}  // namespace capnet
