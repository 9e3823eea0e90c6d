// The pieces of the two-piece f16 arithmetic that every kernel of the split-f16 family shares (conv_f16x3.hip and its
// siblings conv3x3_patch.hip, conv1x1_areg.hip, fused_block.hip, conv_stem.hip; lstm_persist.hip takes the splits and
// the counted wait): an fp32 operand x (scaled by a power of two) is x = h + l with h = f16(x), l = f16(x - h) -- the
// subtraction is exact in fp32 -- and a product is h h' + (h l' + l h') on the f16 MFMAs, accumulated in fp32.
// Nothing here issues a memory instruction: gload16 / glds16 / gstore32 live in mfma_core.h.
#pragma once
#include "mfma_core.h"

namespace capnet {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));

// ---- operand splits ----
// one value -> its two pieces (the pack kernels: weights are split once per weight version)
__device__ __forceinline__ void split1(float x, _Float16& h, _Float16& l) {
  h = (_Float16)x;
  l = (_Float16)(x - (float)h);
}
// (x0, x1) -> packed f16 pairs of the two pieces
__device__ __forceinline__ void split2(float x0, float x1, unsigned& h, unsigned& l) {
  const f2 v = {x0, x1};
  const h2 hh = __builtin_convertvector(v, h2);          // v_cvt_pk_f16_f32 (round to nearest even)
  const f2 r = v - __builtin_convertvector(hh, f2);
  h = __builtin_bit_cast(unsigned, hh);
  l = __builtin_bit_cast(unsigned, __builtin_convertvector(r, h2));
}
__device__ __forceinline__ void split4(const f32x4 v, h4& h, h4& l) {
  const f2 a = {v[0], v[1]}, b = {v[2], v[3]};
  const h2 ha = __builtin_convertvector(a, h2), hb = __builtin_convertvector(b, h2);      // v_cvt_pk_f16_f32
  const f2 ra = a - __builtin_convertvector(ha, f2), rb = b - __builtin_convertvector(hb, f2);   // exact
  const h2 la = __builtin_convertvector(ra, h2), lb = __builtin_convertvector(rb, h2);
  h = h4{ha[0], ha[1], hb[0], hb[1]};
  l = h4{la[0], la[1], lb[0], lb[1]};
}
__device__ __forceinline__ h8 cat8(const h4 a, const h4 b) { return h8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }

// ---- the packed weight image of conv_f16x3_pack ----
// byte offset of the 16-B cell (row, 8-channel half c) inside one (plane, k16 group) sub-image: the cell position is
// XOR-ed with bit 3 of the row, so that the ds_read_b128 fragment reads are conflict-free
__host__ __device__ inline unsigned f16x3_cell(int row, int c) {
  const int r = row & 15;
  return (unsigned)((row * 2 + (c ^ ((r >> 3) & 1))) * 16);
}

// Every weight image (conv_f16x3_pack, fused_block_pack, conv_stem_f16x3_pack) starts with this header:
//   word 0: ew, the weights' power-of-two scale (the planes hold w 2^ew; the epilogue multiplies by 2^-ew);
//   word 1: the bits of max |w| -- pack scratch (f16x3_pack_header's absmax kernel writes it, the layout kernel reads it);
//   word 2: fused_block_pack only: 1 = the image is laid out for fb_fused_wide_kernel;
//   word 3: unused (keeps the image 16-B aligned).
constexpr int kF16x3HdrWords = 4;

// ew from the bits of max |w|: max |w| 2^ew in [2^13, 2^14) -- a factor 4 below the f16 range, the residuals of all but
// the smallest weights normal f16 numbers
__device__ __forceinline__ int f16x3_weight_shift(unsigned absmax_bits) {
  if (absmax_bits == 0u) return 0;
  const int e = (int)((absmax_bits >> 23) & 0xffu) - 127;       // floor(log2 max|w|)
  const int ew = 13 - e;
  return ew < -100 ? -100 : (ew > 100 ? 100 : ew);
}
// the epilogue's factor 2^-(ew + in_exp): undoes the weights' scale and the input's prescale (exact)
__device__ __forceinline__ float f16x3_out_scale(unsigned ew, int in_exp) {      // ew: word 0 of the image header
  return ldexpf(1.f, -((int)ew + in_exp));
}

// counted wait for the hand-issued vector-memory operations (vmcnt retires in issue order; a 6-bit counter)
template <int N> __device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt immediate");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

}  // namespace capnet
