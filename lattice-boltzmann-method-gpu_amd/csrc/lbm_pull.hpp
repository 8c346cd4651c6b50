// lbm_pull.hpp -- neighbour addressing and the one-cell pulls shared by the kernel translation
// units (lbm_kernels.hip: the step and the lazy macros; lbm_stress.hip: the stress read-out).
// Device code only; everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "lbm_d3q19.hpp"
#include "lbm_kernels.hpp"

namespace lbm {

namespace {

// Storage direction of population Q.  The layout's rows run along physical x, or along y
// when SW (lbm_desc.row_axis: a pipe along y then fills whole rows); z is always the slab
// axis.  Only addresses change with SW -- the arithmetic stays in physical q order.
template <int Q, bool SW>
struct SDir {
  static constexpr int x = SW ? Dir<Q>::y : Dir<Q>::x;  // along the row: +-1 cell
  static constexpr int y = SW ? Dir<Q>::x : Dir<Q>::y;  // across rows: +-pitch
  static constexpr int z = Dir<Q>::z;                   // across planes: +-plane
};

template <int Q, bool SW>
constexpr int64_t row_off(int pitch, int64_t plane) {
  return SDir<Q, SW>::y * (int64_t)pitch + SDir<Q, SW>::z * plane;
}
// storage offset of e_Q: population Q of cell c is pulled from c - cell_off
template <int Q, bool SW>
constexpr int64_t cell_off(int pitch, int64_t plane) {
  return SDir<Q, SW>::x + row_off<Q, SW>(pitch, plane);
}

// Neighbour addressing of a lane's cell c (a 4-cell lane: its first cell):
//   slice<Q>() -- the cell c - e_Q with e_x = 0: the aligned 16-B slice a 4-cell lane pulls,
//   nb<Q>()    -- the cell c - e_Q.
// AddrD: the dense box -- cell (zs, s1, s0) at s0 - xshift + s1 * pitch + zs * plane, every
// neighbour a constant offset.  Rows: compact rows (sparse lattices, lbm_create's choice) --
// storage row r = zs * nrow + s1 keeps only the span of its stored cells, the spans packed one
// after the other in storage order, so cell (r, s0) lives at roff[r] + s0; a lane holds the
// offsets of the nine rows around its own (loaded once, Rows::load).  Inside a span x +- 1 is
// still c +- 1, and a fluid cell's neighbours are always stored, so they lie inside theirs.
// float index of slot q of cell c (aidx): 64-bit for the dense box, 32-bit for compact rows
// (lbm_create keeps their buffers, guards included, under 2^31 floats)
__device__ __forceinline__ int64_t fidx(int64_t c, int q) { return aidx(c, q); }
__device__ __forceinline__ int fidx(int c, int q) { return ((c >> 8) * kQ + q) * kChunk + (c & (kChunk - 1)); }
// a compact cell id as the 32-bit index of the compact paths (kCompactMaxFloats bounds every id
// of a compact buffer); -DLBM_DEBUG_INDEX traps on an id outside that bound instead of letting
// a 32-bit offset wrap
__device__ __forceinline__ int compact_id(int64_t c) {
#ifdef LBM_DEBUG_INDEX
  if (c < -int64_t(kChunk) * 64 || ((c >> 8) * kQ + kQ) * kChunk > kCompactMaxFloats) __builtin_trap();
#endif
  return (int)c;
}

template <int Q, bool SW>
constexpr int row_k() {  // Rows::rb index of the row population Q is pulled from
  return (-SDir<Q, SW>::y + 1) * 3 + (-SDir<Q, SW>::z + 1);
}
struct Rows {
  int rb[9];  // roff[r + dy + dz * nrow], index (dy + 1) * 3 + dz + 1
  int s0;     // the cell's position in its row: c - roff[r]
  template <int Q, bool SW>
  __device__ __forceinline__ int slice() const { return rb[row_k<Q, SW>()] + s0; }
  template <int Q, bool SW>
  __device__ __forceinline__ int nb() const { return rb[row_k<Q, SW>()] + s0 - SDir<Q, SW>::x; }
  __device__ __forceinline__ void opaque() {
    asm volatile("" : "+v"(rb[0]), "+v"(rb[1]), "+v"(rb[2]), "+v"(rb[3]), "+v"(rb[4]), "+v"(rb[5]), "+v"(rb[6]),
                 "+v"(rb[7]), "+v"(rb[8]), "+v"(s0));
  }
  __device__ __forceinline__ Rows get() const { return *this; }
  // the row record of row r (MainArgs::rowrec: 12 ints, the nine offsets first) -- three 16-B loads
  __device__ __forceinline__ static Rows load(const int4* __restrict__ rowrec, int64_t c, int r) {
    const int4* p = rowrec + (int64_t)r * 3;
    const int4 x = p[0], y = p[1], z = p[2];
    Rows R;
    R.rb[0] = x.x; R.rb[1] = x.y; R.rb[2] = x.z; R.rb[3] = x.w;
    R.rb[4] = y.x; R.rb[5] = y.y; R.rb[6] = y.z; R.rb[7] = y.w;
    R.rb[8] = z.x;
    R.s0 = compact_id(c) - R.rb[4];
    return R;
  }
};

using AllQ = std::make_integer_sequence<int, kQ>;

// One cell's 19 pulls through an address policy with bounce-back on the consumer side
// (MainArgs::bb_pull): where bit q of wl is set (c - e_q a wall), population q comes from the
// cell's own slot opp(q) -- Poiseulle.cu:601-746's d_dst[q][W] = d_dst[opp q][W + e_q] with
// W + e_q = c, read where it was stored.
// Plain (temporal) loads: the compact lattices' buffers stay in the caches from one step to the
// next: non-temporal -> plain loads took C4 from 8.13 to 7.75 us per step and the coronary tree
// from 35.9 to 31.2 us (profiles/r05_c1_temporal_ab.log)
template <bool SW, class A, class CT, int... Qs>
__device__ __forceinline__ void pull1_bb(float* f, const float* __restrict__ src, const A& ad, CT c, uint32_t wl,
                                         std::integer_sequence<int, Qs...>) {
  ((f[Qs] = *(
        src + ((wl >> Qs) & 1u ? fidx(c, Dir<Qs>::opp) : fidx(ad.template nb<Qs, SW>(), Qs)))),
   ...);
}

// The same for a cell of the dense box (the lazy read-outs): wl = 0 pulls every population
// plainly, as a producer-side step does
template <bool SW, int... Qs>
__device__ __forceinline__ void pull1_links(float* f, const float* __restrict__ src, int64_t c, uint32_t wl, int pitch,
                                            int64_t plane, std::integer_sequence<int, Qs...>) {
  ((f[Qs] = src[(wl >> Qs) & 1u ? aidx(c, Dir<Qs>::opp) : aidx(c - cell_off<Qs, SW>(pitch, plane), Qs)]), ...);
}

}  // namespace

}  // namespace lbm
