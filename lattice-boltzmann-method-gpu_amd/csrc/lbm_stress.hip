// lbm_stress.hip -- lbm_get_stress / lbm_get_shear: the viscous stress tensor and the shear-
// stress magnitude of the last step, read out lazily like the macros (k_moments).
//
// In LBM the stress is a local moment of the populations a step pulled,
//   sigma = -(1 - 1/(2 tau)) sum_q e_q e_q (f_q - feq_q),
// so a cell needs its own 19 pulls and nothing else.  k_stress / k_stress_compact repeat the
// pulls of k_moments / k_moments_compact on the last step's source buffer (pull1_links /
// pull1_bb: bounce-back slots, NEE slots, ghost planes) and evaluate include/lbm.h's fixed fp64
// expressions: the non-equilibrium moment is a difference of O(1/3) sums that leaves 1e-4 ..
// 1e-6, so fp32 sums would add an error of the size of the answer.
// The kernels write raster arrays of a batch of planes in a transient scratch; the context keeps
// no per-cell results (a 512^3 lattice would grow by 3.8 GB).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/lbm.h"
#include "lbm_d3q19.hpp"
#include "lbm_kernels.hpp"
#include "lbm_pull.hpp"

namespace lbm {

namespace {

constexpr int64_t kStressScratchBytes = int64_t(256) << 20;  // include/lbm.h's bound

struct StressArgs {
  const float* src;
  const uint8_t* type;
  const uint32_t* bb_links;
  const int* cmap;       // compact rows only
  const int* row_of;
  const int4* rowrec;
  int64_t c_lo, c_hi;
  int pitch, plane;      // the storage plane's cells fit 31 bits (launch_stress checks)
  int xshift, n0;        // row length: nx, or ny when the rows run along y
  int nx, ny;
  int zs0, nplanes;      // storage planes [zs0, zs0 + nplanes) = local planes + 1
  int wall_only;
  double k;              // 1.0 - 0.5 / (double)tau
  StressOut o;
};

// include/lbm.h's expressions on one cell's pulls, and the stores of the requested outputs at
// raster index at.  Plain C++ doubles, left to right; the translation unit is compiled with
// -ffp-contract=off like the rest of the library.
__device__ __forceinline__ void stress_cell(const float* f, const StressArgs& a, int64_t at, bool report) {
  double d[kQ];
#pragma unroll
  for (int q = 0; q < kQ; ++q) d[q] = (double)f[q];
  double r = d[0];
#pragma unroll
  for (int q = 1; q < kQ; ++q) r = r + d[q];
  const double mx = d[1] - d[2] + d[7] + d[8] - d[9] - d[10] + d[11] + d[12] - d[13] - d[14];
  const double my = d[3] - d[4] + d[7] - d[8] + d[9] - d[10] + d[15] - d[16] + d[17] - d[18];
  const double mz = d[5] - d[6] + d[11] - d[12] + d[13] - d[14] + d[15] + d[16] - d[17] - d[18];
  const double pxx = d[1] + d[2] + d[7] + d[8] + d[9] + d[10] + d[11] + d[12] + d[13] + d[14];
  const double pyy = d[3] + d[4] + d[7] + d[8] + d[9] + d[10] + d[15] + d[16] + d[17] + d[18];
  const double pzz = d[5] + d[6] + d[11] + d[12] + d[13] + d[14] + d[15] + d[16] + d[17] + d[18];
  const double pxy = d[7] - d[8] - d[9] + d[10];
  const double pxz = d[11] - d[12] - d[13] + d[14];
  const double pyz = d[15] - d[16] - d[17] + d[18];
  const double c = r / 3.0;
  const double nk = -a.k;
  const double sxx = nk * ((pxx - c) - (mx * mx) / r);
  const double syy = nk * ((pyy - c) - (my * my) / r);
  const double szz = nk * ((pzz - c) - (mz * mz) / r);
  const double sxy = nk * (pxy - (mx * my) / r);
  const double sxz = nk * (pxz - (mx * mz) / r);
  const double syz = nk * (pyz - (my * mz) / r);
  if (a.o.s[0]) a.o.s[0][at] = (float)sxx;
  if (a.o.s[1]) a.o.s[1][at] = (float)syy;
  if (a.o.s[2]) a.o.s[2][at] = (float)szz;
  if (a.o.s[3]) a.o.s[3][at] = (float)sxy;
  if (a.o.s[4]) a.o.s[4][at] = (float)sxz;
  if (a.o.s[5]) a.o.s[5][at] = (float)syz;
  if (a.o.shear && report) {
    const double p = ((sxx + syy) + szz) / 3.0;
    const double dxx = sxx - p, dyy = syy - p, dzz = szz - p;
    const double j = 0.5 * ((dxx * dxx + dyy * dyy) + dzz * dzz) + ((sxy * sxy + sxz * sxz) + syz * syz);
    a.o.shear[at] = (float)__builtin_sqrt(j);
  }
}

// The cells a block (4 waves) reported, into the block's own slot: the host adds the slots.  No
// atomics -- one per wave on a single counter serialised across the XCDs and made the kernel 7x
// slower than its pulls (12 ns per wave, LDC 256^3).
__device__ __forceinline__ void stress_count(unsigned* counts, unsigned n) {
  __shared__ unsigned wave_n[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0)
    counts[blockIdx.y * gridDim.x + blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// raster index of the cell at position i = s0 + s1 * pitch of batch plane zp; -1 for a padding slot
template <bool SW>
__device__ __forceinline__ int64_t stress_raster(const StressArgs& a, unsigned i, int zp) {
  const unsigned s1 = i / (unsigned)a.pitch, s0 = i - s1 * (unsigned)a.pitch;
  if ((int)s0 >= a.n0) return -1;
  const int x = SW ? (int)s1 : (int)s0, y = SW ? (int)s0 : (int)s1;
  return ((int64_t)zp * a.ny + y) * a.nx + x;
}

// The dense box: thread (blockIdx.x, threadIdx.x) takes position i of every batch plane
// blockIdx.y, blockIdx.y + gridDim.y, ...; the cell of position i in storage plane zs is
// i - xshift + zs * plane (Layout).
template <bool SW>
__global__ void __launch_bounds__(256) k_stress(const StressArgs a) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned n = 0;
  if (i < (unsigned)a.plane) {
    for (int zp = blockIdx.y; zp < a.nplanes; zp += gridDim.y) {
      const int64_t c = (int64_t)i - a.xshift + (int64_t)(a.zs0 + zp) * a.plane;
      const uint8_t t = a.type[c];
      if ((t & kClassMask) != kFluid) continue;
      const int64_t at = stress_raster<SW>(a, i, zp);
      if (at < 0) continue;
      const bool report = !a.wall_only || (t & kWallAdj);
      float f[kQ];
      pull1_links<SW>(f, a.src, c, (a.bb_links && (t & kWallAdj)) ? a.bb_links[c] : 0u, a.pitch, (int64_t)a.plane,
                      AllQ{});
      stress_cell(f, a, at, report);
      n += report ? 1u : 0u;
    }
  }
  stress_count(a.o.counts, n);
}

// Compact rows: compact cell c pulls through its row record as k_moments_compact does; its
// dense cell cmap[c] gives the plane and the raster position.
template <bool SW>
__global__ void __launch_bounds__(256) k_stress_compact(const StressArgs a) {
  unsigned n = 0;
  for (int64_t c = a.c_lo + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < a.c_hi;
       c += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t t = a.type[c];
    const int d = a.cmap[c];
    if ((t & kClassMask) != kFluid || d < 0) continue;
    const unsigned u = (unsigned)(d + a.xshift);
    const int zp = (int)(u / (unsigned)a.plane) - a.zs0;
    if (zp < 0 || zp >= a.nplanes) continue;
    const int64_t at = stress_raster<SW>(a, u - (unsigned)(zp + a.zs0) * (unsigned)a.plane, zp);
    if (at < 0) continue;
    const bool report = !a.wall_only || (t & kWallAdj);
    float f[kQ];
    pull1_bb<SW>(f, a.src, Rows::load(a.rowrec, c, a.row_of[c >> 2]), compact_id(c),
                 (a.bb_links && (t & kWallAdj)) ? a.bb_links[c] : 0u, AllQ{});
    stress_cell(f, a, at, report);
    n += report ? 1u : 0u;
  }
  stress_count(a.o.counts, n);
}

// Launch grid: the dense box takes plane / 256 blocks along x and as many plane groups along y as
// give about kStressBlocks blocks (each thread then loops over its planes); compact rows a
// grid-stride loop of at most kStressBlocks blocks.
constexpr int kStressBlocks = 8192;
dim3 stress_grid(const StressView& v, int nplanes) {
  if (v.compact) return dim3((unsigned)std::min<int64_t>((v.c_hi - v.c_lo + 255) / 256, kStressBlocks));
  const int64_t gx = (v.L.plane + 255) / 256;
  return dim3((unsigned)gx, (unsigned)std::min<int64_t>(nplanes, std::max<int64_t>(1, kStressBlocks / gx)));
}

}  // namespace

int stress_blocks(const StressView& v, int nplanes) {
  const dim3 g = stress_grid(v, nplanes);
  return (int)(g.x * g.y);
}

hipError_t launch_stress(const StressView& v, int z0, int nplanes, int wall_only, const StressOut& o) {
  const Layout& L = v.L;
  if (nplanes <= 0) return hipSuccess;
  // 32-bit positions inside a plane; compact contexts also hold their dense cell ids in ints
  if (L.plane >= (int64_t(1) << 31) || z0 < 0 || z0 + nplanes > L.nz) return hipErrorInvalidValue;
  if (v.compact && L.ncell + 4 >= (int64_t(1) << 31)) return hipErrorInvalidValue;
  StressArgs a{};
  a.src = v.src; a.type = v.type; a.bb_links = v.bb_links;
  a.cmap = v.cmap; a.row_of = v.row_of; a.rowrec = v.rowrec;
  a.c_lo = v.c_lo; a.c_hi = v.c_hi;
  a.pitch = L.pitch; a.plane = (int)L.plane;
  a.xshift = L.xshift;
  a.n0 = L.swap ? L.ny : L.nx;
  a.nx = L.nx; a.ny = L.ny;
  a.zs0 = z0 + 1; a.nplanes = nplanes;
  a.wall_only = wall_only ? 1 : 0;
  a.k = 1.0 - 0.5 / (double)v.tau;
  a.o = o;
  const dim3 g = stress_grid(v, nplanes);
  if (v.compact) {
    if (v.c_hi <= v.c_lo) return hipSuccess;
    if (L.swap) hipLaunchKernelGGL(k_stress_compact<true>, g, dim3(256), 0, v.stream, a);
    else hipLaunchKernelGGL(k_stress_compact<false>, g, dim3(256), 0, v.stream, a);
  } else {
    if (L.swap) hipLaunchKernelGGL(k_stress<true>, g, dim3(256), 0, v.stream, a);
    else hipLaunchKernelGGL(k_stress<false>, g, dim3(256), 0, v.stream, a);
  }
  return hipGetLastError();
}

}  // namespace lbm

using namespace lbm;

namespace {

#define STRESS_HIP(ctx, expr)                \
  do {                                       \
    hipError_t e_ = (expr);                  \
    if (e_ != hipSuccess) {                  \
      stress_set_error(ctx, #expr, e_);      \
      return LBM_ERR_HIP;                    \
    }                                        \
  } while (0)

struct DevFree {
  void* p = nullptr;
  ~DevFree() { (void)hipFree(p); }
};

// outs[0..5]: the components, outs[6]: the shear (nullable); the plane range in batches whose
// requested outputs fit the scratch, each batch zeroed, filled by one launch and copied out
int stress_readout(lbm_ctx* c, int z0, int z1, int wall_only, float* const outs[7], int64_t* n_cells) {
  if (!c) return LBM_ERR_ARG;
  StressView v;
  const int rc = stress_view(c, &v);  // sets the device; state and communicator errors first
  if (rc != LBM_OK) return rc;
  const Layout& L = v.L;
  if (z0 < 0 || z1 > L.nz || z0 >= z1) {
    stress_set_error(c, "plane range outside 0 <= z0 < z1 <= nz", hipErrorInvalidValue);
    return LBM_ERR_ARG;
  }
  int nout = 0;
  for (int k = 0; k < 7; ++k) nout += outs[k] ? 1 : 0;
  const int64_t per_plane = (int64_t)L.nx * L.ny;
  const int64_t fit = nout ? kStressScratchBytes / ((int64_t)sizeof(float) * nout * per_plane) : z1 - z0;
  const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(z1 - z0, fit));
  DevFree scratch, counter;
  if (nout) STRESS_HIP(c, hipMalloc(&scratch.p, sizeof(float) * nout * per_plane * batch));
  const size_t nblocks = (size_t)std::max(1, stress_blocks(v, batch));  // the largest batch's grid
  std::vector<unsigned> counts(nblocks);
  STRESS_HIP(c, hipMalloc(&counter.p, sizeof(unsigned) * nblocks));
  int64_t reported = 0;
  for (int zb = z0; zb < z1; zb += batch) {
    const int np = std::min(batch, z1 - zb);
    const int64_t cells = per_plane * np;
    StressOut o{};
    float* dev[7] = {};
    int j = 0;
    for (int k = 0; k < 7; ++k)
      if (outs[k]) dev[k] = (float*)scratch.p + (int64_t)(j++) * per_plane * batch;
    for (int k = 0; k < 6; ++k) o.s[k] = dev[k];
    o.shear = dev[6];
    o.counts = (unsigned*)counter.p;
    if (nout) STRESS_HIP(c, hipMemsetAsync(scratch.p, 0, sizeof(float) * nout * per_plane * batch, v.stream));
    STRESS_HIP(c, hipMemsetAsync(counter.p, 0, sizeof(unsigned) * nblocks, v.stream));
    STRESS_HIP(c, launch_stress(v, zb, np, wall_only, o));
    STRESS_HIP(c, hipStreamSynchronize(v.stream));
    for (int k = 0; k < 7; ++k)
      if (outs[k])
        STRESS_HIP(c, hipMemcpy(outs[k] + per_plane * (zb - z0), dev[k], sizeof(float) * cells, hipMemcpyDeviceToHost));
    if (n_cells) {
      STRESS_HIP(c, hipMemcpy(counts.data(), counter.p, sizeof(unsigned) * nblocks, hipMemcpyDeviceToHost));
      for (unsigned n : counts) reported += n;
    }
  }
  if (n_cells) *n_cells = reported;
  return LBM_OK;
}

}  // namespace

extern "C" {

int lbm_get_stress(lbm_ctx* c, int z0, int z1, float* sxx, float* syy, float* szz, float* sxy, float* sxz,
                   float* syz) {
  float* const outs[7] = {sxx, syy, szz, sxy, sxz, syz, nullptr};
  return stress_readout(c, z0, z1, 0, outs, nullptr);
}

int lbm_get_shear(lbm_ctx* c, int z0, int z1, int wall_only, float* shear, int64_t* n_cells) {
  float* const outs[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, shear};
  return stress_readout(c, z0, z1, wall_only, outs, n_cells);
}

}  // extern "C"
