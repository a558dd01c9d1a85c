// swrt_map.hpp — packet density and wave-energy maps (swrt_map_series_*): where
// the ensemble's wave energy sits, as generate_image.m:9-34 and
// raytracing_figures.m:6-24 draw it packet by packet.
//
// A frame is four m x m planes of 64-bit integers [count, sum q(omega),
// sum q(k1), sum q(k2)] over the periodic square of side L, cell (i, j) at
// plane[i + m*j] (first index x, column-major, as a pv.bin frame), and two
// stats [n, rejected].  The cell is interpolate.m:21-31's with dxm = L/m
// (cell_frac); omega = sqrt(f^2 + Cg^2*(k1*k1 + k2*k2)) in load_data.m:33's
// operation order; each moment v is quantised once per packet,
// q = rint(v * 2^frac_bits) (round half even).  A packet with a non-finite
// x, y, k1, k2 or omega, or any |v * 2^frac_bits| >= 2^38, adds to no cell and
// counts as rejected.  With n <= 2^24 every sum stays below 2^62: integer
// addition is exact and order-free, so a frame depends on the packet set
// alone — not on the storage order, the binning, the launch shape or a shard
// split.  Sums of negative q wrap in two's complement: the planes are read
// back as int64.
//
// Two kernels give the same integers:
//   map_general_kernel: one lane per packet (grid stride), four global 64-bit
//     atomics; any packet order, also the history frames.
//   map_tile_kernel: one workgroup per tile of the leapfrog's binning (the
//     same starts / order / clamping as tile_leapfrog_kernel).  Almost every
//     packet of a tile falls into the tile's own map cells or a ring of
//     ceil(M/c) cells around them (c field cells per map cell): those add with
//     LDS 64-bit atomics and the non-zero cells are flushed with one global
//     atomic each; a packet that drifted further since the re-binning (a
//     stray) adds through global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swrt_kernels.hpp"
#include "swrt_share.hpp"
#include "swrt_tile.hpp"

namespace swrt {

constexpr int kMapThreads = 256;
constexpr int kMapBlocks = 2048;          // at most: the general grid strides over the packets
constexpr int kMapPlanes = 4;             // count, sum q(omega), sum q(k1), sum q(k2)
constexpr int kMapStats = 2;              // n, rejected
constexpr int kMapMaxCells = 4096;        // m
constexpr int kMapMaxFracBits = 32;
constexpr int64_t kMapMaxPackets = (int64_t)1 << 24;
constexpr int kMapHistoryChunk = 256;     // history frames per launch (the grid's second dimension)

struct MapGeom {
  double dxm, inv_dxm;  // L/m and RN(1/dxm)
  double pm, inv_pm;    // m as a double and RN(1/m)
  int m;
  double f2, Cg2;
  double scale;         // 2^frac_bits
};

// The three quantised moments of a packet; false: the packet is rejected.
// (A NaN fails every comparison; scale >= 1, so a product below 2^38 has a
// finite factor.)
__device__ __forceinline__ bool map_moments(const MapGeom& g, double x, double y, double k1, double k2,
                                            unsigned long long q[3]) {
  const double w = sqrt(g.f2 + g.Cg2 * (k1 * k1 + k2 * k2));  // load_data.m:33
  const double sw = w * g.scale, sk = k1 * g.scale, sl = k2 * g.scale;
  constexpr double lim = 0x1p38;
  if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && fabs(sw) < lim && fabs(sk) < lim && fabs(sl) < lim))
    return false;
  q[0] = (unsigned long long)(long long)rint(sw);
  q[1] = (unsigned long long)(long long)rint(sk);
  q[2] = (unsigned long long)(long long)rint(sl);
  return true;
}

__device__ __forceinline__ void map_cell(const MapGeom& g, double x, double y, int& i, int& j) {
  double a;
  i = cell_frac(x, g.dxm, g.inv_dxm, g.pm, g.inv_pm, g.m, g.m, a);
  j = cell_frac(y, g.dxm, g.inv_dxm, g.pm, g.inv_pm, g.m, g.m, a);
}

__device__ __forceinline__ void map_add_global(unsigned long long* planes, size_t mm, size_t cell,
                                               const unsigned long long q[3]) {
  atomicAdd(&planes[cell], 1ull);
  atomicAdd(&planes[mm + cell], q[0]);
  atomicAdd(&planes[2 * mm + cell], q[1]);
  atomicAdd(&planes[3 * mm + cell], q[2]);
}

// Frame blockIdx.y of the launch: packets x, k (N x 2 column-major, any
// order; frame f's at x + f*stride) into the frame's planes and stats, zeroed
// on the stream before the launch.
__global__ void __launch_bounds__(kMapThreads) map_general_kernel(const double* __restrict__ x,
                                                                  const double* __restrict__ k, int64_t n,
                                                                  int64_t stride, MapGeom g,
                                                                  unsigned long long* __restrict__ planes,
                                                                  unsigned long long* __restrict__ stats) {
  __shared__ unsigned int nrej;
  if (threadIdx.x == 0) nrej = 0;
  __syncthreads();
  const size_t mm = (size_t)g.m * g.m;
  x += (size_t)blockIdx.y * stride;
  k += (size_t)blockIdx.y * stride;
  planes += (size_t)blockIdx.y * kMapPlanes * mm;
  stats += (size_t)blockIdx.y * kMapStats;
  unsigned int rej = 0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const double px = x[p], py = x[n + p];
    unsigned long long q[3];
    if (!map_moments(g, px, py, k[p], k[n + p], q)) {
      ++rej;
      continue;
    }
    int i, j;
    map_cell(g, px, py, i, j);
    map_add_global(planes, mm, (size_t)i + (size_t)g.m * j, q);
  }
  if (rej) atomicAdd(&nrej, rej);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (nrej) atomicAdd(&stats[1], (unsigned long long)nrej);
    if (blockIdx.x == 0) stats[0] = (unsigned long long)n;
  }
}

struct MapTileArgs {
  const double* x;     // the packets in the binning's order
  const double* k;
  int64_t n;
  const int* starts;   // ntiles + 1 packet offsets of the tiles
  const int* order;    // band slot -> tile (bin_scan_kernel)
  int ntx;             // tiles per side
  int c;               // field cells per map cell side (divides the tile side)
  MapGeom g;
  unsigned long long* planes;  // the frame's, zeroed before the launch
  unsigned long long* stats;
  unsigned long long* strays;  // the context's stray counter (SWRT_DEBUG_MAP_STRAYS)
};

// a mod m for a in (-2m, 2m)
__device__ __forceinline__ int map_wrap(int a, int m) {
  a %= m;
  return a < 0 ? a + m : a;
}

// T: field cells per tile side, M: the leapfrog's drift margin (field cells).
template <int T, int M>
__global__ void __launch_bounds__(kMapThreads) map_tile_kernel(MapTileArgs a) {
  constexpr int WMAX = T + 2 * M;  // window side at c = 1
  __shared__ unsigned long long acc[kMapPlanes * WMAX * WMAX];
  __shared__ unsigned int nrej, nstray;
  const int tid = threadIdx.x;
  const int m = a.g.m;
  const size_t mm = (size_t)m * m;
  const int own = T / a.c, R = (M + a.c - 1) / a.c;
  const int W = own + 2 * R, WW = W * W;  // W <= WMAX
  for (int e = tid; e < kMapPlanes * WW; e += kMapThreads) acc[e] = 0ull;
  if (tid == 0) nrej = 0, nstray = 0;
  int pbeg, pend;
  TileShare sh;
  sh.ntiles = a.ntx * a.ntx;
  const int tile = wg_work_range(a.starts, a.order, a.n, sh, pbeg, pend);
  const int bx = (tile / a.ntx) * own - R, by = (tile % a.ntx) * own - R;  // the window's first map cell
  __syncthreads();
  unsigned int rej = 0, stray = 0;
  for (int p = pbeg + tid; p < pend; p += kMapThreads) {
    const double px = a.x[p], py = a.x[a.n + p];
    unsigned long long q[3];
    if (!map_moments(a.g, px, py, a.k[p], a.k[a.n + p], q)) {
      ++rej;
      continue;
    }
    int i, j;
    map_cell(a.g, px, py, i, j);
    const int di = map_wrap(i - bx, m), dj = map_wrap(j - by, m);
    if (di < W && dj < W) {
      const int e = di + W * dj;
      atomicAdd(&acc[e], 1ull);
      atomicAdd(&acc[WW + e], q[0]);
      atomicAdd(&acc[2 * WW + e], q[1]);
      atomicAdd(&acc[3 * WW + e], q[2]);
    } else {
      ++stray;
      map_add_global(a.planes, mm, (size_t)i + (size_t)m * j, q);
    }
  }
  if (rej) atomicAdd(&nrej, rej);
  if (stray) atomicAdd(&nstray, stray);
  __syncthreads();
  for (int e = tid; e < WW; e += kMapThreads) {
    const unsigned long long cnt = acc[e];
    if (!cnt) continue;  // (no packet: the three sums are zero as well)
    const int gi = map_wrap(bx + e % W, m), gj = map_wrap(by + e / W, m);
    const size_t cell = (size_t)gi + (size_t)m * gj;
    atomicAdd(&a.planes[cell], cnt);
    // (a sum may be zero with packets in the cell: adding it changes nothing)
    atomicAdd(&a.planes[mm + cell], acc[WW + e]);
    atomicAdd(&a.planes[2 * mm + cell], acc[2 * WW + e]);
    atomicAdd(&a.planes[3 * mm + cell], acc[3 * WW + e]);
  }
  if (tid == 0) {
    if (nrej) atomicAdd(&a.stats[1], (unsigned long long)nrej);
    if (nstray) atomicAdd(a.strays, (unsigned long long)nstray);
    if (blockIdx.x == 0) a.stats[0] = (unsigned long long)a.n;
  }
}

}  // namespace swrt
