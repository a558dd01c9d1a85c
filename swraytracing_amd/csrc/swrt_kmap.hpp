// swrt_kmap.hpp — the wave-vector plane series (swrt_kmap_series_*): the
// density of the ensemble over the (k, l) plane and the first and second
// moments of the wavevector, as raytracing_figures.m:19-26,76-83,
// SW_zero_background_raytracing.m:103-104 and qgflow_animation.m:59-63 draw
// them packet by packet.
//
// A frame is one m x m plane of 64-bit counts over [-K, K) x [-K, K), cell
// (i, j) at plane[i + m*j] (first index k), and eight stats [n, rejected,
// outside, sum q(k), sum q(l), sum q(k*k), sum q(l*l), sum q(k*l)].  A record
// reads the packets' k and l only.  Each of the five values v is quantised
// once per packet, q = rint(v * 2^frac_bits) (round half even); a packet with
// a non-finite k or l, or any |v * 2^frac_bits| >= 2^38, is rejected and adds
// to nothing else.  A packet is inside iff -K <= k < K and -K <= l < K; its
// index is min((int)floor((k + K) * s), m - 1) with s = m / (2K) from the
// host (the product may round up to m for the last double below K).  A packet
// neither rejected nor inside counts as outside and still adds to the moments.
// With n <= 2^24 every sum stays below 2^62: integer addition is exact and
// order-free, so a frame depends on the packet set alone.  Sums of negative q
// wrap in two's complement: the frame is read back as int64.
//
// Contention, not bandwidth, sets the time: a frame reads 16 B per packet,
// the packets are stored in spatial order (neighbouring lanes hold unrelated
// wavevectors), and every driver run starts with the whole ensemble on one
// ring |k| = k0, about pi*m*k0/K cells.  Two kernels give the same integers:
//   kmap_lds_kernel (m <= kKmapLdsCells): a private int32 plane per workgroup
//     in LDS, LDS atomics per packet, one global 64-bit atomic per non-zero
//     cell at the end.
//   kmap_global_kernel (any m): one lane per packet, one global 64-bit atomic
//     per inside packet; with MERGE the lanes of a wave that share the first
//     pending lane's cell add through one lane first (hist_add_wave's form).
// Both sum the stats per lane, reduce them over the wave (shuffles) and the
// workgroup (LDS), and add one global atomic per non-zero stat.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace swrt {

constexpr int kKmapThreads = 256;
constexpr int kKmapWaves = kKmapThreads / 64;
constexpr int kKmapBlocks = 2048;         // at most, the global path: the grid strides over the packets
constexpr int kKmapStats = 8;             // n, rejected, outside, and the five moment sums
constexpr int kKmapSums = 7;              // stats a lane sums (n is the launch's)
constexpr int kKmapMaxCells = 4096;       // m
constexpr int kKmapMaxFracBits = 32;
constexpr int64_t kKmapMaxPackets = (int64_t)1 << 24;
constexpr int kKmapHistoryChunk = 256;    // history frames per launch (the grid's second dimension)
// The largest m of the LDS path.  128 x 128 int32 cells are 64 KB: two
// workgroups (eight waves) fit in a CU's 160 KB, enough to hide the 16 B per
// packet of loads behind the LDS atomics, and a workgroup's flush scans 64
// cells per lane.  One more doubling (m = 256, 256 KB) does not fit at all;
// sizes between would leave one workgroup per CU.  Measured at 1e6 packets:
// 0.023-0.030 ms a frame at m = 64 and 128 on the ring and on spread packets
// alike, against 0.16-0.46 ms through the global kernel.
constexpr int kKmapLdsCells = 128;
// Workgroups of the LDS path, at most: two per CU of 256.  Every workgroup
// zeroes and scans its whole plane, so more of them only add flush atomics.
constexpr int kKmapLdsBlocks = 512;
constexpr int kKmapMergeRounds = 4;       // as kHistAggRounds
// The global path's wave merge stays (profiles/kmap_series/README.md, 1e6
// packets): a driver's first frame, the ring in the order it was set, takes
// 0.038 ms with it and 0.40 ms without at m = 512; on packets in spatial order
// it is 0-8 % faster and never slower beyond the run-to-run spread.
constexpr bool kKmapGlobalMerge = true;

struct KmapGeom {
  double K;      // half-width of the plane
  double s;      // m / (2K), the host's division
  int m;
  double scale;  // 2^frac_bits
};

// What one packet adds: the cell (or -1) and the lane's stats sums
// [rejected, outside, q(k), q(l), q(k*k), q(l*l), q(k*l)].
__device__ __forceinline__ int kmap_packet(const KmapGeom& g, double k, double l, unsigned long long acc[kKmapSums]) {
  const double v[5] = {k, l, k * k, l * l, k * l};
  constexpr double lim = 0x1p38;
  bool ok = __builtin_isfinite(k) && __builtin_isfinite(l);
  double sv[5];
  for (int q = 0; q < 5; ++q) {
    sv[q] = v[q] * g.scale;
    ok = ok && fabs(sv[q]) < lim;  // (false for NaN)
  }
  if (!ok) {
    acc[0] += 1ull;
    return -1;
  }
  for (int q = 0; q < 5; ++q) acc[2 + q] += (unsigned long long)(long long)rint(sv[q]);
  if (!(k >= -g.K && k < g.K && l >= -g.K && l < g.K)) {
    acc[1] += 1ull;
    return -1;
  }
  // (inside: 0 <= (v + K) * s <= m, so the clamps only catch the rounding up to m;
  // the lower one costs nothing and keeps any index an address)
  const int i = max(0, min((int)floor((k + g.K) * g.s), g.m - 1));
  const int j = max(0, min((int)floor((l + g.K) * g.s), g.m - 1));
  return i + g.m * j;
}

// The lanes' sums over the wave, then the workgroup; lane t < kKmapSums adds
// stat 1 + t if it is non-zero, and the launch's first workgroup stores n.
// red: kKmapSums x kKmapWaves words of LDS nobody else uses any more.
__device__ __forceinline__ void kmap_stats_flush(unsigned long long acc[kKmapSums], unsigned long long* red,
                                                 int64_t n, unsigned long long* stats) {
  const int lane = (int)__lane_id(), wave = (int)threadIdx.x / 64;
  for (int q = 0; q < kKmapSums; ++q) {
    unsigned long long v = acc[q];
    for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, 64);
    if (lane == 0) red[q * kKmapWaves + wave] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < kKmapSums) {
    unsigned long long v = 0ull;
    for (int w = 0; w < kKmapWaves; ++w) v += red[threadIdx.x * kKmapWaves + w];
    if (v) atomicAdd(&stats[1 + threadIdx.x], v);
  }
  if (threadIdx.x == 0 && blockIdx.x == 0) stats[0] = (unsigned long long)n;
}

// Every lane of the wave calls this (cell < 0: nothing to add).
template <bool MERGE>
__device__ __forceinline__ void kmap_add_wave(unsigned long long* plane, int cell) {
  bool pending = cell >= 0;
  if constexpr (MERGE) {
    const int lane = (int)__lane_id();
    for (int r = 0; r < kKmapMergeRounds; ++r) {
      if (pending) {  // (the lanes inside are exactly the pending ones: readfirstlane and ballot see those)
        const int lead = __builtin_amdgcn_readfirstlane(cell);
        if (cell == lead) {
          const unsigned long long m = __ballot(1);
          if (lane == __ffsll((long long)m) - 1) atomicAdd(&plane[lead], (unsigned long long)__popcll(m));
          pending = false;
        }
      }
    }
  }
  if (pending) atomicAdd(&plane[cell], 1ull);
}

// Frame blockIdx.y of the launch: the packets' k (N x 2 column-major, any
// order; frame f's at k + f*stride) into the frame's plane and stats, zeroed
// on the stream before the launch.
template <bool MERGE>
__global__ void __launch_bounds__(kKmapThreads) kmap_global_kernel(const double* __restrict__ k, int64_t n,
                                                                   int64_t stride, KmapGeom g,
                                                                   unsigned long long* __restrict__ planes,
                                                                   unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long red[kKmapSums * kKmapWaves];
  k += (size_t)blockIdx.y * stride;
  planes += (size_t)blockIdx.y * g.m * g.m;
  stats += (size_t)blockIdx.y * kKmapStats;
  unsigned long long acc[kKmapSums] = {};
  // (the bound is the same for every lane of a wave: all of them reach kmap_add_wave)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = base + threadIdx.x;
    const int cell = p < n ? kmap_packet(g, k[p], k[n + p], acc) : -1;
    kmap_add_wave<MERGE>(planes, cell);
  }
  kmap_stats_flush(acc, red, n, stats);
}

// The same frame through a private plane of the workgroup in LDS (m <=
// kKmapLdsCells).  int32 cells: a workgroup sees fewer than 2^31 packets.
__global__ void __launch_bounds__(kKmapThreads) kmap_lds_kernel(const double* __restrict__ k, int64_t n,
                                                                int64_t stride, KmapGeom g,
                                                                unsigned long long* __restrict__ planes,
                                                                unsigned long long* __restrict__ stats) {
  __shared__ unsigned int cells[kKmapLdsCells * kKmapLdsCells];
  static_assert(sizeof(unsigned long long) * kKmapSums * kKmapWaves <= sizeof(cells), "the stats' scratch reuses the plane");
  const int mm = g.m * g.m;  // <= kKmapLdsCells^2 (the host chose this kernel)
  for (int e = threadIdx.x; e < mm; e += kKmapThreads) cells[e] = 0u;
  __syncthreads();
  k += (size_t)blockIdx.y * stride;
  planes += (size_t)blockIdx.y * mm;
  stats += (size_t)blockIdx.y * kKmapStats;
  unsigned long long acc[kKmapSums] = {};
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const int cell = kmap_packet(g, k[p], k[n + p], acc);
    if (cell >= 0) atomicAdd(&cells[cell], 1u);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < mm; e += kKmapThreads)
    if (const unsigned int cnt = cells[e]) atomicAdd(&planes[e], (unsigned long long)cnt);
  __syncthreads();  // (the plane is flushed: its first words hold the stats' partial sums now)
  kmap_stats_flush(acc, reinterpret_cast<unsigned long long*>(cells), n, stats);
}

}  // namespace swrt
