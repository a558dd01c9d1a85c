// swrt_cond.hpp — the conditional spectrum series (swrt_cond_series_*): the
// energy-vs-omega distribution of the packets (analysis/load_data.m:33-52)
// split by a scalar of the flow at each packet, the vorticity, the strain or
// Okubo-Weiss of RaytracingScheme.m:18-31.
//
// Per packet: omega = sqrt(f^2 + Cg^2 (k k + l l)) in omega_frame_kernel's
// operation order, and q = zeta, sigma or D (which = 0, 1, 2) through
// eval_flow and ray_point_flow (swrt_raydiag.hpp), i.e. the bits
// swrt_raydiag_sample returns.  Both are classed by hist_slot (swrt_diag.hpp:
// [below, bins, above], last bin closed, NaN -1), omega over nw bins and q
// over nq.  A frame is
//   counts  (nq + 2) x (nw + 2) 64-bit counts, cell qc * (nw + 2) + wc;
//   sums    nq + 2 64-bit sums of rint(omega * 2^frac_bits) per q class;
//   stats   [n, rejected].
// A packet whose omega or q is NaN, or with |omega * 2^frac_bits| >= 2^38
// (kmap_packet's test), is rejected and adds to nothing else.  With n <= 2^24
// every sum stays below 2^62: integer addition is exact and order-free, so a
// frame depends on the packet set alone and the kernel reads x and k in the
// storage order, coalesced, without the set's perm.
//
// One lane per packet on a fixed grid striding over the packets, every wave
// with one trip count so that all its lanes reach the wave-level merge.  The
// gather is ray_diag_kernel's (nslots a run-time branch: its comment).  Two
// forms give the same integers:
//   cond_kernel<true> (at most kCondLdsCells cells): a private uint32 count
//     plane of the workgroup in LDS, the lanes of a wave that share a cell
//     adding through one lane (hist_add_wave), then one global 64-bit atomic
//     per non-zero cell (hist_flush);
//   cond_kernel<false> (any shape): one global 64-bit atomic per packet with
//     the same merge first (kmap_add_wave).
// Both keep the edges, the per-class sums (64-bit LDS atomics) and the
// workgroup's rejected count in LDS and flush the non-zero ones.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swrt_diag.hpp"
#include "swrt_kmap.hpp"
#include "swrt_raydiag.hpp"

namespace swrt {

constexpr int kCondThreads = 256;
constexpr int kCondStats = 2;                 // n, rejected
constexpr int kCondMaxBins = 4096;            // nw, nq
constexpr int kCondMaxCells = 65536;          // (nq + 2) * (nw + 2): 512 KB a frame
constexpr int kCondMaxFracBits = 32;
constexpr int64_t kCondMaxPackets = (int64_t)1 << 24;
constexpr int kCondHistoryChunk = 256;        // history frames per launch (the grid's second dimension)
// The largest plane of the LDS path: 64 KB of uint32, two workgroups in a
// CU's 160 KB beside the edges (kKmapLdsCells' reasoning).
constexpr int kCondLdsCells = 16384;
// Workgroups, at most.  The gather wants every wave a CU can hold (four
// workgroups at ray_diag_kernel's 126 registers); a plane above 32 KB leaves
// room for two.
constexpr int kCondBlocks = 1024;
constexpr int kCondBigPlaneBlocks = 512;
constexpr size_t kCondBigPlaneBytes = (size_t)32 << 10;

struct CondArgs {
  FieldView f0, f1;
  int nslots;
  double alpha, bump;
  const double* alphas;   // one alpha per frame of the launch (device; NULL: `alpha`)
  const double* x;        // frame 0's N x 2 column-major positions, any order; frame i's at x + i*stride
  const double* k;
  int64_t stride;
  int64_t n;
  double f2, Cg2;
  const double* wedges;   // nw + 1
  const double* qedges;   // nq + 1
  int nw, nq;
  int which;              // 0 zeta, 1 sigma, 2 D
  double scale;           // 2^frac_bits
  unsigned long long* counts;  // frame 0's (nq + 2) x (nw + 2), zeroed before the launch; frames follow each other
  unsigned long long* tail;    // frame 0's nq + 2 sums and kCondStats stats, zeroed likewise
};

// Dynamic LDS of cond_kernel: the two edge arrays, the per-class sums, one
// word pair for the rejected count, then (LDS form) the count plane.
inline size_t cond_lds_bytes(int nw, int nq, bool lds_plane) {
  const size_t words8 = (size_t)(nw + 1) + (nq + 1) + (nq + 2) + 1;
  return 8 * words8 + (lds_plane ? sizeof(unsigned int) * (size_t)(nq + 2) * (nw + 2) : 0);
}

// What one packet adds: its cell (or -1: rejected), its q class and q(omega).
__device__ __forceinline__ int cond_packet(const CondArgs& a, const double* wedges, const double* qedges, double alpha,
                                           double x, double y, double k1, double k2, int& qc,
                                           unsigned long long& qw) {
  double I[kRec];
  eval_flow(a.f0, a.f1, a.nslots, alpha, x, y, a.bump, I);
  RayPoint pt;
  ray_point_flow(I, pt);
  const double q = a.which == 0 ? pt.zeta : a.which == 1 ? pt.sigma : pt.D;
  const double w = sqrt(a.f2 + a.Cg2 * (k1 * k1 + k2 * k2));  // load_data.m:33
  const double sw = w * a.scale;
  constexpr double lim = 0x1p38;
  if (!(fabs(sw) < lim) || q != q) return -1;  // (a NaN omega fails the first test)
  qc = hist_slot(q, qedges, a.nq);
  qw = (unsigned long long)(long long)rint(sw);
  return qc * (a.nw + 2) + hist_slot(w, wedges, a.nw);
}

// Frame blockIdx.y of the launch.
template <bool LDS>
__global__ void __launch_bounds__(kCondThreads) cond_kernel(CondArgs a) {
  extern __shared__ double cond_lds[];
  double* wedges = cond_lds;
  double* qedges = wedges + a.nw + 1;
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(qedges + a.nq + 1);
  unsigned int* rejected = reinterpret_cast<unsigned int*>(sums + a.nq + 2);
  unsigned int* cells = rejected + 2;
  const int nqs = a.nq + 2, ncell = nqs * (a.nw + 2);
  for (int e = threadIdx.x; e <= a.nw; e += kCondThreads) wedges[e] = a.wedges[e];
  for (int e = threadIdx.x; e <= a.nq; e += kCondThreads) qedges[e] = a.qedges[e];
  for (int e = threadIdx.x; e < nqs; e += kCondThreads) sums[e] = 0ull;
  if (threadIdx.x == 0) *rejected = 0u;
  if constexpr (LDS)
    for (int e = threadIdx.x; e < ncell; e += kCondThreads) cells[e] = 0u;
  __syncthreads();
  const double* x = a.x + (size_t)blockIdx.y * a.stride;
  const double* k = a.k + (size_t)blockIdx.y * a.stride;
  const double alpha = a.alphas ? a.alphas[blockIdx.y] : a.alpha;
  unsigned long long* counts = a.counts + (size_t)blockIdx.y * ncell;
  unsigned long long* tail = a.tail + (size_t)blockIdx.y * (nqs + kCondStats);
  unsigned int rej = 0u;
  // (the bound is the same for every lane of a wave: all of them reach the merge)
  for (int64_t base = (int64_t)blockIdx.x * kCondThreads; base < a.n; base += (int64_t)gridDim.x * kCondThreads) {
    const int64_t p = base + threadIdx.x;
    int cell = -1;
    if (p < a.n) {
      int qc = 0;
      unsigned long long qw = 0ull;
      cell = cond_packet(a, wedges, qedges, alpha, x[p], x[a.n + p], k[p], k[a.n + p], qc, qw);
      if (cell >= 0)
        atomicAdd(&sums[qc], qw);
      else
        ++rej;
    }
    if constexpr (LDS)
      hist_add_wave(cells, cell);
    else
      kmap_add_wave<true>(counts, cell);
  }
  for (int off = 32; off > 0; off >>= 1) rej += (unsigned int)__shfl_xor((int)rej, off, 64);
  if (__lane_id() == 0 && rej) atomicAdd(rejected, rej);
  __syncthreads();
  if constexpr (LDS) hist_flush(cells, ncell, counts);
  for (int e = threadIdx.x; e < nqs; e += kCondThreads)
    if (const unsigned long long s = sums[e]) atomicAdd(&tail[e], s);
  if (threadIdx.x == 0) {
    if (*rejected) atomicAdd(&tail[nqs + 1], (unsigned long long)*rejected);
    if (blockIdx.x == 0) tail[nqs] = (unsigned long long)a.n;
  }
}

}  // namespace swrt
