// swrt_trans.hpp — the transition series (swrt_trans_series_*): the
// energy-vs-omega distribution of the packets (analysis/load_data.m:33-52)
// split by a source value the device keeps per packet, by ORIGINAL index:
// the packet's omega at an earlier mark (the propagator of the distribution
// along the omega axis), or any value the caller gives (the ring a packet
// started on: parameters.txt's near_inertial_factor sweep in one run).
//
// Per packet in storage order, o = perm[p] (a history frame is in the
// original order already: perm NULL, o = p):
//   omega = sqrt(f^2 + Cg^2 (k k + l l)) in omega_frame_kernel's operation order;
//   s     = src[o];  d = omega - s;  d2 = d * d.
// A packet is rejected, and adds to nothing else, if omega, s or d is NaN or
// any of |omega|, |d|, |d2| times 2^frac_bits is not below 2^38 (kmap_packet's
// test).  Otherwise sc = hist_slot(s, src_edges, ns), wc = hist_slot(omega,
// omega_edges, nw) (swrt_diag.hpp: [below, bins, above], last bin closed) and
// a frame is
//   counts  (ns + 2) x (nw + 2) 64-bit counts, cell sc * (nw + 2) + wc;
//   sums    (ns + 2) x 3 64-bit sums per source class of rint(omega * scale),
//           rint(d * scale), rint(d2 * scale) (two's complement);
//   stats   [n, rejected, mark serial].
// With n <= 2^24 every sum stays below 2^62: integer addition is exact and
// order-free, so a frame depends on the packet set and the source values
// alone.
//
// The source lives at the original index because the storage order does not
// last: a re-binning between the mark and the record permutes x, k and perm
// together, and would have to carry every per-packet extra along.  Kept by
// original index the source is written once, never moved, and read through the
// 4 B of perm the set keeps anyway (an 8 B gather per packet).
//
// One lane per packet on a fixed grid striding over the packets, every wave
// with one trip count so that all its lanes reach the wave-level merges.  Two
// forms give the same integers, as cond_kernel's:
//   trans_kernel<true> (at most kCondLdsCells cells): a private uint32 count
//     plane of the workgroup in LDS (hist_add_wave), flushed as its non-zero
//     cells (hist_flush);
//   trans_kernel<false> (any shape): one global 64-bit atomic per packet with
//     the same merge first (kmap_add_wave).
// The per-class sums: on the drivers' initial ring a whole wave shares one
// source class, and three 64-bit atomics per lane on one address would
// serialise its 64 lanes three times.  trans_sums_wave merges first: for
// kTransMergeRounds rounds the lanes that share the first pending lane's class
// sum their three values over the wave (a masked butterfly) and lanes 0..2 add
// one total each; lanes still pending after the rounds (many classes in one wave:
// little contention) add for themselves.  The sums are in LDS up to
// kTransLdsClasses rows (24 KB) and go straight to the frame beyond.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swrt_cond.hpp"
#include "swrt_diag.hpp"
#include "swrt_kmap.hpp"

namespace swrt {

constexpr int kTransThreads = 256;
constexpr int kTransSums = 3;                  // per source class: omega, d, d2
constexpr int kTransStats = 3;                 // n, rejected, mark serial
constexpr int kTransMaxBins = kCondMaxBins;    // nw, ns
constexpr int kTransMaxCells = kCondMaxCells;  // (ns + 2) * (nw + 2): 512 KB a frame
constexpr int kTransMaxFracBits = 32;
constexpr int64_t kTransMaxPackets = (int64_t)1 << 24;
constexpr int kTransHistoryChunk = 256;        // history frames per launch (the grid's second dimension)
constexpr int kTransLdsClasses = 1024;         // rows of sums kept in LDS, at most
constexpr int kTransMergeRounds = 4;
// Workgroups, at most: no gather to hide, so the spectrum series' grid; a
// plane above 32 KB leaves room for two workgroups a CU.
constexpr int kTransBlocks = 1024;
constexpr int kTransBigPlaneBlocks = 512;
constexpr size_t kTransBigPlaneBytes = (size_t)32 << 10;

struct TransArgs {
  const double* k;        // frame 0's N x 2 column-major k in storage order; frame i's at k + i*stride
  const int* perm;        // storage slot -> original index (NULL: identity)
  const double* src;      // the source value by original index
  int64_t stride;
  int64_t n;
  double f2, Cg2;
  const double* wedges;   // nw + 1
  const double* sedges;   // ns + 1
  int nw, ns;
  double scale;           // 2^frac_bits
  unsigned long long serial;
  unsigned long long* counts;  // frame 0's (ns + 2) x (nw + 2), zeroed before the launch; frames follow each other
  unsigned long long* tail;    // frame 0's 3 (ns + 2) sums and kTransStats stats, zeroed likewise
};

__host__ __device__ inline bool trans_sums_in_lds(int ns) { return ns + 2 <= kTransLdsClasses; }

// Dynamic LDS of trans_kernel: the two edge arrays, the per-class sums (if
// kept there), one word pair for the rejected count, then (LDS form) the plane.
inline size_t trans_lds_bytes(int nw, int ns, bool lds_plane) {
  const size_t words8 = (size_t)(nw + 1) + (ns + 1) + (trans_sums_in_lds(ns) ? (size_t)kTransSums * (ns + 2) : 0) + 1;
  return 8 * words8 + (lds_plane ? sizeof(unsigned int) * (size_t)(ns + 2) * (nw + 2) : 0);
}

__device__ __forceinline__ double trans_omega(double f2, double Cg2, double k1, double k2) {
  return sqrt(f2 + Cg2 * (k1 * k1 + k2 * k2));  // load_data.m:33
}

// src[original index] = omega of the packet.
__global__ void __launch_bounds__(kTransThreads) trans_mark_kernel(const double* __restrict__ k,
                                                                   const int* __restrict__ perm, int64_t n, double f2,
                                                                   double Cg2, double* __restrict__ src) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  src[perm[p]] = trans_omega(f2, Cg2, k[p], k[n + p]);
}

// What one packet adds: its cell (or -1: rejected), its source class and its
// three quantised values.
__device__ __forceinline__ int trans_packet(const TransArgs& a, const double* wedges, const double* sedges, double s,
                                            double k1, double k2, int& sc, unsigned long long q[kTransSums]) {
  const double w = trans_omega(a.f2, a.Cg2, k1, k2);
  const double d = w - s;
  const double d2 = d * d;
  const double sw = w * a.scale, sd = d * a.scale, sd2 = d2 * a.scale;
  constexpr double lim = 0x1p38;
  // (a NaN omega, s or d fails one of the first two tests; s = +-inf makes d infinite)
  if (!(fabs(sw) < lim) || !(fabs(sd) < lim) || !(fabs(sd2) < lim) || s != s) return -1;
  sc = hist_slot(s, sedges, a.ns);
  q[0] = (unsigned long long)(long long)rint(sw);
  q[1] = (unsigned long long)(long long)rint(sd);
  q[2] = (unsigned long long)(long long)rint(sd2);
  return sc * (a.nw + 2) + hist_slot(w, wedges, a.nw);
}

// Every lane of the wave calls this (sc < 0: nothing to add): q[j] added to
// sums[3 * sc + j], the lanes that share a class adding through one lane.
__device__ __forceinline__ void trans_sums_wave(unsigned long long* sums, int sc,
                                                const unsigned long long q[kTransSums]) {
  const int lane = (int)__lane_id();
  bool pending = sc >= 0;
  for (int r = 0; r < kTransMergeRounds; ++r) {
    const unsigned long long pm = __ballot(pending);
    if (!pm) break;  // (wave-uniform: every lane takes the butterfly below or none does)
    const int lead = __shfl(sc, __ffsll((long long)pm) - 1, 64);
    const bool mine = pending && sc == lead;
    unsigned long long v[kTransSums];
    for (int j = 0; j < kTransSums; ++j) {
      v[j] = mine ? q[j] : 0ull;
      for (int off = 32; off > 0; off >>= 1) v[j] += (unsigned long long)__shfl_xor((long long)v[j], off, 64);
    }
    if (lane < kTransSums) {  // (lanes 0..2 hold every total: one atomic each)
      const unsigned long long t = lane == 0 ? v[0] : lane == 1 ? v[1] : v[2];
      if (t) atomicAdd(&sums[kTransSums * lead + lane], t);
    }
    if (mine) pending = false;
  }
  if (pending)
    for (int j = 0; j < kTransSums; ++j)
      if (q[j]) atomicAdd(&sums[kTransSums * sc + j], q[j]);
}

// Frame blockIdx.y of the launch.
template <bool LDS>
__global__ void __launch_bounds__(kTransThreads) trans_kernel(TransArgs a) {
  extern __shared__ double trans_lds[];
  const int nss = a.ns + 2, ncell = nss * (a.nw + 2);
  const bool lsums = trans_sums_in_lds(a.ns);
  double* wedges = trans_lds;
  double* sedges = wedges + a.nw + 1;
  unsigned long long* sums_l = reinterpret_cast<unsigned long long*>(sedges + a.ns + 1);
  unsigned int* rejected = reinterpret_cast<unsigned int*>(sums_l + (lsums ? kTransSums * nss : 0));
  unsigned int* cells = rejected + 2;
  for (int e = threadIdx.x; e <= a.nw; e += kTransThreads) wedges[e] = a.wedges[e];
  for (int e = threadIdx.x; e <= a.ns; e += kTransThreads) sedges[e] = a.sedges[e];
  if (lsums)
    for (int e = threadIdx.x; e < kTransSums * nss; e += kTransThreads) sums_l[e] = 0ull;
  if (threadIdx.x == 0) *rejected = 0u;
  if constexpr (LDS)
    for (int e = threadIdx.x; e < ncell; e += kTransThreads) cells[e] = 0u;
  __syncthreads();
  const double* k = a.k + (size_t)blockIdx.y * a.stride;
  unsigned long long* counts = a.counts + (size_t)blockIdx.y * ncell;
  unsigned long long* tail = a.tail + (size_t)blockIdx.y * (kTransSums * nss + kTransStats);
  unsigned long long* sums = lsums ? sums_l : tail;
  unsigned int rej = 0u;
  // (the bound is the same for every lane of a wave: all of them reach the merges)
  for (int64_t base = (int64_t)blockIdx.x * kTransThreads; base < a.n; base += (int64_t)gridDim.x * kTransThreads) {
    const int64_t p = base + threadIdx.x;
    int cell = -1, sc = -1;
    unsigned long long q[kTransSums] = {0ull, 0ull, 0ull};
    if (p < a.n) {
      const int64_t o = a.perm ? (int64_t)a.perm[p] : p;
      cell = trans_packet(a, wedges, sedges, a.src[o], k[p], k[a.n + p], sc, q);
      if (cell < 0) {
        sc = -1;
        ++rej;
      }
    }
    trans_sums_wave(sums, sc, q);
    if constexpr (LDS)
      hist_add_wave(cells, cell);
    else
      kmap_add_wave<true>(counts, cell);
  }
  for (int off = 32; off > 0; off >>= 1) rej += (unsigned int)__shfl_xor((int)rej, off, 64);
  if (__lane_id() == 0 && rej) atomicAdd(rejected, rej);
  __syncthreads();
  if constexpr (LDS) hist_flush(cells, ncell, counts);
  if (lsums)
    for (int e = threadIdx.x; e < kTransSums * nss; e += kTransThreads)
      if (const unsigned long long s = sums_l[e]) atomicAdd(&tail[e], s);
  if (threadIdx.x == 0) {
    if (*rejected) atomicAdd(&tail[kTransSums * nss + 1], (unsigned long long)*rejected);
    if (blockIdx.x == 0) {
      tail[kTransSums * nss] = (unsigned long long)a.n;
      tail[kTransSums * nss + 2] = a.serial;
    }
  }
}

}  // namespace swrt
