// swrt_diag.hpp — on-device diagnostics of the packet ensemble.
//
// analysis/load_data.m:33-52,63: omega = sqrt(f^2 + Cg^2*dot(k,k,2)) per
// packet and frame, histcounts over given edges (energy = centre * counts),
// and the mean omega per frame.  Runs on the device-resident packets, so a
// diagnostic frame costs one pass over k instead of a trajectory download.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swrt_kernels.hpp"

namespace swrt {

constexpr int kHistThreads = 256;
constexpr int kMaxHistBins = 4096;

// histcounts(w, edges): bin i holds edges[i] <= w < edges[i+1]; the last bin
// also holds w == edges[nb] (MATLAB / numpy semantics); others not counted.
__device__ __forceinline__ int hist_bin(double w, const double* edges, int nb) {
  if (!(w >= edges[0]) || !(w <= edges[nb])) return -1;
  if (w == edges[nb]) return nb - 1;
  int lo = 0, hi = nb;  // edges[lo] <= w < edges[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (w >= edges[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

// Per-block LDS histogram -> global 64-bit counts; per-block omega sums into
// `partial` (summed in block order by omega_sum_kernel: deterministic).
__global__ void __launch_bounds__(kHistThreads) omega_hist_kernel(const double* k, int64_t n, double f2,
                                                                  double Cg2, const double* edges, int nb,
                                                                  unsigned long long* counts,
                                                                  double* partial) {
  __shared__ unsigned int h[kMaxHistBins];
  __shared__ double red[kHistThreads];
  __shared__ double sedges[kMaxHistBins + 1];
  for (int b = threadIdx.x; b < nb; b += blockDim.x) h[b] = 0;
  for (int b = threadIdx.x; b <= nb; b += blockDim.x) sedges[b] = edges[b];
  __syncthreads();
  double s = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const double k1 = k[p], k2 = k[n + p];
    const double w = sqrt(f2 + Cg2 * (k1 * k1 + k2 * k2));  // load_data.m:33
    s += w;
    const int b = hist_bin(w, sedges, nb);
    if (b >= 0) atomicAdd(&h[b], 1u);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = blockDim.x / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
  for (int b = threadIdx.x; b < nb; b += blockDim.x)
    if (h[b]) atomicAdd(&counts[b], (unsigned long long)h[b]);
}

__global__ void omega_sum_kernel(const double* partial, int nblk, double* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nblk; ++i) s += partial[i];
    *out = s;
  }
}

// ---- the spectrum series (swrt_omega_series_*, swrt_omega_ideal) ----
//
// A frame is a row of nb + 2 counts [below, bin 0 .. bin nb-1, above] and four
// doubles [n, sum omega, min omega, max omega] (load_data.m:33-52,63).  A NaN
// omega is counted nowhere and ignored by min and max; it makes the sum NaN.
//
// A frame depends on the packets alone.  omega_scatter_kernel leaves every
// packet's omega at its ORIGINAL index (the set's perm); omega_frame_kernel
// then walks that index with a fixed grid — counts, min and max do not care
// about the order, and the sum is each lane's running sum over its stride,
// the workgroup's tree over the lanes, and omega_stats_kernel's fixed order
// over the workgroups' partials.  A history frame is in the original order
// already, so omega_frame_kernel<true> computes omega from its k in the same
// walk: the same bits as the current packets set to that frame.
//
// Contention: the drivers start every packet on one |k| ring
// (qgsw_raytrace.m:56-60), so for the first frames a whole wave adds to one or
// two LDS addresses, and a per-lane atomic serialises its 64 lanes there.
// hist_add_wave first lets the lanes that share the first pending lane's bin
// add their count through one lane, for kHistAggRounds rounds; the lanes
// still pending after them (a spread distribution) add for themselves.
// LDS holds the nb + 1 edges and the nb + 2 counts of the open series, not
// the 4096-bin maximum: 3.6 KB at 300 bins.

constexpr int kOmegaThreads = 256;
constexpr int kOmegaBlocks = 1024;       // at most: the grid strides over the packets
constexpr int kOmegaStats = 4;           // doubles per frame: n, sum, min, max
constexpr int kOmegaPartials = 3;        // per workgroup: sum, min, max
constexpr int kOmegaHistoryChunk = 256;  // history frames per launch (the grid's second dimension)
#ifndef SWRT_HIST_AGG_ROUNDS
#define SWRT_HIST_AGG_ROUNDS 4           // 0: per-lane atomics only (A/B builds)
#endif
constexpr int kHistAggRounds = SWRT_HIST_AGG_ROUNDS;

// Slot of w in a row [below, bins, above]; -1 for NaN.  The bin is hist_bin's.
__device__ __forceinline__ int hist_slot(double w, const double* edges, int nb) {
  if (w != w) return -1;
  if (w < edges[0]) return 0;
  if (w > edges[nb]) return nb + 1;
  return 1 + hist_bin(w, edges, nb);
}

// Every lane of the wave calls this (slot < 0: nothing to add).
__device__ __forceinline__ void hist_add_wave(unsigned int* h, int slot) {
  bool pending = slot >= 0;
  const int lane = (int)__lane_id();
  for (int r = 0; r < kHistAggRounds; ++r) {
    if (pending) {  // (the lanes inside are exactly the pending ones: readfirstlane and ballot see those)
      const int lead = __builtin_amdgcn_readfirstlane(slot);
      if (slot == lead) {
        const unsigned long long m = __ballot(1);
        if (lane == __ffsll((long long)m) - 1) atomicAdd(&h[lead], (unsigned int)__popcll(m));
        pending = false;
      }
    }
  }
  if (pending) atomicAdd(&h[slot], 1u);
}

// The workgroup's LDS counts added to a global row.
__device__ __forceinline__ void hist_flush(const unsigned int* h, int nslot, unsigned long long* row) {
  for (int b = threadIdx.x; b < nslot; b += blockDim.x)
    if (h[b]) atomicAdd(&row[b], (unsigned long long)h[b]);
}

// omega of the packets in storage order to w[original index]; workgroup 0
// zeroes the frame's count row for the launch that follows on the stream.
__global__ void __launch_bounds__(kOmegaThreads) omega_scatter_kernel(const double* __restrict__ k,
                                                                      const int* __restrict__ perm, int64_t n,
                                                                      double f2, double Cg2, double* __restrict__ w,
                                                                      unsigned long long* __restrict__ row,
                                                                      int nslot) {
  if (blockIdx.x == 0)
    for (int b = threadIdx.x; b < nslot; b += blockDim.x) row[b] = 0ull;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const double k1 = k[p], k2 = k[n + p];
  w[perm[p]] = sqrt(f2 + Cg2 * (k1 * k1 + k2 * k2));  // load_data.m:33
}

struct OmegaFrameArgs {
  const double* src;       // FROM_K: frame 0's k (N x 2 column-major, original order); else omega by original index
  int64_t src_stride;      // doubles from one frame's src to the next
  int64_t n;
  double f2, Cg2;
  const double* edges;     // nb + 1
  int nb;
  unsigned long long* counts;  // frame 0's row of nb + 2, zeroed before the launch; rows follow each other
  double* partial;         // per frame kOmegaPartials x gridDim.x
};

// Frame blockIdx.y: counts into its row, the workgroup's sum / min / max into
// its partials.  Dynamic LDS: (nb + 1) doubles, then (nb + 2) counts.
template <bool FROM_K>
__global__ void __launch_bounds__(kOmegaThreads) omega_frame_kernel(OmegaFrameArgs a) {
  extern __shared__ double omega_lds[];
  __shared__ double red[kOmegaPartials][kOmegaThreads];
  double* sedges = omega_lds;
  unsigned int* h = reinterpret_cast<unsigned int*>(omega_lds + a.nb + 1);
  const int nb = a.nb, nslot = a.nb + 2;
  for (int b = threadIdx.x; b < nslot; b += blockDim.x) h[b] = 0;
  for (int b = threadIdx.x; b <= nb; b += blockDim.x) sedges[b] = a.edges[b];
  __syncthreads();
  const double* src = a.src + (size_t)blockIdx.y * a.src_stride;
  double s = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
  // (the bound is the same for every lane of a wave: all of them reach hist_add_wave)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < a.n; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = base + threadIdx.x;
    int slot = -1;
    if (o < a.n) {
      double w;
      if constexpr (FROM_K) {
        const double k1 = src[o], k2 = src[a.n + o];
        w = sqrt(a.f2 + a.Cg2 * (k1 * k1 + k2 * k2));  // load_data.m:33
      } else {
        w = src[o];
      }
      s += w;
      if (w < mn) mn = w;  // (false for NaN)
      if (w > mx) mx = w;
      slot = hist_slot(w, sedges, nb);
    }
    hist_add_wave(h, slot);
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = mn;
  red[2][threadIdx.x] = mx;
  __syncthreads();
  for (int off = kOmegaThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] = fmin(red[1][threadIdx.x], red[1][threadIdx.x + off]);
      red[2][threadIdx.x] = fmax(red[2][threadIdx.x], red[2][threadIdx.x + off]);
    }
    __syncthreads();
  }
  double* part = a.partial + (size_t)blockIdx.y * kOmegaPartials * gridDim.x;
  if (threadIdx.x < kOmegaPartials) part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = red[threadIdx.x][0];
  hist_flush(h, nslot, a.counts + (size_t)blockIdx.y * nslot);
}

// Frame blockIdx.x: the workgroups' partials into its stats, in an order fixed
// by their number alone: lane t takes partials t, t + 256, ... in turn, then
// the tree over the lanes.  (One lane walking all 1024 partials waits for a
// global load per entry; this form takes a few microseconds.)
__global__ void __launch_bounds__(kOmegaThreads) omega_stats_kernel(const double* __restrict__ partial, int nblk,
                                                                    int64_t n, double* __restrict__ stats) {
  __shared__ double red[kOmegaPartials][kOmegaThreads];
  const double* col = partial + (size_t)blockIdx.x * kOmegaPartials * nblk;
  double s = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
  for (int i = threadIdx.x; i < nblk; i += kOmegaThreads) {
    s += col[i];
    mn = fmin(mn, col[nblk + i]);
    mx = fmax(mx, col[2 * nblk + i]);
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = mn;
  red[2][threadIdx.x] = mx;
  __syncthreads();
  for (int off = kOmegaThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] = fmin(red[1][threadIdx.x], red[1][threadIdx.x + off]);
      red[2][threadIdx.x] = fmax(red[2][threadIdx.x], red[2][threadIdx.x + off]);
    }
    __syncthreads();
  }
  double* out = stats + (size_t)blockIdx.x * kOmegaStats;
  if (threadIdx.x == 0) out[0] = (double)n;
  if (threadIdx.x < kOmegaPartials) out[1 + threadIdx.x] = red[threadIdx.x][0];
}

// ideal_omega_distribution.m:3-11: Omega = omega0 + (u_g*kx_j + v_g*ky_j) for
// every node g of the slot's nx x nx grid and every ring vector j, binned into
// a row [below, bins, above] (zeroed before the launch).  Sample s is node
// s / m, ring vector s % m.  Dynamic LDS as omega_frame_kernel.
__global__ void __launch_bounds__(kOmegaThreads) omega_ideal_kernel(const double* __restrict__ nodes, int nx,
                                                                    int npad, const double* __restrict__ ring,
                                                                    int64_t m, double omega0,
                                                                    const double* __restrict__ edges, int nb,
                                                                    unsigned long long* __restrict__ row) {
  extern __shared__ double omega_lds[];
  double* sedges = omega_lds;
  unsigned int* h = reinterpret_cast<unsigned int*>(omega_lds + nb + 1);
  const int nslot = nb + 2;
  for (int b = threadIdx.x; b < nslot; b += blockDim.x) h[b] = 0;
  for (int b = threadIdx.x; b <= nb; b += blockDim.x) sedges[b] = edges[b];
  __syncthreads();
  const int64_t total = (int64_t)nx * nx * m;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = base + threadIdx.x;
    int slot = -1;
    if (s < total) {
      const int64_t g = s / m, j = s - g * m;
      const int ig = (int)(g % nx), jg = (int)(g / nx);
      const double* rec = nodes + ((int64_t)(ig + kPadLo) * npad + (jg + kPadLo)) * kRec;
      const double Om = omega0 + (rec[0] * ring[j] + rec[1] * ring[m + j]);  // ideal_omega_distribution.m:6,10
      slot = hist_slot(Om, sedges, nb);
    }
    hist_add_wave(h, slot);
  }
  __syncthreads();
  hist_flush(h, nslot, row);
}

}  // namespace swrt
