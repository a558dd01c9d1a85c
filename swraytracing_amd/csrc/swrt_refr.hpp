// swrt_refr.hpp — the refraction series (swrt_refr_series_*): how fast the
// flow's gradients move each packet along the omega axis right now, and how
// its wavevector lies in the local strain.  The kick computes the rate
// kdot = -(grad U)^T k every step (RaytracingScheme.m:9-16) and drops it; here
// it is formed once more at a frame and reduced per class.
//
// Per packet, every operation rounded on its own (no contraction), with
// I = (u, v, u_x, u_y, v_x, v_y) from eval_flow, i.e. the bits swrt_eval and
// swrt_raydiag_sample give:
//   kk  = k1*k1 + k2*k2
//   w   = sqrt(f2 + Cg2*kk)                    the spectrum series' omega (load_data.m:33)
//   kd  = -(I[2]*k1 + I[4]*k2)                 RaytracingScheme.m:14
//   ld  = -(I[3]*k1 + I[5]*k2)                 RaytracingScheme.m:15
//   g   = k1*kd + k2*ld
//   wd  = (Cg2*g)/w                            omega-dot
//   gam = g/kk                                 d ln|k| / dt
//   s1  = I[2]-I[5], s2 = I[4]+I[3], sig = sqrt(s1*s1 + s2*s2)   ray_point_flow's sigma
//   c   = (gam+gam)/sig                        alignment: -cos 2 theta in a non-divergent flow
// wc = hist_slot(w, omega_edges, nw), ac = hist_slot(c, a_edges, na)
// (swrt_diag.hpp: [below, bins, above], last bin closed).  With S = 2^frac_bits
// a packet is rejected, and adds to stats[1] alone, if c is NaN or any of
// |w*S|, |wd*S|, (wd*wd)*S, |gam*S| is not below 2^38.  A frame is
//   counts  (na + 2) x (nw + 2) 64-bit counts, cell ac * (nw + 2) + wc;
//   sums    3 (nw + 2) + (na + 2) 64-bit sums (signed, two's complement):
//           rint(wd*S), rint((wd*wd)*S) and rint(gam*S) per omega class, then
//           rint(wd*S) per alignment class;
//   stats   [n, rejected].
// With n <= 2^24 every sum stays below 2^62: integer addition is exact and
// order-free, so a frame depends on the packet set alone and the kernel reads
// x and k in the storage order, coalesced, without the set's perm.
//
// The kernel is cond_kernel's with another per-packet reduction: one lane per
// packet on a fixed grid striding over the packets, every wave with one trip
// count so that all its lanes reach the wave-level merge; the gather is
// ray_diag_kernel's (nslots a run-time branch: its comment).  Two forms give
// the same integers:
//   refr_kernel<true>: a private uint32 count plane of the workgroup in LDS
//     (hist_add_wave), flushed as its non-zero cells (hist_flush);
//   refr_kernel<false> (any shape): one global 64-bit atomic per packet with
//     the same merge first (kmap_add_wave).
// Both keep the edges, the sums (64-bit LDS atomics, four per packet) and the
// workgroup's rejected count in LDS and flush the non-zero ones.
//
// LDS budget.  The tail (edges, sums, rejected) takes 8 (4 nw + 2 na + 11)
// bytes: 6 KB at 126 x 126, 128.3 KB at the largest shape the series admits
// (nw = 4096, na = 13), which one workgroup may still declare of a CU's
// 160 KB.  The LDS form is taken while the plane has at most kCondLdsCells
// cells (64 KB of uint32) AND tail and plane together stay within
// kRefrLdsFormBytes = 80 KB, so that two workgroups fit into a CU: a plane of
// few alignment rows over thousands of omega classes has a tail that alone
// breaks that, and goes the global way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swrt_cond.hpp"
#include "swrt_diag.hpp"
#include "swrt_kmap.hpp"
#include "swrt_raydiag.hpp"

namespace swrt {

constexpr int kRefrThreads = 256;
constexpr int kRefrStats = 2;                  // n, rejected
constexpr int kRefrWSums = 3;                  // per omega class: wd, wd^2, gam
constexpr int kRefrMaxBins = kCondMaxBins;     // nw, na
constexpr int kRefrMaxCells = kCondMaxCells;   // (na + 2) * (nw + 2): 512 KB a frame
constexpr int kRefrMaxFracBits = 32;
constexpr int64_t kRefrMaxPackets = (int64_t)1 << 24;
constexpr int kRefrHistoryChunk = 256;         // history frames per launch (the grid's second dimension)
constexpr size_t kRefrLdsFormBytes = (size_t)80 << 10;  // the LDS form's tail and plane, at most (header comment)
constexpr int kRefrMaxLdsBytes = 132 << 10;    // what the kernels may ask for: the largest tail, 131368 B
// Workgroups, at most (kCondBlocks' reasoning): four a CU while the gather's
// registers set the limit, two above 32 KB of LDS, one above 80 KB.
constexpr int kRefrBlocks = 1024;
constexpr int kRefrBigPlaneBlocks = 512;
constexpr int kRefrHugeTailBlocks = 256;
constexpr size_t kRefrBigPlaneBytes = (size_t)32 << 10;

struct RefrArgs {
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
  const double* aedges;   // na + 1
  int nw, na;
  double scale;           // 2^frac_bits
  unsigned long long* counts;  // frame 0's (na + 2) x (nw + 2), zeroed before the launch; frames follow each other
  unsigned long long* tail;    // frame 0's 3 (nw + 2) + (na + 2) sums and kRefrStats stats, zeroed likewise
};

__host__ __device__ inline int refr_nsums(int nw, int na) { return kRefrWSums * (nw + 2) + (na + 2); }

// Dynamic LDS of refr_kernel: the two edge arrays, the sums, one word pair for
// the rejected count, then (LDS form) the count plane.
inline size_t refr_lds_bytes(int nw, int na, bool lds_plane) {
  const size_t words8 = (size_t)(nw + 1) + (na + 1) + refr_nsums(nw, na) + 1;
  return 8 * words8 + (lds_plane ? sizeof(unsigned int) * (size_t)(na + 2) * (nw + 2) : 0);
}

// The LDS form's shapes (header comment).
inline bool refr_lds_form(int nw, int na) {
  return (size_t)(na + 2) * (nw + 2) <= (size_t)kCondLdsCells && refr_lds_bytes(nw, na, true) <= kRefrLdsFormBytes;
}

// What one packet adds: its cell (or -1: rejected), its two classes and its
// three quantised values.
__device__ __forceinline__ int refr_packet(const RefrArgs& a, const double* wedges, const double* aedges, double alpha,
                                           double x, double y, double k1, double k2, int& wc, int& ac,
                                           unsigned long long q[kRefrWSums]) {
  double I[kRec];
  eval_flow(a.f0, a.f1, a.nslots, alpha, x, y, a.bump, I);
  const double kk = k1 * k1 + k2 * k2;
  const double w = sqrt(a.f2 + a.Cg2 * kk);  // load_data.m:33
  const double kd = -(I[2] * k1 + I[4] * k2);  // RaytracingScheme.m:14
  const double ld = -(I[3] * k1 + I[5] * k2);  // RaytracingScheme.m:15
  const double g = k1 * kd + k2 * ld;
  const double wd = (a.Cg2 * g) / w;
  const double gam = g / kk;
  const double s1 = I[2] - I[5], s2 = I[4] + I[3];
  const double sig = sqrt(s1 * s1 + s2 * s2);  // RaytracingScheme.m:25
  const double c = (gam + gam) / sig;
  const double sw = w * a.scale, sd = wd * a.scale, sd2 = (wd * wd) * a.scale, sg = gam * a.scale;
  constexpr double lim = 0x1p38;
  if (!(fabs(sw) < lim) || c != c || !(fabs(sd) < lim) || !(sd2 < lim) || !(fabs(sg) < lim)) return -1;
  wc = hist_slot(w, wedges, a.nw);
  ac = hist_slot(c, aedges, a.na);
  q[0] = (unsigned long long)(long long)rint(sd);
  q[1] = (unsigned long long)(long long)rint(sd2);
  q[2] = (unsigned long long)(long long)rint(sg);
  return ac * (a.nw + 2) + wc;
}

// Frame blockIdx.y of the launch.
template <bool LDS>
__global__ void __launch_bounds__(kRefrThreads) refr_kernel(RefrArgs a) {
  extern __shared__ double refr_lds[];
  const int nws = a.nw + 2, nas = a.na + 2, ncell = nas * nws, nsum = kRefrWSums * nws + nas;
  double* wedges = refr_lds;
  double* aedges = wedges + a.nw + 1;
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(aedges + a.na + 1);
  unsigned int* rejected = reinterpret_cast<unsigned int*>(sums + nsum);
  unsigned int* cells = rejected + 2;
  for (int e = threadIdx.x; e <= a.nw; e += kRefrThreads) wedges[e] = a.wedges[e];
  for (int e = threadIdx.x; e <= a.na; e += kRefrThreads) aedges[e] = a.aedges[e];
  for (int e = threadIdx.x; e < nsum; e += kRefrThreads) sums[e] = 0ull;
  if (threadIdx.x == 0) *rejected = 0u;
  if constexpr (LDS)
    for (int e = threadIdx.x; e < ncell; e += kRefrThreads) cells[e] = 0u;
  __syncthreads();
  const double* x = a.x + (size_t)blockIdx.y * a.stride;
  const double* k = a.k + (size_t)blockIdx.y * a.stride;
  const double alpha = a.alphas ? a.alphas[blockIdx.y] : a.alpha;
  unsigned long long* counts = a.counts + (size_t)blockIdx.y * ncell;
  unsigned long long* tail = a.tail + (size_t)blockIdx.y * (nsum + kRefrStats);
  unsigned int rej = 0u;
  // (the bound is the same for every lane of a wave: all of them reach the merge)
  for (int64_t base = (int64_t)blockIdx.x * kRefrThreads; base < a.n; base += (int64_t)gridDim.x * kRefrThreads) {
    const int64_t p = base + threadIdx.x;
    int cell = -1;
    if (p < a.n) {
      int wc = 0, ac = 0;
      unsigned long long q[kRefrWSums] = {0ull, 0ull, 0ull};
      cell = refr_packet(a, wedges, aedges, alpha, x[p], x[a.n + p], k[p], k[a.n + p], wc, ac, q);
      if (cell >= 0) {
        atomicAdd(&sums[wc], q[0]);
        atomicAdd(&sums[nws + wc], q[1]);
        atomicAdd(&sums[2 * nws + wc], q[2]);
        atomicAdd(&sums[kRefrWSums * nws + ac], q[0]);
      } else {
        ++rej;
      }
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
  for (int e = threadIdx.x; e < nsum; e += kRefrThreads)
    if (const unsigned long long s = sums[e]) atomicAdd(&tail[e], s);
  if (threadIdx.x == 0) {
    if (*rejected) atomicAdd(&tail[nsum + 1], (unsigned long long)*rejected);
    if (blockIdx.x == 0) tail[nsum] = (unsigned long long)a.n;
  }
}

}  // namespace swrt
