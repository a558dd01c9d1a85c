// swrt_absfreq.hpp — the absolute-frequency series (swrt_absfreq_series_*):
// the distribution of the ray Hamiltonian Omega = omega(k) + U.k over the
// packets beside that of omega, and the rate dOmega/dt = k . dU/dt that only
// an unsteady flow gives it (symplectic_full_fourier.m:41,54-57,
// SW_zero_background_raytracing.m:57,85-87).  The packets move in a flow that
// is linear in time between two snapshots (interpolate_U.m:19-23), so for the
// ODE they solve dU/dt = (U2 - U1)/tau exactly, and gather6<true> returns both
// snapshots' values before any blend: the rate costs a subtraction and a
// division per component behind a gather every blended frame pays anyway.
//
// Per packet, every operation rounded on its own (no contraction), with
// A = slot a's and B = slot b's (u, v) from flow_pair (gather6 on slot a's
// stencil, the sums swrt_eval(nslots = 1) gives on either slot):
//   two snapshots:  oma = 1 - alpha
//                   u  = oma*A[0] + alpha*B[0]    eval_flow's bits
//                   v  = oma*A[1] + alpha*B[1]
//                   ut = (B[0] - A[0]) / tau
//                   vt = (B[1] - A[1]) / tau
//   one snapshot:   u = A[0], v = A[1]; Od below is the literal 0.0
//   kk = k1*k1 + k2*k2
//   w  = sqrt(f2 + Cg2*kk)                        the spectrum series' omega (load_data.m:33)
//   D  = u*k1 + v*k2                              ray_point_omega's dot(U, k)
//   Om = w + D                                    swrt_raydiag_sample's Omega when gH == Cg*Cg
//   Od = ut*k1 + vt*k2                            dOmega/dt along the ray
// wc = hist_slot(w, omega_edges, nw), oc = hist_slot(Om, abs_edges, no)
// (swrt_diag.hpp: [below, bins, above], last bin closed).  With S = 2^frac_bits
// a packet is rejected, and adds to stats[1] alone, if Om or Od is NaN or any
// of |w*S|, |Om*S|, |D*S|, |Od*S|, (Od*Od)*S is not below 2^38.  A frame is
//   counts  (no + 2) x (nw + 2) 64-bit counts, cell oc * (nw + 2) + wc;
//   sums    3 (nw + 2) + 2 (no + 2) 64-bit sums (signed, two's complement):
//           rint(Od*S), rint((Od*Od)*S) and rint(D*S) per omega class, then
//           rint(Od*S) and rint((Od*Od)*S) per Omega class;
//   stats   [n, rejected].
// With n <= 2^24 every sum stays below 2^62: integer addition is exact and
// order-free, so a frame depends on the packet set and the two snapshots
// alone and the kernel reads x and k in the storage order, coalesced, without
// the set's perm.
//
// The kernel is refr_kernel's with another per-packet reduction: one lane per
// packet on a fixed grid striding over the packets, every wave with one trip
// count so that all its lanes reach the wave-level merge.  Two forms give the
// same integers:
//   absfreq_kernel<true>: a private uint32 count plane of the workgroup in LDS
//     (hist_add_wave), flushed as its non-zero cells (hist_flush);
//   absfreq_kernel<false> (any shape): one global 64-bit atomic per packet
//     with the same merge first (kmap_add_wave).
// Both keep the edges, the sums (64-bit LDS atomics, five per packet) and the
// workgroup's rejected count in LDS and flush the non-zero ones.
//
// Registers.  Only u and v of the two records are used, so the inlined gather
// keeps two accumulators per snapshot and loads one double2 per node and
// snapshot: the four other fields' sums and loads are dead and dropped.
//
// LDS budget.  The tail (edges, sums, rejected) takes 8 (4 nw + 3 no + 13)
// bytes: 128.4 KB at the largest shape the series admits (nw = 4096, no = 13),
// which one workgroup may still declare of a CU's 160 KB.  The LDS form is
// taken while the plane has at most kCondLdsCells cells (64 KB of uint32) AND
// tail and plane together stay within kAbsfreqLdsFormBytes = 80 KB, so that
// two workgroups fit into a CU (the refraction series' rule).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swrt_cond.hpp"
#include "swrt_diag.hpp"
#include "swrt_kmap.hpp"
#include "swrt_raydiag.hpp"

namespace swrt {

constexpr int kAbsfreqThreads = 256;
constexpr int kAbsfreqStats = 2;                  // n, rejected
constexpr int kAbsfreqWSums = 3;                  // per omega class: Od, Od^2, D
constexpr int kAbsfreqOSums = 2;                  // per Omega class: Od, Od^2
constexpr int kAbsfreqMaxBins = kCondMaxBins;     // nw, no
constexpr int kAbsfreqMaxCells = kCondMaxCells;   // (no + 2) * (nw + 2): 512 KB a frame
constexpr int kAbsfreqMaxFracBits = 32;
constexpr int64_t kAbsfreqMaxPackets = (int64_t)1 << 24;
constexpr int kAbsfreqHistoryChunk = 256;         // history frames per launch (the grid's second dimension)
constexpr size_t kAbsfreqLdsFormBytes = (size_t)80 << 10;  // the LDS form's tail and plane, at most (header comment)
constexpr int kAbsfreqMaxLdsBytes = 132 << 10;    // what the kernels may ask for: the largest tail, 131488 B
// Workgroups, at most (kRefrBlocks' reasoning): four a CU while the gather's
// registers set the limit, two above 32 KB of LDS, one above 80 KB.
constexpr int kAbsfreqBlocks = 1024;
constexpr int kAbsfreqBigPlaneBlocks = 512;
constexpr int kAbsfreqHugeTailBlocks = 256;
constexpr size_t kAbsfreqBigPlaneBytes = (size_t)32 << 10;

struct AbsfreqArgs {
  FieldView fa, fb;       // the flow at alpha = 0 and at alpha = 1 (fb = fa with one snapshot)
  int two;                // two snapshots
  double alpha, tau, bump;
  const double* alphas;   // one alpha per frame of the launch (device; NULL: `alpha`)
  const double* x;        // frame 0's N x 2 column-major positions, any order; frame i's at x + i*stride
  const double* k;
  int64_t stride;
  int64_t n;
  double f2, Cg2;
  const double* wedges;   // nw + 1
  const double* oedges;   // no + 1
  int nw, no;
  double scale;           // 2^frac_bits
  unsigned long long* counts;  // frame 0's (no + 2) x (nw + 2), zeroed before the launch; frames follow each other
  unsigned long long* tail;    // frame 0's 3 (nw + 2) + 2 (no + 2) sums and kAbsfreqStats stats, zeroed likewise
};

__host__ __device__ inline int absfreq_nsums(int nw, int no) {
  return kAbsfreqWSums * (nw + 2) + kAbsfreqOSums * (no + 2);
}

// Dynamic LDS of absfreq_kernel: the two edge arrays, the sums, one word pair
// for the rejected count, 8 (4 nw + 3 no + 13) bytes, then (LDS form) the
// count plane.
inline size_t absfreq_lds_bytes(int nw, int no, bool lds_plane) {
  const size_t words8 = (size_t)(nw + 1) + (no + 1) + absfreq_nsums(nw, no) + 1;
  return 8 * words8 + (lds_plane ? sizeof(unsigned int) * (size_t)(no + 2) * (nw + 2) : 0);
}

// The LDS form's shapes (header comment).
inline bool absfreq_lds_form(int nw, int no) {
  return (size_t)(no + 2) * (nw + 2) <= (size_t)kCondLdsCells &&
         absfreq_lds_bytes(nw, no, true) <= kAbsfreqLdsFormBytes;
}

// What one packet adds: its cell (or -1: rejected), its two classes and its
// three quantised values (Od, Od^2, D).
template <bool TWO>
__device__ __forceinline__ int absfreq_packet(const AbsfreqArgs& a, const double* wedges, const double* oedges,
                                              double alpha, double x, double y, double k1, double k2, int& wc,
                                              int& oc, unsigned long long q[kAbsfreqWSums]) {
  double A[kRec], B[kRec];
  flow_pair<TWO>(a.fa, a.fb, x, y, a.bump, A, B);
  double u = A[0], v = A[1], Od = 0.0;
  if constexpr (TWO) {
    const double oma = 1 - alpha;
    u = oma * A[0] + alpha * B[0];  // interpolate_U.m:19-23
    v = oma * A[1] + alpha * B[1];
    const double ut = (B[0] - A[0]) / a.tau;
    const double vt = (B[1] - A[1]) / a.tau;
    Od = ut * k1 + vt * k2;
  }
  const double kk = k1 * k1 + k2 * k2;
  const double w = sqrt(a.f2 + a.Cg2 * kk);  // load_data.m:33
  const double D = u * k1 + v * k2;
  const double Om = w + D;
  const double sw = w * a.scale, so = Om * a.scale, sD = D * a.scale, sd = Od * a.scale, sd2 = (Od * Od) * a.scale;
  constexpr double lim = 0x1p38;
  if (Om != Om || Od != Od || !(fabs(sw) < lim) || !(fabs(so) < lim) || !(fabs(sD) < lim) || !(fabs(sd) < lim) ||
      !(sd2 < lim))
    return -1;
  wc = hist_slot(w, wedges, a.nw);
  oc = hist_slot(Om, oedges, a.no);
  q[0] = (unsigned long long)(long long)rint(sd);
  q[1] = (unsigned long long)(long long)rint(sd2);
  q[2] = (unsigned long long)(long long)rint(sD);
  return oc * (a.nw + 2) + wc;
}

// Frame blockIdx.y of the launch.
template <bool LDS>
__global__ void __launch_bounds__(kAbsfreqThreads) absfreq_kernel(AbsfreqArgs a) {
  extern __shared__ double absfreq_lds[];
  const int nws = a.nw + 2, nos = a.no + 2, ncell = nos * nws, nsum = kAbsfreqWSums * nws + kAbsfreqOSums * nos;
  double* wedges = absfreq_lds;
  double* oedges = wedges + a.nw + 1;
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(oedges + a.no + 1);
  unsigned int* rejected = reinterpret_cast<unsigned int*>(sums + nsum);
  unsigned int* cells = rejected + 2;
  for (int e = threadIdx.x; e <= a.nw; e += kAbsfreqThreads) wedges[e] = a.wedges[e];
  for (int e = threadIdx.x; e <= a.no; e += kAbsfreqThreads) oedges[e] = a.oedges[e];
  for (int e = threadIdx.x; e < nsum; e += kAbsfreqThreads) sums[e] = 0ull;
  if (threadIdx.x == 0) *rejected = 0u;
  if constexpr (LDS)
    for (int e = threadIdx.x; e < ncell; e += kAbsfreqThreads) cells[e] = 0u;
  __syncthreads();
  const double* x = a.x + (size_t)blockIdx.y * a.stride;
  const double* k = a.k + (size_t)blockIdx.y * a.stride;
  const double alpha = a.alphas ? a.alphas[blockIdx.y] : a.alpha;
  unsigned long long* counts = a.counts + (size_t)blockIdx.y * ncell;
  unsigned long long* tail = a.tail + (size_t)blockIdx.y * (nsum + kAbsfreqStats);
  unsigned int rej = 0u;
  // (the bound is the same for every lane of a wave: all of them reach the merge)
  for (int64_t base = (int64_t)blockIdx.x * kAbsfreqThreads; base < a.n;
       base += (int64_t)gridDim.x * kAbsfreqThreads) {
    const int64_t p = base + threadIdx.x;
    int cell = -1;
    if (p < a.n) {
      int wc = 0, oc = 0;
      unsigned long long q[kAbsfreqWSums] = {0ull, 0ull, 0ull};
      // (the snapshot count is a run-time branch, uniform over the launch: ray_diag_kernel's comment)
      cell = a.two ? absfreq_packet<true>(a, wedges, oedges, alpha, x[p], x[a.n + p], k[p], k[a.n + p], wc, oc, q)
                   : absfreq_packet<false>(a, wedges, oedges, alpha, x[p], x[a.n + p], k[p], k[a.n + p], wc, oc, q);
      if (cell >= 0) {
        atomicAdd(&sums[wc], q[0]);
        atomicAdd(&sums[nws + wc], q[1]);
        atomicAdd(&sums[2 * nws + wc], q[2]);
        atomicAdd(&sums[kAbsfreqWSums * nws + oc], q[0]);
        atomicAdd(&sums[kAbsfreqWSums * nws + nos + oc], q[1]);
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
  for (int e = threadIdx.x; e < nsum; e += kAbsfreqThreads)
    if (const unsigned long long s = sums[e]) atomicAdd(&tail[e], s);
  if (threadIdx.x == 0) {
    if (*rejected) atomicAdd(&tail[nsum + 1], (unsigned long long)*rejected);
    if (blockIdx.x == 0) tail[nsum] = (unsigned long long)a.n;
  }
}

}  // namespace swrt
