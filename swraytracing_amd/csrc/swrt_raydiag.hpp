// swrt_raydiag.hpp — the run's invariant and the flow along the rays, sampled
// on the device-resident packets.
//
// In a steady flow the absolute frequency Omega = omega(k) + U(x).k is constant
// along a ray: symplectic_full_fourier.m:41 keeps Omega_0 and :54-57 plot
// (Omega_abs - Omega_0)./Omega_0 against time (SW_zero_background_raytracing.m:
// 57,85-87 the same).  RaytracingScheme.m:18-31 gives the flow a packet sees:
// vorticity (:20), strain (:25) and Okubo-Weiss (:30, in the form of that line:
// v_y.^2 + v_x.*u_y).
//
// ray_diag_kernel: one lane per packet in the storage (binned) order, so
// neighbouring lanes read neighbouring nodes; U and grad U through eval_flow,
// i.e. the bits swrt_eval gives at the same point (periodic wrap, layered
// y-period, two-snapshot blend).  Omega_0 and everything a packet leaves are
// indexed by the original packet index (the set's perm).
//
// sqrt() here is the compiler's IEEE sequence with its input scaling and its
// zero / infinity select: the strain of a flow at rest is sqrt(0) = 0 and f may
// be 0, both outside sqrt_rn_normal's range.
//
// A frame is eight doubles [n, max|r|, sum r, sum r^2, sum omega, sum zeta,
// sum sigma, sum D] with r = (Omega - Omega_0)/Omega_0 (0 without a mark):
// sums, not means, so the frames of shards combine by adding (max for entry 1).
// The sums run over the packets' records in the ORIGINAL order
// (ray_diag_reduce_kernel: a fixed grid striding over the index, per-workgroup
// partials, ray_diag_frame_kernel combining them in block order).  The storage
// order is the binning's, and within a bin it is whatever order the scatter's
// atomics gave: a sum over it would differ in the last bits from one run, one
// context or one re-binning to the next.  This one depends on the packets alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swrt_kernels.hpp"

namespace swrt {

constexpr int kRayDiagThreads = 256;
constexpr int kRayDiagBlocks = 1024;  // at most: the reduction's grid strides over the packets
constexpr int kRayDiagStats = 7;      // max|r|, then the six sums
constexpr int kRayDiagFrame = 8;      // doubles per frame
constexpr int kRayDiagRec = 6;        // doubles a packet leaves for the reduction: r, omega, zeta, sigma, D, Omega

struct RayDiagArgs {
  FieldView f0, f1;
  int nslots;
  double alpha, bump;
  const double* x;   // N x 2 column-major, storage order
  const double* k;
  const int* perm;   // storage slot -> original packet index (NULL: the identity, a history frame)
  int64_t n;
  double f2, gH;     // f2 = f*f
  double* omega0;    // by original index.  MARK: written; else read (NULL: no mark, r = 0)
  double* sample4;   // N x 4 column-major [Omega zeta sigma D] by original index (NULL: none)
  double* rec;       // N records of kRayDiagRec doubles by original index (not MARK)
};

// What one packet at (x, y, k, l) leaves: omega(k), Omega and the flow's three
// scalars, in the operation order of the header comment.  ray_diag_kernel's
// record and the track series' frame (swrt_track.hpp) are both this function,
// hence the same bits.
struct RayPoint {
  double w, Om, zeta, sigma, D;
};

__device__ __forceinline__ void ray_point_omega(const double I[kRec], double k1, double k2, double f2, double gH,
                                                RayPoint& r) {
  const double w = sqrt(f2 + gH * (k1 * k1 + k2 * k2));
  const double Om = w + (I[0] * k1 + I[1] * k2);
  r.w = w;
  r.Om = Om;
}

__device__ __forceinline__ void ray_point_flow(const double I[kRec], RayPoint& r) {
  const double zeta = I[4] - I[3];               // RaytracingScheme.m:20
  const double s1 = I[2] - I[5], s2 = I[4] + I[3];
  const double sigma = sqrt(s1 * s1 + s2 * s2);  // RaytracingScheme.m:25
  const double D = I[5] * I[5] + I[4] * I[3];    // RaytracingScheme.m:30
  r.zeta = zeta;
  r.sigma = sigma;
  r.D = D;
}

// MARK: Omega_0 of every packet (symplectic_full_fourier.m:41) and nothing else.
// nslots is a run-time branch as in eval_kernel: with the two-snapshot gather
// alone in straight-line code the compiler issues every tap's loads at once,
// takes all 256 registers and spills; this form needs 126 and no scratch.
template <bool MARK>
__global__ void __launch_bounds__(kRayDiagThreads) ray_diag_kernel(RayDiagArgs a) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const double k1 = a.k[p], k2 = a.k[a.n + p];
  double I[kRec];  // u, v, u_x, u_y, v_x, v_y
  eval_flow(a.f0, a.f1, a.nslots, a.alpha, a.x[p], a.x[a.n + p], a.bump, I);
  RayPoint pt;
  ray_point_omega(I, k1, k2, a.f2, a.gH, pt);
  const double w = pt.w, Om = pt.Om;
  const int64_t o = a.perm ? a.perm[p] : p;
  if constexpr (MARK) {
    a.omega0[o] = Om;
  } else {
    ray_point_flow(I, pt);
    const double zeta = pt.zeta, sigma = pt.sigma, D = pt.D;
    double r = 0.0;
    if (a.omega0 != nullptr) {
      const double Om0 = a.omega0[o];
      r = (Om - Om0) / Om0;                        // symplectic_full_fourier.m:56
    }
    if (a.sample4 != nullptr) {
      a.sample4[o] = Om;
      a.sample4[a.n + o] = zeta;
      a.sample4[2 * a.n + o] = sigma;
      a.sample4[3 * a.n + o] = D;
    }
    double2* q = reinterpret_cast<double2*>(a.rec + (size_t)o * kRayDiagRec);
    q[0] = make_double2(r, w);
    q[1] = make_double2(zeta, sigma);
    q[2] = make_double2(D, Om);
  }
}

// The records in the original order -> per-workgroup partials, statistic-major.
__global__ void __launch_bounds__(kRayDiagThreads) ray_diag_reduce_kernel(const double* __restrict__ rec, int64_t n,
                                                                          double* __restrict__ partial) {
  __shared__ double red[kRayDiagStats][kRayDiagThreads];
  double acc[kRayDiagStats];
#pragma unroll
  for (int q = 0; q < kRayDiagStats; ++q) acc[q] = 0.0;
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n; o += (int64_t)gridDim.x * blockDim.x) {
    const double2* q = reinterpret_cast<const double2*>(rec + (size_t)o * kRayDiagRec);
    const double2 a0 = q[0], a1 = q[1], a2 = q[2];
    const double r = a0.x;
    acc[0] = fmax(acc[0], fabs(r));
    acc[1] += r;
    acc[2] += r * r;
    acc[3] += a0.y;
    acc[4] += a1.x;
    acc[5] += a1.y;
    acc[6] += a2.x;
  }
#pragma unroll
  for (int q = 0; q < kRayDiagStats; ++q) red[q][threadIdx.x] = acc[q];
  __syncthreads();
  for (int off = kRayDiagThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      red[0][threadIdx.x] = fmax(red[0][threadIdx.x], red[0][threadIdx.x + off]);
#pragma unroll
      for (int q = 1; q < kRayDiagStats; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x < kRayDiagStats) partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = red[threadIdx.x][0];
}

// The workgroups' partials in block order, one lane per statistic, into a frame.
__global__ void ray_diag_frame_kernel(const double* __restrict__ partial, int nblk, int64_t n,
                                      double* __restrict__ frame) {
  const int q = threadIdx.x;
  if (blockIdx.x != 0 || q >= kRayDiagStats) return;
  const double* col = partial + (size_t)q * nblk;
  double s = 0.0;
  if (q == 0) {
    for (int i = 0; i < nblk; ++i) s = fmax(s, col[i]);
    frame[0] = (double)n;
  } else {
#pragma unroll 8
    for (int i = 0; i < nblk; ++i) s += col[i];
  }
  frame[1 + q] = s;
}

}  // namespace swrt
