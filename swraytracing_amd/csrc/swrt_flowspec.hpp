// swrt_flowspec.hpp — the flow spectrum series (swrt_flow_spectrum_*): the
// background flow's shell spectra from the spectral PV of one layer, as the
// reference's analysis scripts compute them (scratch/energy_spectrum.m:3-13:
// psik = -qk./(K_d2 + K2), KE = K2.*|psik|^2 summed over the shells
// (j - 1/2)^2 <= K^2 < (j + 1/2)^2; rsw/isospectrum.m:14-21 writes the same
// rule floor(K + .5) == j).
//
// A frame is 3 x nshell doubles [E(0..J), Z(0..J), Q(0..J)]: kinetic energy,
// enstrophy of the relative vorticity and PV variance per shell, each half the
// full-plane sum (the half plane ky >= 0, the mean mode with weight 1/2), and
// four stats [t, sum E, sum Z, sum Q].  include/swrt.h states the per-mode
// arithmetic and the summation order; both are fixed, so a frame is a function
// of qk alone and equals the numpy restatement bit for bit.
//
// It is a gather: the shell of (kx, ky) is the integer j with
// j(j-1) < kx^2 + ky^2 <= j(j+1) (j = 0: the mean mode), so along a row kx the
// modes of shell j are one run of consecutive ky, found from two integer
// square roots.  flow_spectrum_kernel runs one workgroup per shell: a lane
// takes the rows of slots i and i + nx/2 (the pair the halving tree adds
// first), sums each row's run in ascending ky and stores the pair's sum to
// LDS; the tree's remaining levels fold there.  Every mode is read once, by
// the one lane whose row and shell hold it; nothing is added through memory,
// so no order depends on the launch.  The half plane is addressed by the
// element strides of kx and ky: the QG state's order (ky fastest) and the
// host's (kx fastest) go through the same code.  flow_spectrum_totals_kernel
// then sums the shells in ascending j.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace swrt {

constexpr int kFlowSpecThreads = 256;
constexpr int kFlowSpecStats = 4;  // t and the three totals
constexpr int kFlowSpecAhead = 8;  // modes of a row's run loaded ahead of the sequential sums
constexpr int kFlowSpecTotalsChunk = 512;  // shells the totals kernel holds in LDS at a time (12 KB)

// floor(sqrt(v)), v >= 0 (below 2^24 here: v <= 2 kmax^2 + 2 kmax, kmax <= 2047)
__host__ __device__ inline int flow_isqrt(int v) {
  int s = (int)sqrt((double)v);
  while (s * s > v) --s;
  while ((s + 1) * (s + 1) <= v) ++s;
  return s;
}

// The shell of the index wavenumber with kx^2 + ky^2 = r2: the j >= 0 with
// (2j-1)^2 <= 4 r2 < (2j+1)^2, i.e. j(j-1) < r2 <= j(j+1); 0 for r2 = 0.
__host__ __device__ inline int flow_shell_of(int r2) {
  const int s = flow_isqrt(r2);
  return r2 <= s * (s + 1) ? s : s + 1;
}

// shells of an nx^2 grid: the corner mode's shell and those below it
inline int flow_shells(int nx) {
  const int kmax = nx / 2 - 1;
  return flow_shell_of(2 * kmax * kmax) + 1;
}

struct FlowSpecArgs {
  const double2* qk;  // the half plane: mode (kx, ky) at (kx + kmax)*skx + ky*sky
  int64_t skx, sky;
  int nx;
  int nshell;
  double k_scale, K_d2;
  double* frame;      // 3 x nshell
};

// Row kx's modes of the shell lo2 <= kx^2 + ky^2 <= hi2, summed in ascending
// ky from +0.0 (include/swrt.h: the per-mode arithmetic, one IEEE operation
// each; the translation unit is built with FP contraction off).
__device__ __forceinline__ void flow_row_sums(const FlowSpecArgs& a, int kx, int kmax, int lo2, int hi2, double& E,
                                              double& Z, double& Q) {
  E = 0.0;
  Z = 0.0;
  Q = 0.0;
  const int kx2 = kx * kx;
  if (hi2 < kx2) return;
  int hi = flow_isqrt(hi2 - kx2);
  if (hi > kmax) hi = kmax;
  int lo = lo2 > kx2 ? flow_isqrt(lo2 - kx2 - 1) + 1 : 0;
  if (kx < 0 && lo < 1) lo = 1;  // (ky = 0, kx < 0: fulspec.m:16 overwrites them, whatever they hold)
  const double kxs = (double)kx * a.k_scale;
  const double2* row = a.qk + (int64_t)(kx + kmax) * a.skx;
  // The sums are sequential, the loads need not be: kFlowSpecAhead modes are
  // fetched before the first is used (a run near |kx| = j holds about sqrt(2j)
  // modes, and one load at a time made the longest lane the whole launch).
  for (int ky0 = lo; ky0 <= hi; ky0 += kFlowSpecAhead) {
    double2 qv[kFlowSpecAhead];
#pragma unroll
    for (int u = 0; u < kFlowSpecAhead; ++u)
      qv[u] = row[(int64_t)(ky0 + u <= hi ? ky0 + u : hi) * a.sky];  // (past the run: mode hi again, unused)
#pragma unroll
    for (int u = 0; u < kFlowSpecAhead; ++u) {
      const int ky = ky0 + u;
      if (ky > hi) break;
      const double2 q = qv[u];
      const double kys = (double)ky * a.k_scale;
      const double K2 = kxs * kxs + kys * kys;
      const double den = a.K_d2 + K2;
      double pr = 0.0, pi = 0.0;
      if (den != 0.0) {
        pr = -q.x / den;
        pi = -q.y / den;
      }
      const double aa = pr * pr + pi * pi;
      const double w = (kx == 0 && ky == 0) ? 0.5 : 1.0;
      E = E + w * (K2 * aa);
      Z = Z + w * ((K2 * K2) * aa);
      Q = Q + w * (q.x * q.x + q.y * q.y);
    }
  }
}

// One workgroup per shell; dynamic LDS: 3 x nx/2 doubles.
__global__ __launch_bounds__(kFlowSpecThreads) void flow_spectrum_kernel(FlowSpecArgs a) {
  extern __shared__ double flow_lds[];
  const int nh = a.nx / 2, kmax = nh - 1;
  double* sE = flow_lds;
  double* sZ = sE + nh;
  double* sQ = sZ + nh;
  const int j = (int)blockIdx.x;
  if (j >= a.nshell) return;
  const int lo2 = j == 0 ? 0 : j * (j - 1) + 1, hi2 = j * (j + 1);
  // the tree's first level, h = nx/2: slot i (kx = i - kmax <= 0) + slot i + nx/2
  // (kx = i + 1; slot nx - 1 holds no row: +0.0)
  for (int i = (int)threadIdx.x; i < nh; i += kFlowSpecThreads) {
    double e0, z0, q0, e1 = 0.0, z1 = 0.0, q1 = 0.0;
    flow_row_sums(a, i - kmax, kmax, lo2, hi2, e0, z0, q0);
    if (i + 1 <= kmax) flow_row_sums(a, i + 1, kmax, lo2, hi2, e1, z1, q1);
    sE[i] = e0 + e1;
    sZ[i] = z0 + z1;
    sQ[i] = q0 + q1;
  }
  __syncthreads();
  for (int h = nh / 2; h >= 1; h >>= 1) {
    for (int i = (int)threadIdx.x; i < h; i += kFlowSpecThreads) {
      sE[i] = sE[i] + sE[i + h];
      sZ[i] = sZ[i] + sZ[i + h];
      sQ[i] = sQ[i] + sQ[i + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.frame[j] = sE[0];
    a.frame[a.nshell + j] = sZ[0];
    a.frame[2 * a.nshell + j] = sQ[0];
  }
}

// stats4 = [t, sum E, sum Z, sum Q], each total summed in ascending j from
// +0.0 by one lane.  One workgroup: the shells go through LDS a chunk at a
// time, loaded by all lanes, so the sequential sums wait for no global load.
__global__ __launch_bounds__(kFlowSpecThreads) void flow_spectrum_totals_kernel(const double* frame, int nshell,
                                                                                double t, double* stats4) {
  __shared__ double buf[3 * kFlowSpecTotalsChunk];
  const int tid = (int)threadIdx.x;
  double s = 0.0;
  for (int base = 0; base < nshell; base += kFlowSpecTotalsChunk) {
    const int n = nshell - base < kFlowSpecTotalsChunk ? nshell - base : kFlowSpecTotalsChunk;
    for (int e = tid; e < 3 * n; e += kFlowSpecThreads) {
      const int q = e / n, i = e - q * n;
      buf[q * kFlowSpecTotalsChunk + i] = frame[q * nshell + base + i];
    }
    __syncthreads();
    if (tid < 3)
      for (int i = 0; i < n; ++i) s = s + buf[tid * kFlowSpecTotalsChunk + i];
    __syncthreads();
  }
  if (tid < 3) stats4[1 + tid] = s;
  if (tid == 3) stats4[0] = t;
}

}  // namespace swrt
