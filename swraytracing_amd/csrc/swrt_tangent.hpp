// swrt_tangent.hpp — the ray-tube tangent map (swrt_tangent_*): the exact
// derivative of the DISCRETE leapfrog step, carried along every ray.
//
// Per packet M = d(x, y, k, l) / d(x0, y0, k0, l0) since the last mark, 4 x 4
// row-major, rows X0, X1 (position) and K0, K1 (wave vector), I at a mark.  M
// is the Jacobian of the map leapfrog_kernel applies (drift, Euler kick,
// drift), not of the flow of the ray equations: det M != 1 measures the
// scheme (the Euler kick is not symplectic), not the flow.  J = M00 M11 -
// M01 M10 is the ray tube's area ratio for a packet launched as a plane wave;
// `caustics` counts its sign changes, step by step.
//
// M and the counters live by ORIGINAL packet index (the transition series'
// reasoning, swrt_trans.hpp): a re-binning moves x, k and perm and leaves the
// 128-byte rows where they are; a lane reads and writes row perm[p].
//
// x and k are computed by leapfrog_kernel's own expressions (drift_inc's
// quotients, stencil_at's cell and weights, gather6's sums in gather6's
// order, the same blend and kick), so they keep their bits.  The operation
// order of everything else is the contract tests/tangent_ref.py restates; no
// FMA is formed (-ffp-contract=off), every `/` is an IEEE division.
//
//   t_j    = (a - j) + bump, j = -2..3            (lagrange_w's t)
//   P(i,m) = t_j1 * t_j2 * t_j3 * t_j4            (the j not in {i, m}, ascending, left to right)
//   c(i,m) = 1 / ((m - i) * prod_{j != i,m} (j - i))    (an integer denominator, one division)
//   w'_i   = sum over m != i, ascending, left to right, of c(i,m) * P(i,m)
//
//   per tap (i outer, j inner), record {u, v, ux, uy, vx, vy} of a snapshot:
//     wij = wx_i * wy_j;  dxw = wx'_i * wy_j;  dyw = wx_i * wy'_j
//     o[f] = o[f] + wij * F_f                      (gather6's six sums)
//     d[0] += dxw * u;  d[1] += dyw * u;  d[2] += dxw * v;  d[3] += dyw * v
//     ta = ux * k + vx * l;  tb = uy * k + vy * l  (k, l: the pre-kick wave vector)
//     d[4] += dxw * ta;  d[5] += dyw * ta;  d[6] += dxw * tb;  d[7] += dyw * tb
//   (every sum starts from its first term.)  Two snapshots: each of the 14
//   sums is blended as the fields are, (1 - alpha) * s0 + alpha * s1.  Then
//   d[q] = d[q] * RN(1 / dx): (Ux, Uy, Vx, Vy, Ax, Ay, Bx, By).
//
//   drift matrix of a wave vector (k, l), with (qx, qy) = gH (k, l) / omega
//   exactly as the drift forms them:
//     g = gH / omega;  dxx = g - (qx * qx) / omega;  dxy = -((qx * qy) / omega);
//     dyy = g - (qy * qy) / omega
//   drift(h), every column c:
//     X0[c] = X0[c] + h * (dxx * K0[c] + dxy * K1[c])
//     X1[c] = X1[c] + h * (dxy * K0[c] + dyy * K1[c])
//   kick(dt), every column c, from the rows before the kick:
//     X0' = X0 + dt * (Ux * X0 + Uy * X1)
//     X1' = X1 + dt * (Vx * X0 + Vy * X1)
//     K0' = K0 - dt * ((Ax * X0 + Ay * X1) + (ux * K0 + vx * K1))
//     K1' = K1 - dt * ((Bx * X0 + By * X1) + (uy * K0 + vy * K1))
//   (ux, uy, vx, vy: the blended gradient fields the packet's kick uses.)
//   A step is drift(dt/2) with the drift matrix of the old k, the kick, and
//   drift(dt/2) with that of the new k; then J = M00 * M11 - M01 * M10 and the
//   counter increments when (J < 0) differs from its value after the previous
//   step (at launch start it is recomputed from M; J = 1 at a mark).
//
// tangent_record_kernel makes one class-plane frame (PlaneLayout) from the M
// rows and the packets' omega, in the spectrum series' bits:
//   s = (M0*M0 + M1*M1 + ... + M15*M15) / 4  (row-major, left to right),
//   e(v) = frexp exponent of v minus 1 (floor(log2 v): exact, an integer),
//   counts  (ns + 2) x (nw + 2), cell gc * (nw + 2) + wc, gc = hist_slot(s,
//           growth_edges), wc = hist_slot(omega, omega_edges): comparisons only;
//   sums    per omega class e(s), e(|J|), caustics (three rows of nw + 2), then
//           per growth class the caustics (ns + 2);
//   stats   [n, rejected, mark serial].
// A packet is rejected, and adds to nothing else, if omega, s or J is not
// finite or J == 0.  Integer sums: a frame is order-free and shards add.  The
// LDS-plane and global-atomic forms are refr_kernel's (same tail shape).
//
// NaN, Inf, k = 0 and huge k: stencil_at keeps every cell index in range, the
// rows are indexed by perm alone and the classes by hist_slot; nothing is
// indexed by a computed value without a range check.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swrt_diag.hpp"
#include "swrt_kernels.hpp"
#include "swrt_kmap.hpp"
#include "swrt_refr.hpp"

namespace swrt {

constexpr int kTanM = 16;                      // doubles per packet: M, row-major
constexpr int kTanThreads = 256;
constexpr int kTanStats = 3;                   // n, rejected, mark serial
constexpr int kTanWSums = 3;                   // per omega class: e(s), e(|J|), caustics
constexpr int64_t kTanMaxPackets = (int64_t)1 << 24;  // of a recorded frame

struct TangentArgs {
  double* M;       // n x 16 by original packet index
  int* caustics;   // n, likewise
};

// P(i, m) and c(i, m) of the header; i, m and j are constants after unrolling.
__device__ __forceinline__ double tan_pairprod(int i, int m, const double* t) {
  double p = 1.0;  // (1 * t == t: the product starts from its first factor)
#pragma unroll
  for (int j = -2; j <= 3; ++j)
    if (j != i && j != m) p = p * t[j + 2];
  return p;
}
constexpr double tan_coef(int i, int m) {
  int den = m - i;
  for (int j = -2; j <= 3; ++j)
    if (j != i && j != m) den *= j - i;
  return 1.0 / (double)den;
}

__device__ __forceinline__ void lagrange_dw(double a, double bump, double wp[kNT]) {
  double t[kNT];
#pragma unroll
  for (int j = -2; j <= 3; ++j) t[j + 2] = (a - (double)j) + bump;
#pragma unroll
  for (int i = -2; i <= 3; ++i) {
    double s = -0.0;  // the additive identity: the sum starts from its first term
#pragma unroll
    for (int m = -2; m <= 3; ++m)
      if (m != i) s = s + tan_coef(i, m) * tan_pairprod(i, m, t);
    wp[i + 2] = s;
  }
}

struct TanStencil {
  Stencil s;
  double wxp[kNT], wyp[kNT];
};

// stencil_at with the weights' derivatives: the same cell, offsets and weights
// (its statements, which keep the offsets to themselves), then lagrange_dw.
__device__ __forceinline__ void tan_stencil_at(const FieldView& fv, double x, double y, double bump, TanStencil& ts) {
  double ax, ay, rx, ry;
  const double qx = cell_quot(x, fv.dx, fv.inv_dx, fv.inv_px, rx);
  const double qy = cell_quot(y, fv.dx, fv.inv_dx, fv.inv_py, ry);
  if (!fv.inv_exact) {
    rx = cell_quot_fix(qx, rx, fv.px, fv.inv_px);
    ry = cell_quot_fix(qy, ry, fv.py, fv.inv_py);
  }
  ts.s.ic = cell_tail(qx, rx, fv.px, fv.nx, fv.nx, ax, true);
  ts.s.jc = cell_tail(qy, ry, fv.py, fv.ipy, fv.nx, ay, fv.ywrap1 != 0);
  lagrange_w(ax, bump, ts.s.wx);
  lagrange_w(ay, bump, ts.s.wy);
  lagrange_dw(ax, bump, ts.wxp);
  lagrange_dw(ay, bump, ts.wyp);
}

__device__ __forceinline__ double tap_sel(const double (&v)[kNT], int i) {
  return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : i == 3 ? v[3] : i == 4 ? v[4] : v[5];
}

constexpr int kTanD = 8;  // derivative sums: u,x u,y v,x v,y and the contracted A,x A,y B,x B,y

// gather6's six sums (its expressions, its order) and the eight derivative sums.
template <bool TWO>
__device__ __forceinline__ void gather_tangent(const double* nodes0, const double* nodes1, int npad,
                                               const TanStencil& ts, double k, double l, double o0[kRec],
                                               double o1[kRec], double d0[kTanD], double d1[kTanD]) {
#pragma unroll
  for (int f = 0; f < kRec; ++f) { o0[f] = -0.0; o1[f] = -0.0; }
#pragma unroll
  for (int f = 0; f < kTanD; ++f) { d0[f] = -0.0; d1[f] = -0.0; }
  const Stencil& s = ts.s;
  const size_t off = ((size_t)s.ic * npad + s.jc) * kRec;
  // A real loop over the stencil rows (the row's weights by constant-index
  // selects, as stage_sel): unrolled, all 36 taps' loads are issued ahead of
  // the sums and the kernel spills.
#pragma unroll 1
  for (int i = 0; i < kNT; ++i) {
    const size_t ro = off + (size_t)i * npad * kRec;
    const double2* r0 = reinterpret_cast<const double2*>(nodes0 + ro);
    const double2* r1 = reinterpret_cast<const double2*>(nodes1 + ro);
    const double wxi = tap_sel(s.wx, i), wxpi = tap_sel(ts.wxp, i);
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      const double wij = wxi * s.wy[j];
      const double dxw = wxpi * s.wy[j];
      const double dyw = wxi * ts.wyp[j];
      const double2 a0 = r0[3 * j + 0], a1 = r0[3 * j + 1], a2 = r0[3 * j + 2];
      o0[0] = o0[0] + wij * a0.x; o0[1] = o0[1] + wij * a0.y;
      o0[2] = o0[2] + wij * a1.x; o0[3] = o0[3] + wij * a1.y;
      o0[4] = o0[4] + wij * a2.x; o0[5] = o0[5] + wij * a2.y;
      d0[0] = d0[0] + dxw * a0.x; d0[1] = d0[1] + dyw * a0.x;
      d0[2] = d0[2] + dxw * a0.y; d0[3] = d0[3] + dyw * a0.y;
      const double ta = a1.x * k + a2.x * l, tb = a1.y * k + a2.y * l;
      d0[4] = d0[4] + dxw * ta; d0[5] = d0[5] + dyw * ta;
      d0[6] = d0[6] + dxw * tb; d0[7] = d0[7] + dyw * tb;
      if constexpr (TWO) {
        const double2 b0 = r1[3 * j + 0], b1 = r1[3 * j + 1], b2 = r1[3 * j + 2];
        o1[0] = o1[0] + wij * b0.x; o1[1] = o1[1] + wij * b0.y;
        o1[2] = o1[2] + wij * b1.x; o1[3] = o1[3] + wij * b1.y;
        o1[4] = o1[4] + wij * b2.x; o1[5] = o1[5] + wij * b2.y;
        d1[0] = d1[0] + dxw * b0.x; d1[1] = d1[1] + dyw * b0.x;
        d1[2] = d1[2] + dxw * b0.y; d1[3] = d1[3] + dyw * b0.y;
        const double ua = b1.x * k + b2.x * l, ub = b1.y * k + b2.y * l;
        d1[4] = d1[4] + dxw * ua; d1[5] = d1[5] + dyw * ua;
        d1[6] = d1[6] + dxw * ub; d1[7] = d1[7] + dyw * ub;
      }
    }
  }
}

// drift_quot's quotients (its expressions) and the drift matrix of the header.
__device__ __forceinline__ void tan_drift(double k, double l, double f2, double gH, bool fast, double& qx, double& qy,
                                          double& dxx, double& dxy, double& dyy) {
  const double x = f2 + gH * (k * k + l * l);
  double w;
  if (fast) {
    w = sqrt_rn_normal(x);
    const double rw = rcp_rn_normal(w);
    qx = div_rn_z(gH * k, w, rw);
    qy = div_rn_z(gH * l, w, rw);
  } else {
    w = sqrt(x);
    qx = gH * k / w;
    qy = gH * l / w;
  }
  const double g = gH / w;
  dxx = g - (qx * qx) / w;
  dxy = -((qx * qy) / w);
  dyy = g - (qy * qy) / w;
}

// leapfrog_kernel with M and the caustic counter in registers beside x and k.
template <bool TWO>
__global__ void __launch_bounds__(256) leapfrog_tangent_kernel(StepArgs a, TangentArgs g) {
  const int64_t p = xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  double x0 = a.x[p], y0 = a.x[a.n + p];
  double k0 = a.k[p], l0 = a.k[a.n + p];
  const int64_t o = a.perm[p];
  double* Mo = g.M + o * kTanM;
  double X0[4], X1[4], K0[4], K1[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    X0[c] = Mo[c]; X1[c] = Mo[4 + c]; K0[c] = Mo[8 + c]; K1[c] = Mo[12 + c];
  }
  int ncaus = g.caustics[o];
  bool neg = (X0[0] * X1[1] - X0[1] * X1[0]) < 0;
  double qx, qy, dxx, dxy, dyy;
  tan_drift(k0, l0, a.f2, a.gH, a.fastdisp, qx, qy, dxx, dxy, dyy);
  double hcx = a.half * qx, hcy = a.half * qy;  // (drift_inc's increments)
  for (int s = 0; s < a.nsteps; ++s) {
    const int64_t sg = a.s0 + s;
    const double x1 = x0 + hcx;
    const double y1 = y0 + hcy;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double b0 = K0[c], b1 = K1[c];
      X0[c] = X0[c] + a.half * (dxx * b0 + dxy * b1);
      X1[c] = X1[c] + a.half * (dxy * b0 + dyy * b1);
    }
    double I[kRec], d[kTanD];
    {
      TanStencil ts;
      tan_stencil_at(a.f0, x1, y1, a.bump, ts);
      double I1[kRec], d1[kTanD];
      gather_tangent<TWO>(a.f0.nodes, a.f1.nodes, a.f0.npad, ts, k0, l0, I, I1, d, d1);
      if constexpr (TWO) {
        const double alpha = a.alpha0 + (double)sg * a.dalpha;
        const double oma = 1 - alpha;
#pragma unroll
        for (int q = 0; q < kRec; ++q) I[q] = oma * I[q] + alpha * I1[q];
#pragma unroll
        for (int q = 0; q < kTanD; ++q) d[q] = oma * d[q] + alpha * d1[q];
      }
#pragma unroll
      for (int q = 0; q < kTanD; ++q) d[q] = d[q] * a.f0.inv_dx;
    }
    const double x2 = x1 + a.dt * I[0];
    const double y2 = y1 + a.dt * I[1];
    const double k2 = k0 - a.dt * (I[2] * k0 + I[4] * l0);
    const double l2 = l0 - a.dt * (I[3] * k0 + I[5] * l0);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double a0 = X0[c], a1 = X1[c], b0 = K0[c], b1 = K1[c];
      X0[c] = a0 + a.dt * (d[0] * a0 + d[1] * a1);
      X1[c] = a1 + a.dt * (d[2] * a0 + d[3] * a1);
      K0[c] = b0 - a.dt * ((d[4] * a0 + d[5] * a1) + (I[2] * b0 + I[4] * b1));
      K1[c] = b1 - a.dt * ((d[6] * a0 + d[7] * a1) + (I[3] * b0 + I[5] * b1));
    }
    tan_drift(k2, l2, a.f2, a.gH, a.fastdisp, qx, qy, dxx, dxy, dyy);
    hcx = a.half * qx;
    hcy = a.half * qy;
    x0 = x2 + hcx;
    y0 = y2 + hcy;
    k0 = k2;
    l0 = l2;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double b0 = K0[c], b1 = K1[c];
      X0[c] = X0[c] + a.half * (dxx * b0 + dxy * b1);
      X1[c] = X1[c] + a.half * (dxy * b0 + dyy * b1);
    }
    const bool nneg = (X0[0] * X1[1] - X0[1] * X1[0]) < 0;
    if (nneg != neg) ++ncaus;
    neg = nneg;
    if (a.hist_x != nullptr && ((sg + 1) % a.save_every) == 0) {
      const int64_t fr = a.frame0 + (sg + 1) / a.save_every - 1;
      double* hx = a.hist_x + fr * 2 * a.n;
      double* hk = a.hist_k + fr * 2 * a.n;
      hx[o] = x0; hx[a.n + o] = y0;  // frames are stored in the original packet order
      hk[o] = k0; hk[a.n + o] = l0;
    }
  }
  a.x[p] = x0; a.x[a.n + p] = y0;
  a.k[p] = k0; a.k[a.n + p] = l0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    Mo[c] = X0[c]; Mo[4 + c] = X1[c]; Mo[8 + c] = K0[c]; Mo[12 + c] = K1[c];
  }
  g.caustics[o] = ncaus;
}

// A mark: M = I and the counters 0, every row.
__global__ void __launch_bounds__(kTanThreads) tangent_mark_kernel(int64_t n, TangentArgs g) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * kTanM) return;
  const int r = (int)(e % kTanM);
  g.M[e] = (r % 5 == 0) ? 1.0 : 0.0;
  if (r == 0) g.caustics[e / kTanM] = 0;
}

struct TangentRecordArgs {
  const double* k;        // N x 2 column-major, storage order
  const int* perm;        // storage slot -> original index
  const double* M;        // by original index
  const int* caustics;
  int64_t n;
  double f2, Cg2;
  const double* wedges;   // nw + 1
  const double* sedges;   // ns + 1 (growth)
  int nw, ns;
  unsigned long long serial;
  unsigned long long* counts;  // (ns + 2) x (nw + 2), zeroed before the launch
  unsigned long long* tail;    // 3 (nw + 2) + (ns + 2) sums and kTanStats stats, zeroed likewise
};

// frexp exponent - 1 of a finite v > 0 (0 gives -1)
__device__ __forceinline__ long long tan_exp(double v) {
  int e = 0;
  (void)frexp(v, &e);
  return (long long)e - 1;
}

template <bool LDS>
__global__ void __launch_bounds__(kTanThreads) tangent_record_kernel(TangentRecordArgs a) {
  extern __shared__ double tan_lds[];
  const int nws = a.nw + 2, nss = a.ns + 2, ncell = nss * nws, nsum = kTanWSums * nws + nss;
  double* wedges = tan_lds;
  double* sedges = wedges + a.nw + 1;
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(sedges + a.ns + 1);
  unsigned int* rejected = reinterpret_cast<unsigned int*>(sums + nsum);
  unsigned int* cells = rejected + 2;
  for (int e = threadIdx.x; e <= a.nw; e += kTanThreads) wedges[e] = a.wedges[e];
  for (int e = threadIdx.x; e <= a.ns; e += kTanThreads) sedges[e] = a.sedges[e];
  for (int e = threadIdx.x; e < nsum; e += kTanThreads) sums[e] = 0ull;
  if (threadIdx.x == 0) *rejected = 0u;
  if constexpr (LDS)
    for (int e = threadIdx.x; e < ncell; e += kTanThreads) cells[e] = 0u;
  __syncthreads();
  unsigned int rej = 0u;
  // (the bound is the same for every lane of a wave: all of them reach the merge)
  for (int64_t base = (int64_t)blockIdx.x * kTanThreads; base < a.n; base += (int64_t)gridDim.x * kTanThreads) {
    const int64_t p = base + threadIdx.x;
    int cell = -1;
    if (p < a.n) {
      const int64_t o = a.perm[p];
      const double k1 = a.k[p], k2 = a.k[a.n + p];
      const double w = sqrt(a.f2 + a.Cg2 * (k1 * k1 + k2 * k2));  // load_data.m:33
      const double* Mo = a.M + o * kTanM;
      double m[kTanM];
#pragma unroll
      for (int q = 0; q < kTanM; ++q) m[q] = Mo[q];
      double acc = m[0] * m[0];
#pragma unroll
      for (int q = 1; q < kTanM; ++q) acc = acc + m[q] * m[q];
      const double s = acc / 4;
      const double J = m[0] * m[5] - m[1] * m[4];
      constexpr double inf = __builtin_inf();
      if (fabs(w) < inf && fabs(s) < inf && fabs(J) < inf && J != 0.0) {  // (a NaN fails its comparison)
        const int wc = hist_slot(w, wedges, a.nw), gc = hist_slot(s, sedges, a.ns);
        const unsigned long long cz = (unsigned long long)(long long)a.caustics[o];
        atomicAdd(&sums[wc], (unsigned long long)tan_exp(s));
        atomicAdd(&sums[nws + wc], (unsigned long long)tan_exp(fabs(J)));
        atomicAdd(&sums[2 * nws + wc], cz);
        atomicAdd(&sums[kTanWSums * nws + gc], cz);
        cell = gc * nws + wc;
      } else {
        ++rej;
      }
    }
    if constexpr (LDS)
      hist_add_wave(cells, cell);
    else
      kmap_add_wave<true>(a.counts, cell);
  }
  for (int off = 32; off > 0; off >>= 1) rej += (unsigned int)__shfl_xor((int)rej, off, 64);
  if (__lane_id() == 0 && rej) atomicAdd(rejected, rej);
  __syncthreads();
  if constexpr (LDS) hist_flush(cells, ncell, a.counts);
  for (int e = threadIdx.x; e < nsum; e += kTanThreads)
    if (const unsigned long long s = sums[e]) atomicAdd(&a.tail[e], s);
  if (threadIdx.x == 0) {
    if (*rejected) atomicAdd(&a.tail[nsum + 1], (unsigned long long)*rejected);
    if (blockIdx.x == 0) {
      a.tail[nsum] = (unsigned long long)a.n;
      a.tail[nsum + 2] = a.serial;
    }
  }
}

}  // namespace swrt
