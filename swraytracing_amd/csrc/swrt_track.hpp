// swrt_track.hpp — the trajectories of a chosen few packets, recorded on the
// device.
//
// The reference's figures are per packet: x against time (images/QG_spread*),
// the (k, l) paths of raytracing_figures.m:76-83, Omega against time, and
// analysis/load_data.m:29-33 reads packet_x.bin / packet_k.bin of Npackets x 2
// per frame.  It runs 50 packets.  At 1e6 nobody downloads the ensemble per
// frame; the caller names m of them (swrt_track_begin) and every record
// appends one m x 8 frame, column-major: row j is packet ids[j], the columns
// [x, y, k, l, Omega, zeta, sigma, D].  x, y, k, l are the stored bits
// (positions unwrapped); the other four are ray_diag_kernel's per-packet
// values through the same device functions (eval_flow, ray_point_*), hence
// the bits swrt_raydiag_sample's sample4_out holds.  Without a flow
// (nslots == 0) they are the quiet NaN 0x7ff8000000000000.
//
// The live packets sit in the binning's storage order with perm[p] their
// original index, so a record finds its m among n without un-permuting: a
// table slot_of[original index] = row or -1 (n x int32, written by
// swrt_track_begin), one lane per stored packet reading perm[p] and
// slot_of[perm[p]] — 8 B per stored packet, the table's reads scattered over
// a 4 MB table at 1e6 packets, which stays in L2 — and the lanes that hit do
// the 6 x 6 gather and eight plain stores to frame[j + m*c].
//
// Hits are not compacted first.  At the sizes this is for (m of a few thousand
// in 1e6) a wave of 64 holds 0.06 hits on average, so a wave with a hit has
// one, and its gather runs at one lane's width whatever order the wave's
// lanes are in; compacting across waves needs a pass and a launch of its own
// to save the ~m divergent gathers.  Measured at 1e6 packets, two snapshots
// (profiles/track_series/README.md): the scan alone 0.016 ms (m = 64), the
// hits about 4 ns each on top — 0.010 ms at m = 1024, less than a launch
// boundary and a second pass would cost; 0.067 ms at m = 16384, where a
// compaction would pay if frames of that size ever matter.  With m near n
// every lane hits and the launch is ray_diag_kernel's.
//
// A history frame is in the original order already: track_kernel<true> runs
// one lane per tracked packet and reads ids[j] directly, no table and no scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swrt_kernels.hpp"
#include "swrt_raydiag.hpp"

namespace swrt {

constexpr int kTrackThreads = 256;
constexpr int kTrackCols = 8;              // x, y, k, l, Omega, zeta, sigma, D
constexpr int64_t kTrackMax = 1 << 20;     // tracked packets at most
constexpr unsigned long long kTrackNaN = 0x7ff8000000000000ull;  // columns 4..7 without a flow

struct TrackArgs {
  FieldView f0, f1;
  int nslots;         // 0: no flow (columns 4..7 are kTrackNaN)
  double alpha, bump;
  const double* x;    // N x 2 column-major: storage order, or a history frame (original order)
  const double* k;
  const int* perm;    // storage slot -> original packet index (not HIST)
  const int* lookup;  // slot_of[original index] = row or -1 (n entries); HIST: ids[row] (m entries)
  int64_t n;
  int64_t m;
  double f2, gH;      // f2 = f*f
  double* frame;      // m x 8 column-major
};

// Row j of the frame from the packet at index p of a.x / a.k.
__device__ __forceinline__ void track_row(const TrackArgs& a, int64_t p, int64_t j) {
  const double x1 = a.x[p], x2 = a.x[a.n + p];
  const double k1 = a.k[p], k2 = a.k[a.n + p];
  double* out = a.frame + j;
  out[0] = x1;
  out[a.m] = x2;
  out[2 * a.m] = k1;
  out[3 * a.m] = k2;
  if (a.nslots == 0) {
    const double nan = __longlong_as_double((long long)kTrackNaN);
    out[4 * a.m] = nan;
    out[5 * a.m] = nan;
    out[6 * a.m] = nan;
    out[7 * a.m] = nan;
    return;
  }
  double I[kRec];  // u, v, u_x, u_y, v_x, v_y
  eval_flow(a.f0, a.f1, a.nslots, a.alpha, x1, x2, a.bump, I);
  RayPoint pt;
  ray_point_omega(I, k1, k2, a.f2, a.gH, pt);
  ray_point_flow(I, pt);
  out[4 * a.m] = pt.Om;
  out[5 * a.m] = pt.zeta;
  out[6 * a.m] = pt.sigma;
  out[7 * a.m] = pt.D;
}

// HIST: one lane per tracked packet over a frame in the original order; else
// one lane per stored packet, the tracked ones found through the table.
template <bool HIST>
__global__ void __launch_bounds__(kTrackThreads) track_kernel(TrackArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (HIST) {
    if (t >= a.m) return;
    track_row(a, (int64_t)a.lookup[t], t);
  } else {
    if (t >= a.n) return;
    const int j = a.lookup[a.perm[t]];
    if (j < 0) return;
    track_row(a, t, (int64_t)j);
  }
}

}  // namespace swrt
