// swrt_recycle.hpp — packet recycling (swrt_recycle_*): at an event every
// packet whose omega has reached omega_cut is absorbed and re-injected in the
// same slot with its home wavevector and a fresh uniform position, so a long
// run holds a source at omega_0, a sink at omega_cut and N fixed.
//
// State per packet by ORIGINAL index (as the transition series keeps src: the
// storage order does not last): home (2 doubles, column-major n x 2), gen
// (re-injections so far) and born (the event serial of the last injection).
//
// One event with serial s, per packet p in storage order, o = perm[p]:
//   w = sqrt(f^2 + Cg^2 (k k + l l))            (trans_omega's operation order)
//   rejected  if !(w * 2^frac_bits < 2^38)       (NaN and infinity included):
//             counted, left untouched;
//   absorbed  else if w >= omega_cut: tally rint(w * scale),
//             rint(omega(home[o]) * scale) and age = s - born[o]; then
//             gen[o] += 1, born[o] = s, (k, l) = home[o],
//             x = (u1 - 0.5) L, y = (u2 - 0.5) L;
//   untouched otherwise.
// u1, u2 come from a counter-based hash of (seed, index_base + o, gen[o] after
// the increment) (recycle_mix, the splitmix64 finaliser), so a packet's new
// position does not depend on the storage order or on the shard it lives in.
//
// The frame, 8 x 64-bit: [n, absorbed, rejected, sum q(omega_out),
// sum q(omega_home), sum age, max age, serial].  Integer sums and a max are
// order-free: a frame depends on the packet set alone.
//
// One lane per packet on a fixed grid striding over the 16 B of k per packet,
// coalesced; only the (rare) absorb branch touches perm, home, gen, born, x
// and writes k.  Each lane keeps its six tallies in registers, a wave merges
// them by shuffles, the workgroup's waves through LDS, and the workgroup adds
// one 64-bit atomic per non-zero statistic: none at all when it absorbed and
// rejected nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swrt_trans.hpp"

namespace swrt {

constexpr int kRecycleThreads = 256;
constexpr int kRecycleBlocks = 1024;  // workgroups, at most (the spectrum series' grid: no gather to hide)
constexpr int kRecycleFrame = 8;      // n, absorbed, rejected, sum out, sum home, sum age, max age, serial
constexpr int kRecycleTallies = 6;    // absorbed .. max age: what the workgroups merge
constexpr int kRecycleMaxFracBits = 32;
constexpr int64_t kRecycleSeriesMin = 4096;  // frames reserved by the first event (256 KiB)

struct RecycleArgs {
  double* x;          // N x 2 column-major, storage order
  double* k;
  const int* perm;    // storage slot -> original index
  int64_t n;
  double f2, Cg2;
  double cut;         // omega_cut
  double L;
  double scale;       // 2^frac_bits
  uint64_t seed;
  uint64_t base;      // index_base: the global id of original index 0
  int serial;         // this event's, from 1
  const double* home; // N x 2 column-major, original order
  int* gen;           // original order
  int* born;
  unsigned long long* frame;  // kRecycleFrame words, zeroed before the launch
};

__host__ __device__ inline uint64_t recycle_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double recycle_unit(uint64_t h) { return (double)(h >> 11) * 0x1p-53; }

// omega * scale is representable in the frame's sums (NaN and infinity are not)
__device__ __forceinline__ bool recycle_fits(double w, double scale) { return w * scale < 0x1p38; }

// home[o] := the k of the packet whose original index is o (begin with home NULL)
__global__ void __launch_bounds__(kRecycleThreads) recycle_home_kernel(const double* __restrict__ k,
                                                                       const int* __restrict__ perm, int64_t n,
                                                                       double* __restrict__ home) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t o = perm[p];
  home[o] = k[p];
  home[n + o] = k[n + p];
}

// *bad := 1 if any home wavevector would be rejected or absorbed at once
__global__ void __launch_bounds__(kRecycleThreads) recycle_home_check_kernel(const double* __restrict__ home, int64_t n,
                                                                             double f2, double Cg2, double cut,
                                                                             double scale, int* __restrict__ bad) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) return;
  const double w = trans_omega(f2, Cg2, home[o], home[n + o]);
  if (!recycle_fits(w, scale) || w >= cut) *bad = 1;  // (every writer stores the same value)
}

__global__ void __launch_bounds__(kRecycleThreads) recycle_kernel(RecycleArgs a) {
  __shared__ unsigned long long part[kRecycleThreads / 64][kRecycleTallies];
  // absorbed, rejected, sum q(omega_out), sum q(omega_home), sum age, max age
  unsigned long long t[kRecycleTallies] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  for (int64_t p = (int64_t)blockIdx.x * kRecycleThreads + threadIdx.x; p < a.n;
       p += (int64_t)gridDim.x * kRecycleThreads) {
    const double w = trans_omega(a.f2, a.Cg2, a.k[p], a.k[a.n + p]);
    if (!recycle_fits(w, a.scale)) {
      ++t[1];
    } else if (w >= a.cut) {
      const int64_t o = a.perm[p];
      const double hk = a.home[o], hl = a.home[a.n + o];
      const unsigned long long age = (unsigned long long)(a.serial - a.born[o]);
      const int g = a.gen[o] + 1;
      ++t[0];
      t[2] += (unsigned long long)(long long)rint(w * a.scale);
      t[3] += (unsigned long long)(long long)rint(trans_omega(a.f2, a.Cg2, hk, hl) * a.scale);
      t[4] += age;
      t[5] = age > t[5] ? age : t[5];
      a.gen[o] = g;
      a.born[o] = a.serial;
      const uint64_t h1 = recycle_mix(recycle_mix(a.seed ^ recycle_mix(a.base + (uint64_t)o)) + (uint64_t)g);
      const uint64_t h2 = recycle_mix(h1);
      a.k[p] = hk;
      a.k[a.n + p] = hl;
      a.x[p] = (recycle_unit(h1) - 0.5) * a.L;
      a.x[a.n + p] = (recycle_unit(h2) - 0.5) * a.L;
    }
  }
  // (every lane is back here: the shuffles below run with the whole wave)
  for (int off = 32; off > 0; off >>= 1) {
    for (int j = 0; j < kRecycleTallies - 1; ++j) t[j] += (unsigned long long)__shfl_xor((long long)t[j], off, 64);
    const unsigned long long m = (unsigned long long)__shfl_xor((long long)t[5], off, 64);
    t[5] = m > t[5] ? m : t[5];
  }
  const int wave = threadIdx.x / 64;
  if (__lane_id() == 0)
    for (int j = 0; j < kRecycleTallies; ++j) part[wave][j] = t[j];
  __syncthreads();
  if (threadIdx.x < kRecycleTallies) {
    const int j = threadIdx.x;
    unsigned long long v = part[0][j];
    for (int w = 1; w < kRecycleThreads / 64; ++w) {
      const unsigned long long q = part[w][j];
      v = j == 5 ? (q > v ? q : v) : v + q;
    }
    if (v) {
      if (j == 5)
        atomicMax(&a.frame[6], v);
      else
        atomicAdd(&a.frame[1 + j], v);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // (the host's values: plain stores to words nobody adds to)
    a.frame[0] = (unsigned long long)a.n;
    a.frame[7] = (unsigned long long)a.serial;
  }
}

}  // namespace swrt
