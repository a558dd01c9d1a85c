// swrt_host_packets.hpp — host side of the packet steppers: the leapfrog
// launches (per-packet and LDS-tiled, split over the packet streams and
// checked by the hazard model), spatial re-binning, the advance loops and
// the history buffers.  (debug_spin_kernel and debug_corrupt_count_kernel are
// defined by swrt_api.hip before it includes this header.)
#pragma once
#include <algorithm>
#include <vector>

#include "swrt_ctx.hpp"
#include "swrt_host_fields.hpp"
#include "swrt_bin.hpp"
#include "swrt_kernels.hpp"
#include "swrt_tile.hpp"
#include "swrt_share.hpp"
#include "swrt_xka.hpp"
#include "swrt_spectral.hpp"
#include "swrt_tangent.hpp"

namespace {

bool use_tile_kernel(const swrt_ctx* c) {
  if (c->tan.live) return false;  // a live tangent set: the per-packet route carries M (swrt_tangent.hpp)
  if (c->rebin_every <= 0) return false;
  if (c->kernel == 2) return true;
  return c->kernel == 0 && c->slot[0].nx >= 2 * kTile;
}

// a binning of slot 0's grid into the tile kernel's tiles is in force
bool tile_binned(const swrt_ctx* c) { return use_tile_kernel(c) && c->bin.tiled_for(tiles_per_side(c->slot[0].nx)); }

// the packet step is the leapfrog step (swrt_set_integrator's default)
bool default_integrator(const swrt_ctx* c) { return c->integ_kick == 0 && c->integ_comp == 0; }

// Stage weights w and blend offsets off (in steps) of a composition: 0 none,
// 1 Yoshida's triple jump, 2 Suzuki's five stages; the stage count, or 0 for
// an unknown composition.  The literals are 1/(2 - 2^(1/3)) and
// 1/(4 - 4^(1/3)) to within an ulp, as constants rather than a cbrt call (the
// remaining weight is formed from them, so the sum is 1 to rounding).  Stage j sits at the midpoint of its
// own share of the step: off_j = (w_1 + .. + w_{j-1}) + w_j/2 - 0.5, summed
// left to right over the first half and mirrored with the opposite sign, the
// middle one exactly 0.  The one place these numbers are made: the kernels
// and swrt_integrator_weights take them from here.
int integrator_stages(int composition, double* w, double* off) {
  int S;
  if (composition == 0) {
    S = 1;
    w[0] = 1.0;
  } else if (composition == 1) {
    const double w1 = 1.3512071919596578;
    S = 3;
    w[0] = w[2] = w1;
    w[1] = 1.0 - 2.0 * w1;
  } else if (composition == 2) {
    const double s = 0.4144907717943757;
    S = 5;
    w[0] = w[1] = w[3] = w[4] = s;
    w[2] = 1.0 - 4.0 * s;
  } else {
    return 0;
  }
  double acc = 0.0;
  for (int j = 0; j < S / 2; ++j) {
    off[j] = (acc + w[j] / 2) - 0.5;
    off[S - 1 - j] = -off[j];
    acc = acc + w[j];
  }
  off[S / 2] = 0.0;
  return S;
}

StageArgs stage_args(const swrt_ctx* c) {
  StageArgs g = {};
  g.kick = c->integ_kick;
  g.iters = c->integ_iters;
  g.nstages = integrator_stages(c->integ_comp, g.w, g.off);
  return g;
}

// the intervals of one multi-interval tile launch (swrt_advance_intervals)
struct IvLaunch {
  int nint;
  FieldView views[kMaxIntervals + 1];
  double dts[kMaxIntervals];
  bool div_free;
};

// Launch a packet kernel on the context stream; inside a timed launch the
// start/stop events take the kernel's own begin/end timestamps.
template <typename F, typename... Args>
void launch_k(swrt_ctx* c, F kernel, dim3 grid, dim3 block, Args... args) {
  hipEvent_t stop = c->kev1 ? c->kev1 : (slot_events(c) ? c->use_ev.get() : nullptr);
  hipExtLaunchKernelGGL(kernel, grid, block, 0, c->stream, c->kev0, stop, 0, args...);
  c->tail_ev = stop;
}

// Ensembles below this run every tile launch on one stream: the split's
// fork/join costs more than the overlap returns (profiles/r03_streams_ab:
// 3e4 packets 3.0 vs 3.4e9, 1e4 at 256^2 1.8 vs 2.8e9; 6.25e4 even; 1.25e5
// +3 %, 2.5e5 +6 %, 5e5 +4 %, 1e6 +3.7 %).
constexpr int64_t kMultiStreamFrom = 65536;

// The LDS-tiled launch of TileArgs t: one launch over every tile, or (two
// packet streams) two part launches, each a share of every XCD band's tiles
// (swrt_share.hpp), the second on the extra stream after everything queued
// on the packet stream so far (this call's re-binning, memsets and history
// growth).  A timed pair brackets the first part's start and the last
// part's end.
//
// Hazard checker: the accesses of the launch's parts (part p on stream p),
// forked from the packet stream when split, each over the band slots its
// workgroups take — enumerated with the device's own mapping (share_slot),
// so a launch whose tile-to-stream mapping differs from the previous
// launch's is seen to touch the other stream's tiles.  Checked on a copy of
// the checker state, committed only if every access is ordered: a hazard
// refuses the launch before anything is queued.
int hz_tile_launch(swrt_ctx* c, const TileArgs& t, const TileShare* parts, int nparts, bool zero_counts,
                   bool fork = true) {
  HazardChecker h = c->hz;
  if (zero_counts) {  // the next-binning counts' memset, on the packet stream before the parts
    const uint64_t tm = h.op(0);
    if (!h.access(0, tm, t.next_counts, kHzWrite, HzRegion::all(), "the next-binning counts' memset"))
      return fail(c, SWRT_ERR_STATE, h.err);
  }
  if (nparts > 1 && fork) {
    h.record(c->fork_ev.get(), 0);
    for (int i = 1; i < nparts; ++i) h.wait(i, c->fork_ev.get());
  }
  const StepArgs& a = t.s;
  for (int p = 0; p < nparts; ++p) {
    const uint64_t tp = h.op(p);
    const HzRegion r = HzRegion::of_share(h.epoch, parts[p]);
    const char* what = t.src ? "a part of the sort launch after a re-binning" : "a part launch";
    // the sort launch after an indirect re-binning gathers its input through
    // src_idx from any slot of the input buffers
    const HzRegion rin = t.src ? HzRegion::all() : r;
    bool ok = h.access(p, tp, a.x, kHzRead, rin, what) && h.access(p, tp, a.k, kHzRead, rin, what) &&
              h.access(p, tp, a.perm, kHzRead, rin, what) && h.access(p, tp, t.src, kHzRead, r, what) &&
              h.access(p, tp, t.starts, kHzRead, HzRegion::all(), what) &&
              h.access(p, tp, t.order, kHzRead, HzRegion::all(), what) &&
              h.access(p, tp, t.x_out, kHzWrite, r, what) && h.access(p, tp, t.k_out, kHzWrite, r, what) &&
              h.access(p, tp, t.perm_out, kHzWrite, r, what) &&
              h.access(p, tp, t.next_keys, kHzWrite, r, what) &&
              h.access(p, tp, t.next_counts, kHzAtomic, HzRegion::all(), what) &&
              h.access(p, tp, a.hist_x, kHzWrite, r, what) && h.access(p, tp, a.hist_k, kHzWrite, r, what);
    if (!ok) return fail(c, SWRT_ERR_STATE, h.err);
  }
  c->hz = std::move(h);
  return SWRT_OK;
}

// zero_counts: clear t.next_counts (the next binning's counts) first, on the
// packet stream — after the hazard check, so a refused launch queues nothing.
int launch_tiles(swrt_ctx* c, void (*kernel)(TileArgs), int nt, TileArgs t, bool zero_counts) {
  const int ntiles = t.ntx * t.ntx;
  const int S = c->n >= kMultiStreamFrom ? c->packet_streams : 1;
  // test-only (SWRT_DEBUG_SHARE_SKEW): the launch that ends a re-binning
  // cycle takes an uneven share — a mapping that differs from the previous
  // launch's, round 4's race; only ever run with the checker on, which
  // refuses it (swrt_debug_set enforces that)
  const bool skew = c->dbg.share_skew && t.next_keys != nullptr;
  if (skew && !c->hz.on) return fail(c, SWRT_ERR_STATE, "the skewed share runs only under the hazard checker");
  const bool multi = S == 2 && c->stream == c->stream0.get() && c->sx[0].get() != nullptr &&
                     (skew ? ntiles % 8 == 0 && ntiles / 8 >= 3 : ntiles % 16 == 0);
  if (!multi) {
    // one launch over every tile on the packet stream: it reads and writes
    // packets that the extra stream's part launch of an earlier call may
    // still be writing
    t.sh = TileShare{ntiles, -1, 1, kShareEven};
    HIPCHK_RC(join_b(c));
    if (c->hz.on) HIPCHK_RC(hz_tile_launch(c, t, &t.sh, 1, zero_counts));
    if (zero_counts) HIPCHK(c, hipMemsetAsync(t.next_counts, 0, sizeof(int) * ntiles, c->stream));
    launch_k(c, kernel, dim3((unsigned)share_grid(t.sh)), dim3(nt), t);
    c->s0_dirty = true;  // every tile on the packet stream
    return SWRT_OK;
  }
  const TileShare sh[2] = {TileShare{ntiles, 0, 2, skew ? kShareSkew : kShareEven},
                           TileShare{ntiles, 1, 2, skew ? kShareSkew : kShareEven}};
  // the fork: only when the packet stream has had other work since the last
  // split launch (s0_dirty), the counts' memset included; the hazard checker
  // models exactly the orderings the launch queues
  const bool fork = c->s0_dirty || zero_counts || skew;
  if (c->hz.on) HIPCHK_RC(hz_tile_launch(c, t, sh, 2, zero_counts, fork));
  if (zero_counts) HIPCHK(c, hipMemsetAsync(t.next_counts, 0, sizeof(int) * ntiles, c->stream));
  // Part p takes the same slots at every launch of a binning (the product
  // rule, kShareEven): a stream's consecutive part launches own the same
  // tiles, so stream order alone orders them, and stream 0's next launch may
  // start while stream 1's previous one still runs.  A launch with another
  // mapping races it unless joined first — the checker, which enumerates the
  // slots each part takes, refuses it (round 4's hang, profiles/r04_stream_split).
  if (fork) {
    HIPCHK(c, hipEventRecord(c->fork_ev.get(), c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->sx[0].get(), c->fork_ev.get(), 0));
  }
  c->s0_dirty = false;
  t.sh = sh[0];
  hipExtLaunchKernelGGL(kernel, dim3((unsigned)share_grid(sh[0])), dim3(nt), 0, c->stream, c->kev0, nullptr, 0, t);
  if (c->dbg.spin_us > 0)
    hipLaunchKernelGGL(debug_spin_kernel, dim3(1), dim3(64), 0, c->sx[0].get(), (c->dbg.spin_us + 3) / 4);
  t.sh = sh[1];
  hipExtLaunchKernelGGL(kernel, dim3((unsigned)share_grid(sh[1])), dim3(nt), 0, c->sx[0].get(), nullptr, c->kev1, 0, t);
  c->b_pending = 1;
  c->tail_ev = nullptr;  // slot uses are marked after the join (swrt_advance)
  return SWRT_OK;
}

// The sparse-tile launch shape (kSparseThreads threads, prefetch depth
// kSparsePrefetch) for the two-snapshot five-sum launches over `ntiles` tiles.
bool sparse_tiles(const swrt_ctx* c, int64_t ntiles) {
  if (!default_integrator(c)) return false;  // the staged step has the dense shape only
  if (c->sparse_mode == 1) return false;
  if (c->sparse_mode == 2) return true;
  return c->n < (int64_t)kSparseBelow * ntiles;
}

// Threads per workgroup of the LDS-tiled leapfrog launch over `ntiles` tiles
// of snapshots that are (v5) two divergence-free slots: ONE decision for the
// launch (tile_launch) and for the re-binning's longest-first tile order,
// which ranks tiles by the rounds of this many lanes their workgroup runs.
int tile_threads(const swrt_ctx* c, bool v5_two, int64_t ntiles) {
  return v5_two && sparse_tiles(c, ntiles) ? kSparseThreads : kTileThreads;
}

// slots sa .. sa+nslots-1 are two divergence-free snapshots (the five-sum kernels)
bool two_v5(const swrt_ctx* c, int nslots, int sa) {
  bool v5 = nslots >= 2;
  for (int i = 0; i < nslots && v5; ++i) v5 = c->slot[sa + i].div_free;
  return v5;
}

int tile_cells(const swrt_ctx* c, int64_t nx) {
  if (use_tile_kernel(c)) return kTile;
  if (c->tile > 0) return (int)std::min<int64_t>(c->tile, nx);
  // default: 8x8-cell tiles, coarser on big grids so bins stay <= 4096
  int t = 8;
  while ((nx + t - 1) / t > 64) t *= 2;
  return t;
}

// the per-packet leapfrog kernel blending `nslots` snapshots
using LeapKernel = void (*)(StepArgs);
LeapKernel leap_kernel(int nslots) { return nslots == 2 ? leapfrog_kernel<true> : leapfrog_kernel<false>; }
// ... and its staged form (swrt_set_integrator)
using LeapStageKernel = void (*)(StepArgs, StageArgs);
LeapStageKernel leap_stage_kernel(int nslots) {
  return nslots == 2 ? leapfrog_stage_kernel<true> : leapfrog_stage_kernel<false>;
}
// ... and the form that carries the tangent map (swrt_tangent_begin)
using LeapTangentKernel = void (*)(StepArgs, TangentArgs);
LeapTangentKernel leap_tangent_kernel(int nslots) {
  return nslots == 2 ? leapfrog_tangent_kernel<true> : leapfrog_tangent_kernel<false>;
}
TangentArgs tangent_args(const swrt_ctx* c) { return TangentArgs{c->tan.M.get(), c->tan.caustics.get()}; }

// The leapfrog calls' check while a tangent set is live: M is the derivative
// of the default step with its mul-then-add sums.
int tangent_step_check(swrt_ctx* c) {
  if (!c->tan.live) return SWRT_OK;
  if (!default_integrator(c))
    return fail(c, SWRT_ERR_ARG,
                "a tangent set is live: the tangent map has the leapfrog step only (set the integrator back to "
                "(0, 1, 0) or call swrt_tangent_end)");
  if (c->gather_mode == 1)
    return fail(c, SWRT_ERR_ARG,
                "a tangent set is live: the tangent map has the mul-then-add gather only (set the gather mode to 0 "
                "or call swrt_tangent_end)");
  return SWRT_OK;
}

// The calls that move packets some other way, while a tangent set is live.
int tangent_refuse(swrt_ctx* c, const char* call) {
  if (!c->tan.live) return SWRT_OK;
  return fail(c, SWRT_ERR_STATE,
              std::string(call) + ": a tangent set is live and this call would move packets without their tangent "
                                  "maps (swrt_tangent_end first)");
}

// Counting-sort the packets by spatial tile of slot 0's grid (swrt_bin.hpp).
// indirect: only build the source index of the binned order (c->src_idx);
// the tile launch that follows reads through it and writes the packets in
// binned order (saves moving 36 B per packet twice).  Callers other than the
// leapfrog loop need the packets moved (indirect = false).  lanes: the
// workgroup width of the launches this binning serves (tile_threads), by
// which the scan ranks the tile order.
int rebin(swrt_ctx* c, bool indirect, int tile = 0, int lanes = kTileThreads) {
  if (int rc = join_b(c)) return rc;  // the second stream's half launches wrote packets this pass reads
  c->s0_dirty = true;  // a new binning: the next split launch forks
  const Slot& s = c->slot[0];
  const FieldView v = view_of(s);
  BinGeom g;
  g.dx = v.dx; g.px = v.px; g.py = v.py; g.inv_px = v.inv_px; g.inv_py = v.inv_py; g.inv_dx = v.inv_dx;
  g.nx = v.nx;
  g.tile = tile > 0 ? tile : tile_cells(c, s.nx);
  g.ntx = (int)((s.nx + g.tile - 1) / g.tile);  // (any tile size: not tiles_per_side)
  const int nbins = g.ntx * g.ntx;
  if (nbins > kMaxBins) return fail(c, SWRT_ERR_ARG, "too many spatial bins (raise tile size)");
  const int64_t n = c->n;
  const unsigned grid = nblocks(n, 256 * kBinPerThread);
  const bool keys_valid = c->bin.keys_valid_for(nbins, v.nx, v.dx);
  const PacketSet &in = c->pk.cur, &out = c->pk.out;
  if (c->hz.on) {  // count, scan and scatter on the packet stream
    HazardChecker& h = c->hz;
    const uint64_t t = h.op(0);
    const char* what = "a re-binning";
    const bool ok =
        hz_whole(h, t, kHzRead, what, {in.x.get(), in.k.get(), in.perm.get()}) &&
        hz_whole(h, t, keys_valid ? kHzRead : kHzWrite, what, {c->keys.get()}) &&
        hz_whole(h, t, kHzWrite, what, {c->bins.counts(), c->bins.cursor(), c->bins.starts(), c->bins.tile_order()}) &&
        (indirect ? hz_whole(h, t, kHzWrite, what, {c->src_idx.get()})
                  : hz_whole(h, t, kHzWrite, what, {out.x.get(), out.k.get(), out.perm.get()}));
    if (!ok) return fail(c, SWRT_ERR_STATE, h.err);
    ++h.epoch;  // a new partition of the packets into tiles
  }
  if (!keys_valid) {
    // (no memset at every second ode23 interval's re-binning: profiles/r06_ode23/README.md)
    if (c->bin.needs_count_memset(nbins))
      HIPCHK(c, hipMemsetAsync(c->bins.counts(), 0, sizeof(int) * nbins, c->stream));
    hipLaunchKernelGGL(bin_count_kernel, dim3(grid), dim3(256), sizeof(int) * nbins, c->stream, g, in.x.get(), n,
                       nbins, c->keys.get(), c->bins.counts());
    HIPCHK(c, hipGetLastError());
  }
  if (c->dbg.corrupt_count != 0) {  // test-only: one corrupted count, once
    hipLaunchKernelGGL(debug_corrupt_count_kernel, dim3(1), dim3(64), 0, c->stream, c->bins.counts(), nbins / 2,
                       c->dbg.corrupt_count);
    c->dbg.corrupt_count = 0;
  }
  hipLaunchKernelGGL(bin_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->bins.counts(), nbins, c->bins.cursor(),
                     c->bins.starts(), n, c->dev_err.dev(), c->bins.tile_order(), lanes);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(indirect ? bin_scatter_kernel<true> : bin_scatter_kernel<false>, dim3(grid), dim3(256),
                     2 * sizeof(int) * nbins, c->stream, in.x.get(), in.k.get(), in.perm.get(), c->keys.get(), n, nbins,
                     c->bins.cursor(), out.x.get(), out.k.get(), out.perm.get(), indirect ? c->src_idx.get() : nullptr);
  HIPCHK(c, hipGetLastError());
  if (!indirect) c->pk.flip();  // (the packets were moved)
  c->bin.rebinned(nbins, g.tile, lanes, indirect);
  return SWRT_OK;
}

// The LDS-tiled leapfrog kernel and its workgroup width: two blended snapshots
// or one, divergence-free (v5: the five-sum gather), its sums as fused
// multiply-adds (v5 only), the sparse launch shape (two v5 snapshots only).
// Each in two forms: plain (X = false: no history frames, one interval) and
// everything on (X = true), for calls that write history frames or run
// several intervals.
struct TileKernel { void (*fn)(TileArgs); int threads; };
template <bool X>
TileKernel tile_kernel_of(bool two, bool v5, bool fma, bool sparse) {
  constexpr int T = kTile, M = kMargin, NT = kTileThreads, ST = kSparseThreads, PF = kSparsePrefetch;
  constexpr int MW = kSparseMinWaves, W4 = SWRT_TILE_MIN_WAVES;
  if (two && v5 && sparse)
    return {fma ? tile_leapfrog_kernel<true, T, M, ST, true, true, PF, MW, X, X>
                : tile_leapfrog_kernel<true, T, M, ST, true, false, PF, MW, X, X>, ST};
  if (two && v5)
    return {fma ? tile_leapfrog_kernel<true, T, M, NT, true, true, 1, W4, X, X>
                : tile_leapfrog_kernel<true, T, M, NT, true, false, 1, W4, X, X>, NT};
  if (two) return {tile_leapfrog_kernel<true, T, M, NT, false, false, 1, W4, X, X>, NT};
  if (v5)
    return {fma ? tile_leapfrog_kernel<false, T, M, NT, true, true, 1, W4, X, X>
                : tile_leapfrog_kernel<false, T, M, NT, true, false, 1, W4, X, X>, NT};
  return {tile_leapfrog_kernel<false, T, M, NT, false, false, 1, W4, X, X>, NT};
}
TileKernel tile_kernel_of(bool two, bool v5, bool fma, bool sparse, bool hist, bool multi) {
  return hist || multi ? tile_kernel_of<true>(two, v5, fma, sparse) : tile_kernel_of<false>(two, v5, fma, sparse);
}
// The staged step (swrt_set_integrator): the general form in the dense shape, mul-then-add sums.
TileKernel tile_stage_kernel_of(bool two, bool v5) {
  constexpr int T = kTile, M = kMargin, NT = kTileThreads, W4 = SWRT_TILE_MIN_WAVES;
  if (two)
    return {v5 ? tile_leapfrog_kernel<true, T, M, NT, true, false, 1, W4, true, true, true>
               : tile_leapfrog_kernel<true, T, M, NT, false, false, 1, W4, true, true, true>, NT};
  return {v5 ? tile_leapfrog_kernel<false, T, M, NT, true, false, 1, W4, true, true, true>
             : tile_leapfrog_kernel<false, T, M, NT, false, false, 1, W4, true, true, true>, NT};
}

int tile_launch(swrt_ctx* c, const StepArgs& a, bool count_next, const IvLaunch* iv = nullptr) {
  TileArgs t;
  t.s = a;
  t.ivmode = iv != nullptr;
  t.nint = iv ? iv->nint : 1;
  if (iv) {
    for (int i = 0; i <= iv->nint; ++i) t.ivn[i] = iv->views[i].nodes;
    for (int i = 0; i < iv->nint; ++i) t.ivdt[i] = iv->dts[i];
  }
  t.stg = stage_args(c);
  t.x_out = c->pk.out.x.get();
  t.k_out = c->pk.out.k.get();
  t.perm_out = c->pk.out.perm.get();
  t.starts = c->bins.starts();
  t.order = c->bins.tile_order();
  if (c->bin.tile() != kTile) return fail(c, SWRT_ERR_STATE, "the binning is not the LDS-tiled kernel's");
  t.ntx = tiles_per_side(a.f0.nx);
  const int ntiles = t.ntx * t.ntx;
  t.next_keys = nullptr;
  t.next_counts = nullptr;
  t.sort_cells = c->bin.cells_sorted() ? 0 : 1;
  t.src = nullptr;
  // sort keys lead by half the steps until the next sort (swrt_tile.hpp)
  t.sort_lead = c->sort_lead ? 0.5 * a.dt * (double)std::max<int64_t>(1, c->rebin_every) : 0.0;
  if (c->bin.src_pending()) {  // first launch after an indirect re-binning (always a sort launch)
    t.src = c->src_idx.get();
    t.sort_cells = 1;
  }
  bool zero = false;  // the counts' memset, queued by launch_tiles after its hazard check
  if (count_next && ntiles == c->bin.nbins()) {
    zero = !c->bin.counts_zero();
    t.next_keys = c->keys.get();
    t.next_counts = c->bins.counts();
  }
  const bool two = a.nslots == 2;
  const bool v5 = two ? (iv ? iv->div_free : two_v5(c, 2, 0)) : c->slot[0].div_free;
  const TileKernel tk = !default_integrator(c)
                            ? tile_stage_kernel_of(two, v5)
                            : tile_kernel_of(two, v5, c->gather_mode == 1,
                                             two && v5 && tile_threads(c, true, ntiles) == kSparseThreads,
                                             a.hist_x != nullptr, iv != nullptr);
  HIPCHK_RC(launch_tiles(c, tk.fn, tk.threads, t, zero));
  HIPCHK(c, hipGetLastError());
  // (a.f0: the view this launch bins by; a multi-interval launch: slot i0's)
  c->bin.tile_launched(t.next_keys != nullptr, a.f0.nx, a.f0.dx);
  if (t.src != nullptr && c->b_pending && !c->dbg.legacy_park) {
    // The first launch after an indirect re-binning reads its input through
    // src_idx from any slot of the packets while its parts run on two streams;
    // the next launch's parts would overwrite them at their own tiles' slots
    // before the other part has read them.  The next launches write the third
    // set instead and the old packets are parked there until the next
    // re-binning (which orders every stream's work first).
    c->pk.park_cur();
  } else {
    c->pk.flip();
  }
  return SWRT_OK;
}

// The per-packet leapfrog launch (packets updated in place on the packet
// stream): order the extra stream's part launches of an earlier call first
// (swrt_set_locality(0, ..) after split launches lands here), and tell the
// hazard checker.
int leap_launch(swrt_ctx* c, const StepArgs& a, unsigned grid) {
  HIPCHK_RC(join_b(c));
  c->s0_dirty = true;
  if (c->hz.on) {
    HazardChecker& h = c->hz;
    const uint64_t t = h.op(0);
    const char* what = "the per-packet leapfrog launch";
    if (!(hz_whole(h, t, kHzWrite, what, {a.x, a.k}) && hz_whole(h, t, kHzRead, what, {a.perm}) &&
          hz_whole(h, t, kHzWrite, what, {a.hist_x, a.hist_k}) &&
          (!c->tan.live || hz_whole(h, t, kHzWrite, what, {c->tan.M.get(), c->tan.caustics.get()}))))
      return fail(c, SWRT_ERR_STATE, h.err);
  }
  c->bin.per_packet_launched();
  if (c->tan.live) {  // (tangent_step_check: the default step)
    launch_k(c, leap_tangent_kernel(a.nslots), dim3(grid), dim3(256), a, tangent_args(c));
  } else if (!default_integrator(c)) {
    launch_k(c, leap_stage_kernel(a.nslots), dim3(grid), dim3(256), a, stage_args(c));
  } else if (c->kev1) {  // a timed launch: the dispatch stamps the events
    launch_k(c, leap_kernel(a.nslots), dim3(grid), dim3(256), a);
  } else {
    hipLaunchKernelGGL(leap_kernel(a.nslots), dim3(grid), dim3(256), 0, c->stream, a);
    c->tail_ev = nullptr;
  }
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}

// Time every timing_every-th leapfrog launch with a pair of HIP events.
int timed_launch(swrt_ctx* c, const StepArgs& a, unsigned grid, bool count_next, const IvLaunch* iv = nullptr) {
  const bool timed = c->timing_every > 0 && (c->launch_count++ % c->timing_every) == 0;
  const auto launch = [&] { return use_tile_kernel(c) ? tile_launch(c, a, count_next, iv) : leap_launch(c, a, grid); };
  if (!timed) return launch();
  // timing events (pairs), grown on demand; fold into a running sum when full
  if (c->timing.used + 2 > kMaxEvents) {
    if (int rc = sync_sx(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i + 1 < c->timing.used; i += 2) {
      float ms = 0.f;
      HIPCHK(c, hipEventElapsedTime(&ms, c->timing.ev[i].get(), c->timing.ev[i + 1].get()));
      c->timing.folded_ms += ms;
      c->timing.folded_n += 1;
    }
    c->timing.used = 0;
  }
  if (c->timing.used + 2 > c->timing.ev.size()) {
    for (int e = 0; e < 64; ++e) {
      Event ev;
      HIPCHK(c, ev.create(hipEventDefault));
      c->timing.ev.push_back(std::move(ev));
    }
  }
  c->kev0 = c->timing.ev[c->timing.used].get();
  c->kev1 = c->timing.ev[c->timing.used + 1].get();
  c->timing.used += 2;
  const int rc = launch();
  c->kev0 = c->kev1 = nullptr;
  return rc;
}

// the re-binning of a leapfrog call over slots sa .. sa+nslots-1, when due
int leap_rebin_if_due(swrt_ctx* c, int nslots, int sa) {
  if (c->rebin_every <= 0) return SWRT_OK;
  const bool tiled = use_tile_kernel(c);
  const int64_t ntx = tiles_per_side(c->slot[sa].nx), ntiles = tiled ? ntx * ntx : 0;
  const int lanes = tiled ? tile_threads(c, two_v5(c, nslots, sa), ntiles) : kTileThreads;
  if (c->bin.due(c->rebin_every) || (tiled && (c->bin.tile() != kTile || c->bin.lanes() != lanes)))
    return rebin(c, tiled, tiled ? kTile : 0, lanes);
  return SWRT_OK;
}

// the arguments every launch of an advance call shares (history frames from the current one)
StepArgs step_args(swrt_ctx* c, const FieldView& f0, const FieldView& f1, int nslots, double dt, double f, double gH,
                   double alpha0, double dalpha, double bump, int64_t save_every) {
  StepArgs a;
  a.f0 = f0;
  a.f1 = f1;
  a.nslots = nslots;
  a.n = c->n;
  a.dt = dt;
  a.half = dt / 2;
  a.f2 = f * f;
  a.fastdisp = dispersion_fast(a.f2);
  a.gH = gH;
  a.alpha0 = alpha0;
  a.dalpha = dalpha;
  a.bump = bump;
  a.save_every = save_every > 0 ? save_every : 1;
  a.hist_x = save_every > 0 ? c->hist.a.get() : nullptr;
  a.hist_k = save_every > 0 ? c->hist.b.get() : nullptr;
  a.frame0 = c->hist.ext.frames();
  return a;
}

// One leapfrog launch over the current packets, nsteps steps (iv: per interval) from step s0, `steps` in all.
// The launch that ends at a re-binning point also counts the next bins.
int advance_launch(swrt_ctx* c, StepArgs& a, int64_t s0, int64_t nsteps, int64_t steps, const IvLaunch* iv = nullptr) {
  a.x = c->pk.cur.x.get();
  a.k = c->pk.cur.k.get();
  a.perm = c->pk.cur.perm.get();
  a.s0 = s0;
  a.nsteps = (int)nsteps;
  const bool count_next = c->rebin_every > 0 && steps >= c->bin.steps_left(c->rebin_every);
  slot_writes_wait(c);  // after the re-binning: it reads no slot
  HIPCHK_RC(timed_launch(c, a, nblocks(c->n, 256), count_next, iv));
  c->bin.stepped(steps);
  return SWRT_OK;
}

int run_advance(swrt_ctx* c, double dt, int64_t nsteps, double f, double gH, int nslots,
                double alpha0, double dalpha, double bump, int64_t save_every, int sa = 0) {
  const FieldView f0 = view_of(c->slot[sa]);
  StepArgs a = step_args(c, f0, nslots == 2 ? view_of(c->slot[sa + 1]) : f0, nslots, dt, f, gH, alpha0, dalpha, bump,
                         save_every);
  int64_t s0 = 0;
  while (s0 < nsteps) {
    int64_t chunk = std::min<int64_t>(kMaxStepsPerLaunch, nsteps - s0);
    HIPCHK_RC(leap_rebin_if_due(c, nslots, sa));
    if (c->rebin_every > 0) chunk = std::min<int64_t>(chunk, c->bin.steps_left(c->rebin_every));
    HIPCHK_RC(advance_launch(c, a, s0, chunk, chunk));
    s0 += chunk;
  }
  return SWRT_OK;
}

// nint PDE intervals of nsub steps each, interval i blending slots i, i+1 at
// step size hs[i]: whole intervals per tile launch (up to kMaxIntervals, never
// across a re-binning), else one interval at a time through run_advance.
int run_advance_intervals(swrt_ctx* c, int nint, const double* hs, int64_t nsub, double f, double gH,
                          double alpha0, double dalpha, double bump, int64_t save_every) {
  const bool fused = use_tile_kernel(c) && c->rebin_every > 0 && c->rebin_every % nsub == 0 &&
                     nsub <= kMaxStepsPerLaunch;
  const int64_t fpi = save_every > 0 ? nsub / save_every : 0;  // frames per interval
  int i0 = 0;
  while (i0 < nint) {
    int k = 0;
    if (fused) {
      HIPCHK_RC(leap_rebin_if_due(c, std::min(nint - i0, kMaxIntervals) + 1, i0));
      k = (int)std::min<int64_t>({(int64_t)(nint - i0), c->bin.steps_left(c->rebin_every) / nsub,
                                  (int64_t)kMaxIntervals});
    }
    if (k < 1) {  // one interval on its own (it may straddle a re-binning)
      HIPCHK_RC(run_advance(c, hs[i0], nsub, f, gH, 2, alpha0, dalpha, bump, save_every, i0));
      c->hist.ext.committed(fpi);
      i0 += 1;
      continue;
    }
    IvLaunch iv;
    iv.nint = k;
    iv.div_free = true;
    for (int i = 0; i <= k; ++i) {
      iv.views[i] = view_of(c->slot[i0 + i]);
      iv.div_free = iv.div_free && c->slot[i0 + i].div_free;
    }
    for (int i = 0; i < k; ++i) iv.dts[i] = hs[i0 + i];
    StepArgs a = step_args(c, iv.views[0], iv.views[1], 2, hs[i0], f, gH, alpha0, dalpha, bump, save_every);
    HIPCHK_RC(advance_launch(c, a, 0, nsub, k * nsub, &iv));
    c->hist.ext.committed(k * fpi);
    i0 += k;
  }
  return SWRT_OK;
}

// Room for new_frames more history frames of the current ensemble (2 x n
// doubles in each column; SeriesExtent keeps the capacity right when n changes).
int ensure_history(swrt_ctx* c, int64_t new_frames) {
  const int64_t per = 2 * c->n;
  if (c->hist.ext.fits(new_frames, per)) return SWRT_OK;
  if (int rc = join_b(c)) return rc;  // the second stream may still write frames into the old buffers
  c->s0_dirty = true;
  const double *old_x = c->hist.a.get(), *old_k = c->hist.b.get();
  HIPCHK_RC(series_reserve(c, c->hist, per, per, new_frames, 0, "history allocation failed"));
  if (c->hz.on) {
    c->hz.bufs.erase(old_x);
    c->hz.bufs.erase(old_k);
    c->hz.name(c->hist.a.get(), "history x frames");
    c->hz.name(c->hist.b.get(), "history k frames");
  }
  return SWRT_OK;
}

// the template kernels the wave-action and spectral entry points choose from
// (8- or 16-cell tiles; sums in fp64 or fp32, precision 64 / 32)
auto xka_tile_kernel_of(int tile) {
  return tile == 8 ? xka_tile_kernel<8, kXkaMargin, 256> : xka_tile_kernel<16, kXkaMargin, 256>;
}
auto spectral_eval_kernel_of(int precision) {
  return precision == 64 ? spectral_eval_kernel<double> : spectral_eval_kernel<float>;
}
auto spectral_leapfrog_kernel_of(int precision) {
  return precision == 64 ? spectral_leapfrog_kernel<double> : spectral_leapfrog_kernel<float>;
}
}  // namespace
