// swrt_ctx.hpp — the context behind the C ABI (include/swrt.h): the tuning
// constants, each subsystem's state (the handles of swrt_res.hpp own every GPU
// resource), swrt_ctx, the entry points' error/guard macros, the
// cross-stream ordering helpers and the one reserve / get / release of every
// device-side frame series.  Internal to swrt_api.hip, the library's one
// HIP translation unit, like the swrt_host_*.hpp headers that build on it.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "../../include/swrt.h"
#include "swrt_bin.hpp"
#include "swrt_kernels.hpp"
#include "swrt_qg.hpp"
#include "swrt_spectral.hpp"
#include "swrt_hazard.hpp"
#include "swrt_map.hpp"
#include "swrt_kmap.hpp"
#include "swrt_flowspec.hpp"
#include "swrt_ode23_ctl.hpp"
#include "swrt_res.hpp"
#include "swrt_packet_state.hpp"

using namespace swrt;

namespace {

constexpr int kMaxStepsPerLaunch = 64;  // bound one launch's run time
// a host copy of an attempt workgroup's error max not yet written (no max of
// non-negative doubles, NaN included, has this bit pattern)
constexpr unsigned long long kHpartEmpty = ~0ull;
constexpr int kXkaMargin = 3;           // xka_tile_kernel: drift margin (cells) of a tile's window
#ifndef SWRT_TILE
#define SWRT_TILE 16
#endif
#ifndef SWRT_MARGIN
#define SWRT_MARGIN 3
#endif
#ifndef SWRT_SORT_LEAD
#define SWRT_SORT_LEAD 1
#endif
#ifndef SWRT_TILE_THREADS
#define SWRT_TILE_THREADS 512
#endif
constexpr int kTile = SWRT_TILE;                // LDS tile kernel: cells per tile side
constexpr int kMargin = SWRT_MARGIN;            // LDS tile kernel: drift margin (cells)
constexpr int kTileThreads = SWRT_TILE_THREADS;
inline int tiles_per_side(int64_t nx) { return (int)((nx + kTile - 1) / kTile); }  // of the LDS tile kernel
// Sparse-tile launches: below SWRT_SPARSE_BELOW packets per 16x16 tile on
// average (a strong-scaling shard: ~120 at 1.25e5 packets on 512^2) a
// 512-thread workgroup has one or two busy waves, one per SIMD, each capped
// at 128 VGPRs by the dense launch's 4-waves-per-SIMD budget and waiting on
// LDS reads issued one tap earlier, and its idle waves hold their registers
// until the workgroup ends.  The sparse form is the same kernel with 256
// threads per workgroup, a 256-VGPR budget and the gather's reads issued
// three taps ahead (gather5_lds PF): same arithmetic, same bits.  Packets
// alone it measured the same as the dense shape at 1.25e5 and 2.5e5 and 4 %
// slower at 5e5 (profiles/r04_v1/ab_*.json); beside the replicated PDE at
// the 8-GPU shard (1.25e5) the driver step is 2.5 % shorter, the PDE's
// kernels finding the slots the idle waves no longer hold
// (profiles/r04_sparse_driver): on below 192 packets per tile (1.25e5 on
// 512^2, not 2.5e5).
#ifndef SWRT_SPARSE_BELOW
#define SWRT_SPARSE_BELOW 192
#endif
constexpr int kSparseBelow = SWRT_SPARSE_BELOW;
#ifndef SWRT_SPARSE_THREADS
#define SWRT_SPARSE_THREADS 256
#endif
#ifndef SWRT_SPARSE_PREFETCH
#define SWRT_SPARSE_PREFETCH 3
#endif
#ifndef SWRT_SPARSE_MINW
#define SWRT_SPARSE_MINW 2
#endif
constexpr int kSparseThreads = SWRT_SPARSE_THREADS;
constexpr int kSparsePrefetch = SWRT_SPARSE_PREFETCH;
constexpr int kSparseMinWaves = SWRT_SPARSE_MINW;  // waves per SIMD the sparse shape's registers are sized for

// one set of packet buffers (device order = spatially binned; perm maps to the original index)
struct PacketSet {
  DevBuf<double> x, k;  // 2N each
  DevBuf<int> perm;     // N
  hipError_t alloc(size_t n) {
    if (hipError_t e = x.alloc(2 * n); e != hipSuccess) return e;
    if (hipError_t e = k.alloc(2 * n); e != hipSuccess) return e;
    return perm.alloc(n);
  }
};

// the binning's four device arrays, one allocation
struct BinArrays {
  DevBuf<int> buf;  // counts | cursor | starts (kMaxBins + 1) | tile order
  hipError_t alloc() { return buf.alloc(4 * kMaxBins + 1); }
  int* at(int off) const { return buf ? buf.get() + off : nullptr; }
  int* counts() const { return at(0); }
  int* cursor() const { return at(kMaxBins); }
  int* starts() const { return at(2 * kMaxBins); }
  // longest-first tile order of the LDS-tiled launches (every re-binning's bin_scan_kernel writes it)
  int* tile_order() const { return at(3 * kMaxBins + 1); }
};

struct Slot {
  DevBuf<double> nodes;     // padded interleaved records
  DevBuf<double> psi;       // filtered psi plane (swrt_set_field_psi)
  int64_t nx = 0;
  int64_t npad = 0;
  int64_t ny_period = 0;
  double L = 0.0;
  bool set = false;
  bool has_psi = false;
  bool div_free = false;    // every node's v_y is exactly -u_x (five-sum kernels apply)
  uint64_t wgen = 0;        // write generation: a new value at every write of the nodes (ctx slot_wgen)
  // cross-stream order (they travel with the buffers through swaps and renames):
  Event uev;                 // last context-stream use (packet kernels, field writes)
  hipEvent_t uref = nullptr; // the event that marks that use (not owned): uev, or the stop event attached to
                             // the call's last packet launch (context-wide, re-recorded by later
                             // launches: waiting on it waits for a later point, never an earlier one)
  Event wev;                 // last QG-stream write (swrt_qg_snapshot)
  bool upend = false, wpend = false;
};

// device-resident QG PDE state (swrt_qg.hpp)
struct QGState {
  bool init = false;
  QGDev g{};
  int64_t nhalf = 0, nn = 0;
  DevBuf<double2> qk;       // nl * nhalf
  DevBuf<double2> qk_prev;  // prev_qk of the last step
  DevBuf<double2> Qm1;      // Qn_minus(:,:,1) / (:,:,:,1)
  DevBuf<double2> Qm2;
  DevBuf<double2> E1;       // expLdt  (2 layers): 4 per wavenumber
  DevBuf<double2> E2;       // expL2dt
  DevBuf<double2> Z;        // max(2*nl, 3) * nn transform scratch
  DevBuf<double2> T;
  DevBuf<unsigned long long> dmax;
  // The CFL read-back (dmax -> pinned host memory + an event): a FIFO of two,
  // so a speculative step's speed can be queued behind the committed one's.
  HostBuf<double> hmax;        // pinned host copies of dmax, two slots
  Event ev;                    // recorded after the copy into hmax[0]
  Event ev_b;                  // ... into hmax[1]
  int sp_head = 0;             // slot of the next read-back
  int sp_count = 0;            // read-backs pending (0..2), the oldest at (sp_head - sp_count) & 1
  // Speculative step (swrt_qg_step_speculative): computed into the spare
  // buffers from the committed state, which stays untouched until
  // swrt_qg_resolve accepts it (handle swaps) or drops it.
  DevBuf<double2> qk_spare;
  DevBuf<double2> Qm1_spare;
  DevBuf<double2> Qm2_spare;
  bool spec = false;
  double spec_dt = 0.0, spec_t = 0.0;
  int64_t spec_steps = 0;
  const double2* post_of = nullptr;  // the qk whose post-step transforms PZ/PT hold (not owned)
  bool post_jrows = false;     // phase 1 ran fft_cols_jacobian2_kernel: J's first forward pass is in PT[0, nn)
  const double2* Fj = nullptr; // where qg_post left the spectrum of J (the update's input; not owned)
  bool Fj_rows = false;        // Fj is J after its first forward pass only: the update runs the last
                               // (qg_update_cols_kernel) and renames the tendency history
  bool spec_rot = false;       // the pending speculative step stored only its tendency (Qm1_spare)
  bool spec_rb = false;        // the pending speculative step's CFL read-back is still queued (not popped by
                               // swrt_qg_max_speed_result): a reject drops it only then
  int spec_rb_slot = 0;        // ... its FIFO slot
  // fused mode: the post-step transforms of the current qk — the next step's
  // Jacobian spectrum (PT[0, nn) after its forward FFT), the CFL speed
  // (dmax) and layer 0's grid_U (the snapshot) — from ONE batched inverse
  // 2-D FFT, computed once per qk on first use
  DevBuf<double2> PZ;
  DevBuf<double2> PT;
  bool post_valid = false;      // both phases of qg_post done for post_of (valid for the current qk when
  bool post_inv_valid = false;  // post_of == qk); post_inv_valid: its first phase (the inverse transforms)
  double exp_dt = -1.0;        // dt of the current E1/E2
  int64_t steps = 0;
  double t = 0.0;
  bool has_prev = false;
};

struct Timing {
  std::vector<Event> ev;       // pairs
  size_t used = 0;             // events used (2 per launch)
  double folded_ms = 0.0;      // elapsed of pairs already folded (ring recycled)
  int64_t folded_n = 0;
};
constexpr size_t kMaxEvents = 2048;

// wave-action (step_packet_xka) background and state
struct XkaState {
  DevBuf<double> nodes;
  int64_t nx = 0;
  double dx = 0.0, dy = 0.0;
  DevBuf<double> state;   // 5n
  DevBuf<double> state2;  // 5n: the state in binned order
  DevBuf<int> keys;       // n
  DevBuf<int> src;        // n: binned slot -> packet
  DevBuf<int> src2;       // n: a re-binning's slot -> previous slot
  DevBuf<int> perm2;      // n: composed permutation (ping-pong with src)
  DevBuf<int> bins;       // counts | cursor | starts of the xka binning
  int64_t cap = 0;
  DevBuf<double> hist;
  int64_t hcap = 0;  // doubles allocated
};

// exact spectral evaluator (dense coefficient grid)
struct SpectralState {
  DevBuf<double2> modes;
  DevBuf<int2> rows;
  int64_t cap = 0;
  int64_t rows_cap = 0;
  DevBuf<double2> modes_d;  // group-padded spans (ModeGrid::Cd)
  DevBuf<int> modes_d_row;
  DevBuf<float4> modes_f;   // fp32 packed-pair copy (ModeGrid::Cf)
  DevBuf<int> modes_f_row;
  int64_t modes_f_cap = 0;  // float4 allocated
  int64_t modes_f_rcap = 0;
  ModeGrid mg{};
  bool set = false;
  int64_t active = 0;  // coefficients inside the per-row nonzero spans
};

// ode23 stage buffers (cap-sized, device packet order) and the state of swrt_ode23_run
struct Ode23State {
  DevBuf<double> F[4];
  DevBuf<int> order;         // ode23 tile kernel: in-tile cell order of the binned slots
  int64_t order_cap = 0;
  DevBuf<double> ynx;
  DevBuf<double> ynk;
  // a third state set (x, k, F) for swrt_ode23_run's speculative attempt
  DevBuf<double> spx;
  DevBuf<double> spk;
  DevBuf<double> spF;
  int64_t cap = 0;
  // three max slots used in turn: each ode23 launch zeroes the next one for
  // the next launch (no memset launch between attempts); each is read back
  // through its pinned hmax slot, ev marking the copy
  DevBuf<unsigned long long> dmax;
  int dmax_cur = 0;
  HostBuf<unsigned long long> hmax;
  Event ev[3];
  Event evb[3];  // ... of part 1 (split attempts, on sx[0])
  // swrt_ode23_run's attempts store every workgroup's max here (host-mapped,
  // [part][slot][workgroup], kMaxBins per slot): read after the launch's
  // event, no copy queued between consecutive attempts
  HostBuf<unsigned long long> hpart;
  // swrt_ode23_run's first attempt: its coefficients from the device's own
  // step-size computation (ode23_first_step_kernel), and the host-mapped copy
  // {raw, absh, h, tnew, coefficients} the host checks its computation against
  // (coherent; shown[12]: the launch's ticket, stored after the values)
  DevBuf<double> coef;
  HostBuf<double> shown;
  uint64_t ticket = 0;  // the last first-step launch's ticket
  // the next swrt_ode23_run's stage 1, queued at the end of this one
  // (swrt_ode23_chain_next): armed with the slots the next call reads as its
  // slots 0 / 1; `queued` holds what it was computed from, and any API call
  // that may touch the packets drops it (GUARD_BEGIN)
  struct O23Chain {
    bool want = false;
    int sa = -1, sb = -1;
    bool queued = false;
    int dmax_slot = 0;
    const double* nodes[2] = {nullptr, nullptr};
    uint64_t wgen[2] = {0, 0};
    double alpha = 0.0, f = 0.0, Cg = 0.0, thr = 0.0, bump = 0.0;
    int64_t taken = 0;  // calls that took it (SWRT_DEBUG_ODE23_CHAINED)
    // the next call's first attempt, queued behind its stage 1 from the
    // device's own step size for t0 = 0, tfinal = tmax and `rtol`
    // (ode23_chain_first): its max slot, each part's workgroups, the split
    bool first_q = false;
    int first_slot = -1;
    unsigned first_wg[2] = {0, 0};
    bool split = false;
    uint64_t first_ticket = 0;
    double rtol = 0.0, tfinal = 0.0, tmax = 0.0;
    int64_t first_taken = 0;  // calls that took it (SWRT_DEBUG_ODE23_FIRST_CHAINED)
  } chain;
  // the chained first attempt's part 1 is queued on sx[0] and not joined
  // (b_pending stays 0, so the QG calls between two intervals do not join
  // it): a call that drops the chain, or an ode23 call that does not take the
  // attempt, joins it first (chain_join)
  bool chain_b = false;
  Event chain_ev[2];
  bool chain_first = true;  // SWRT_ODE23_CHAIN_FIRST=0 (environment, A/B runs): stage 1 alone is chained
  O23Stats last;            // the last swrt_ode23_run's controller counts
  int64_t first_taken = 0, guesses_taken = 0;  // ... summed over runs (SWRT_DEBUG_ODE23_*)
  int64_t split_runs = 0;  // runs whose attempts ran as two part launches (SWRT_DEBUG_ODE23_SPLIT_RUNS)
  // output at requested times (swrt_ode23_set_dense / _ntrp / _run_at)
  bool dense = false;        // swrt_ode23_attempt keeps F2 and F3
  bool dense_ready = false;  // y, F1..F4 and ynew of a dense attempt sit in the buffers: until the accept, or
                             // any call that may touch the packets (chain_drop)
  int64_t dense_rebin = 8;   // swrt_ode23_run_at: accepted steps per re-binning (SWRT_DEBUG_ODE23_DENSE_REBIN; 0: none)
  int64_t dense_rebins = 0;  // ... and the re-binnings it made inside runs (SWRT_DEBUG_ODE23_DENSE_REBINS)
};

// swrt_snapshot_qk (snapshots from a half plane another context exported):
// transform scratch, the staged host half plane, the cross-stream events
struct SnapshotImport {
  DevBuf<double2> Z;
  DevBuf<double2> T;
  DevBuf<double2> fk;
  int64_t nx = 0;
  bool init = false;   // slot writes may come from the QG stream (slot_events)
  Event ev[2];
};

// ray diagnostics (swrt_raydiag.hpp): the mark and the recorded frame series.
// Buffers of their own, not the context's scratch: a recorded frame is queued
// without a host wait, and a later call may reallocate the scratch.
struct RayDiagState {
  DevBuf<double> omega0;   // Omega_0 by original packet index (swrt_raydiag_mark)
  DevBuf<double> rec;      // kRayDiagRec doubles per packet, original order: what a sample's reduction reads
  int64_t pcap = 0;        // packets omega0 and rec are sized for
  bool marked = false;
  DevBuf<double> partial;  // kRayDiagStats x kRayDiagBlocks workgroup partials, then one frame
  Series<double> series;   // recorded frames, kRayDiagFrame doubles each (one column)
  void drop() {            // the ensemble changed size: the mark and the series describe another one
    marked = false;
    series.ext.cleared();
  }
};
constexpr int64_t kRayDiagSeriesMin = 4096;  // frames reserved by the mark or the first record (256 KiB)

// the spectrum series (swrt_omega_series_*, swrt_diag.hpp).  Buffers of its
// own, as RayDiagState's.  A frame is self-contained (its n is in its stats),
// so swrt_packets_set with another N keeps the series.
struct OmegaSeriesState {
  bool open = false;        // swrt_omega_series_begin was called
  int nb = 0;               // bins of the open series
  double f2 = 0.0, Cg2 = 0.0;
  DevBuf<double> edges;     // nb + 1
  DevBuf<double> w;         // omega by original packet index
  int64_t pcap = 0;         // packets w is sized for
  DevBuf<double> partial;   // kOmegaHistoryChunk frames x kOmegaPartials x kOmegaBlocks
  Series<unsigned long long, double> series;  // recorded rows, nb + 2 counts each, and their kOmegaStats stats
  size_t row() const { return (size_t)nb + 2; }
};
constexpr int64_t kOmegaSeriesMin = 4096;  // frames reserved by the first record

// the map series (swrt_map_series_*, swrt_map.hpp).  Buffers of its own, as
// OmegaSeriesState's; a frame is self-contained (its n is in its stats).
struct MapSeriesState {
  bool open = false;        // swrt_map_series_begin was called
  int m = 0;                // cells per side of the open series
  int frac_bits = 0;
  double L = 0.0, f2 = 0.0, Cg2 = 0.0;
  Series<unsigned long long> series;  // recorded frames, kMapPlanes x m x m each, and their kMapStats stats
  size_t frame() const { return (size_t)kMapPlanes * m * m; }
  DevBuf<unsigned long long> strays;  // one counter: packets the tile path added through global memory
  int64_t tiled_frames = 0; // frames recorded by the tile path (SWRT_DEBUG_MAP_TILED_FRAMES)
};
// Frames reserved by the first record: 64 MiB worth, at least one, at most 4096.
inline int64_t map_series_min(size_t frame_bytes) {
  return std::min<int64_t>(4096, std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / frame_bytes)));
}

// the wave-vector plane series (swrt_kmap_series_*, swrt_kmap.hpp).  Buffers
// of its own, as MapSeriesState's; a frame is self-contained (its n is in its
// stats), so swrt_packets_set with another N keeps the series.
struct KmapSeriesState {
  bool open = false;        // swrt_kmap_series_begin was called
  int m = 0;                // cells per side of the open series
  int frac_bits = 0;
  double K = 0.0;           // half-width of the plane
  double s = 0.0;           // m / (2K)
  Series<unsigned long long> series;  // recorded frames, m x m counts each, and their kKmapStats stats
  size_t frame() const { return (size_t)m * m; }
};

// the track series (swrt_track_*, swrt_track.hpp): the trajectories of m chosen
// packets.  Buffers of its own, as the other recorders'.  A frame's rows are
// packets of one ensemble, so swrt_packets_set with another N closes it.
struct TrackState {
  bool open = false;           // swrt_track_begin was called
  int64_t m = 0;               // tracked packets
  std::vector<int64_t> ids;    // their original indices, in the caller's order
  DevBuf<int> slot_of;         // n entries: the frame row of an original index, or -1
  DevBuf<int> dids;            // m entries: ids on the device (history frames)
  Series<double> series;       // recorded frames, m x 8 doubles each (one column)
  size_t frame() const { return (size_t)8 * m; }
  void drop() {                // the ensemble changed size: the ids name another one's packets
    open = false;
    m = 0;
    ids.clear();
    series.ext.cleared();
  }
};

// the flow spectrum series (swrt_flow_spectrum_*, swrt_flowspec.hpp): the
// background flow's shell spectra, the one recorder on the PDE side.  Buffers
// of its own, as the other recorders'; its work runs on the QG stream
// (OnQGStream), behind the step that made the qk it reads.
struct FlowSpecState {
  bool open = false;        // swrt_flow_spectrum_begin was called
  int nx = 0;               // grid of the open series
  int nshell = 0;
  double k_scale = 0.0, K_d2 = 0.0;
  DevBuf<double2> stage;    // swrt_flow_spectrum_record_qk's half plane on the device
  Series<double> series;    // recorded frames, 3 x nshell doubles each, and their kFlowSpecStats stats
  size_t frame() const { return (size_t)3 * nshell; }
};

// What the four class-plane series share (swrt_host_diag.hpp's plane_*
// functions work on this part alone).  Buffers of its own, as the other
// recorders'; a frame is self-contained (its n is in its stats), so
// swrt_packets_set with another N keeps the series.  `lay` says what a frame
// holds: (n2 + 2) x (nw + 2) counts in the series' first column, the sums and
// then the stats in its second.
struct PlaneSeriesState {
  bool open = false;        // swrt_*_series_begin was called
  PlaneLayout lay;          // bins of the open series; the sums and stats the series' kernels write
  int frac_bits = 0;
  double f2 = 0.0, Cg2 = 0.0;
  DevBuf<double> edges;     // nw + 1 omega edges, then n2 + 1 edges of the second axis
  DevBuf<double> alphas;    // record_history's alphas, one per frame of the call
  int64_t acap = 0;         // frames alphas is sized for
  bool lds_attr = false;    // the dynamic LDS limit of this series' kernel pair was raised
  Series<unsigned long long> series;  // recorded frames
  PlaneSeriesState(int wsums, int csums, int stats) { lay.wsums = wsums, lay.csums = csums, lay.stats = stats; }
};

// the conditional spectrum series (swrt_cond_series_*, swrt_cond.hpp): a sum
// per q class, then [n, rejected]
struct CondSeriesState : PlaneSeriesState {
  CondSeriesState() : PlaneSeriesState(0, 1, 2) {}
  int which = 0;            // 0 zeta, 1 sigma, 2 D
};

// the transition series (swrt_trans_series_*, swrt_trans.hpp): 3 sums per
// source class, then [n, rejected, serial].  The mark (src, one value per
// packet by original index) belongs to the packet set: swrt_packets_set drops
// it, the recorded frames stay (each holds its n and its mark's serial).
struct TransSeriesState : PlaneSeriesState {
  TransSeriesState() : PlaneSeriesState(0, 3, 3) {}
  bool marked = false;      // src holds a value for every packet of the current set
  int64_t serial = 0;       // marks since begin
  DevBuf<double> src;       // the source value by original packet index
  int64_t scap = 0;         // packets src is sized for
  void drop() { marked = false; }  // another packet set: the mark describes the old one
};

// the refraction series (swrt_refr_series_*, swrt_refr.hpp): 3 sums per omega
// class and one per alignment class, then [n, rejected]
struct RefrSeriesState : PlaneSeriesState {
  RefrSeriesState() : PlaneSeriesState(3, 1, 2) {}
};

// the absolute-frequency series (swrt_absfreq_series_*, swrt_absfreq.hpp): 3
// sums per omega class and 2 per Omega class, then [n, rejected].
// swrt_packets_set with another N drops the frames (drop()), the edges stay.
struct AbsfreqSeriesState : PlaneSeriesState {
  AbsfreqSeriesState() : PlaneSeriesState(3, 2, 2) {}
  void drop() { series.ext.cleared(); }  // the ensemble changed size: the frames describe another one
};

// the tangent map (swrt_tangent_*, swrt_tangent.hpp).  M and the caustic
// counters (by original index) belong to the packet set: swrt_packets_set with
// another N drops them (live), with the same N marks.  While live, the
// leapfrog calls take the per-packet route and launch the tangent kernel.  The
// series (3 sums per omega class, 1 per growth class, [n, rejected, serial])
// keeps its frames like the other class-plane series.
struct TangentState : PlaneSeriesState {
  TangentState() : PlaneSeriesState(3, 1, 3) {}
  bool live = false;        // M and caustics describe the current packet set
  int64_t n = 0;            // packets they were allocated for
  int64_t serial = 0;       // marks since begin (begin's is 1)
  DevBuf<double> M;         // n x 16
  DevBuf<int> caustics;     // n
  void drop() { live = false; }  // another packet set: the maps describe the old one
};

// packet recycling (swrt_recycle_*, swrt_recycle.hpp).  The per-packet state
// (home, gen, born, by original index) belongs to the packet set:
// swrt_packets_set drops it (live), the recorded frames stay readable until
// swrt_recycle_end or the next begin.
struct RecycleState {
  bool open = false;        // swrt_recycle_begin was called: the frames can be read
  bool live = false;        // home, gen and born describe the current packet set
  int frac_bits = 0;
  double f2 = 0.0, Cg2 = 0.0, cut = 0.0, L = 0.0;
  uint64_t seed = 0;
  int64_t base = 0;         // index_base
  int64_t serial = 0;       // events since begin or reset
  int64_t n = 0;            // packets the state was built for
  DevBuf<double> home;      // n x 2 column-major
  DevBuf<int> marks;        // gen (n), then born (n)
  DevBuf<int> bad;          // begin's home check: one flag
  Series<unsigned long long> series;  // recorded frames, kRecycleFrame words each
  int* gen() const { return marks.get(); }
  int* born() const { return marks.get() + n; }
  void drop() { live = false; }  // another packet set: the state describes the old one
};

// debug knobs (swrt_debug_set): a spin kernel queued on every extra packet
// stream before each of its part launches (adversarial overlap of consecutive
// calls), and the pre-third-buffer ordering after a source-gather sort
// launch (test-only: reintroduces the race the checker must catch)
struct DebugKnobs {
  int spin_us = 0;
  bool legacy_park = false;
  bool share_skew = false;  // test-only: the cycle-ending launch takes an uneven share (checker on only)
  int corrupt_count = 0;    // test-only: added to one tile count before the next scan (once)
  int kmap_path = 0;        // SWRT_DEBUG_KMAP_GLOBAL: 0 by m; 1 global; 2 / 3 global with / without the wave merge
  bool cond_global = false; // SWRT_DEBUG_COND_GLOBAL: the conditional spectrum series' global kernel for every shape
  bool trans_global = false; // SWRT_DEBUG_TRANS_GLOBAL: the transition series' global kernel for every shape
  bool refr_global = false; // SWRT_DEBUG_REFR_GLOBAL: the refraction series' global kernel for every shape
  bool absfreq_global = false; // SWRT_DEBUG_ABSFREQ_GLOBAL: the absolute-frequency series' global kernel for every shape
  bool tangent_global = false; // SWRT_DEBUG_TANGENT_GLOBAL: the tangent series' global kernel for every shape
};
}  // namespace

struct swrt_ctx {
  // The streams come first: members are destroyed in reverse order, so every
  // buffer and event below is released before the streams are.
  static constexpr int kMaxPacketStreams = 2;
  Stream stream0;  // the packet stream
  // The QG PDE (swrt_qg_*) runs on its own stream so the next PDE step, its
  // CFL speed and snapshot overlap the packet launch reading the previous
  // snapshots.  A snapshot into a slot whose buffer a queued packet launch
  // still reads takes an idle buffer from `spares` instead (renaming): a
  // multi-interval launch reads up to 5 snapshots while the PDE writes the
  // next group's.
  Stream qstream;
  Stream sx[kMaxPacketStreams - 1];  // the extra packet streams
  int device = 0;
  hipStream_t stream = nullptr;  // the stream every helper launches on (not owned): stream0, or
                                 // qstream inside OnQGStream
  std::string err;
  Slot slot[SWRT_MAX_SLOTS];
  bool qg_sep = true;
  bool qg_fused = true;  // swrt_qg_set_fused
  int qg_jfuse = 1;  // fused mode, 2 layers, no packets beside: the column pass fused with the Jacobian (SWRT_DEBUG_QG_JFUSE)
  int qg_update_cols = 1;  // fused mode, no packets beside: J's last forward pass inside the update (SWRT_DEBUG_QG_UPDATE_COLS)
  std::vector<Slot> spares;
  // packets: the current set, the next output (of a tile launch or the binning's scatter) and a third
  // set, the output of the launch after a split source-gather sort launch (see tile_launch)
  SetRing<PacketSet> pk;
  DevBuf<int> keys;   // N
  DevBuf<int> src_idx;   // N: source slot of each binned slot (indirect re-binning)
  BinArrays bins;
  Binning bin;  // the host's picture of the binning (swrt_packet_state.hpp)
  int kernel = 0;        // 0 auto, 1 per-packet global gather, 2 LDS tile kernel
  int64_t n = 0;
  int64_t cap = 0;
  int64_t rebin_every = 4;  // steps between spatial re-binning (0: never)
  int64_t tile = 0;         // cells per tile side (0: automatic)
  bool sort_lead = SWRT_SORT_LEAD;  // in-tile sort keys lead by the group-velocity drift
  int gather_mode = 0;      // 0: stencil sums mul then add (bit-exact); 1: fused multiply-add (tolerance)
  int sparse_mode = 0;      // sparse-tile launches: 0 auto (below kSparseBelow packets per tile), 1 never, 2 always
  // the packet step (swrt_set_integrator): the kick (0 Euler, 1 implicit midpoint with integ_iters
  // fixed-point passes) and the composition (0 none, 1 Yoshida, 2 Suzuki); (0, 1, 0) = the leapfrog step
  int integ_kick = 0, integ_iters = 1, integ_comp = 0;
  // Two packet streams (swrt_set_packet_streams 2, the default): each
  // LDS-tiled leapfrog launch runs as 2 part launches — the even and the odd
  // band positions of every XCD band — on `stream` and the extra stream
  // sx[0].  Within a re-binning cycle the parts touch disjoint packet ranges,
  // so one part's launch k overlaps the other's launch k+1 (one part's tail
  // under the other's body).  The extra stream's work is joined back into
  // `stream` (join_b) before anything else reads the packets.
  int packet_streams = 2;           // default: two (measured +2-4 %, bit-identical); 1 = one launch per step
  Event jx[kMaxPacketStreams - 1];  // the extra streams' join events
  Event fork_ev;
  int b_pending = 0;              // extra streams holding packet work not yet ordered before stream's
  Series<double> hist;  // the history: x frames and k frames, 2 x n doubles each
  int64_t steps_done = 0;  // global step counter since history reset (for save cadence)
  // scratch
  DevBuf<char> scratch;
  size_t scratch_bytes = 0;
  DevBuf<double2> tw;
  int tw_n = 0;
  XkaState xka;
  SpectralState spec;
  QGState qg;
  Ode23State o23;
  RayDiagState rd;
  OmegaSeriesState om;
  MapSeriesState map;
  KmapSeriesState kmap;
  TrackState trk;
  FlowSpecState flow;
  CondSeriesState cond;
  TransSeriesState trans;
  RefrSeriesState refr;
  AbsfreqSeriesState absfreq;
  TangentState tan;
  RecycleState recycle;
  // the packet stream got work since the last split launch's part 0 that the
  // next split launch's part 1 (on sx[0]) must follow: that launch forks (an
  // event marker, ~7 us of idle on each stream).  Only consecutive split
  // launches of swrt_advance / swrt_advance_intervals with nothing in between
  // skip it: part p of a binning owns the same tiles at every launch, so
  // stream order alone orders a part's launches (launch_tiles).
  bool s0_dirty = true;
  uint64_t slot_wgen = 0;  // Slot::wgen source
  Timing timing;
  int timing_every = 1;     // bracket every k-th leapfrog launch with HIP events (0: off)
  int64_t launch_count = 0;
  // set only around a timed packet launch: the dispatch itself stamps them
  // (hipExtLaunchKernel), so they bracket the kernel and nothing else (not owned)
  hipEvent_t kev0 = nullptr, kev1 = nullptr;
  // stop event attached to every untimed packet launch (launch_k), and the
  // stop event of the last stream operation of the current API call if that
  // was a packet launch (else nullptr; not owned): SlotUse marks the slots' use
  // with it instead of recording a separate marker, which cost ~11 us of idle
  // GPU between dependent packet launches (tools/gap_probe.py)
  Event use_ev;
  hipEvent_t tail_ev = nullptr;
  // the packet-buffer hazard checker (swrt_hazard.hpp) and the debug knobs
  HazardChecker hz;
  DebugKnobs dbg;
  // device-raised errors (host-visible pinned memory): [0] the binning scan's
  // count check failed (bin_scan_kernel) — read after host synchronisations
  HostBuf<int> dev_err;
  bool packets_lost = false;  // a failed binning left the packet state undefined (until swrt_packets_set)
  bool in_hook = false;       // an ode23 hook is running (swrt_ode23_run_hooked): packet calls are refused
  SnapshotImport xq;
  // shader-clock probe (swrt_clock_stamp): 2 stamps x kClockWaves waves x
  // {s_memtime, s_memrealtime, XCC id}
  DevBuf<unsigned long long> clk;
};

namespace {
constexpr size_t kMaxSpares = 8;  // renamed snapshot buffers per context

// the work recorded in `ev` has not finished yet
bool event_pending(hipEvent_t ev) {
  const hipError_t e = hipEventQuery(ev);
  (void)hipGetLastError();  // hipErrorNotReady is a status, not an error
  return e == hipErrorNotReady;
}

// Run a swrt_qg_* call on the QG stream: every helper launches on c->stream.
struct OnQGStream {
  swrt_ctx* c;
  hipStream_t saved;
  explicit OnQGStream(swrt_ctx* c_) : c(c_), saved(c_->stream) {
    if (c->qg_sep) c->stream = c->qstream.get();
  }
  ~OnQGStream() { c->stream = saved; }
};

// A context-stream call that reads or writes the field slots: wait for the
// QG-stream snapshots written into them, then mark them used by this call.
// Slot-use events are only needed while a QG stream may write slots beside
// the packet launches (swrt_qg_init on a separate stream); without one a
// packet launch carries no event at all (each costs ~5 us of idle GPU at the
// launch boundary, tools/gap_probe.py).
bool slot_events(const swrt_ctx* c) { return c->qg_sep && (c->qg.init || c->xq.init); }

// From here on packet launches mark their slot use (a QG stream or snapshot
// import starts): everything queued on `st` so far is marked by one record
// per slot.
void mark_slots_used(swrt_ctx* c, hipStream_t st) {
  for (Slot& sl : c->slot)
    if (sl.nodes && hipEventRecord(sl.uev.get(), st) == hipSuccess) {
      sl.uref = sl.uev.get();
      sl.upend = true;
    }
}

// The packet stream waits for the QG stream's pending snapshot writes before
// the first kernel that reads a slot.  Deferred (swrt_advance / _intervals):
// the wait is placed by slot_writes_wait() just before the first packet
// launch, so a re-binning at the start of the call (packet buffers only)
// runs while the PDE chain is still producing the snapshot.
constexpr unsigned kAllSlots = (1u << SWRT_MAX_SLOTS) - 1;
constexpr unsigned kSlots01 = 3u;  // the ode23 calls read slots 0 and 1 only

void slot_writes_wait(swrt_ctx* c, unsigned mask = kAllSlots) {
  if (!c->qg_sep) return;
  for (int i = 0; i < SWRT_MAX_SLOTS; ++i)
    if (Slot& s = c->slot[i]; (mask >> i & 1u) && s.wpend) {
      (void)hipStreamWaitEvent(c->stream, s.wev.get(), 0);
      s.wpend = false;
      c->s0_dirty = true;
    }
}

struct SlotUse {
  swrt_ctx* c;
  // wait_mask: the slots whose pending QG-stream writes this call's reads wait
  // for (the ode23 calls read slots 0 and 1 only: a hook's snapshot into slot
  // 2 keeps running beside their attempts)
  explicit SlotUse(swrt_ctx* c_, bool defer_writes = false, unsigned wait_mask = kAllSlots) : c(c_) {
    c->tail_ev = nullptr;
    if (!defer_writes) slot_writes_wait(c, wait_mask);
  }
  ~SlotUse() {
    if (!slot_events(c)) return;
    for (Slot& s : c->slot) {
      if (!s.nodes) continue;
      if (c->tail_ev) {
        s.uref = c->tail_ev;
        s.upend = true;
      } else if (hipEventRecord(s.uev.get(), c->stream) == hipSuccess) {
        s.uref = s.uev.get();
        s.upend = true;
      }
    }
    c->tail_ev = nullptr;
  }
};
int fail(swrt_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define HIPCHK(ctx, expr)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(ctx, SWRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)

// GUARD_BEGIN also orders any pending second-stream packet work before the
// call (join_b); the split-launch entry points use GUARD_BEGIN_KEEP_SPLIT.
#define HIPCHK_RC(expr)       \
  do {                        \
    const int rc_ = (expr);   \
    if (rc_) return rc_;      \
  } while (0)
// GUARD_BEGIN drops a queued ode23 chain (the packets may change); the calls
// that never touch the packets (QG, clock) use GUARD_BEGIN_KEEP_CHAIN.
// A call that may touch the packets is refused inside an ode23 hook
// (swrt_ode23_run_hooked): it would race the interval's attempts in flight.
#define HOOK_REFUSE \
  if (c->in_hook) return fail(c, SWRT_ERR_STATE, "this call may touch the packets: not allowed inside an ode23 hook");
#define GUARD_BEGIN_KEEP_SPLIT                  \
  HOOK_REFUSE                                   \
  try {                                         \
    {                                           \
      const int crc_ = chain_drop(c);           \
      if (crc_) return crc_;                    \
    }
#define GUARD_BEGIN_KEEP_CHAIN    \
  try {                           \
    {                             \
      const int jrc_ = join_b(c); \
      if (jrc_) return jrc_;      \
      hz_api(c);                  \
      c->s0_dirty = true;         \
    }
#define GUARD_BEGIN              \
  HOOK_REFUSE                    \
  GUARD_BEGIN_KEEP_CHAIN         \
  {                              \
    const int crc_ = chain_drop(c); \
    if (crc_) return crc_;       \
  }
#define GUARD_END(ctx)                                                \
  }                                                                   \
  catch (const std::bad_alloc&) {                                     \
    return fail(ctx, SWRT_ERR_ALLOC, "host allocation failed");       \
  }                                                                   \
  catch (...) {                                                       \
    return fail(ctx, SWRT_ERR_STATE, "unexpected C++ exception");     \
  }

// Order the extra streams' queued packet work before the packet stream's next work.
int join_b(swrt_ctx* c) {
  if (!c || !c->b_pending) return SWRT_OK;
  for (int i = 0; i < c->b_pending; ++i) {
    HIPCHK(c, hipEventRecord(c->jx[i].get(), c->sx[i].get()));
    HIPCHK(c, hipStreamWaitEvent(c->stream0.get(), c->jx[i].get(), 0));
    if (c->hz.on) {
      c->hz.record(c->jx[i].get(), i + 1);
      c->hz.wait(0, c->jx[i].get());
    }
  }
  c->b_pending = 0;
  return SWRT_OK;
}

// Order a chained first attempt's part 1 (sx[0]) before the packet stream's
// next work: the attempt is dropped, or its call runs another.
int chain_join(swrt_ctx* c) {
  if (!c->o23.chain_b) return SWRT_OK;
  c->o23.chain_b = false;
  HIPCHK(c, hipEventRecord(c->jx[0].get(), c->sx[0].get()));
  HIPCHK(c, hipStreamWaitEvent(c->stream0.get(), c->jx[0].get(), 0));
  if (c->hz.on) {
    c->hz.record(c->jx[0].get(), 1);
    c->hz.wait(0, c->jx[0].get());
  }
  return SWRT_OK;
}

// A queued ode23 chain dropped (the packets may change).
int chain_drop(swrt_ctx* c) {
  c->o23.dense_ready = false;  // (a dense attempt's stage buffers describe the packets before this call)
  c->o23.chain.queued = false;
  c->o23.chain.first_q = false;
  return chain_join(c);
}

// operation t of the packet stream accesses each of `bufs` whole, in this order
inline bool hz_whole(HazardChecker& h, uint64_t t, int kind, const char* what, std::initializer_list<const void*> bufs) {
  for (const void* b : bufs)
    if (!h.access(0, t, b, kind, HzRegion::all(), what)) return false;
  return true;
}

// Every other API call runs on the packet stream after join_b: to the checker
// it reads and writes every packet buffer there (conservative: a call that
// lost its join is reported by the next part launch).
void hz_api(swrt_ctx* c) {
  if (!c || !c->hz.on) return;
  const uint64_t t = c->hz.op(0);
  const PacketSet &p0 = c->pk.cur, &p1 = c->pk.out, &p2 = c->pk.park;
  for (const void* b : std::initializer_list<const void*>{
           p0.x.get(), p0.k.get(), p0.perm.get(), p1.x.get(), p1.k.get(), p1.perm.get(), p2.x.get(), p2.k.get(),
           p2.perm.get(), c->keys.get(), c->src_idx.get(), c->bins.counts(), c->bins.cursor(), c->bins.starts(),
           c->bins.tile_order(), c->hist.a.get(), c->hist.b.get()})
    (void)c->hz.access(0, t, b, kHzWrite, HzRegion::all(), "an API call");  // (a null buffer is no access)
}

// The host synchronised the packet stream after join_b: everything queued on
// any packet stream before has completed.
// (A wait for the QG stream, the flow spectrum series', says nothing about them.)
void hz_synced(swrt_ctx* c) {
  if (c->hz.on && c->stream == c->stream0.get()) c->hz.sync(0);
}

// After a host synchronisation with the packet stream: an error the device
// raised since (bin_scan_kernel's count check) becomes SWRT_ERR_STATE here,
// and the packet state — advanced by launches over an empty binning — is
// marked lost until the next swrt_packets_set.
int dev_err_check(swrt_ctx* c) {
  if (!c->dev_err || !c->dev_err[0]) return SWRT_OK;
  c->dev_err[0] = 0;
  c->packets_lost = true;
  c->bin.invalidate();
  return fail(c, SWRT_ERR_STATE,
              "packet binning corrupted: the tile counts do not sum to the packets (device check in "
              "bin_scan_kernel); no packet kernel ran over the bad ranges, but the packet state is lost — "
              "swrt_packets_set again");
}

// The packet state stays refused after a corrupted binning until
// swrt_packets_set (every entry point that reads the packets checks).
int lost_check(swrt_ctx* c) {
  if (c->packets_lost)
    return fail(c, SWRT_ERR_STATE, "the packet state was lost to a corrupted binning (swrt_packets_set again)");
  return SWRT_OK;
}

// The recorders' common check: packets that are present and not lost.
int packets_check(swrt_ctx* c) {
  HIPCHK_RC(lost_check(c));
  if (c->n == 0) return fail(c, SWRT_ERR_ARG, "no packets (swrt_packets_set first)");
  return SWRT_OK;
}

// [first, first + count) must lie inside the frames `e` has recorded.
int frame_range_check(swrt_ctx* c, const SeriesExtent& e, int64_t first, int64_t count, const char* msg) {
  return e.holds(first, count) ? SWRT_OK : fail(c, SWRT_ERR_ARG, msg);
}

// Room for `extra` more frames of pa (and pb) elements in s, at least
// `minimum` frames when it has to grow.  Growing keeps the recorded frames and
// waits for the stream: the old columns may still be written by queued work,
// so they are released only after the wait.  The new columns are locals until
// then: a failed allocation leaves the series as it was (b_failed: the
// history's message for its second column, SWRT_ERR_ALLOC).
template <typename A, typename B>
int series_reserve(swrt_ctx* c, Series<A, B>& s, size_t pa, size_t pb, int64_t extra, int64_t minimum,
                   const char* b_failed = nullptr) {
  if (s.ext.fits(extra, (int64_t)pa)) return SWRT_OK;
  const int64_t ncap = s.ext.grown(extra, (int64_t)pa, minimum);
  DevBuf<A> na;
  DevBuf<B> nb;
  HIPCHK(c, na.alloc(pa * ncap));
  if (pb && b_failed) {
    if (nb.alloc(pb * ncap) != hipSuccess) return fail(c, SWRT_ERR_ALLOC, b_failed);
  } else if (pb) {
    HIPCHK(c, nb.alloc(pb * ncap));
  }
  if (const size_t done = (size_t)s.ext.frames()) {
    HIPCHK(c, hipMemcpyAsync(na.get(), s.a.get(), sizeof(A) * pa * done, hipMemcpyDeviceToDevice, c->stream));
    if (pb) HIPCHK(c, hipMemcpyAsync(nb.get(), s.b.get(), sizeof(B) * pb * done, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  hz_synced(c);
  s.a = std::move(na);
  s.b = std::move(nb);
  s.ext.reserved(ncap, (int64_t)pa);
  return SWRT_OK;
}

// Frames [first, first + count) of s to the host, synchronously; out_b may be NULL.
template <typename A, typename B>
int series_get(swrt_ctx* c, const Series<A, B>& s, size_t pa, size_t pb, int64_t first, int64_t count, void* out_a,
               void* out_b, const char* range_msg) {
  HIPCHK_RC(frame_range_check(c, s.ext, first, count, range_msg));
  if (count == 0) return SWRT_OK;
  if (!out_a) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(out_a, s.a.get() + pa * first, sizeof(A) * pa * count, hipMemcpyDeviceToHost, c->stream));
  if (out_b)
    HIPCHK(c, hipMemcpyAsync(out_b, s.b.get() + pb * first, sizeof(B) * pb * count, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return dev_err_check(c);
}

// Drop s and its buffers (queued records may still write them: wait first).
template <typename A, typename B>
int series_release(swrt_ctx* c, Series<A, B>& s) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  hz_synced(c);
  s.a.reset();
  s.b.reset();
  s.ext.released();
  return SWRT_OK;
}

// Wait for the extra packet streams (host side).
int sync_sx(swrt_ctx* c) {
  for (int i = 0; i < swrt_ctx::kMaxPacketStreams - 1; ++i)
    if (c->sx[i]) {
      HIPCHK(c, hipStreamSynchronize(c->sx[i].get()));
      if (c->hz.on) c->hz.sync(i + 1);
    }
  c->b_pending = 0;
  c->o23.chain_b = false;
  return SWRT_OK;
}

bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

inline unsigned nblocks(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// log2 of a power-of-two transform length
inline int ilog2(int n) {
  int logn = 0;
  while ((1 << logn) < n) ++logn;
  return logn;
}
}  // namespace
