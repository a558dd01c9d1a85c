// swrt_host_diag.hpp — host side of the ten device-side recorders and of
// the packet recycling (swrt_recycle.hpp): the ray
// diagnostics (swrt_raydiag.hpp), the spectrum series (swrt_diag.hpp), the
// map series (swrt_map.hpp), the wave-vector plane series (swrt_kmap.hpp),
// the track series (swrt_track.hpp), the flow spectrum series
// (swrt_flowspec.hpp) and the four class-plane series: conditional spectrum
// (swrt_cond.hpp), transition (swrt_trans.hpp), refraction (swrt_refr.hpp)
// and absolute frequency (swrt_absfreq.hpp, last below).
// Each appends frames to a Series of its
// state (swrt_ctx.hpp) without a host wait: a reserve, the launches that write
// at the series' end, a commit.  The class-plane series share one state
// (PlaneSeriesState) and the plane_* functions ahead of them: begin, reserve,
// the history call, the launch's end, the read-back; what stays per series is
// its check, its kernel arguments and its choice of the LDS or global form.
// The order below (ray, spectrum, map, k-plane,
// track, flow, conditional, transition, recycling, refraction, absolute
// frequency) is the order their template kernels are first named in, hence
// emitted in: plane_launch takes a series' kernel pair as pointers and names
// no kernel itself.
#pragma once
#include <cmath>

#include "swrt_ctx.hpp"
#include "swrt_host_fields.hpp"
#include "swrt_host_packets.hpp"
#include "swrt_diag.hpp"
#include "swrt_raydiag.hpp"
#include "swrt_map.hpp"
#include "swrt_kmap.hpp"
#include "swrt_track.hpp"
#include "swrt_flowspec.hpp"
#include "swrt_cond.hpp"
#include "swrt_trans.hpp"
#include "swrt_recycle.hpp"
#include "swrt_refr.hpp"
#include "swrt_absfreq.hpp"

namespace {

// ---- ray diagnostics ----
// The three calls' common checks: SWRT_ERR_ARG with a message, as the header says.
int raydiag_check(swrt_ctx* c, int nslots) {
  HIPCHK_RC(lost_check(c));
  if (nslots != 1 && nslots != 2) return fail(c, SWRT_ERR_ARG, "nslots must be 1 or 2");
  for (int s = 0; s < nslots; ++s)
    if (!c->slot[s].set) return fail(c, SWRT_ERR_ARG, "field slot not set");
  if (nslots == 2 && (c->slot[1].nx != c->slot[0].nx || c->slot[1].L != c->slot[0].L ||
                      c->slot[1].ny_period != c->slot[0].ny_period))
    return fail(c, SWRT_ERR_ARG, "slots 0 and 1 have different grids");
  return packets_check(c);
}

// The per-packet buffers for the current ensemble and room for `extra` more frames.
int raydiag_reserve(swrt_ctx* c, int64_t extra) {
  RayDiagState& rd = c->rd;
  if (!rd.partial) HIPCHK(c, rd.partial.alloc(kRayDiagStats * kRayDiagBlocks + kRayDiagFrame));
  if (c->n > rd.pcap) {  // (a larger ensemble: swrt_packets_set dropped the mark; releasing waits for queued readers)
    rd.pcap = 0;
    rd.marked = false;
    HIPCHK(c, rd.omega0.alloc(c->n));
    HIPCHK(c, rd.rec.alloc(kRayDiagRec * c->n));
    rd.pcap = c->n;
  }
  return series_reserve(c, rd.series, kRayDiagFrame, 0, extra, kRayDiagSeriesMin);
}

// One pass over the packets on the context's stream: the mark, or a sample
// (then the reduction over its records) whose frame goes to `frame` (device)
// and whose N x 4 values go to `sample4` (device, may be NULL).
int raydiag_launch(swrt_ctx* c, bool mark, double f, double gH, int nslots, double alpha, double bump, double* sample4,
                   double* frame, const double* hist_x = nullptr, const double* hist_k = nullptr) {
  RayDiagState& rd = c->rd;
  RayDiagArgs a;
  a.f0 = view_of(c->slot[0]);
  a.f1 = nslots == 2 ? view_of(c->slot[1]) : a.f0;
  a.nslots = nslots;
  a.alpha = alpha;
  a.bump = bump;
  a.x = c->pk.cur.x.get();
  a.k = c->pk.cur.k.get();
  a.perm = c->pk.cur.perm.get();
  if (hist_x) {  // a history frame: the same layout in the original packet order
    a.x = hist_x;
    a.k = hist_k;
    a.perm = nullptr;
  }
  a.n = c->n;
  a.f2 = f * f;
  a.gH = gH;
  a.omega0 = (mark || rd.marked) ? rd.omega0.get() : nullptr;
  a.sample4 = sample4;
  a.rec = rd.rec.get();
  const dim3 grid(nblocks(c->n, kRayDiagThreads)), block(kRayDiagThreads);
  hipLaunchKernelGGL(mark ? ray_diag_kernel<true> : ray_diag_kernel<false>, grid, block, 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  if (mark) return SWRT_OK;
  const int nblk = (int)std::min<int64_t>(kRayDiagBlocks, grid.x);
  hipLaunchKernelGGL(ray_diag_reduce_kernel, dim3(nblk), block, 0, c->stream, rd.rec.get(), c->n, rd.partial.get());
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(ray_diag_frame_kernel, dim3(1), dim3(64), 0, c->stream, rd.partial.get(), nblk, c->n, frame);
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}

// One more frame of the series: from the packets, or from a history frame.
int raydiag_record_frame(swrt_ctx* c, double f, double gH, int nslots, double alpha, double bump,
                         const double* hist_x = nullptr, const double* hist_k = nullptr) {
  HIPCHK_RC(raydiag_launch(c, false, f, gH, nslots, alpha, bump, nullptr, c->rd.series.end_a(kRayDiagFrame), hist_x,
                           hist_k));
  c->rd.series.ext.committed(1);
  return SWRT_OK;
}

// ---- the spectrum series ----
// swrt_omega_histogram's checks on the edges, finite as well.
int omega_edges_check(swrt_ctx* c, const double* edges, int64_t nbins) {
  if (nbins <= 0 || nbins > kMaxHistBins) return fail(c, SWRT_ERR_ARG, "nbins must be 1..4096");
  if (!edges) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  for (int64_t i = 0; i <= nbins; ++i)
    if (!std::isfinite(edges[i])) return fail(c, SWRT_ERR_ARG, "edges must be finite");
  for (int64_t i = 0; i < nbins; ++i)
    if (!(edges[i] < edges[i + 1])) return fail(c, SWRT_ERR_ARG, "edges must increase");
  return SWRT_OK;
}

inline size_t omega_lds_bytes(int nb) { return sizeof(double) * (nb + 1) + sizeof(unsigned int) * (nb + 2); }

int omega_series_check(swrt_ctx* c) {
  if (!c->om.open) return fail(c, SWRT_ERR_STATE, "call swrt_omega_series_begin first");
  return packets_check(c);
}

// omega's per-packet buffer for the current ensemble and room for `extra` more
// frames.  The rows are zeroed by the launches that fill them.
int omega_reserve(swrt_ctx* c, int64_t extra, bool need_w) {
  OmegaSeriesState& om = c->om;
  if (!om.partial) HIPCHK(c, om.partial.alloc((size_t)kOmegaHistoryChunk * kOmegaPartials * kOmegaBlocks));
  if (need_w && c->n > om.pcap) {  // (releasing the old buffer waits for queued readers)
    om.pcap = 0;
    HIPCHK(c, om.w.alloc(c->n));
    om.pcap = c->n;
  }
  return series_reserve(c, om.series, om.row(), kOmegaStats, extra, kOmegaSeriesMin);
}

// `count` frames from the series' end on: omega_frame_kernel over src (omega
// by original index, or the k of consecutive history frames), then their stats.
int omega_frames_launch(swrt_ctx* c, bool from_k, const double* src, int64_t src_stride, int64_t count) {
  OmegaSeriesState& om = c->om;
  OmegaFrameArgs a;
  a.src = src;
  a.src_stride = src_stride;
  a.n = c->n;
  a.f2 = om.f2;
  a.Cg2 = om.Cg2;
  a.edges = om.edges.get();
  a.nb = om.nb;
  a.counts = om.series.end_a(om.row());
  a.partial = om.partial.get();
  const int nblk = (int)std::min<int64_t>(kOmegaBlocks, nblocks(c->n, kOmegaThreads));
  const dim3 grid(nblk, (unsigned)count), block(kOmegaThreads);
  hipLaunchKernelGGL(from_k ? omega_frame_kernel<true> : omega_frame_kernel<false>, grid, block,
                     omega_lds_bytes(om.nb), c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(omega_stats_kernel, dim3((unsigned)count), dim3(kOmegaThreads), 0, c->stream, om.partial.get(), nblk, c->n,
                     om.series.end_b(kOmegaStats));
  HIPCHK(c, hipGetLastError());
  om.series.ext.committed(count);
  return SWRT_OK;
}

// ---- the count series' zeroed frames (map, k-plane, class planes) ----
// Room in s for `count` more frames of pa and pb words, zeroed on the stream:
// the launches that fill them only add.
int reserve_zeroed(swrt_ctx* c, Series<unsigned long long>& s, size_t pa, size_t pb, int64_t count) {
  using word = unsigned long long;
  HIPCHK_RC(series_reserve(c, s, pa, pb, count, map_series_min(pa * sizeof(word))));
  HIPCHK(c, hipMemsetAsync(s.end_a(pa), 0, sizeof(word) * pa * count, c->stream));
  HIPCHK(c, hipMemsetAsync(s.end_b(pb), 0, sizeof(word) * pb * count, c->stream));
  return SWRT_OK;
}

// `count` history frames from `first` on in launches of at most `chunk`
// frames: launch(i, off, nf) takes nf frames, the i-th of the call first,
// whose x and k start `off` doubles into the history's columns.
template <typename Launch>
int history_chunks(swrt_ctx* c, int64_t first, int64_t count, int64_t chunk, Launch launch) {
  for (int64_t i = 0; i < count; i += chunk)
    HIPCHK_RC(launch(i, (first + i) * 2 * c->n, std::min<int64_t>(chunk, count - i)));
  return SWRT_OK;
}

// ---- the map series ----
int map_series_check(swrt_ctx* c) {
  if (!c->map.open) return fail(c, SWRT_ERR_STATE, "call swrt_map_series_begin first");
  HIPCHK_RC(packets_check(c));
  if (c->n > kMapMaxPackets) return fail(c, SWRT_ERR_ARG, "a map frame takes at most 2^24 packets");
  return SWRT_OK;
}

int map_reserve_zeroed(swrt_ctx* c, int64_t count) {
  return reserve_zeroed(c, c->map.series, c->map.frame(), kMapStats, count);
}

MapGeom map_geom(const MapSeriesState& ms) {
  MapGeom g;
  g.dxm = ms.L / (double)ms.m;  // (as view_of's dx = L/nx)
  g.inv_dxm = 1.0 / g.dxm;
  g.pm = (double)ms.m;
  g.inv_pm = 1.0 / g.pm;
  g.m = ms.m;
  g.f2 = ms.f2;
  g.Cg2 = ms.Cg2;
  g.scale = std::ldexp(1.0, ms.frac_bits);
  return g;
}

// `count` frames from the series' end on by the general kernel: frame i from
// the packets at x + i*stride, k + i*stride (any order).
int map_general_launch(swrt_ctx* c, const double* x, const double* k, int64_t stride, int64_t count) {
  MapSeriesState& ms = c->map;
  const int nblk = (int)std::min<int64_t>(kMapBlocks, nblocks(c->n, kMapThreads));
  hipLaunchKernelGGL(map_general_kernel, dim3(nblk, (unsigned)count), dim3(kMapThreads), 0, c->stream, x, k, c->n,
                     stride, map_geom(ms), ms.series.end_a(ms.frame()), ms.series.end_b(kMapStats));
  HIPCHK(c, hipGetLastError());
  ms.series.ext.committed(count);
  return SWRT_OK;
}

// The tile path applies: the packets are in the order of the LDS tile kernel's
// binning of slot 0's grid, the map covers that grid's square, and a map cell
// is c x c field cells with c dividing the tile side.
bool map_tiled(const swrt_ctx* c) {
  const MapSeriesState& ms = c->map;
  const Slot& s = c->slot[0];
  if (!s.set || !tile_binned(c) || c->bin.tile() != kTile) return false;
  if (ms.L != s.L || s.nx % ms.m != 0) return false;
  return kTile % (s.nx / ms.m) == 0;
}

// One frame at the series' end from the binned packets, a workgroup per tile.
int map_tile_launch(swrt_ctx* c) {
  MapSeriesState& ms = c->map;
  MapTileArgs a;
  a.x = c->pk.cur.x.get();
  a.k = c->pk.cur.k.get();
  a.n = c->n;
  a.starts = c->bins.starts();
  a.order = c->bins.tile_order();
  a.ntx = tiles_per_side(c->slot[0].nx);
  a.c = (int)(c->slot[0].nx / ms.m);
  a.g = map_geom(ms);
  a.planes = ms.series.end_a(ms.frame());
  a.stats = ms.series.end_b(kMapStats);
  a.strays = ms.strays.get();
  hipLaunchKernelGGL((map_tile_kernel<kTile, kMargin>), dim3((unsigned)(a.ntx * a.ntx)), dim3(kMapThreads), 0,
                     c->stream, a);
  HIPCHK(c, hipGetLastError());
  ms.series.ext.committed(1);
  ++ms.tiled_frames;
  return SWRT_OK;
}

// ---- the wave-vector plane series ----
int kmap_series_check(swrt_ctx* c) {
  if (!c->kmap.open) return fail(c, SWRT_ERR_STATE, "call swrt_kmap_series_begin first");
  HIPCHK_RC(packets_check(c));
  if (c->n > kKmapMaxPackets) return fail(c, SWRT_ERR_ARG, "a k-plane frame takes at most 2^24 packets");
  return SWRT_OK;
}

int kmap_reserve_zeroed(swrt_ctx* c, int64_t count) {
  return reserve_zeroed(c, c->kmap.series, c->kmap.frame(), kKmapStats, count);
}

// `count` frames from the series' end on: frame i from the packets' k at
// k + i*stride (any order).  The LDS kernel while the plane fits a workgroup's
// LDS, the global one beyond (or when SWRT_DEBUG_KMAP_GLOBAL says so).
int kmap_launch(swrt_ctx* c, const double* k, int64_t stride, int64_t count) {
  KmapSeriesState& ks = c->kmap;
  KmapGeom g;
  g.K = ks.K;
  g.s = ks.s;
  g.m = ks.m;
  g.scale = std::ldexp(1.0, ks.frac_bits);
  unsigned long long* planes = ks.series.end_a(ks.frame());
  unsigned long long* stats = ks.series.end_b(kKmapStats);
  const int path = c->dbg.kmap_path;
  const dim3 block(kKmapThreads);
  if (path == 0 && ks.m <= kKmapLdsCells) {
    const int nblk = (int)std::min<int64_t>(kKmapLdsBlocks, nblocks(c->n, kKmapThreads));
    hipLaunchKernelGGL(kmap_lds_kernel, dim3(nblk, (unsigned)count), block, 0, c->stream, k, c->n, stride, g, planes,
                       stats);
  } else {
    const int nblk = (int)std::min<int64_t>(kKmapBlocks, nblocks(c->n, kKmapThreads));
    const bool merge = path == 2 || (path != 3 && kKmapGlobalMerge);
    hipLaunchKernelGGL(merge ? kmap_global_kernel<true> : kmap_global_kernel<false>, dim3(nblk, (unsigned)count), block,
                       0, c->stream, k, c->n, stride, g, planes, stats);
  }
  HIPCHK(c, hipGetLastError());
  ks.series.ext.committed(count);
  return SWRT_OK;
}

// Frames [first, first + count) to the host, synchronously; either output may
// be NULL, not both.
int kmap_series_get(swrt_ctx* c, int64_t first, int64_t count, int64_t* plane_out, int64_t* stats_out) {
  const KmapSeriesState& ks = c->kmap;
  HIPCHK_RC(frame_range_check(c, ks.series.ext, first, count, "frame range out of bounds"));
  if (!plane_out && !stats_out) return fail(c, SWRT_ERR_ARG, "NULL buffer (plane_out and stats8_out)");
  if (count == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t fr = ks.frame();
  if (plane_out)
    HIPCHK(c, hipMemcpyAsync(plane_out, ks.series.a.get() + fr * first, sizeof(int64_t) * fr * count,
                             hipMemcpyDeviceToHost, c->stream));
  if (stats_out)
    HIPCHK(c, hipMemcpyAsync(stats_out, ks.series.b.get() + (size_t)kKmapStats * first,
                             sizeof(int64_t) * kKmapStats * count, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return dev_err_check(c);
}

// ---- the track series ----
// The two records' common checks; nslots == 0 (no flow) needs no slot.
int track_check(swrt_ctx* c, int nslots) {
  if (!c->trk.open) return fail(c, SWRT_ERR_STATE, "call swrt_track_begin first");
  if (nslots == 0) return packets_check(c);
  if (nslots != 1 && nslots != 2) return fail(c, SWRT_ERR_ARG, "nslots must be 0, 1 or 2");
  return raydiag_check(c, nslots);
}

// The field slots a record with `nslots` snapshots reads (SlotUse's wait mask).
inline unsigned track_slot_mask(int nslots) { return nslots <= 0 ? 0u : nslots == 1 ? 1u : kSlots01; }

int track_reserve(swrt_ctx* c, int64_t extra) {
  TrackState& tr = c->trk;
  return series_reserve(c, tr.series, tr.frame(), 0, extra, map_series_min(tr.frame() * sizeof(double)));
}

// One frame at the series' end: from the packets, or from a history frame.
int track_record_frame(swrt_ctx* c, double f, double gH, int nslots, double alpha, double bump,
                       const double* hist_x = nullptr, const double* hist_k = nullptr) {
  TrackState& tr = c->trk;
  TrackArgs a;
  a.f0 = nslots ? view_of(c->slot[0]) : FieldView{};
  a.f1 = nslots == 2 ? view_of(c->slot[1]) : a.f0;
  a.nslots = nslots;
  a.alpha = alpha;
  a.bump = bump;
  a.x = hist_x ? hist_x : c->pk.cur.x.get();
  a.k = hist_x ? hist_k : c->pk.cur.k.get();
  a.perm = c->pk.cur.perm.get();
  a.lookup = hist_x ? tr.dids.get() : tr.slot_of.get();
  a.n = c->n;
  a.m = tr.m;
  a.f2 = f * f;
  a.gH = gH;
  a.frame = tr.series.end_a(tr.frame());
  const dim3 grid(nblocks(hist_x ? tr.m : c->n, kTrackThreads)), block(kTrackThreads);
  hipLaunchKernelGGL(hist_x ? track_kernel<true> : track_kernel<false>, grid, block, 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  tr.series.ext.committed(1);
  return SWRT_OK;
}

// ---- the flow spectrum series ----
// One frame at the series' end on the context's current stream (the QG
// stream inside OnQGStream) from the half plane at `qk`, mode (kx, ky) at
// (kx + kmax)*skx + ky*sky, stamped with the time t.
int flow_spectrum_record_frame(swrt_ctx* c, const double2* qk, int64_t skx, int64_t sky, double t) {
  FlowSpecState& fs = c->flow;
  HIPCHK_RC(series_reserve(c, fs.series, fs.frame(), kFlowSpecStats, 1, map_series_min(fs.frame() * sizeof(double))));
  FlowSpecArgs a;
  a.qk = qk;
  a.skx = skx;
  a.sky = sky;
  a.nx = fs.nx;
  a.nshell = fs.nshell;
  a.k_scale = fs.k_scale;
  a.K_d2 = fs.K_d2;
  a.frame = fs.series.end_a(fs.frame());
  hipLaunchKernelGGL(flow_spectrum_kernel, dim3((unsigned)fs.nshell), dim3(kFlowSpecThreads),
                     sizeof(double) * 3 * (size_t)(fs.nx / 2), c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(flow_spectrum_totals_kernel, dim3(1), dim3(kFlowSpecThreads), 0, c->stream, a.frame, fs.nshell, t,
                     fs.series.end_b(kFlowSpecStats));
  HIPCHK(c, hipGetLastError());
  fs.series.ext.committed(1);
  return SWRT_OK;
}

// Frames [first, first + count) to the host, synchronously; either output may
// be NULL, not both.
int flow_spectrum_get(swrt_ctx* c, int64_t first, int64_t count, double* spectra_out, double* stats_out) {
  const FlowSpecState& fs = c->flow;
  HIPCHK_RC(frame_range_check(c, fs.series.ext, first, count, "frame range out of bounds"));
  if (!spectra_out && !stats_out) return fail(c, SWRT_ERR_ARG, "NULL buffer (spectra_out and stats4_out)");
  if (count == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t fr = fs.frame();
  if (spectra_out)
    HIPCHK(c, hipMemcpyAsync(spectra_out, fs.series.a.get() + fr * first, sizeof(double) * fr * count,
                             hipMemcpyDeviceToHost, c->stream));
  if (stats_out)
    HIPCHK(c, hipMemcpyAsync(stats_out, fs.series.b.get() + (size_t)kFlowSpecStats * first,
                             sizeof(double) * kFlowSpecStats * count, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
}

// ---- the class-plane series: what cond, trans, refr and absfreq share ----
// The four keep a PlaneSeriesState (swrt_ctx.hpp) and differ in their kernels,
// their own checks and the members beside it; the frame's layout is
// PlaneLayout's (swrt_packet_state.hpp), filled in by each state's constructor.
static_assert(kTransMaxCells == kCondMaxCells && kRefrMaxCells == kCondMaxCells && kAbsfreqMaxCells == kCondMaxCells &&
              kTransMaxFracBits == kCondMaxFracBits && kRefrMaxFracBits == kCondMaxFracBits &&
              kAbsfreqMaxFracBits == kCondMaxFracBits, "plane_series_begin checks the four against one cap");
static_assert(kCondStats == 2 && kTransSums == 3 && kTransStats == 3 && kRefrWSums == 3 && kRefrStats == 2 &&
              kAbsfreqWSums == 3 && kAbsfreqOSums == 2 && kAbsfreqStats == 2,
              "the states' PlaneLayout (swrt_ctx.hpp) restates what the kernels write");

// swrt_*_series_begin after the guard.  cap_msg names the second axis' count;
// own_err, when not NULL, is the failed check of the series' own argument
// (cond's `which`); `released` runs once the old series is gone, before the
// edges are replaced (trans forgets its mark there).
template <typename Released>
int plane_series_begin(swrt_ctx* c, PlaneSeriesState& ps, double f, double Cg, const double* omega_edges, int64_t nw,
                       const double* edges2, int64_t n2, int frac_bits, const char* cap_msg, const char* own_err,
                       Released released) {
  HIPCHK_RC(omega_edges_check(c, omega_edges, nw));
  HIPCHK_RC(omega_edges_check(c, edges2, n2));
  if ((n2 + 2) * (nw + 2) > kCondMaxCells) return fail(c, SWRT_ERR_ARG, cap_msg);
  if (own_err) return fail(c, SWRT_ERR_ARG, own_err);
  if (frac_bits < 0 || frac_bits > kCondMaxFracBits) return fail(c, SWRT_ERR_ARG, "frac_bits must be 0..32");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(series_release(c, ps.series));  // (waits: queued records read the old edges too)
  ps.open = false;
  released();
  HIPCHK(c, ps.edges.alloc(nw + n2 + 2));
  HIPCHK(c, hipMemcpyAsync(ps.edges.get(), omega_edges, sizeof(double) * (nw + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(ps.edges.get() + nw + 1, edges2, sizeof(double) * (n2 + 1), hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ps.lay.nw = (int)nw;
  ps.lay.n2 = (int)n2;
  ps.frac_bits = frac_bits;
  ps.f2 = f * f;
  ps.Cg2 = Cg * Cg;
  ps.open = true;
  return SWRT_OK;
}

int plane_reserve_zeroed(swrt_ctx* c, PlaneSeriesState& ps, int64_t count) {
  return reserve_zeroed(c, ps.series, ps.lay.frame(), ps.lay.tail(), count);
}

// The frames' alphas of a two-snapshot record_history to the device (*dalphas);
// the caller's buffer is free on return.
int history_alphas(swrt_ctx* c, PlaneSeriesState& ps, const double* alphas, int64_t count, const double** dalphas) {
  if (count > ps.acap) {  // (releasing the old buffer waits for queued readers)
    ps.acap = 0;
    HIPCHK(c, ps.alphas.alloc(count));
    ps.acap = count;
  }
  HIPCHK(c, hipMemcpyAsync(ps.alphas.get(), alphas, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *dalphas = ps.alphas.get();
  return SWRT_OK;
}

// swrt_*_series_record_history after the series' own check: `count` history
// frames from `first` on, `chunk` a launch; two: the flow between two
// snapshots at alphas[i].  launch(dalphas, x, k, nf) queues nf frames from the
// history's x and k (dalphas: the first frame's alpha on the device, or NULL).
template <typename Launch>
int plane_record_history(swrt_ctx* c, PlaneSeriesState& ps, int64_t first, int64_t count, bool two,
                         const double* alphas, int64_t chunk, Launch launch) {
  HIPCHK_RC(frame_range_check(c, c->hist.ext, first, count, "history frame range out of bounds"));
  if (two && !alphas && count > 0) return fail(c, SWRT_ERR_ARG, "NULL buffer (alphas, two snapshots)");
  if (count == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const double* dalphas = nullptr;
  if (two) HIPCHK_RC(history_alphas(c, ps, alphas, count, &dalphas));
  HIPCHK_RC(plane_reserve_zeroed(c, ps, count));
  return history_chunks(c, first, count, chunk, [&](int64_t i, int64_t off, int64_t nf) {
    return launch(dalphas ? dalphas + i : nullptr, c->hist.a.get() + off, c->hist.b.get() + off, nf);
  });
}

// How a series' kernel pair is launched: the most blocks by the launch's
// dynamic LDS bytes, and the limit the pair asks for above 64 KB.
struct PlaneLaunchShape {
  int threads, max_lds_bytes;
  int blocks, big_blocks, huge_blocks;  // up to big_bytes, above it, above huge_bytes
  size_t big_bytes, huge_bytes;
};

// The end of the four launches: `count` frames at the series' end by the LDS
// or the global kernel of the pair with `bytes` of dynamic LDS, committed.
template <typename Args>
int plane_launch(swrt_ctx* c, PlaneSeriesState& ps, void (*lds_kernel)(Args), void (*global_kernel)(Args), bool lds,
                 size_t bytes, const PlaneLaunchShape& sh, const Args& a, int64_t count) {
  if (bytes > ((size_t)64 << 10) && !ps.lds_attr) {  // (above 64 KB of dynamic LDS a kernel has to ask once)
    for (auto* kernel : {lds_kernel, global_kernel})
      HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    sh.max_lds_bytes));
    ps.lds_attr = true;
  }
  const int most = bytes > sh.huge_bytes ? sh.huge_blocks : bytes > sh.big_bytes ? sh.big_blocks : sh.blocks;
  const int nblk = (int)std::min<int64_t>(most, nblocks(c->n, sh.threads));
  hipLaunchKernelGGL(lds ? lds_kernel : global_kernel, dim3(nblk, (unsigned)count), dim3(sh.threads), bytes, c->stream,
                     a);
  HIPCHK(c, hipGetLastError());
  ps.series.ext.committed(count);
  return SWRT_OK;
}

// Frames [first, first + count) to the host, synchronously; every output may
// be NULL.  The sums and the stats share the series' second column.
int plane_series_get(swrt_ctx* c, const PlaneSeriesState& ps, int64_t first, int64_t count, int64_t* counts_out,
                     int64_t* sums_out, int64_t* stats_out) {
  HIPCHK_RC(frame_range_check(c, ps.series.ext, first, count, "frame range out of bounds"));
  if (count == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t fr = ps.lay.frame(), tl = ps.lay.tail(), nsum = ps.lay.nsums();
  std::vector<int64_t> tails;
  if (counts_out)
    HIPCHK(c, hipMemcpyAsync(counts_out, ps.series.a.get() + fr * first, sizeof(int64_t) * fr * count,
                             hipMemcpyDeviceToHost, c->stream));
  if (sums_out || stats_out) {
    tails.resize(tl * count);
    HIPCHK(c, hipMemcpyAsync(tails.data(), ps.series.b.get() + tl * first, sizeof(int64_t) * tl * count,
                             hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int64_t t = 0; t < count && !tails.empty(); ++t) {
    const int64_t *row = tails.data() + tl * t, *stats = row + nsum;
    if (sums_out) std::copy(row, stats, sums_out + nsum * t);
    if (stats_out) std::copy(stats, row + tl, stats_out + (size_t)ps.lay.stats * t);
  }
  return dev_err_check(c);
}

// The bodies of swrt_*_series_frames, _bins and _reset (c may be NULL).
template <typename S>
int64_t plane_series_frames(const swrt_ctx* c, S swrt_ctx::*which) {
  return c ? (c->*which).series.ext.frames() : -1;
}

template <typename S>
int plane_series_bins(const swrt_ctx* c, S swrt_ctx::*which, int64_t* nw_out, int64_t* n2_out) {
  if (!c) return SWRT_ERR_ARG;
  const PlaneSeriesState& ps = c->*which;
  if (nw_out) *nw_out = ps.open ? ps.lay.nw : 0;
  if (n2_out) *n2_out = ps.open ? ps.lay.n2 : 0;
  return SWRT_OK;
}

template <typename S>
int plane_series_reset(swrt_ctx* c, S swrt_ctx::*which) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (as swrt_raydiag_series_reset)
  (c->*which).series.ext.cleared();
  return SWRT_OK;
}

// ---- the conditional spectrum series ----
// The records' common checks: an open series, then swrt_raydiag_record's.
int cond_series_check(swrt_ctx* c, int nslots) {
  if (!c->cond.open) return fail(c, SWRT_ERR_STATE, "call swrt_cond_series_begin first");
  HIPCHK_RC(raydiag_check(c, nslots));
  if (c->n > kCondMaxPackets) return fail(c, SWRT_ERR_ARG, "a conditional spectrum frame takes at most 2^24 packets");
  return SWRT_OK;
}

// `count` frames from the series' end on: frame i from the packets at
// x + i*stride, k + i*stride (any order) and the flow at alphas[i] (device;
// NULL: `alpha` for every frame).  The LDS kernel while the count plane fits
// a workgroup's LDS, the global one beyond (or when SWRT_DEBUG_COND_GLOBAL
// says so).
int cond_launch(swrt_ctx* c, int nslots, double alpha, const double* alphas, double bump, const double* x,
                const double* k, int64_t stride, int64_t count) {
  CondSeriesState& cs = c->cond;
  CondArgs a;
  a.f0 = view_of(c->slot[0]);
  a.f1 = nslots == 2 ? view_of(c->slot[1]) : a.f0;
  a.nslots = nslots;
  a.alpha = alpha;
  a.bump = bump;
  a.alphas = alphas;
  a.x = x;
  a.k = k;
  a.stride = stride;
  a.n = c->n;
  a.f2 = cs.f2;
  a.Cg2 = cs.Cg2;
  a.wedges = cs.edges.get();
  a.qedges = cs.edges.get() + cs.lay.nw + 1;
  a.nw = cs.lay.nw;
  a.nq = cs.lay.n2;
  a.which = cs.which;
  a.scale = std::ldexp(1.0, cs.frac_bits);
  a.counts = cs.series.end_a(cs.lay.frame());
  a.tail = cs.series.end_b(cs.lay.tail());
  const bool lds = !c->dbg.cond_global && cs.lay.frame() <= (size_t)kCondLdsCells;
  const size_t bytes = cond_lds_bytes(cs.lay.nw, cs.lay.n2, lds);
  // (the limit: edges 33 KB at most, sums 32 KB at most (never both), the plane 64 KB)
  const PlaneLaunchShape shape = {kCondThreads, 128 << 10, kCondBlocks, kCondBigPlaneBlocks, kCondBigPlaneBlocks,
                                         kCondBigPlaneBytes, SIZE_MAX};
  return plane_launch(c, cs, cond_kernel<true>, cond_kernel<false>, lds, bytes, shape, a, count);
}

// ---- the transition series ----
// The records' common checks: an open series, packets, a valid mark.
int trans_series_check(swrt_ctx* c, bool need_mark) {
  if (!c->trans.open) return fail(c, SWRT_ERR_STATE, "call swrt_trans_series_begin first");
  HIPCHK_RC(packets_check(c));
  if (c->n > kTransMaxPackets) return fail(c, SWRT_ERR_ARG, "a transition frame takes at most 2^24 packets");
  if (need_mark && !c->trans.marked)
    return fail(c, SWRT_ERR_STATE, "no mark for this packet set (swrt_trans_series_mark or _mark_values first)");
  return SWRT_OK;
}

// Room in src for every packet of the set.  Growing releases the old buffer,
// which waits for its queued readers; the old mark is gone either way.
int trans_src_reserve(swrt_ctx* c) {
  TransSeriesState& ts = c->trans;
  ts.marked = false;
  if (c->n <= ts.scap) return SWRT_OK;
  ts.scap = 0;
  HIPCHK(c, ts.src.alloc(c->n));
  ts.scap = c->n;
  if (c->hz.on) c->hz.name(ts.src.get(), "transition source values");
  return SWRT_OK;
}

// `count` frames from the series' end on: frame i from the k at k + i*stride
// in the order `perm` names (NULL: the original order), joined to the mark.
// The LDS kernel while the count plane fits a workgroup's LDS, the global one
// beyond (or when SWRT_DEBUG_TRANS_GLOBAL says so).
int trans_launch(swrt_ctx* c, const double* k, const int* perm, int64_t stride, int64_t count) {
  TransSeriesState& ts = c->trans;
  TransArgs a;
  a.k = k;
  a.perm = perm;
  a.src = ts.src.get();
  a.stride = stride;
  a.n = c->n;
  a.f2 = ts.f2;
  a.Cg2 = ts.Cg2;
  a.wedges = ts.edges.get();
  a.sedges = ts.edges.get() + ts.lay.nw + 1;
  a.nw = ts.lay.nw;
  a.ns = ts.lay.n2;
  a.scale = std::ldexp(1.0, ts.frac_bits);
  a.serial = (unsigned long long)ts.serial;
  a.counts = ts.series.end_a(ts.lay.frame());
  a.tail = ts.series.end_b(ts.lay.tail());
  const bool lds = !c->dbg.trans_global && ts.lay.frame() <= (size_t)kCondLdsCells;
  const size_t bytes = trans_lds_bytes(ts.lay.nw, ts.lay.n2, lds);
  // (the limit: edges 33 KB at most, sums 24 KB at most, the plane 64 KB)
  const PlaneLaunchShape shape = {kTransThreads, 128 << 10, kTransBlocks, kTransBigPlaneBlocks,
                                         kTransBigPlaneBlocks, kTransBigPlaneBytes, SIZE_MAX};
  return plane_launch(c, ts, trans_kernel<true>, trans_kernel<false>, lds, bytes, shape, a, count);
}

// ---- packet recycling ----
int recycle_check(swrt_ctx* c) {
  if (!c->recycle.open) return fail(c, SWRT_ERR_STATE, "call swrt_recycle_begin first");
  if (!c->recycle.live)
    return fail(c, SWRT_ERR_STATE, "the recycle state belonged to an earlier packet set (swrt_recycle_begin again)");
  return packets_check(c);
}

// One event: a zeroed frame at the series' end, the pass over the packets in
// place, the binning told that packets jumped.
int recycle_launch(swrt_ctx* c) {
  RecycleState& rs = c->recycle;
  HIPCHK_RC(series_reserve(c, rs.series, kRecycleFrame, 0, 1, kRecycleSeriesMin));
  RecycleArgs a;
  a.x = c->pk.cur.x.get();
  a.k = c->pk.cur.k.get();
  a.perm = c->pk.cur.perm.get();
  a.n = c->n;
  a.f2 = rs.f2;
  a.Cg2 = rs.Cg2;
  a.cut = rs.cut;
  a.L = rs.L;
  a.scale = std::ldexp(1.0, rs.frac_bits);
  a.seed = rs.seed;
  a.base = (uint64_t)rs.base;
  a.serial = (int)(rs.serial + 1);
  a.home = rs.home.get();
  a.gen = rs.gen();
  a.born = rs.born();
  a.frame = rs.series.end_a(kRecycleFrame);
  if (c->hz.on) {
    HazardChecker& h = c->hz;
    const uint64_t t = h.op(0);
    const char* what = "the recycle launch";
    if (!(hz_whole(h, t, kHzWrite, what, {a.x, a.k, a.gen, a.home}) && hz_whole(h, t, kHzRead, what, {a.perm})))
      return fail(c, SWRT_ERR_STATE, h.err);
  }
  HIPCHK(c, hipMemsetAsync(a.frame, 0, sizeof(unsigned long long) * kRecycleFrame, c->stream));
  const int nblk = (int)std::min<int64_t>(kRecycleBlocks, nblocks(c->n, kRecycleThreads));
  hipLaunchKernelGGL(recycle_kernel, dim3(nblk), dim3(kRecycleThreads), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  ++rs.serial;
  rs.series.ext.committed(1);
  c->bin.invalidate();  // re-injected packets jump across tiles: the next packet call re-bins
  return SWRT_OK;
}

// ---- the refraction series ----
// The records' common checks: an open series, then swrt_raydiag_record's.
int refr_series_check(swrt_ctx* c, int nslots) {
  if (!c->refr.open) return fail(c, SWRT_ERR_STATE, "call swrt_refr_series_begin first");
  HIPCHK_RC(raydiag_check(c, nslots));
  if (c->n > kRefrMaxPackets) return fail(c, SWRT_ERR_ARG, "a refraction frame takes at most 2^24 packets");
  return SWRT_OK;
}

// `count` frames from the series' end on: frame i from the packets at
// x + i*stride, k + i*stride (any order) and the flow at alphas[i] (device;
// NULL: `alpha` for every frame).  The LDS kernel for refr_lds_form's shapes,
// the global one beyond (or when SWRT_DEBUG_REFR_GLOBAL says so).
int refr_launch(swrt_ctx* c, int nslots, double alpha, const double* alphas, double bump, const double* x,
                const double* k, int64_t stride, int64_t count) {
  RefrSeriesState& rs = c->refr;
  RefrArgs a;
  a.f0 = view_of(c->slot[0]);
  a.f1 = nslots == 2 ? view_of(c->slot[1]) : a.f0;
  a.nslots = nslots;
  a.alpha = alpha;
  a.bump = bump;
  a.alphas = alphas;
  a.x = x;
  a.k = k;
  a.stride = stride;
  a.n = c->n;
  a.f2 = rs.f2;
  a.Cg2 = rs.Cg2;
  a.wedges = rs.edges.get();
  a.aedges = rs.edges.get() + rs.lay.nw + 1;
  a.nw = rs.lay.nw;
  a.na = rs.lay.n2;
  a.scale = std::ldexp(1.0, rs.frac_bits);
  a.counts = rs.series.end_a(rs.lay.frame());
  a.tail = rs.series.end_b(rs.lay.tail());
  const bool lds = !c->dbg.refr_global && refr_lds_form(rs.lay.nw, rs.lay.n2);
  const size_t bytes = refr_lds_bytes(rs.lay.nw, rs.lay.n2, lds);
  const PlaneLaunchShape shape = {kRefrThreads, kRefrMaxLdsBytes, kRefrBlocks, kRefrBigPlaneBlocks,
                                         kRefrHugeTailBlocks, kRefrBigPlaneBytes, kRefrLdsFormBytes};
  return plane_launch(c, rs, refr_kernel<true>, refr_kernel<false>, lds, bytes, shape, a, count);
}

// ---- the absolute-frequency series ----
// The records' common checks: an open series, then swrt_raydiag_record's on
// the two slots the call names (slot_b < 0: one snapshot, alpha and tau unused).
int absfreq_series_check(swrt_ctx* c, int slot_a, int slot_b, double tau) {
  if (!c->absfreq.open) return fail(c, SWRT_ERR_STATE, "call swrt_absfreq_series_begin first");
  HIPCHK_RC(lost_check(c));
  if (slot_a < 0 || slot_a >= SWRT_MAX_SLOTS || slot_b < -1 || slot_b >= SWRT_MAX_SLOTS)
    return fail(c, SWRT_ERR_ARG, "slot out of range");
  if (slot_a == slot_b) return fail(c, SWRT_ERR_ARG, "slot_a and slot_b must differ");
  if (!c->slot[slot_a].set || (slot_b >= 0 && !c->slot[slot_b].set)) return fail(c, SWRT_ERR_ARG, "field slot not set");
  if (slot_b >= 0) {
    const Slot &sa = c->slot[slot_a], &sb = c->slot[slot_b];
    if (sb.nx != sa.nx || sb.L != sa.L || sb.ny_period != sa.ny_period)
      return fail(c, SWRT_ERR_ARG, "slots a and b have different grids");
    if (!std::isfinite(tau) || tau == 0.0) return fail(c, SWRT_ERR_ARG, "tau must be finite and non-zero");
  }
  HIPCHK_RC(packets_check(c));
  if (c->n > kAbsfreqMaxPackets)
    return fail(c, SWRT_ERR_ARG, "an absolute-frequency frame takes at most 2^24 packets");
  return SWRT_OK;
}

// The slots a record reads, for SlotUse (out-of-range arguments: none; the
// check refuses them before anything is queued).
inline unsigned absfreq_slot_mask(int slot_a, int slot_b) {
  unsigned m = 0u;
  if (slot_a >= 0 && slot_a < SWRT_MAX_SLOTS) m |= 1u << slot_a;
  if (slot_b >= 0 && slot_b < SWRT_MAX_SLOTS) m |= 1u << slot_b;
  return m;
}

// `count` frames from the series' end on: frame i from the packets at
// x + i*stride, k + i*stride (any order) and the flow of slots a and b at
// alphas[i] (device; NULL: `alpha` for every frame).  The LDS kernel for
// absfreq_lds_form's shapes, the global one beyond (or when
// SWRT_DEBUG_ABSFREQ_GLOBAL says so).
int absfreq_launch(swrt_ctx* c, int slot_a, int slot_b, double alpha, const double* alphas, double tau, double bump,
                   const double* x, const double* k, int64_t stride, int64_t count) {
  AbsfreqSeriesState& as = c->absfreq;
  AbsfreqArgs a;
  a.fa = view_of(c->slot[slot_a]);
  a.fb = slot_b >= 0 ? view_of(c->slot[slot_b]) : a.fa;
  a.two = slot_b >= 0 ? 1 : 0;
  a.alpha = alpha;
  a.tau = slot_b >= 0 ? tau : 1.0;
  a.bump = bump;
  a.alphas = alphas;
  a.x = x;
  a.k = k;
  a.stride = stride;
  a.n = c->n;
  a.f2 = as.f2;
  a.Cg2 = as.Cg2;
  a.wedges = as.edges.get();
  a.oedges = as.edges.get() + as.lay.nw + 1;
  a.nw = as.lay.nw;
  a.no = as.lay.n2;
  a.scale = std::ldexp(1.0, as.frac_bits);
  a.counts = as.series.end_a(as.lay.frame());
  a.tail = as.series.end_b(as.lay.tail());
  const bool lds = !c->dbg.absfreq_global && absfreq_lds_form(as.lay.nw, as.lay.n2);
  const size_t bytes = absfreq_lds_bytes(as.lay.nw, as.lay.n2, lds);
  const PlaneLaunchShape shape = {kAbsfreqThreads, kAbsfreqMaxLdsBytes, kAbsfreqBlocks, kAbsfreqBigPlaneBlocks,
                                         kAbsfreqHugeTailBlocks, kAbsfreqBigPlaneBytes, kAbsfreqLdsFormBytes};
  return plane_launch(c, as, absfreq_kernel<true>, absfreq_kernel<false>, lds, bytes, shape, a, count);
}

// ---- the tangent map ----
static_assert(kTanWSums == kRefrWSums && kTanStats == 3,
              "TangentState's PlaneLayout (swrt_ctx.hpp) and refr_lds_bytes restate what tangent_record_kernel writes");

// A mark, queued: M = I, the counters 0, a new serial.
int tangent_mark_queue(swrt_ctx* c) {
  TangentState& ts = c->tan;
  if (c->hz.on) {
    HazardChecker& h = c->hz;
    if (!hz_whole(h, h.op(0), kHzWrite, "a tangent mark", {ts.M.get(), ts.caustics.get()}))
      return fail(c, SWRT_ERR_STATE, h.err);
  }
  hipLaunchKernelGGL(tangent_mark_kernel, dim3(nblocks(ts.n * kTanM, kTanThreads)), dim3(kTanThreads), 0, c->stream, ts.n,
                     TangentArgs{ts.M.get(), ts.caustics.get()});
  HIPCHK(c, hipGetLastError());
  ++ts.serial;
  return SWRT_OK;
}

// The calls that need a live set.
int tangent_check(swrt_ctx* c) {
  if (!c->tan.live) return fail(c, SWRT_ERR_STATE, "no tangent set is live (swrt_tangent_begin first)");
  return packets_check(c);
}

// One frame at the series' end from the current packets and their M rows: the
// LDS kernel for refr_lds_form's shapes (the tail has the refraction series'
// shape), the global one beyond (or when SWRT_DEBUG_TANGENT_GLOBAL says so).
int tangent_record_launch(swrt_ctx* c) {
  TangentState& ts = c->tan;
  TangentRecordArgs a;
  a.k = c->pk.cur.k.get();
  a.perm = c->pk.cur.perm.get();
  a.M = ts.M.get();
  a.caustics = ts.caustics.get();
  a.n = c->n;
  a.f2 = ts.f2;
  a.Cg2 = ts.Cg2;
  a.wedges = ts.edges.get();
  a.sedges = ts.edges.get() + ts.lay.nw + 1;
  a.nw = ts.lay.nw;
  a.ns = ts.lay.n2;
  a.serial = (unsigned long long)ts.serial;
  a.counts = ts.series.end_a(ts.lay.frame());
  a.tail = ts.series.end_b(ts.lay.tail());
  if (c->hz.on) {
    HazardChecker& h = c->hz;
    if (!hz_whole(h, h.op(0), kHzRead, "a tangent record", {a.k, a.perm, a.M, a.caustics}))
      return fail(c, SWRT_ERR_STATE, h.err);
  }
  const bool lds = !c->dbg.tangent_global && refr_lds_form(ts.lay.nw, ts.lay.n2);
  const size_t bytes = refr_lds_bytes(ts.lay.nw, ts.lay.n2, lds);
  const PlaneLaunchShape shape = {kTanThreads, kRefrMaxLdsBytes, kRefrBlocks, kRefrBigPlaneBlocks, kRefrHugeTailBlocks,
                                  kRefrBigPlaneBytes, kRefrLdsFormBytes};
  return plane_launch(c, ts, tangent_record_kernel<true>, tangent_record_kernel<false>, lds, bytes, shape, a, 1);
}

}  // namespace
