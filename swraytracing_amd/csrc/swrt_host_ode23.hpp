// swrt_host_ode23.hpp — host side of the ode23 device stages (swrt_ode23.hpp):
// stage buffers, the stage and attempt launches, swrt_ode23_run's executor
// for the controller (swrt_ode23_ctl.cpp) and the chain that queues the next
// call's stage 1 and first attempt.
#pragma once
#include <atomic>
#include <chrono>
#include <cmath>

#include "swrt_ctx.hpp"
#include "swrt_host_fields.hpp"
#include "swrt_host_packets.hpp"
#include "swrt_ode23.hpp"
#include "swrt_ode23_ctl.hpp"
#include "swrt_share.hpp"

namespace {

// ode23 calls per spatial re-binning (ode23_f1_queue)
#ifndef SWRT_ODE23_REBIN
#define SWRT_ODE23_REBIN 2  // every 1 / 2 / 4 calls: 1.843-1.845 / 1.824-1.830 / 1.878-1.892 ms per driver interval (profiles/r05_ode23)
#endif
constexpr int kOde23RebinEvery = SWRT_ODE23_REBIN;

int ode23_prepare(swrt_ctx* c, int nslots, Ode23Args& a, double tmax, double f, double Cg, double thr,
                  double bump) {
  if (c->n <= 0 || !c->pk.cur.x) return fail(c, SWRT_ERR_STATE, "no packets (swrt_packets_set)");
  if (nslots != 1 && nslots != 2) return fail(c, SWRT_ERR_ARG, "nslots must be 1 or 2");
  if (!c->slot[0].set || (nslots == 2 && !c->slot[1].set)) return fail(c, SWRT_ERR_STATE, "field slot not set");
  if (nslots == 2 && c->slot[1].nx != c->slot[0].nx) return fail(c, SWRT_ERR_ARG, "slots differ in nx");
  if (c->o23.cap < c->cap) {
    c->o23.cap = 0;
    for (DevBuf<double>& b : c->o23.F) HIPCHK(c, b.alloc(4 * c->cap));
    for (DevBuf<double>* b : {&c->o23.ynx, &c->o23.ynk, &c->o23.spx, &c->o23.spk}) HIPCHK(c, b->alloc(2 * c->cap));
    HIPCHK(c, c->o23.spF.alloc(4 * c->cap));
    c->o23.cap = c->cap;
  }
  if (!c->o23.dmax) {  // 3 max slots per part (part 1: split attempts)
    HIPCHK(c, c->o23.dmax.alloc(6));
    HIPCHK(c, hipMemsetAsync(c->o23.dmax.get(), 0, 6 * sizeof(unsigned long long), c->stream));
    c->o23.dmax_cur = 0;
  }
  if (!c->o23.hmax) HIPCHK(c, c->o23.hmax.alloc(3));
  if (!c->o23.hpart) {
    // coherent (fine-grained): the attempt kernels' stores reach host memory
    // without the system-scope release of a separate event marker
    HIPCHK(c, c->o23.hpart.alloc(6 * kMaxBins, hipHostMallocMapped | hipHostMallocCoherent));
    std::fill(c->o23.hpart.get(), c->o23.hpart.get() + 6 * kMaxBins, kHpartEmpty);
  }
  if (!c->o23.shown) {
    HIPCHK(c, c->o23.coef.alloc(8));
    HIPCHK(c, c->o23.shown.alloc(13, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(c->o23.shown.get(), 0, 13 * sizeof(double));  // (ticket 0: never a launch's)
  }
  for (Event& e : c->o23.ev)
    if (!e) HIPCHK(c, e.create());
  for (Event& e : c->o23.evb)
    if (!e) HIPCHK(c, e.create());
  a.f0 = view_of(c->slot[0]);
  a.f1 = nslots == 2 ? view_of(c->slot[1]) : a.f0;
  a.nslots = nslots;
  a.n = c->n;
  a.yx = c->pk.cur.x.get();
  a.yk = c->pk.cur.k.get();
  for (int s = 0; s < 4; ++s) a.F[s] = c->o23.F[s].get();
  a.ynx = c->o23.ynx.get();
  a.ynk = c->o23.ynk.get();
  a.tmax = tmax;
  a.inv_tmax = 0.0;
  a.f2 = f * f;
  a.Cg = Cg;
  a.Cg2 = Cg * Cg;
  a.fastdisp = dispersion_fast(a.f2);
  a.thr = thr;
  a.bump = bump;
  a.dmax = c->o23.dmax.get() + c->o23.dmax_cur;
  a.dmax_clear = c->o23.dmax.get() + (c->o23.dmax_cur + 1) % 3;
  a.gate = nullptr;
  a.gate_scale = 0.0;
  a.gate_limit = 0.0;
  a.order = nullptr;
  a.hpart = nullptr;
  a.sh = TileShare{};
  a.coef = nullptr;
  return SWRT_OK;
}

// an attempt's stage times and coefficients (swrt_ode23.hpp o23_coeffs)
void attempt_coeffs(Ode23Args& a, double t, double h, double tnew) {
  double cf[8];
  o23_coeffs(t, h, tnew, cf);
  a.ts = cf[0];
  a.c[0] = cf[1];
  a.ts3 = cf[2];
  a.c3 = cf[3];
  a.ts4 = cf[4];
  a.c4[0] = cf[5];
  a.c4[1] = cf[6];
  a.c4[2] = cf[7];
}

// the max of the launch just queued (slot o_dmax_cur), then the next slot
int read_max(swrt_ctx* c, double* out) {
  const int slot = c->o23.dmax_cur;
  c->o23.dmax_cur = (slot + 1) % 3;
  if (!out) return SWRT_OK;
  HIPCHK(c, hipMemcpyAsync(c->o23.hmax.get() + slot, c->o23.dmax.get() + slot, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, c->stream));
  // (spinning on an event instead measured within noise: 2.55-2.59 vs 2.60-2.62 ms)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(out, c->o23.hmax.get() + slot, sizeof(double));
  return dev_err_check(c);
}

// one ode23 stage over all packets: the LDS-tiled kernel when the packets are
// binned by the tile kernel's 16x16-cell tiles, else one lane per packet
template <int STAGE, bool TWO, bool V5>
void ode23_tile_launch(swrt_ctx* c, const Ode23Args& a, unsigned grid, const int* starts, int ntx, hipStream_t st,
                       hipEvent_t stop, bool dense) {
  if constexpr (STAGE == 0) {
    if (dense) {  // F2 and F3 kept for ode23_ntrp_kernel (never with device coefficients)
      hipExtLaunchKernelGGL((tile_ode23_kernel<0, TWO, kTile, kMargin, kTileThreads, V5, false, true>), dim3(grid),
                            dim3(kTileThreads), 0, st, nullptr, stop, 0, a, starts, ntx);
      return;
    }
    if (a.coef) {  // coefficients from device memory (swrt_ode23_run's first attempt)
      hipExtLaunchKernelGGL((tile_ode23_kernel<0, TWO, kTile, kMargin, kTileThreads, V5, true>), dim3(grid),
                            dim3(kTileThreads), 0, st, nullptr, stop, 0, a, starts, ntx);
      return;
    }
  }
  hipExtLaunchKernelGGL((tile_ode23_kernel<STAGE, TWO, kTile, kMargin, kTileThreads, V5>), dim3(grid),
                        dim3(kTileThreads), 0, st, nullptr, stop, 0, a, starts, ntx);
}

// swrt_ode23_run may split each attempt into two part launches (the even and
// the odd band positions of every XCD band, swrt_share.hpp), part 1 on the
// extra packet stream: consecutive attempts then overlap one part's tail with
// the other's next launch.  Parts touch disjoint packets of one binning, so
// stream order alone orders each part's attempts; the packets must already be
// in the tiles' cell order (no order kernel between the parts).
bool ode23_split_ok(swrt_ctx* c) {
  const int ntx = tiles_per_side(c->slot[0].nx);
  return tile_binned(c) && c->bin.ode23_is_sorted() && (ntx * ntx) % 16 == 0 && c->n >= kMultiStreamFrom &&
         c->packet_streams == 2 && c->stream == c->stream0.get() && c->sx[0].get() != nullptr;
}

// part -1: one launch over every tile on the packet stream; 0 / 1: that part
// of a split attempt (part 1 on sx[0]).  *wg_out: the workgroups of the tile
// launch (each stores its max to a.hpart, whose host copy is first marked
// empty), 0 for the per-packet kernels.  `stop`: an event the tile launch
// itself completes (*stop_done = true) — no marker between consecutive
// attempts (a separate event record cost ~7 us of idle stream per launch,
// profiles/r06_ode23); the per-packet kernels leave it to the caller.
// `dense` (STAGE 0): the tile kernel also stores F2 and F3, as the per-packet
// stage kernels always do.
template <int STAGE>
int ode23_launch(swrt_ctx* c, const Ode23Args& a0, int part = -1, unsigned* wg_out = nullptr,
                 hipEvent_t stop = nullptr, bool* stop_done = nullptr, bool dense = false) {
  if (wg_out) *wg_out = 0;
  if (stop_done) *stop_done = false;
  const int ntx = tiles_per_side(c->slot[0].nx);
  if (part >= 0 && !ode23_split_ok(c)) return fail(c, SWRT_ERR_STATE, "ode23 split attempt without a split binning");
  if (tile_binned(c)) {
    const int* starts = c->bins.starts();
    const unsigned ntiles = (unsigned)(ntx * ntx);
    Ode23Args a = a0;
    a.sh = TileShare{(int)ntiles, part, part < 0 ? 1 : 2, kShareEven};
    const unsigned grid = (unsigned)share_grid(a.sh);
    const hipStream_t st = part == 1 ? c->sx[0].get() : c->stream;
    if (wg_out) *wg_out = grid;
    // in-tile cell order of this binning, once (swrt_ode23.hpp): the packets'
    // own order after swrt_ode23_f1's sort, else an order array
    if (!c->bin.ode23_is_sorted() && !c->bin.ode23_order()) {
      if (c->o23.order_cap < c->cap) {
        HIPCHK(c, c->o23.order.alloc(c->cap));
        c->o23.order_cap = c->cap;
      }
      const FieldView v = view_of(c->slot[0]);
      hipLaunchKernelGGL((tile_cell_order_kernel<kTile, kTileThreads>), dim3(grid), dim3(kTileThreads), 0,
                         c->stream, c->pk.cur.x.get(), c->n, starts, ntx, v.inv_dx, v.nx, c->o23.order.get());
      HIPCHK(c, hipGetLastError());
      c->bin.ode23_order_built();
    }
    a.order = c->bin.ode23_is_sorted() ? nullptr : c->o23.order.get();
    if (a.hpart) {
      unsigned long long* hh = c->o23.hpart.get() + (a.hpart - c->o23.hpart.dev());
      std::fill(hh, hh + grid, kHpartEmpty);
    }
    const bool v5 = c->slot[0].div_free && (a.nslots == 1 || c->slot[1].div_free);
    if (a.nslots == 2) {
      if (v5) ode23_tile_launch<STAGE, true, true>(c, a, grid, starts, ntx, st, stop, dense);
      else ode23_tile_launch<STAGE, true, false>(c, a, grid, starts, ntx, st, stop, dense);
    } else {
      if (v5) ode23_tile_launch<STAGE, false, true>(c, a, grid, starts, ntx, st, stop, dense);
      else ode23_tile_launch<STAGE, false, false>(c, a, grid, starts, ntx, st, stop, dense);
    }
    if (stop_done) *stop_done = stop != nullptr;
  } else if constexpr (STAGE == 0) {  // one lane per packet: the three stage launches
    const dim3 grid(nblocks(c->n, 256)), block(256);
    Ode23Args b = a0;
    hipLaunchKernelGGL(ode23_stage_kernel<2>, grid, block, 0, c->stream, b);
    b.ts = a0.ts3;
    b.c[0] = a0.c3;
    hipLaunchKernelGGL(ode23_stage_kernel<3>, grid, block, 0, c->stream, b);
    b.ts = a0.ts4;
    for (int i = 0; i < 3; ++i) b.c[i] = a0.c4[i];
    hipLaunchKernelGGL(ode23_stage_kernel<4>, grid, block, 0, c->stream, b);
  } else {
    hipLaunchKernelGGL(ode23_stage_kernel<STAGE>, dim3(nblocks(c->n, 256)), dim3(256), 0, c->stream, a0);
  }
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}

// swrt_ode23_f1 without the read: re-binning, in-tile sort and the stage-1
// launch queued (its max in slot o_dmax_cur, not yet advanced)
int ode23_f1_queue(swrt_ctx* c, double t, double tmax, double f, double Cg, int nslots, double thr, double bump) {
  HIPCHK(c, hipSetDevice(c->device));
  c->o23.dense_ready = false;  // (F1 is rewritten, perhaps in another packet order)
  int rc;
  // a spatial re-binning per kOde23RebinEvery ode23 calls (the packet order
  // is free: the error norm is a max over all components; a packet that has
  // left its tile's window since takes the global gather, so a skipped
  // re-binning changes speed only)
  const bool binned = tile_binned(c) && c->bin.tile() == kTile && c->bin.ode23_is_sorted();
  const bool due = !binned || c->bin.ode23_call_due(kOde23RebinEvery);
  if (c->rebin_every > 0 && c->slot[0].set && due) {
    if ((rc = rebin(c, false, use_tile_kernel(c) ? kTile : 0))) return rc;  // the ode23 tile kernel's 16x16 tiles
    if (tile_binned(c)) {
      // the in-tile cell order applied to the packets (swrt_ode23.hpp tile_cell_sort_kernel)
      const FieldView v = view_of(c->slot[0]);
      const int ntx = tiles_per_side(c->slot[0].nx);
      const PacketSet &in = c->pk.cur, &out = c->pk.out;
      hipLaunchKernelGGL((tile_cell_sort_kernel<kTile, kTileThreads>), dim3((unsigned)(ntx * ntx)),
                         dim3(kTileThreads), 0, c->stream, (const double*)in.x.get(), (const double*)in.k.get(),
                         (const int*)in.perm.get(), c->n, (const int*)c->bins.starts(), ntx, v.inv_dx, (int)v.nx,
                         out.x.get(), out.k.get(), out.perm.get());
      HIPCHK(c, hipGetLastError());
      c->pk.flip();
      c->bin.ode23_sorted();  // (and restarts the count of calls until the next re-binning)
    }
  }
  Ode23Args a;
  if ((rc = ode23_prepare(c, nslots, a, tmax, f, Cg, thr, bump))) return rc;
  a.ts = t;
  return ode23_launch<1>(c, a);
}

double o23_alpha(double t, double tmax) { return tmax != 0.0 ? t / tmax : 0.0; }  // the kernels' alpha_of

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// The first-step kernel (the first attempt's step size on the device) on the
// packet stream, stage 1's max slot event o_ev[sl_f1] attached to it: the
// first attempt's part 0 follows it with no marker between them, part 1 waits
// for that event, and the host reads the step size once the launch's ticket
// has reached shown[12] (DeviceExec::stage1).  (A marker after it instead
// cost ~7-12 us of idle GPU before the first attempt, profiles/r06_ode23.)
int ode23_first_step_queue(swrt_ctx* c, int sl_f1, double c0, double hmax, double htspan, double t0, double tfinal,
                           bool split, uint64_t* ticket) {
  const double tdir = std::copysign(1.0, tfinal - t0);
  const uint64_t tk = ++c->o23.ticket;
  const hipEvent_t stop = c->o23.ev[sl_f1].get();
  // (part 1's slots start at zero, cleared here; each launch then clears its next one)
  hipExtLaunchKernelGGL(ode23_first_step_kernel, dim3(1), dim3(64), 0, c->stream, nullptr, stop, 0,
                        c->o23.dmax.get() + sl_f1, c0, hmax, htspan, 16 * o23_spacing(t0), tdir, t0, tfinal,
                        c->o23.coef.get(), c->o23.shown.dev(), c->o23.dmax.get() + 3, split ? 3 : 0,
                        (unsigned long long)tk);
  HIPCHK(c, hipGetLastError());
  *ticket = tk;
  return SWRT_OK;
}

// swrt_ode23_run's stages for the controller (ode23_control, swrt_ode23_ctl.cpp):
// each attempt one tile launch — two part launches when the binning allows
// (ode23_split_ok), part 1 on the extra packet stream, part p keeping max
// slots o_dmax[3p + sl] and its own events — its maxima read from host-mapped
// memory after the launch's event; three state sets (x, k, F1/F4): an attempt
// reads set `from` and writes ynew and F4 into set `to`.
class DeviceExec final : public O23Exec {
 public:
  DeviceExec(swrt_ctx* c_, const Ode23Args& base_, bool split_, bool dev_first_, int sl_f1_, void (*hook_)(void*),
             void* hook_user_, int (*reduce_)(double*, void*) = nullptr, void* reduce_user_ = nullptr)
      : c(c_), base(base_), split(split_), P(split_ ? 2 : 1), dev_first(dev_first_), sl_f1(sl_f1_), hook(hook_),
        hook_user(hook_user_), reduce(reduce_), reduce_user(reduce_user_),
        S{{c_->pk.cur.x.get(), c_->pk.cur.k.get(), c_->o23.F[0].get()},
          {c_->o23.ynx.get(), c_->o23.ynk.get(), c_->o23.F[3].get()},
          {c_->o23.spx.get(), c_->o23.spk.get(), c_->o23.spF.get()}} {}

  // queue an attempt (coef: its coefficients from device memory, the first attempt)
  int launch(int from, int to, double ta, double ha, double tnewa, int gate_slot, double gscale, double glimit,
             int* slot, const double* coef) {
    Ode23Args a = base;
    a.coef = coef;
    a.yx = S[from].x;
    a.yk = S[from].k;
    a.F[0] = S[from].F;
    a.F[3] = S[to].F;
    a.ynx = S[to].x;
    a.ynk = S[to].k;
    attempt_coeffs(a, ta, ha, tnewa);
    const int sl = c->o23.dmax_cur;
    // The host polls a slot's maxima without waiting for the launch's event
    // (wait_max), so a launch whose maxima were never read (a guess its
    // gate discarded; in a sharded run one that ran on this rank's part of
    // the max) must have finished before its slot's host copy is re-marked
    // empty for this launch.  Its events still hold that launch.
    if (unread[sl]) {
      HIPCHK(c, hipEventSynchronize(c->o23.ev[sl].get()));
      if (P == 2) HIPCHK(c, hipEventSynchronize(c->o23.evb[sl].get()));
    }
    unread[sl] = true;
    a.gate_scale = gscale;
    a.gate_limit = glimit;
    for (int p = 0; p < P; ++p) {
      a.dmax = c->o23.dmax.get() + 3 * p + sl;
      a.dmax_clear = c->o23.dmax.get() + 3 * p + (sl + 1) % 3;
      // a part's guess is gated on its own part of the previous max: when the
      // whole max passes, so does every part (err = absh * max is monotone)
      a.gate = gate_slot >= 0 ? c->o23.dmax.get() + 3 * p + gate_slot : nullptr;
      a.hpart = c->o23.hpart.dev() + (size_t)(3 * p + sl) * kMaxBins;
      const hipStream_t st = p == 0 ? c->stream : c->sx[0].get();
      const hipEvent_t ev = p == 0 ? c->o23.ev[sl].get() : c->o23.evb[sl].get();
      bool attached = false;
      HIPCHK_RC((ode23_launch<0>(c, a, split ? p : -1, &wg[p][sl], ev, &attached)));
      if (!attached) {
        if (wg[p][sl] == 0)  // the per-packet stage kernels (never split): copy the max
          HIPCHK(c, hipMemcpyAsync(c->o23.hmax.get() + sl, c->o23.dmax.get() + sl, sizeof(unsigned long long),
                                   hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipEventRecord(ev, st));
      }
    }
    c->o23.dmax_cur = (sl + 1) % 3;
    if (P == 2) b_last = sl;  // the extra stream's last work
    *slot = sl;
    return SWRT_OK;
  }
  // the device's first attempt, from its own step size (before the hook)
  int queue_first() { return launch(0, 1, 0.0, 0.0, 0.0, -1, 0.0, 0.0, &first_slot, c->o23.coef.get()); }
  int first() const { return first_slot; }
  unsigned workgroups(int p, int sl) const { return wg[p][sl]; }
  // the first attempt the previous call queued (ode23_chain_first): its slot
  // and workgroups; the hook then waits for the first wait_max, so the
  // controller queues its next guess before the hook's host work
  void adopt_first(int sl, const unsigned wg_[2]) {
    first_slot = sl;
    unread[sl] = true;
    if (P == 2) b_last = sl;
    wg[0][sl] = wg_[0];
    wg[1][sl] = wg_[1];
    defer_hook = true;
  }

  int run_hook() {
    // the hook may call the library (e.g. the next QG step on the QG stream);
    // it must not touch the packets (c->in_hook refuses those calls).  Its
    // calls must not join the extra stream's attempt parts into the packet
    // stream (they run on), so the split is hidden from them and re-marked after.
    hook_due = false;
    c->b_pending = 0;
    c->in_hook = true;
    hook(hook_user);
    c->in_hook = false;
    if (split) c->b_pending = 1;
    return SWRT_OK;
  }

  int stage1(double* raw) override {
    if (hook) {
      hook_due = true;
      if (!defer_hook) HIPCHK_RC(run_hook());
    }
    // (the first-step kernel's values: read once its ticket is in, no event wait)
    if (!dev_first) HIPCHK(c, hipEventSynchronize(c->o23.ev[sl_f1].get()));
    if (dev_first) {
      HIPCHK_RC(await_shown());
      std::memcpy(raw, &c->o23.shown[0], sizeof(double));
    } else
      std::memcpy(raw, c->o23.hmax.get() + sl_f1, sizeof(double));
    HIPCHK_RC(dev_err_check(c));
    return global_max(raw);
  }
  // a sharded run: this rank's max -> the max over every rank (the caller's
  // collective, e.g. an RCCL all_reduce), in place
  int global_max(double* v) {
    if (reduce && reduce(v, reduce_user) != 0) return fail(c, SWRT_ERR_STATE, "ode23: the reduce callback failed");
    return SWRT_OK;
  }
  bool first_attempt(double absh, double h, double tnew, const double cf[8], int* slot) override {
    if (!dev_first) return false;
    // the host's computation against the kernel's mapped copy
    bool same = absh == c->o23.shown[1] && h == c->o23.shown[2] && tnew == c->o23.shown[3];
    for (int i = 0; i < 8; ++i) same = same && cf[i] == c->o23.shown[4 + i];
    *slot = first_slot;
    return same;  // else left to be overwritten by the attempt queued from the host's values
  }
  int queue(int from, int to, double t, double h, double tnew, int gate_slot, double gate_scale, double gate_limit,
            int* slot) override {
    return launch(from, to, t, h, tnew, gate_slot, gate_scale, gate_limit, slot, nullptr);
  }
  // the raw error max of the attempt in slot sl: the bit-pattern max (= the
  // value max of these non-negative doubles, as the device's atomicMax)
  int wait_max(int sl, double* out) override {
    if (hook_due) HIPCHK_RC(run_hook());
    unread[sl] = false;
    unsigned long long m = 0;
    for (int p = 0; p < P; ++p) {
      const unsigned g = wg[p][sl];
      // The tile launches' maxima are polled in host memory, every workgroup
      // storing its own at its end: no wait for the launch's event, whose
      // host wake-up trailed the kernel by ~10-20 us (the end of an interval
      // waits for it, profiles/r06_ode23).  The per-packet kernels' copied
      // max is read after its event.
      // (polling hipEventQuery instead: 1.802 / 1.831 vs 1.849 / 1.805 ms, noise; profiles/r05_ode23)
      if (g == 0) HIPCHK(c, hipEventSynchronize(p == 0 ? c->o23.ev[sl].get() : c->o23.evb[sl].get()));
      if (g == 0) {
        m = std::max(m, c->o23.hmax[sl]);
      } else {
        // (after an event too: the launch's own completion event carries no
        // system-scope release, so a store may land a moment after it)
        const volatile unsigned long long* hp = c->o23.hpart.get() + (size_t)(3 * p + sl) * kMaxBins;
        for (unsigned i = 0; i < g; ++i) {
          unsigned long long v = hp[i];
          if (v == kHpartEmpty) HIPCHK_RC(await_hpart(hp + i, p, &v));
          m = std::max(m, v);
        }
      }
    }
    if (c->hz.on) {  // debug: the host-mapped maxima against the device's atomicMax slots
      unsigned long long d = 0;
      for (int p = 0; p < P; ++p) {
        unsigned long long v = 0;
        HIPCHK(c, hipMemcpy(&v, c->o23.dmax.get() + 3 * p + sl, sizeof(v), hipMemcpyDeviceToHost));
        d = std::max(d, v);
      }
      if (d != m) return fail(c, SWRT_ERR_STATE, "ode23: host-mapped error max differs from the device's");
    }
    std::memcpy(out, &m, sizeof(double));
    return global_max(out);
  }
  // the first-step launch's values, once its ticket is in shown[12] (its
  // event has completed; the values may land a moment after it)
  void expect_ticket(uint64_t t) { ticket = t; }
  int await_shown() {
    const volatile unsigned long long* tk =
        reinterpret_cast<const volatile unsigned long long*>(c->o23.shown.get() + 12);
    const auto t0 = std::chrono::steady_clock::now();
    while (*tk != ticket) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(100)) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (*tk != ticket) return fail(c, SWRT_ERR_STATE, "ode23: the first step size never reached host memory");
        break;
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return SWRT_OK;
  }
  int await_hpart(const volatile unsigned long long* e, int p, unsigned long long* out) {
    const auto t0 = std::chrono::steady_clock::now();
    while ((*out = *e) == kHpartEmpty) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(100)) {
        HIPCHK(c, hipStreamSynchronize(p == 0 ? c->stream : c->sx[0].get()));
        if ((*out = *e) == kHpartEmpty)
          return fail(c, SWRT_ERR_STATE, "ode23: a workgroup's error max never reached host memory");
        break;
      }
    }
    return SWRT_OK;
  }
  // The extra stream's part launches ordered before the packet stream's next
  // work; set `cur` becomes the packets (and F1), the others the spares.
  int finish(int cur, bool failed) override {
    if (split) {
      if (!failed && b_last >= 0) {
        // the join is the extra stream's last launch's own event (a marker
        // recorded there would put ~7 us between the last attempt and the
        // next work); none once it has completed
        const hipEvent_t ev = c->o23.evb[b_last].get();
        const hipError_t q = hipEventQuery(ev);
        if (q == hipErrorNotReady)
          HIPCHK(c, hipStreamWaitEvent(c->stream0.get(), ev, 0));
        else
          HIPCHK(c, q);
        c->b_pending = 0;
        if (c->hz.on) {
          c->hz.record(ev, 1);
          c->hz.wait(0, ev);
        }
      } else {
        c->b_pending = 1;
        HIPCHK_RC(join_b(c));
      }
    }
    if (failed) HIPCHK(c, hipStreamSynchronize(c->stream));  // a queued guess may still be running
    // the owning handles of the three sets, rotated so that set (cur + i) % 3
    // of this run becomes set i: two swaps of whole sets
    Ode23State& o = c->o23;
    DevBuf<double>* H[3][3] = {{&c->pk.cur.x, &c->pk.cur.k, &o.F[0]}, {&o.ynx, &o.ynk, &o.F[3]}, {&o.spx, &o.spk, &o.spF}};
    auto swap_sets = [&](int i, int j) {
      for (int m = 0; m < 3; ++m) std::swap(*H[i][m], *H[j][m]);
    };
    if (cur != 0) {
      swap_sets(0, cur);
      swap_sets(1, 2);
    }
    c->bin.packets_replaced();
    return SWRT_OK;
  }

 private:
  swrt_ctx* c;
  Ode23Args base;
  bool split;
  int P;
  bool dev_first;
  int sl_f1;
  int first_slot = -1;
  void (*hook)(void*);
  void* hook_user;
  int (*reduce)(double*, void*);
  void* reduce_user;
  bool defer_hook = false, hook_due = false;
  uint64_t ticket = 0;
  int b_last = -1;  // the max slot of the last part-1 launch (its event: the extra stream's last work)
  bool unread[3] = {false, false, false};  // a launch in this slot whose maxima wait_max has not read
  struct Set {
    double *x, *k, *F;
  } S[3];
  unsigned wg[2][3] = {};  // workgroups of each part's launch in each slot (0: the max was copied)
};

// The next call's first step size and first attempt, queued behind the stage
// 1 the chain just queued (slots arranged as that call's 0 / 1): what
// swrt_ode23_run_hooked queues for t0 = 0, tfinal = tmax and `rtol`, on the
// tile path only.  Part 1 of a split attempt stays unjoined (c->o23.chain_b); the
// slots' use mark of this call covers it (c->tail_ev, after sx[0] has waited
// for the packet stream's tail).
int ode23_chain_first(swrt_ctx* c, int sl_f1, double tmax, double f, double Cg, double thr, double bump,
                      double rtol) {
  Ode23State::O23Chain& ch = c->o23.chain;
  ch.first_q = false;
  if (!c->o23.chain_first || !tile_binned(c)) return SWRT_OK;
  const bool split = ode23_split_ok(c);
  const double t0 = 0.0, tfinal = tmax;
  const double rtol_c = std::max(rtol, 100 * 2.220446049250313e-16);
  const double htspan = std::fabs(tfinal - t0);
  const double hmax = 0.1 * htspan;
  const double c0 = 0.8 * std::pow(rtol_c, 1.0 / 3.0);
  uint64_t ticket = 0;
  HIPCHK_RC(ode23_first_step_queue(c, sl_f1, c0, hmax, htspan, t0, tfinal, split, &ticket));
  if (split) {
    HIPCHK(c, hipStreamWaitEvent(c->sx[0].get(), c->o23.ev[sl_f1].get(), 0));
    if (c->hz.on) {
      c->hz.record(c->o23.ev[sl_f1].get(), 0);
      c->hz.wait(1, c->o23.ev[sl_f1].get());
    }
  }
  Ode23Args base;
  int rc;
  if ((rc = ode23_prepare(c, 2, base, tmax, f, Cg, thr, bump))) return rc;
  DeviceExec ex(c, base, split, true, sl_f1, nullptr, nullptr);
  if ((rc = ex.queue_first())) return rc;
  ch.first_ticket = ticket;
  ch.first_slot = ex.first();
  for (int p = 0; p < 2; ++p) ch.first_wg[p] = ex.workgroups(p, ch.first_slot);
  if (split) {
    // one event after both parts: sx[0] waits for part 0's own (attached)
    // event, so no marker lands on the packet stream between the attempt and
    // the next call's next one
    hipEvent_t p0 = c->o23.chain_ev[0].get();
    if (ch.first_wg[0] != 0)
      p0 = c->o23.ev[ch.first_slot].get();
    else
      HIPCHK(c, hipEventRecord(p0, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->sx[0].get(), p0, 0));
    HIPCHK(c, hipEventRecord(c->o23.chain_ev[1].get(), c->sx[0].get()));
    if (c->hz.on) {
      c->hz.record(p0, 0);
      c->hz.wait(1, p0);
    }
    c->tail_ev = c->o23.chain_ev[1].get();
    c->o23.chain_b = true;
  }
  ch.first_q = true;
  ch.split = split;
  ch.rtol = rtol;
  ch.tfinal = tfinal;
  ch.tmax = tmax;  // (the attempt's alpha = t / tmax; stage 1's alpha(0) does not see it)
  return SWRT_OK;
}

// The chain (swrt_ode23_chain_next): at the end of an ode23 call, the next
// call's stage 1 — re-binning when due, in-tile sort, f at t = 0 — queued on
// the accepted packets with the armed slots as slots 0 / 1, so the device runs
// it while the host returns and prepares that call.  The next call takes it
// only if it would compute exactly that (ode23_chain_take).  Behind stage 1
// go the next call's first step size and its first attempt, as that call
// would queue them (ode23_chain_first), taken only if the call's t0, tfinal,
// tmax and RelTol are the ones assumed (never in a sharded run: its first
// step size comes from every rank's stage 1).  (Round 5 chained an unsplit first attempt,
// 186 us against 123 us split, and measured no faster: profiles/r05_chain.)
int ode23_chain_queue(swrt_ctx* c, double tmax, double f, double Cg, int nslots, double thr, double bump,
                      double rtol, bool with_first) {
  Ode23State::O23Chain& ch = c->o23.chain;
  const bool want = ch.want;
  ch.want = false;
  ch.queued = false;
  ch.first_q = false;
  if (!want || nslots != 2 || ch.sa < 0 || ch.sb < 0 || ch.sa == ch.sb || c->packets_lost) return SWRT_OK;
  if (!c->slot[ch.sa].set || !c->slot[ch.sb].set || c->slot[ch.sa].nx != c->slot[ch.sb].nx) return SWRT_OK;
  slot_writes_wait(c);  // e.g. the hook's snapshot into slot sb on the QG stream
  // the armed slots as slots 0 / 1 for the launches below (they read no
  // other slot), by swaps undone in reverse order: `at` is where slot sb's
  // record sits after the first swap
  const int at = ch.sb == 0 ? ch.sa : ch.sb;
  std::swap(c->slot[0], c->slot[ch.sa]);
  std::swap(c->slot[1], c->slot[at]);
  int rc = ode23_f1_queue(c, 0.0, tmax, f, Cg, 2, thr, bump);
  const int sl_f1 = c->o23.dmax_cur;
  if (!rc) {
    c->o23.dmax_cur = (sl_f1 + 1) % 3;
    if (with_first) rc = ode23_chain_first(c, sl_f1, tmax, f, Cg, thr, bump, rtol);
  }
  std::swap(c->slot[1], c->slot[at]);
  std::swap(c->slot[0], c->slot[ch.sa]);
  if (rc) return rc;
  ch.dmax_slot = sl_f1;
  for (int i = 0; i < 2; ++i) {
    const Slot& s = c->slot[i == 0 ? ch.sa : ch.sb];
    ch.nodes[i] = s.nodes.get();
    ch.wgen[i] = s.wgen;
  }
  ch.alpha = o23_alpha(0.0, tmax);
  ch.f = f;
  ch.Cg = Cg;
  ch.thr = thr;
  ch.bump = bump;
  ch.queued = true;
  return SWRT_OK;
}

// The queued chain is this call's stage 1: nothing touched the packets since
// (GUARD_BEGIN drops the chain), slots 0 / 1 hold the same, unrewritten nodes,
// and stage 1's inputs are the same bits.
bool ode23_chain_take(swrt_ctx* c, double t0, double tmax, double f, double Cg, int nslots, double thr,
                      double bump) {
  Ode23State::O23Chain& ch = c->o23.chain;
  const bool q = ch.queued;
  ch.queued = false;
  if (!q || nslots != 2) return false;
  for (int i = 0; i < 2; ++i)
    if (!c->slot[i].set || c->slot[i].nodes.get() != ch.nodes[i] || c->slot[i].wgen != ch.wgen[i]) return false;
  return same_bits(o23_alpha(t0, tmax), ch.alpha) && same_bits(f, ch.f) && same_bits(Cg, ch.Cg) &&
         same_bits(thr, ch.thr) && same_bits(bump, ch.bump);
}

// ---------------------------------------------------------------------------
// Output at requested times (MATLAB ode23 with numel(tspan) > 2): the steps are
// chosen as ever, and the solution at every tspan entry an accepted step
// passes is ntrp23 inside that step (ode23_ntrp_kernel), appended to the
// history as a frame.
// ---------------------------------------------------------------------------

// accept: y = ynew, F1 = F4 (FSAL)
void ode23_accept_sets(swrt_ctx* c) {
  std::swap(c->pk.cur.x, c->o23.ynx);
  std::swap(c->pk.cur.k, c->o23.ynk);
  std::swap(c->o23.F[0], c->o23.F[3]);
  c->bin.packets_replaced();
  c->o23.dense_ready = false;
}

// One attempt on the packet stream and its raw error max (the host waits for
// it; raw NULL: queued only).  ode23: f(:,2) at t + h*A(1), y + f*hB(:,1);
// f(:,3) at t + h*A(2), y + f*hB(:,2); h = tnew - t; ynew = y + f*hB(:,3);
// f(:,4) at tnew — one launch (stage 0: the tile kernel runs the three stages
// per packet, registers between them).  dense: F2 and F3 are kept in memory
// for ode23_ntrp_queue.
int ode23_attempt(swrt_ctx* c, double t, double h, double tnew, double tmax, double f, double Cg, int nslots,
                  double thr, double bump, bool dense, double* raw) {
  Ode23Args a;
  HIPCHK_RC(ode23_prepare(c, nslots, a, tmax, f, Cg, thr, bump));
  attempt_coeffs(a, t, h, tnew);
  HIPCHK_RC(ode23_launch<0>(c, a, -1, nullptr, nullptr, nullptr, dense));
  HIPCHK_RC(read_max(c, raw));
  c->o23.dense_ready = dense;
  return SWRT_OK;
}

// The frames at tout[0 .. nout) of the step from t to tnew whose dense attempt
// sits in the stage buffers (before the accept): kNtrpFrames per launch,
// appended to the history, whose capacity the caller has reserved.
int ode23_ntrp_queue(swrt_ctx* c, double t, double tnew, const double* tout, int64_t nout) {
  if (nout <= 0) return SWRT_OK;
  const int64_t n = c->n;
  if (!c->hist.ext.fits(nout, 2 * n)) return fail(c, SWRT_ERR_STATE, "ode23 ntrp: history capacity not reserved");
  const double h = tnew - t;
  NtrpArgs a;
  a.yx = c->pk.cur.x.get();
  a.yk = c->pk.cur.k.get();
  for (int s = 0; s < 4; ++s) a.F[s] = c->o23.F[s].get();
  a.ynx = c->o23.ynx.get();
  a.ynk = c->o23.ynk.get();
  a.perm = c->pk.cur.perm.get();
  a.n = n;
  // h*BI, BI = [1 -4/3 5/9; 0 1 -2/3; 0 4/3 -8/9; 0 -1 1] (ntrp23.m), column by column
  const double hb[9] = {h * 1.0,         h * (-4.0 / 3.0), h * 1.0,          h * (4.0 / 3.0), h * (-1.0),
                        h * (5.0 / 9.0), h * (-2.0 / 3.0), h * (-8.0 / 9.0), h * 1.0};
  for (int i = 0; i < 9; ++i) a.hb[i] = hb[i];
  for (int64_t i0 = 0; i0 < nout; i0 += kNtrpFrames) {
    a.nf = (int)std::min<int64_t>(kNtrpFrames, nout - i0);
    a.exact = 0u;
    for (int j = 0; j < kNtrpFrames; ++j) {
      const double ti = j < a.nf ? tout[i0 + j] : tnew;
      if (j < a.nf && same_bits(ti, tnew)) a.exact |= 1u << j;
      const double s = (ti - t) / h;
      const double s2 = s * s;
      a.s[j] = s;
      a.s2[j] = s2;
      a.s3[j] = s2 * s;
    }
    a.hx = c->hist.end_a(2 * n);
    a.hk = c->hist.end_b(2 * n);
    hipLaunchKernelGGL(ode23_ntrp_kernel, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    c->hist.ext.committed(a.nf);
  }
  return SWRT_OK;
}

// swrt_ode23_run_at: MATLAB ode23's loop (integrate.py ode23_packets,
// operation for operation, the arithmetic of swrt_ode23_ctl.hpp) over the
// plain sequence stage 1 -> dense attempt -> max -> ntrp -> accept on the
// packet stream: no guessed attempts, no part launches, no chaining.  hmax
// comes from the whole span, the initial step's bound from the first output
// gap (odearguments' htspan); the output times enter nothing else.  Every
// c->o23.dense_rebin accepted steps stage 1 is queued again at the current t
// with a fresh binning: F1 = odefun(t, y) recomputed is the FSAL F4 bit for
// bit, so the cadence changes the speed only.
int ode23_run_at(swrt_ctx* c, const double* tspan, int64_t nt, double tmax, double f, double Cg, int nslots,
                 double rtol, double atol, double bump, double* ts_out, int64_t ts_cap, int64_t* nts_out,
                 O23Stats* st_out) {
  const double t0 = tspan[0], tfinal = tspan[nt - 1];
  const double tdir = std::copysign(1.0, tfinal - t0);
  const double pw = 1.0 / 3.0;
  rtol = std::max(rtol, 100 * 2.220446049250313e-16);
  const double thr = atol / rtol;
  const double hmax = 0.1 * std::fabs(tfinal - t0);
  const double htspan = std::fabs(tspan[1] - tspan[0]);
  const double c0 = 0.8 * std::pow(rtol, pw);
  O23Stats st;
  int64_t nts = 0;
  auto leave = [&](int rc) {
    st.steps = nts > 0 ? nts - 1 : 0;
    *st_out = st;
    *nts_out = nts;
    return rc;
  };
  HIPCHK_RC(ensure_history(c, nt - 1));
  HIPCHK_RC(ode23_f1_queue(c, t0, tmax, f, Cg, nslots, thr, bump));
  double raw = 0.0;
  HIPCHK_RC(read_max(c, &raw));
  double t = t0;
  double absh = o23_initial_absh(raw, c0, hmax, htspan, 16 * o23_spacing(t));
  if (ts_cap > 0) ts_out[0] = t;
  ++nts;
  int64_t next = 1, since_rebin = 0;
  bool done = false;
  while (!done) {
    const double hmin = 16 * o23_spacing(t);
    double h, tnew;
    done = o23_step_head(absh, hmax, hmin, tdir, t, tfinal, h, tnew);
    bool nofailed = true;
    double err;
    while (true) {
      tnew = t + h * 1.0;
      if (done) tnew = tfinal;
      ++st.attempts;
      if (int rc = ode23_attempt(c, t, h, tnew, tmax, f, Cg, nslots, thr, bump, true, &raw)) return leave(rc);
      err = absh * raw;
      h = tnew - t;
      if (err > rtol) {
        ++st.failed;
        if (absh <= hmin) return leave(kO23BelowHmin);
        if (nofailed) {
          nofailed = false;
          absh = std::max(hmin, absh * std::max(0.5, 0.8 * std::pow(rtol / err, pw)));
        } else {
          absh = std::max(hmin, 0.5 * absh);
        }
        h = tdir * absh;
        done = false;
      } else {
        break;
      }
    }
    // the frames of every requested time this step reaches, in order
    int64_t cnt = 0;
    while (next + cnt < nt && tdir * (tnew - tspan[next + cnt]) >= 0) ++cnt;
    if (int rc = ode23_ntrp_queue(c, t, tnew, tspan + next, cnt)) return leave(rc);
    next += cnt;
    ode23_accept_sets(c);
    t = tnew;
    if (nts < ts_cap) ts_out[nts] = t;
    ++nts;
    if (done) break;
    if (nofailed) {
      const double temp = 1.25 * std::pow(err / rtol, pw);
      absh = temp > 0.2 ? absh / temp : 5.0 * absh;
    }
    if (c->o23.dense_rebin > 0 && c->rebin_every > 0 && ++since_rebin >= c->o23.dense_rebin) {
      since_rebin = 0;
      c->bin.invalidate();
      if (int rc = ode23_f1_queue(c, t, tmax, f, Cg, nslots, thr, bump)) return leave(rc);
      if (int rc = read_max(c, nullptr)) return leave(rc);
      ++c->o23.dense_rebins;
    }
  }
  return leave(SWRT_OK);
}
}  // namespace
