// swrt_host_qg.hpp — host side of the QG PDE stepper (swrt_qg.hpp): the step's
// launches, the fused post-step transforms, the CFL speed read-back FIFO,
// snapshots into the field slots (renaming through the spares) and the
// cross-stream order of the owner-driver hand-off.
#pragma once
#include "swrt_ctx.hpp"
#include "swrt_host_fields.hpp"
#include "swrt_fft.hpp"
#include "swrt_qg.hpp"

namespace {

// fused g2k crop + AB3 update from the forward-transformed Jacobian F into
// qk_prev (out of place: the new qk goes to the other buffer, the old one
// becomes prev_qk)
// The AB3 update of the current qk into qk_out, the tendency history into
// Qm1_out/Qm2_out (the committed buffers, or a speculative step's spares).
int qg_update_launch(swrt_ctx* c, double dt, int abstep, const double2* F, double2* qk_out, double2* Qm1_out,
                     double2* Qm2_out) {
  QGState& q = c->qg;
  hipLaunchKernelGGL(q.g.nl == 2 ? qg_update_kernel<2> : qg_update_kernel<1>, dim3(nblocks(q.nhalf, 256)), dim3(256),
                     0, c->stream, F, q.g, dt, abstep, q.E1.get(), q.E2.get(), (const double2*)q.qk.get(), qk_out,
                     (const double2*)q.Qm1.get(), (const double2*)q.Qm2.get(), Qm1_out, Qm2_out);
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}

// Fused mode: J's last forward pass and the update in one launch from J after
// its first pass (Zr); the new tendency goes to Qn_out only (the caller
// renames the history buffers).
int qg_update_cols_launch(swrt_ctx* c, double dt, int abstep, const double2* Zr, double2* qk_out,
                          double2* Qn_out) {
  QGState& q = c->qg;
  const int n = q.g.n;
  const int logn = ilog2(n);
  const size_t lds = sizeof(double2) * 2 * (size_t)(n + 1);
  hipLaunchKernelGGL(q.g.nl == 2 ? qg_update_cols_kernel<2> : qg_update_cols_kernel<1>, dim3((unsigned)(n / 2)),
                     dim3((unsigned)(n / 2)), lds, c->stream, Zr, q.g, logn, (const double2*)c->tw.get(), dt, abstep,
                     q.E1.get(), q.E2.get(), (const double2*)q.qk.get(), qk_out, (const double2*)q.Qm1.get(),
                     (const double2*)q.Qm2.get(), Qn_out);
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}

// The kernel sequence of one QG step (update of qgsw_raytrace.m:270-286 /
// qg2layersw_raytrace.m:309-323 + the AB3 step): spectra -> inverse 2-D FFT ->
// Jacobian -> forward 2-D FFT -> fused g2k crop + AB3 update into qk_prev.
int qg_step_launches(swrt_ctx* c, double dt, int abstep) {
  QGState& q = c->qg;
  const int n = q.g.n, nl = q.g.nl;
  int rc;
  hipLaunchKernelGGL(nl == 2 ? qg_jac_spectra_kernel<2> : qg_jac_spectra_kernel<1>, dim3(nblocks(q.nn, 256)),
                     dim3(256), 0, c->stream, q.qk.get(), q.g, q.Z.get());
  HIPCHK(c, hipGetLastError());
  if ((rc = inverse_2d(c, q.Z.get(), q.T.get(), n, 2 * nl))) return rc;
  double2* Zj = q.Z.get();  // J1 + i J2, grid layout (x contiguous)
  hipLaunchKernelGGL(qg_jacobian_kernel, dim3(nblocks(q.nn, 256)), dim3(256), 0, c->stream, q.T.get(), nl, q.nn, Zj);
  HIPCHK(c, hipGetLastError());
  if ((rc = transform_2d(c, Zj, q.T.get(), n, 1, 0))) return rc;  // along x, then y: [ky + n*kx]
  return qg_update_launch(c, dt, abstep, q.T.get(), q.qk_prev.get(), q.Qm1.get(), q.Qm2.get());
}

// Post-step transforms of the current qk (fused mode), see QGState::PZ.
// Every transform is the one the unfused calls make (same spectra kernels,
// same per-vector FFT), so results are bit-identical to them.  Two phases:
// the inverse transforms (all a snapshot needs) and the Jacobian + CFL max
// + forward transform of J (what the speed and the next step need), so a
// snapshot's pack — and the packet launch waiting for it — need not queue
// behind the second phase.
int qg_post_inverse(swrt_ctx* c) {
  QGState& q = c->qg;
  if (q.post_inv_valid && q.post_of == q.qk.get()) return SWRT_OK;
  q.post_valid = false;
  q.post_of = q.qk.get();
  const int n = q.g.n, nl = q.g.nl;
  const int nb = 2 * nl + (nl - 1) + 3;  // Jacobian inputs | layer-1 u+iv | layer-0 grid_U (u+iv first)
  if (!q.PZ) {
    HIPCHK(c, q.PZ.alloc(nb * q.nn));
    HIPCHK(c, q.PT.alloc(nb * q.nn));
  }
  int rc;
  if ((rc = ensure_twiddles(c, n))) return rc;
  const dim3 grid((unsigned)nblocks(q.nn, 256)), block(256);
  // Jacobian inputs | layer-1 u+iv | swrt_qg_snapshot(which 0, layer 0)'s
  // grid_U spectra (grid_U.m inversion, ky-fastest half plane) — one launch
  double2* uv = q.PZ.get() + 2 * nl * q.nn;
  if (nb * n / 4 <= 1024) {
    // spectra fused into the first inverse pass (qg_post_rows_kernel), then
    // the column pass — the same values as the three launches below
    const int logn = ilog2(n);
    const size_t lds = sizeof(double2) * nb * n;
    if (nl == 2)
      hipLaunchKernelGGL(qg_post_rows_split_kernel, dim3(2 * (unsigned)n), dim3(n), sizeof(double2) * 4 * n, c->stream,
                         (const double2*)q.qk.get(), q.g, q.nhalf, logn, (const double2*)c->tw.get(), q.PZ.get(),
                         q.dmax.get());
    else
      hipLaunchKernelGGL(qg_post_rows_kernel<1>, dim3((unsigned)n), dim3(nb * n / 4), lds, c->stream,
                         (const double2*)q.qk.get(), q.g, q.nhalf, logn, (const double2*)c->tw.get(), q.PZ.get(),
                         q.dmax.get());
    HIPCHK(c, hipGetLastError());
    // (not beside packets: its four-plane 512-lane workgroups then wait for
    // packet workgroups to retire — driver step +2 %, 8-GPU shard +10 %,
    // profiles/r04_qg_ab — where the separate column pass runs one plane per
    // 128-lane workgroup)
    if (nl == 2 && n % 8 == 0 && c->qg_jfuse == 1 && !(c->qg_sep && c->n > 0)) {
      // the column pass fused with the Jacobian, the CFL max and J's first
      // forward pass (swrt_fft.hpp): planes 0-4 stay on chip; J -> PT[0, nn)
      hipLaunchKernelGGL(fft_cols_jacobian2_kernel, dim3(2 * (unsigned)n), dim3(n), sizeof(double2) * 4 * (n + 1),
                         c->stream, (const double2*)q.PZ.get(), q.PT.get(), q.PT.get(), n, logn, q.g.shear,
                         q.dmax.get(), (const double2*)c->tw.get());
      q.post_jrows = true;
    } else {
      launch_fft<true>(c, q.PZ.get(), q.PT.get(), n, logn, nb * n, 1);
      q.post_jrows = false;
    }
    HIPCHK(c, hipGetLastError());
  } else {
    if (nl == 2)
      hipLaunchKernelGGL(qg_post_spectra_kernel<2>, grid, block, 0, c->stream, (const double2*)q.qk.get(), q.g, q.nhalf,
                         q.PZ.get(), uv, uv + q.nn, q.dmax.get());
    else
      hipLaunchKernelGGL(qg_post_spectra_kernel<1>, grid, block, 0, c->stream, (const double2*)q.qk.get(), q.g, q.nhalf,
                         q.PZ.get(), uv, uv, q.dmax.get());
    HIPCHK(c, hipGetLastError());
    if ((rc = inverse_2d(c, q.PZ.get(), q.PT.get(), n, nb))) return rc;
    q.post_jrows = false;
  }
  q.post_inv_valid = true;
  return SWRT_OK;
}

int qg_post(swrt_ctx* c) {
  QGState& q = c->qg;
  if (q.post_valid && q.post_of == q.qk.get()) return SWRT_OK;
  int rc;
  if ((rc = qg_post_inverse(c))) return rc;
  const int n = q.g.n, nl = q.g.nl;
  const dim3 block(256);
  // Jacobian and the CFL speed over every layer's u + i v (layer 1, then
  // layer 0: contiguous); the spectrum of J then lands in PT[0, nn)
  const double2* uvT = q.PT.get() + 2 * nl * q.nn;
  q.Fj = q.PT.get();
  q.Fj_rows = false;
  // J's last forward pass is left to the update (qg_update_cols_kernel) —
  // not beside packets: PDE alone -7 %, but the driver step +1.3 % with the
  // QG stream beside packet launches (profiles/r04_update_cols), as for
  // fft_cols_jacobian2_kernel
  const bool cols =
      n >= 16 && c->qg_update_cols == 1 && !(c->qg_sep && c->n > 0);
  if (q.post_jrows) {
    // J's first pass came with the inverse column pass: its second pass only
    if (cols) {
      q.Fj_rows = true;  // J's first pass is in PT[0, nn)
    } else {
      const int logn = ilog2(n);
      launch_fft<true>(c, q.PT.get(), q.PZ.get(), n, logn, n, 0);
      HIPCHK(c, hipGetLastError());
      q.Fj = q.PZ.get();
    }
  } else if (n <= 1024) {
    // J computed in the load of the forward transform's first pass (same
    // values, same per-vector FFT as the separate kernel + transform_2d)
    const int logn = ilog2(n);
    const int R = fft_group(c, n, n, false);  // rows per workgroup
    const dim3 jg((unsigned)(n / R)), jb((unsigned)(R * n / 4));
    const size_t jl = sizeof(double2) * R * n;
    hipLaunchKernelGGL(nl == 2 ? fft_jacobian_rows_kernel<2> : fft_jacobian_rows_kernel<1>, jg, jb, jl, c->stream,
                       (const double2*)q.PT.get(), n, logn, uvT, q.g.shear, q.dmax.get(), (const double2*)c->tw.get(),
                       q.PZ.get());
    HIPCHK(c, hipGetLastError());
    if (cols) {
      q.Fj = q.PZ.get();
      q.Fj_rows = true;
    } else {
      launch_fft<true>(c, q.PZ.get(), q.PT.get(), n, logn, n, 0);
      HIPCHK(c, hipGetLastError());
    }
  } else {
    const dim3 jgrid((unsigned)nblocks(q.nn, 256 * kQgMaxPer));
    hipLaunchKernelGGL(qg_jacobian_max_kernel, jgrid, block, 0, c->stream, (const double2*)q.PT.get(), nl, q.nn,
                       q.PZ.get(), uvT, q.g.shear, q.dmax.get());
    HIPCHK(c, hipGetLastError());
    if ((rc = transform_2d(c, q.PZ.get(), q.PT.get(), n, 1, 0))) return rc;
  }
  q.post_valid = true;
  return SWRT_OK;
}

// dmax -> the next FIFO slot of pinned host memory, and its event
int qg_speed_copy(swrt_ctx* c) {
  QGState& q = c->qg;
  const int slot = q.sp_head;
  HIPCHK(c, hipMemcpyAsync(q.hmax.get() + slot, q.dmax.get(), sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(slot ? q.ev_b.get() : q.ev.get(), c->stream));
  q.sp_head ^= 1;
  q.sp_count += 1;
  return SWRT_OK;
}

// grid_U speed of the current qk -> device max -> pinned host copy + event
int qg_speed_launch(swrt_ctx* c) {
  QGState& q = c->qg;
  int rc;
  const int n = q.g.n, nl = q.g.nl;
  if (q.sp_count >= 2) return fail(c, SWRT_ERR_STATE, "two CFL read-backs already pending");
  if (c->qg_fused) {  // the speed comes with the post-step transforms
    if ((rc = qg_post(c))) return rc;
    return qg_speed_copy(c);
  }
  if ((rc = ensure_twiddles(c, n))) return rc;
  hipLaunchKernelGGL(nl == 2 ? qg_vel_spectra_kernel<2> : qg_vel_spectra_kernel<1>, dim3(nblocks(q.nn, 256)),
                     dim3(256), 0, c->stream, q.qk.get(), q.g, q.Z.get());
  HIPCHK(c, hipGetLastError());
  if ((rc = inverse_2d(c, q.Z.get(), q.T.get(), n, nl))) return rc;
  q.post_valid = false;  // dmax is overwritten (and the first phase clears it)
  q.post_inv_valid = false;
  HIPCHK(c, hipMemsetAsync(q.dmax.get(), 0, sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(qg_max_speed2_kernel, dim3(256), dim3(256), 0, c->stream, q.T.get(), q.nn * nl, q.g.shear,
                     q.dmax.get());
  HIPCHK(c, hipGetLastError());
  return qg_speed_copy(c);
}

// the oldest pending read-back (FIFO)
int qg_speed_wait(swrt_ctx* c, double* U0_out) {
  QGState& q = c->qg;
  const int slot = (q.sp_head - q.sp_count) & 1;
  HIPCHK(c, hipEventSynchronize(slot ? q.ev_b.get() : q.ev.get()));
  q.sp_count -= 1;
  if (q.spec && q.spec_rb && slot == q.spec_rb_slot) q.spec_rb = false;  // the speculative step's, consumed
  *U0_out = std::sqrt(q.hmax[slot]);  // bits of a non-negative double: the max of (u+shear)^2 + v^2
  return SWRT_OK;
}

// A snapshot written on the QG stream (c->stream = the QG stream, OnQGStream):
// a slot buffer still read by a queued packet launch is renamed (an idle
// spare takes its place), else the write waits for the slot's last reader.
int qg_slot_acquire(swrt_ctx* c, int slot) {
  if (!c->qg_sep) return SWRT_OK;
  if (c->slot[slot].upend && event_pending(c->slot[slot].uref)) {
    int pick = -1;
    for (size_t i = 0; i < c->spares.size() && pick < 0; ++i)
      if (!c->spares[i].upend || !event_pending(c->spares[i].uref)) pick = (int)i;
    if (pick < 0 && c->spares.size() < kMaxSpares) {
      Slot sp;
      HIPCHK(c, sp.uev.create());
      HIPCHK(c, sp.wev.create());
      c->spares.push_back(std::move(sp));
      pick = (int)c->spares.size() - 1;
    }
    if (pick >= 0) std::swap(c->slot[slot], c->spares[pick]);  // else wait for the slot's own reader
  }
  if (c->slot[slot].upend) HIPCHK(c, hipStreamWaitEvent(c->stream, c->slot[slot].uref, 0));
  return SWRT_OK;
}

// ... and done: a new write generation; the packet stream's next reader waits
// for the write's event (slot_writes_wait)
int qg_slot_written(swrt_ctx* c, int slot) {
  Slot& s = c->slot[slot];
  s.set = true;
  s.wgen = ++c->slot_wgen;
  if (c->qg_sep) {
    HIPCHK(c, hipEventRecord(s.wev.get(), c->stream));
    s.wpend = true;
  }
  return SWRT_OK;
}

// swrt_qg_snapshot, or (spec) the same snapshot of the pending speculative
// step's qk: its post-step transforms (swrt_qg_step_speculative) hold layer
// 0's grid_U planes, which a snapshot after accepting the step would pack
// unchanged — so the pack can run before the CFL rule has decided.
int qg_snapshot_impl(swrt_ctx* c, int slot, int which, int layer, int64_t ny_period, bool spec) {
  OnQGStream on_qg(c);
  QGState& q = c->qg;
  if (!q.init) return fail(c, SWRT_ERR_STATE, "swrt_qg_init not called");
  if (spec) {
    if (!q.spec) return fail(c, SWRT_ERR_STATE, "no speculative QG step pending");
    if (!c->qg_fused || which != 0 || layer != 0 || q.g.n % 16 || !q.post_inv_valid || q.post_of != q.qk_spare.get())
      return fail(c, SWRT_ERR_STATE, "a speculative snapshot needs the fused transforms of the pending step (layer 0)");
  } else if (c->qg.spec) {
    return fail(c, SWRT_ERR_STATE, "a speculative QG step is pending (swrt_qg_resolve first)");
  }
  if (which != 0 && which != 1) return fail(c, SWRT_ERR_ARG, "which must be 0 (current) or 1 (previous)");
  if (which == 1 && !q.has_prev) return fail(c, SWRT_ERR_STATE, "no previous qk before the first step");
  if (layer < 0 || layer >= q.g.nl) return fail(c, SWRT_ERR_ARG, "layer out of range");
  const int64_t nx = q.g.n;
  int rc = check_slot_args(c, slot, nx);
  if (rc) return rc;
  if (ny_period == 0) ny_period = nx;
  if (ny_period % nx) return fail(c, SWRT_ERR_ARG, "ny_period must be a multiple of nx");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = qg_slot_acquire(c, slot))) return rc;
  if ((rc = ensure_slot(c, slot, nx))) return rc;
  if ((rc = ensure_twiddles(c, (int)nx))) return rc;
  Slot& s = c->slot[slot];
  if (c->qg_fused && which == 0 && layer == 0 && nx % 16 == 0) {
    // layer 0's grid_U of the current qk is part of the post-step transforms
    // (of the speculative qk: already computed, checked above)
    if (!spec && (rc = qg_post_inverse(c))) return rc;
    const double2* T = q.PT.get() + (3 * q.g.nl - 1) * q.nn;
    hipLaunchKernelGGL(pack_pairs_kernel, dim3(nx / 16, nx / 16), dim3(256), 0, c->stream, T, (int)nx, (int)s.npad,
                       q.g.shear, s.nodes.get());
    HIPCHK(c, hipGetLastError());
    s.has_psi = false;
    s.div_free = true;
  } else {
    const double2* src = (which == 0 ? q.qk.get() : q.qk_prev.get()) + layer * q.nhalf;
    if ((rc = fields_from_halfplane(c, slot, src, (int)nx, 1, q.g.K_d2, q.g.kscale, q.g.shear, 0, q.Z.get(), q.T.get(),
                                    (int)(nx / 2), 1)))
      return rc;
  }
  s.L = q.g.dx * (double)nx;
  s.ny_period = ny_period;
  return qg_slot_written(c, slot);
}

// order `from`'s work so far before `to`'s later work (no-op on one stream)
int stream_order(swrt_ctx* c, hipStream_t from, hipStream_t to, int ev) {
  if (from == to) return SWRT_OK;
  if (!c->xq.ev[ev]) HIPCHK(c, c->xq.ev[ev].create());
  HIPCHK(c, hipEventRecord(c->xq.ev[ev].get(), from));
  HIPCHK(c, hipStreamWaitEvent(to, c->xq.ev[ev].get(), 0));
  return SWRT_OK;
}
}  // namespace
