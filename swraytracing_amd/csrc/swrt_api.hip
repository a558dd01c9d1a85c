// swrt_api.hip — the C ABI (include/swrt.h) over the gfx950 kernels.
//
// Host-side orchestration only: device buffers owned by the context, one HIP
// stream per context, every call synchronous to the host and exception-free
// across the ABI boundary.
// This file holds the entry points; the context and each subsystem's host
// code are in the internal headers below (swrt_ctx.hpp, swrt_host_*.hpp).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <climits>
#include <vector>

#include "../../include/swrt.h"
#include "swrt_bin.hpp"
#include "swrt_fft.hpp"
#include "swrt_kernels.hpp"
#include "swrt_tile.hpp"
#include "swrt_qg.hpp"
#include "swrt_ode23.hpp"
#include "swrt_xka.hpp"
#include "swrt_rsw.hpp"
#include "swrt_spectral.hpp"
#include "swrt_hazard.hpp"
#include "swrt_diag.hpp"
#include "swrt_raydiag.hpp"
#include "swrt_map.hpp"
#include "swrt_kmap.hpp"
#include "swrt_res.hpp"

using namespace swrt;

#include "swrt_ctx.hpp"
#include "swrt_host_fields.hpp"

namespace {

// debug: a kernel that sleeps ~4 us per iteration (every wave returns)
__global__ void debug_spin_kernel(int iters) {
  for (int i = 0; i < iters; ++i) __builtin_amdgcn_s_sleep(127);
}

// debug (SWRT_DEBUG_CORRUPT_COUNT): add `delta` to one tile's count before a
// scan, as a corrupted binning would
__global__ void debug_corrupt_count_kernel(int* counts, int tile, int delta) {
  if (threadIdx.x == 0) counts[tile] += delta;
}

// Shader-clock probe (swrt_clock_stamp): kClockWaves one-wave workgroups
// (several per CU) each record the shader-cycle counter (s_memtime), the
// 100 MHz real-time counter (s_memrealtime) and the CU they ran on (XCD, SE,
// SH, CU ids).  A start and an end stamp of the SAME CU bracket a timed
// region: cycles / seconds = the clock that CU ran at over it
// (MI355X_MICROARCH.md, "DVFS give-back" item 6); s_memtime counters of
// different CUs are not aligned, so only same-CU pairs are used.  Plain
// vector stores, a buffer of its own.
constexpr int kClockWaves = 1024;
constexpr double kRealTimeHz = 100e6;
__global__ void clock_stamp_kernel(unsigned long long* out) {
  unsigned xcc, hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  const unsigned long long t = __builtin_amdgcn_s_memtime();
  const unsigned long long r = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) {
    out[3 * blockIdx.x + 0] = t;
    out[3 * blockIdx.x + 1] = r;
    // CU identity: XCD | SE | SH | CU (the wave/SIMD bits masked off)
    out[3 * blockIdx.x + 2] = ((unsigned long long)(xcc & 0xf) << 16) | ((hw >> 8) & 0xffffu);
  }
}

}  // namespace

#include "swrt_host_packets.hpp"
#include "swrt_host_qg.hpp"
#include "swrt_host_ode23.hpp"
#include "swrt_host_diag.hpp"

extern "C" {

int swrt_version(void) { return 100; }

int swrt_create(int device, swrt_ctx** out) {
  if (!out) return SWRT_ERR_ARG;
  *out = nullptr;
  swrt_ctx* c = nullptr;
  try {
    c = new swrt_ctx();
  } catch (...) {
    return SWRT_ERR_ALLOC;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    delete c;
    return SWRT_ERR_HIP;
  }
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || c->stream0.create(hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return SWRT_ERR_HIP;
  }
  // the QG stream at the highest priority: its short dependent kernels are
  // dispatched ahead of the waiting workgroups of a packet launch (measured
  // neither faster nor slower than the default priority)
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  const int prio = prio_greatest;
  bool ok = c->qstream.create(hipStreamNonBlocking, prio) == hipSuccess;
  for (Slot& s : c->slot) ok = ok && s.uev.create() == hipSuccess && s.wev.create() == hipSuccess;
  ok = ok && c->use_ev.create() == hipSuccess;
  ok = ok && c->fork_ev.create() == hipSuccess && c->sx[0].create(hipStreamNonBlocking) == hipSuccess;
  for (Event& e : c->jx) ok = ok && e.create() == hipSuccess;
  for (Event& e : c->o23.chain_ev) ok = ok && e.create() == hipSuccess;
  ok = ok && c->dev_err.alloc(4, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
  if (c->dev_err) std::memset(c->dev_err.get(), 0, sizeof(int) * 4);
  c->stream = c->stream0.get();
  if (const char* e = getenv("SWRT_HAZARD_CHECK")) c->hz.on = atoi(e) != 0;
  if (const char* e = getenv("SWRT_ODE23_CHAIN_FIRST")) c->o23.chain_first = atoi(e) != 0;
  if (!ok) {
    swrt_destroy(c);
    return SWRT_ERR_HIP;
  }
  *out = c;
  return SWRT_OK;
}

void swrt_destroy(swrt_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (const Stream& s : c->sx)
    if (s) (void)hipStreamSynchronize(s.get());
  if (c->qstream) (void)hipStreamSynchronize(c->qstream.get());
  // every buffer and event is released by its handle, the streams last
  // (swrt_ctx's member order)
  delete c;
}

const char* swrt_last_error(const swrt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int swrt_set_field_grid(swrt_ctx* c, int slot, const double* fields6, int64_t nx, double L,
                        int64_t ny_period) {
  int rc = check_slot_args(c, slot, nx);
  if (rc) return rc;
  GUARD_BEGIN
  SlotUse slot_use(c);
  if (!fields6) return fail(c, SWRT_ERR_ARG, "fields6 is NULL");
  if (!(L > 0)) return fail(c, SWRT_ERR_ARG, "L must be > 0");
  if (ny_period == 0) ny_period = nx;
  if (ny_period % nx) return fail(c, SWRT_ERR_ARG, "ny_period must be a multiple of nx");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_slot(c, slot, nx))) return rc;
  const size_t bytes = sizeof(double) * 6 * nx * nx;
  if ((rc = ensure_scratch(c, bytes))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->scratch.get(), fields6, bytes, hipMemcpyHostToDevice, c->stream));
  if ((rc = pack_slot(c, slot, (const double*)c->scratch.get(), 0.0))) return rc;
  // host-given fields take the five-sum kernels only if v_y == -u_x bit for bit
  bool div_free = true;
  {
    const int64_t plane = nx * nx;
    const uint64_t* ux = reinterpret_cast<const uint64_t*>(fields6 + 2 * plane);
    const uint64_t* vy = reinterpret_cast<const uint64_t*>(fields6 + 5 * plane);
    for (int64_t i = 0; i < plane && div_free; ++i) div_free = vy[i] == (ux[i] ^ 0x8000000000000000ull);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  Slot& s = c->slot[slot];
  s.div_free = div_free;
  s.L = L;
  s.ny_period = ny_period;
  s.has_psi = false;
  s.set = true;
  s.wgen = ++c->slot_wgen;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_set_field_psi(swrt_ctx* c, int slot, const double* psi_grid, int64_t nx, double L) {
  int rc = check_slot_args(c, slot, nx);
  if (rc) return rc;
  GUARD_BEGIN
  SlotUse slot_use(c);
  if (!psi_grid) return fail(c, SWRT_ERR_ARG, "psi_grid is NULL");
  if (!is_pow2(nx)) return fail(c, SWRT_ERR_ARG, "nx must be a power of two for the GPU FFT");
  if (!(L > 0)) return fail(c, SWRT_ERR_ARG, "L must be > 0");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_slot(c, slot, nx))) return rc;
  if ((rc = ensure_twiddles(c, (int)nx))) return rc;
  const int n = (int)nx;
  const int64_t nn = nx * nx;
  const int kmax = n / 2 - 1;
  const int64_t nhalf = (int64_t)(2 * kmax + 1) * (kmax + 1);
  // scratch: Z (4 nn complex) | T (4 nn complex) | fk (nhalf complex) | raw (nn double)
  const size_t zb = sizeof(double2) * 4 * nn;
  const size_t bytes = 2 * zb + sizeof(double2) * nhalf + sizeof(double) * nn;
  if ((rc = ensure_scratch(c, bytes))) return rc;
  const auto [Z, T, fk, raw] = fft_scratch(c, zb, nhalf);
  HIPCHK(c, hipMemcpyAsync(raw, psi_grid, sizeof(double) * nn, hipMemcpyHostToDevice, c->stream));
  if ((rc = g2k_launches(c, raw, Z, T, fk, n))) return rc;
  if ((rc = fields_from_halfplane(c, slot, fk, n, 0, 0.0, 1.0, 0.0, 1, Z, T, 1, 2 * (n / 2 - 1) + 1))) return rc;
  return slot_set_done(c, slot, L, nx);
  GUARD_END(c)
}

int swrt_set_field_qk(swrt_ctx* c, int slot, const double* qk_interleaved, int64_t nx, double L,
                      double K_d2, double shear, double k_scale, int64_t ny_period) {
  int rc = check_slot_args(c, slot, nx);
  if (rc) return rc;
  GUARD_BEGIN
  SlotUse slot_use(c);
  if (!qk_interleaved) return fail(c, SWRT_ERR_ARG, "qk is NULL");
  if (!is_pow2(nx)) return fail(c, SWRT_ERR_ARG, "nx must be a power of two for the GPU FFT");
  if (!(L > 0)) return fail(c, SWRT_ERR_ARG, "L must be > 0");
  if (ny_period == 0) ny_period = nx;
  if (ny_period % nx) return fail(c, SWRT_ERR_ARG, "ny_period must be a multiple of nx");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_slot(c, slot, nx))) return rc;
  if ((rc = ensure_twiddles(c, (int)nx))) return rc;
  const int n = (int)nx;
  const int64_t nn = nx * nx;
  const int kmax = n / 2 - 1;
  const int64_t nhalf = (int64_t)(2 * kmax + 1) * (kmax + 1);
  const size_t zb = sizeof(double2) * 3 * nn;
  const size_t bytes = 2 * zb + sizeof(double2) * nhalf;
  if ((rc = ensure_scratch(c, bytes))) return rc;
  const auto [Z, T, fk, raw] = fft_scratch(c, zb, nhalf);  // (no raw plane here)
  HIPCHK(c, hipMemcpyAsync(fk, qk_interleaved, sizeof(double2) * nhalf, hipMemcpyHostToDevice,
                           c->stream));
  if ((rc = fields_from_halfplane(c, slot, fk, n, 1, K_d2, k_scale, shear, 0, Z, T, 1, 2 * kmax + 1))) return rc;
  return slot_set_done(c, slot, L, ny_period);
  GUARD_END(c)
}

int swrt_set_field_q(swrt_ctx* c, int slot, const double* q_grid, int64_t nx, double L, double K_d2,
                     double shear, double k_scale, int64_t ny_period) {
  int rc = check_slot_args(c, slot, nx);
  if (rc) return rc;
  GUARD_BEGIN
  SlotUse slot_use(c);
  if (!q_grid) return fail(c, SWRT_ERR_ARG, "q_grid is NULL");
  if (!is_pow2(nx)) return fail(c, SWRT_ERR_ARG, "nx must be a power of two for the GPU FFT");
  if (!(L > 0)) return fail(c, SWRT_ERR_ARG, "L must be > 0");
  if (ny_period == 0) ny_period = nx;
  if (ny_period % nx) return fail(c, SWRT_ERR_ARG, "ny_period must be a multiple of nx");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_slot(c, slot, nx))) return rc;
  if ((rc = ensure_twiddles(c, (int)nx))) return rc;
  const int n = (int)nx;
  const int64_t nn = nx * nx;
  const int kmax = n / 2 - 1;
  const int64_t nhalf = (int64_t)(2 * kmax + 1) * (kmax + 1);
  // scratch: Z (3 nn complex) | T (3 nn complex) | fk (nhalf complex) | raw (nn double)
  const size_t zb = sizeof(double2) * 3 * nn;
  if ((rc = ensure_scratch(c, 2 * zb + sizeof(double2) * nhalf + sizeof(double) * nn))) return rc;
  const auto [Z, T, fk, raw] = fft_scratch(c, zb, nhalf);
  HIPCHK(c, hipMemcpyAsync(raw, q_grid, sizeof(double) * nn, hipMemcpyHostToDevice, c->stream));
  // qk = g2k(q) (g2k.m:8-9), exactly swrt_g2k's transform, kept on the device
  if ((rc = g2k_launches(c, raw, Z, T, fk, n))) return rc;
  // grid_U(qk) (grid_U.m:1-18): the same path as swrt_set_field_qk
  if ((rc = fields_from_halfplane(c, slot, fk, n, 1, K_d2, k_scale, shear, 0, Z, T, 1, 2 * kmax + 1))) return rc;
  return slot_set_done(c, slot, L, ny_period);
  GUARD_END(c)
}

int swrt_g2k(swrt_ctx* c, const double* fg, int64_t nx, double* fk_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!fg || !fk_out) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  if (nx < 8 || nx > 4096 || !is_pow2(nx)) return fail(c, SWRT_ERR_ARG, "nx must be a power of two, 8..4096");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_twiddles(c, (int)nx))) return rc;
  const int n = (int)nx;
  const int64_t nn = nx * nx;
  const int kmax = n / 2 - 1;
  const int64_t nhalf = (int64_t)(2 * kmax + 1) * (kmax + 1);
  const size_t zb = sizeof(double2) * nn;
  if ((rc = ensure_scratch(c, 2 * zb + sizeof(double2) * nhalf + sizeof(double) * nn))) return rc;
  const auto [Z, T, fk, raw] = fft_scratch(c, zb, nhalf);
  HIPCHK(c, hipMemcpyAsync(raw, fg, sizeof(double) * nn, hipMemcpyHostToDevice, c->stream));
  if ((rc = g2k_launches(c, raw, Z, T, fk, n))) return rc;
  HIPCHK(c, hipMemcpyAsync(fk_out, fk, sizeof(double2) * nhalf, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_k2g(swrt_ctx* c, const double* fk_in, int64_t nx, double* fg_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!fk_in || !fg_out) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  if (nx < 8 || nx > 4096 || !is_pow2(nx)) return fail(c, SWRT_ERR_ARG, "nx must be a power of two, 8..4096");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_twiddles(c, (int)nx))) return rc;
  const int n = (int)nx;
  const int64_t nn = nx * nx;
  const int kmax = n / 2 - 1;
  const int64_t nhalf = (int64_t)(2 * kmax + 1) * (kmax + 1);
  const size_t zb = sizeof(double2) * nn;
  if ((rc = ensure_scratch(c, 2 * zb + sizeof(double2) * nhalf + sizeof(double) * nn))) return rc;
  const auto [Z, T, fk, raw] = fft_scratch(c, zb, nhalf);
  HIPCHK(c, hipMemcpyAsync(fk, fk_in, sizeof(double2) * nhalf, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(fulspec_kernel, dim3(nblocks(nn, 256)), dim3(256), 0, c->stream, fk, n, Z, 1, 2 * kmax + 1);
  HIPCHK(c, hipGetLastError());
  if ((rc = inverse_2d(c, Z, T, n, 1))) return rc;
  hipLaunchKernelGGL(real_part_kernel, dim3(nblocks(nn, 256)), dim3(256), 0, c->stream, T, raw, nn);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(fg_out, raw, sizeof(double) * nn, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_field_div_free(swrt_ctx* c, int slot) {
  if (!c) return SWRT_ERR_ARG;
  if (slot < 0 || slot >= SWRT_MAX_SLOTS || !c->slot[slot].set)
    return fail(c, SWRT_ERR_STATE, "slot not set");
  return c->slot[slot].div_free ? 1 : 0;
}

int swrt_get_field_grid(swrt_ctx* c, int slot, double* out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c);
  if (slot < 0 || slot >= SWRT_MAX_SLOTS || !c->slot[slot].set)
    return fail(c, SWRT_ERR_STATE, "slot not set");
  if (!out) return fail(c, SWRT_ERR_ARG, "out is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  Slot& s = c->slot[slot];
  const int64_t nn = s.nx * s.nx;
  int rc;
  if ((rc = ensure_scratch(c, sizeof(double) * 6 * nn))) return rc;
  hipLaunchKernelGGL(unpack_nodes_kernel, dim3(nblocks(nn, 256)), dim3(256), 0, c->stream, s.nodes.get(),
                     (int)s.nx, (int)s.npad, (double*)c->scratch.get());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, c->scratch.get(), sizeof(double) * 6 * nn, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_get_psi_grid(swrt_ctx* c, int slot, double* out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c);
  if (slot < 0 || slot >= SWRT_MAX_SLOTS || !c->slot[slot].set || !c->slot[slot].has_psi)
    return fail(c, SWRT_ERR_STATE, "slot has no psi grid (use swrt_set_field_psi)");
  if (!out) return fail(c, SWRT_ERR_ARG, "out is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  Slot& s = c->slot[slot];
  HIPCHK(c, hipMemcpyAsync(out, s.psi.get(), sizeof(double) * s.nx * s.nx, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_interpolate(swrt_ctx* c, const double* F, int64_t nx, int64_t nyF, double dx, double dy,
                     double bump, const double* x, const double* y, int64_t n, double* out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (n < 0) return fail(c, SWRT_ERR_ARG, "n < 0");
  if (n == 0) return SWRT_OK;
  if (!F || !x || !y || !out) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  if (nx < 6 || nyF < nx) return fail(c, SWRT_ERR_ARG, "need nx >= 6 and nyF >= nx");
  if (!(dx > 0) || !(dy > 0)) return fail(c, SWRT_ERR_ARG, "dx, dy must be > 0");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t fb = sizeof(double) * nx * nx;  // only the first nx columns are read
  const size_t bytes = fb + sizeof(double) * 3 * n;
  int rc;
  if ((rc = ensure_scratch(c, bytes))) return rc;
  double* dF = (double*)c->scratch.get();
  double* dxp = dF + nx * nx;
  double* dyp = dxp + n;
  double* dout = dyp + n;
  HIPCHK(c, hipMemcpyAsync(dF, F, fb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dxp, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dyp, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  const double py = (double)nyF;
  hipLaunchKernelGGL(interp1_kernel, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, dF, (int)nx, py,
                     1.0 / py, dx, dy, bump, dxp, dyp, n, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_eval(swrt_ctx* c, const double* x, const double* y, int64_t n, int nslots, double alpha,
              double bump, double* out6) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c);
  if (n < 0) return fail(c, SWRT_ERR_ARG, "n < 0");
  if (n == 0) return SWRT_OK;
  if (!x || !y || !out6) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  if (nslots != 1 && nslots != 2) return fail(c, SWRT_ERR_ARG, "nslots must be 1 or 2");
  for (int s = 0; s < nslots; ++s)
    if (!c->slot[s].set) return fail(c, SWRT_ERR_STATE, "field slot not set");
  if (nslots == 2 && (c->slot[1].nx != c->slot[0].nx || c->slot[1].L != c->slot[0].L ||
                      c->slot[1].ny_period != c->slot[0].ny_period))
    return fail(c, SWRT_ERR_ARG, "slots 0 and 1 have different grids");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_scratch(c, sizeof(double) * 8 * n))) return rc;
  double* dxp = (double*)c->scratch.get();
  double* dyp = dxp + n;
  double* dout = dyp + n;
  HIPCHK(c, hipMemcpyAsync(dxp, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dyp, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  FieldView f0 = view_of(c->slot[0]);
  FieldView f1 = nslots == 2 ? view_of(c->slot[1]) : f0;
  hipLaunchKernelGGL(eval_kernel, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, f0, f1, nslots,
                     alpha, bump, dxp, dyp, n, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out6, dout, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_packets_set(swrt_ctx* c, const double* x, const double* k, int64_t n) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (n < 0 || n > INT32_MAX) return fail(c, SWRT_ERR_ARG, "n out of range (0..2^31-1)");
  if (n > 0 && (!x || !k)) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  if (n > c->cap) {
    c->cap = 0;  // (a failed allocation leaves no capacity behind)
    for (PacketSet* s : {&c->pk.cur, &c->pk.out, &c->pk.park}) HIPCHK(c, s->alloc(n));
    for (DevBuf<int>* b : {&c->keys, &c->src_idx}) HIPCHK(c, b->alloc(n));
    c->cap = n;
  }
  if (!c->bins.buf) HIPCHK(c, c->bins.alloc());
  if (n != c->n) c->rd.drop();  // Omega_0 and the frame series belong to an ensemble of the old size
  if (n != c->n) c->trk.drop();  // (the tracked ids too)
  if (n != c->n) c->absfreq.drop();  // (the absolute-frequency frames too)
  c->trans.drop();  // the transition series' mark belongs to the packet set it was taken on
  c->recycle.drop();  // (home, gen and born too)
  if (n != c->n) c->tan.drop();  // (the tangent maps too; with the same N the set is marked below)
  c->n = n;
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(c->pk.cur.x.get(), x, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->pk.cur.k.get(), k, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(iota_kernel, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, c->pk.cur.perm.get(), n);
    HIPCHK(c, hipGetLastError());
  }
  if (c->tan.live && n > 0) HIPCHK_RC(tangent_mark_queue(c));  // new packets: a new window
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->hz.on) {  // every packet stream's work is complete (joined, then synchronised)
    c->hz.quiesce();
    ++c->hz.epoch;
    char tag = 'A';
    for (const PacketSet* s : {&c->pk.cur, &c->pk.out, &c->pk.park}) {
      c->hz.name(s->x.get(), std::string("packet x buffer ") + tag);
      c->hz.name(s->k.get(), std::string("packet k buffer ") + tag);
      c->hz.name(s->perm.get(), std::string("permutation buffer ") + tag);
      ++tag;
    }
    c->hz.name(c->keys.get(), "binning keys");
    c->hz.name(c->src_idx.get(), "re-binning source index");
    c->hz.name(c->bins.counts(), "bin counts");
    c->hz.name(c->bins.cursor(), "bin cursors");
    c->hz.name(c->bins.starts(), "tile starts");
    c->hz.name(c->bins.tile_order(), "tile order");
  }
  // a new ensemble starts a new history and needs binning before the next step
  if (c->dev_err) c->dev_err[0] = 0;  // (an error raised over the old ensemble is superseded)
  c->packets_lost = false;
  c->hist.ext.cleared();
  c->steps_done = 0;
  c->bin.invalidate();
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_packets_get(swrt_ctx* c, double* x, double* k) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (c->n == 0) return SWRT_OK;
  if (!x || !k) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  if (c->packets_lost) return fail(c, SWRT_ERR_STATE, "the packet state was lost to a corrupted binning");
  HIPCHK(c, hipSetDevice(c->device));
  // un-permute into the scatter buffers, then download in original order
  hipLaunchKernelGGL(unpermute_kernel, dim3(nblocks(c->n, 256)), dim3(256), 0, c->stream, c->pk.cur.x.get(),
                     c->pk.cur.k.get(), c->pk.cur.perm.get(), c->n, c->n, c->pk.out.x.get(), c->pk.out.k.get());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(x, c->pk.out.x.get(), sizeof(double) * 2 * c->n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(k, c->pk.out.k.get(), sizeof(double) * 2 * c->n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return dev_err_check(c);
  GUARD_END(c)
}

int swrt_packets_get_device(swrt_ctx* c, double* x_dev, double* k_dev, int64_t ld) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(lost_check(c));  // (perm would be stale: never unpermute a lost state)
  if (c->n == 0) return SWRT_OK;
  if (!x_dev || !k_dev) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  if (ld < c->n) return fail(c, SWRT_ERR_ARG, "leading dimension below the packet count");
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(unpermute_kernel, dim3(nblocks(c->n, 256)), dim3(256), 0, c->stream, c->pk.cur.x.get(),
                     c->pk.cur.k.get(), c->pk.cur.perm.get(), c->n, ld, x_dev, k_dev);
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_set_timing(swrt_ctx* c, int every) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (every < 0) return fail(c, SWRT_ERR_ARG, "timing interval must be >= 0");
  c->timing_every = every;
  c->launch_count = 0;
  return SWRT_OK;
}

int swrt_set_gather_mode(swrt_ctx* c, int mode) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (mode != 0 && mode != 1) return fail(c, SWRT_ERR_ARG, "gather mode must be 0 or 1");
  c->gather_mode = mode;
  return SWRT_OK;
}

int swrt_set_integrator(swrt_ctx* c, int kick, int iterations, int composition) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (kick != 0 && kick != 1) return fail(c, SWRT_ERR_ARG, "integrator kick must be 0 (Euler) or 1 (implicit midpoint)");
  if (composition < 0 || composition > 2)
    return fail(c, SWRT_ERR_ARG, "integrator composition must be 0 (none), 1 (Yoshida) or 2 (Suzuki)");
  if (kick == 1 && (iterations < 1 || iterations > 4))
    return fail(c, SWRT_ERR_ARG, "midpoint iterations must be 1..4");
  c->integ_kick = kick;
  c->integ_iters = kick == 1 ? iterations : 1;
  c->integ_comp = composition;
  return SWRT_OK;
}

int swrt_get_integrator(const swrt_ctx* c, int* kick, int* iterations, int* composition) {
  if (!c) return SWRT_ERR_ARG;
  if (kick) *kick = c->integ_kick;
  if (iterations) *iterations = c->integ_iters;
  if (composition) *composition = c->integ_comp;
  return SWRT_OK;
}

int swrt_integrator_weights(int composition, double* w5, double* off5, int* nstages) {
  if (!w5 || !off5 || !nstages) return SWRT_ERR_ARG;
  double w[kMaxStages] = {}, off[kMaxStages] = {};
  const int S = integrator_stages(composition, w, off);
  if (S == 0) return SWRT_ERR_ARG;
  for (int j = 0; j < kMaxStages; ++j) {
    w5[j] = w[j];
    off5[j] = off[j];
  }
  *nstages = S;
  return SWRT_OK;
}

int swrt_set_packet_streams(swrt_ctx* c, int streams) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (streams != 1 && streams != 2) return fail(c, SWRT_ERR_ARG, "packet streams must be 1 or 2");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = join_b(c)) return rc;
  for (int i = 0; i < streams - 1; ++i)
    if (!c->sx[i]) HIPCHK(c, c->sx[i].create(hipStreamNonBlocking));
  c->packet_streams = streams;
  return SWRT_OK;
}

int swrt_set_sparse_tiles(swrt_ctx* c, int mode) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (mode < 0 || mode > 2) return fail(c, SWRT_ERR_ARG, "sparse tiles must be 0 (auto), 1 (never) or 2 (always)");
  c->sparse_mode = mode;
  c->bin.invalidate();  // the tile order of the next binning is sized for the launch shape
  return SWRT_OK;
}

int swrt_set_kernel(swrt_ctx* c, int variant) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (variant < 0 || variant > 2) return fail(c, SWRT_ERR_ARG, "kernel variant must be 0..2");
  c->kernel = variant;
  c->bin.invalidate();
  return SWRT_OK;
}

int swrt_set_locality(swrt_ctx* c, int64_t rebin_every, int64_t tile) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (rebin_every < 0 || tile < 0) return fail(c, SWRT_ERR_ARG, "negative locality parameter");
  c->rebin_every = rebin_every;
  c->tile = tile;
  c->bin.invalidate();
  return SWRT_OK;
}

int64_t swrt_packets_count(const swrt_ctx* c) { return c ? c->n : -1; }

int swrt_advance(swrt_ctx* c, double dt, int64_t nsteps, double f, double gH, int nslots,
                 double alpha0, double dalpha, double bump, int64_t save_every) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_SPLIT  // the half launches of the second packet stream stay unjoined across calls
  SlotUse slot_use(c, true);  // snapshot writes waited for before the first launch (run_advance)
  if (c->packets_lost) return fail(c, SWRT_ERR_STATE, "the packet state was lost to a corrupted binning");
  if (nsteps < 0) return fail(c, SWRT_ERR_ARG, "nsteps < 0");
  if (nslots != 1 && nslots != 2) return fail(c, SWRT_ERR_ARG, "nslots must be 1 or 2");
  if (save_every < 0) return fail(c, SWRT_ERR_ARG, "save_every < 0");
  if (!default_integrator(c) && c->gather_mode == 1)
    return fail(c, SWRT_ERR_ARG,
                "the FMA gather (swrt_set_gather_mode 1) has the leapfrog step only: set the integrator back to "
                "(0, 1, 0) or the gather mode to 0");
  HIPCHK_RC(tangent_step_check(c));
  for (int s = 0; s < nslots; ++s)
    if (!c->slot[s].set) return fail(c, SWRT_ERR_STATE, "field slot not set");
  if (nslots == 2 && (c->slot[1].nx != c->slot[0].nx || c->slot[1].L != c->slot[0].L ||
                      c->slot[1].ny_period != c->slot[0].ny_period))
    return fail(c, SWRT_ERR_ARG, "slots 0 and 1 have different grids");
  if (c->n == 0 || nsteps == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int64_t new_frames = save_every > 0 ? nsteps / save_every : 0;
  if (save_every > 0 && nsteps % save_every)
    return fail(c, SWRT_ERR_ARG, "nsteps must be a multiple of save_every");
  int rc = ensure_history(c, new_frames);
  if (rc) return rc;
  rc = run_advance(c, dt, nsteps, f, gH, nslots, alpha0, dalpha, bump, save_every);
  if (rc) return rc;
  c->hist.ext.committed(new_frames);
  c->steps_done += nsteps;
  // a QG stream renames slots by their use events: mark them after the second stream's launches too
  if (slot_events(c)) HIPCHK_RC(join_b(c));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_advance_intervals(swrt_ctx* c, int nintervals, const double* dts, int64_t nsub, double f, double gH,
                           double alpha0, double dalpha, double bump, int64_t save_every) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_SPLIT  // the half launches of the second packet stream stay unjoined across calls
  SlotUse slot_use(c, true);  // snapshot writes waited for before the first launch (run_advance*)
  if (c->packets_lost) return fail(c, SWRT_ERR_STATE, "the packet state was lost to a corrupted binning");
  if (nintervals < 1 || nintervals > SWRT_MAX_SLOTS - 1)
    return fail(c, SWRT_ERR_ARG, "nintervals must be 1..SWRT_MAX_SLOTS-1");
  if (!dts) return fail(c, SWRT_ERR_ARG, "dts is NULL");
  if (nsub < 1) return fail(c, SWRT_ERR_ARG, "nsub must be >= 1");
  if (!default_integrator(c) && c->gather_mode == 1)
    return fail(c, SWRT_ERR_ARG,
                "the FMA gather (swrt_set_gather_mode 1) has the leapfrog step only: set the integrator back to "
                "(0, 1, 0) or the gather mode to 0");
  HIPCHK_RC(tangent_step_check(c));
  if (save_every < 0 || (save_every > 0 && nsub % save_every))
    return fail(c, SWRT_ERR_ARG, "save_every must divide nsub");
  for (int s = 0; s <= nintervals; ++s) {
    const Slot& sl = c->slot[s];
    if (!sl.set) return fail(c, SWRT_ERR_STATE, "field slot not set");
    if (sl.nx != c->slot[0].nx || sl.L != c->slot[0].L || sl.ny_period != c->slot[0].ny_period)
      return fail(c, SWRT_ERR_ARG, "slots have different grids");
  }
  for (int i = 0; i < nintervals; ++i)
    if (!(dts[i] > 0) || !std::isfinite(dts[i])) return fail(c, SWRT_ERR_ARG, "dts must be finite and > 0");
  if (c->n == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t new_frames = save_every > 0 ? nintervals * (nsub / save_every) : 0;
  int rc = ensure_history(c, new_frames);
  if (rc) return rc;
  rc = run_advance_intervals(c, nintervals, dts, nsub, f, gH, alpha0, dalpha, bump, save_every);
  if (rc) return rc;
  c->steps_done += nintervals * nsub;
  // a QG stream renames slots by their use events: mark them after the second stream's launches too
  if (slot_events(c)) HIPCHK_RC(join_b(c));
  return SWRT_OK;
  GUARD_END(c)
}

int64_t swrt_history_frames(const swrt_ctx* c) { return c ? c->hist.ext.frames() : -1; }

int swrt_history_get(swrt_ctx* c, int64_t first, int64_t count, double* hist_x, double* hist_k) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  // (both columns are wanted: without hist_k the first counts as missing too)
  return series_get(c, c->hist, 2 * c->n, 2 * c->n, first, count, hist_k ? hist_x : nullptr, hist_k,
                    "history frame range out of bounds");
  GUARD_END(c)
}

int swrt_history_reset(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  c->hist.ext.cleared();
  c->steps_done = 0;
  return SWRT_OK;
}

int swrt_leapfrog(swrt_ctx* c, double* x, double* k, int64_t n, double dt, int64_t nsteps, double f,
                  double gH, int nslots, double alpha0, double dalpha, double bump,
                  int64_t save_every, double* hist_x, double* hist_k) {
  if (!c) return SWRT_ERR_ARG;
  int rc;
  if (!default_integrator(c) && c->gather_mode == 1)
    return fail(c, SWRT_ERR_ARG,
                "the FMA gather (swrt_set_gather_mode 1) has the leapfrog step only: set the integrator back to "
                "(0, 1, 0) or the gather mode to 0");
  HIPCHK_RC(tangent_step_check(c));
  if ((rc = swrt_packets_set(c, x, k, n))) return rc;
  const int64_t se = (hist_x && hist_k) ? save_every : 0;
  if ((rc = swrt_advance(c, dt, nsteps, f, gH, nslots, alpha0, dalpha, bump, se))) return rc;
  if ((rc = swrt_packets_get(c, x, k))) return rc;
  if (se > 0) {
    if ((rc = swrt_history_get(c, 0, c->hist.ext.frames(), hist_x, hist_k))) return rc;
  }
  return SWRT_OK;
}

int swrt_xka_set_fields(swrt_ctx* c, const double* fields7, int64_t nx, double dx, double dy) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!fields7) return fail(c, SWRT_ERR_ARG, "fields7 is NULL");
  if (nx < 6 || nx > 8192) return fail(c, SWRT_ERR_ARG, "nx out of range");
  if (!(dx > 0) || !(dy > 0)) return fail(c, SWRT_ERR_ARG, "dx, dy must be > 0");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = xka_nodes_for(c, nx))) return rc;
  if ((rc = ensure_scratch(c, sizeof(double) * 7 * nx * nx))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->scratch.get(), fields7, sizeof(double) * 7 * nx * nx, hipMemcpyHostToDevice, c->stream));
  if ((rc = xka_pack(c, (const double*)c->scratch.get(), nx))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->xka.dx = dx;
  c->xka.dy = dy;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_xka_set_rsw(swrt_ctx* c, const double* state3, int64_t nx, double f, double Cg, double L) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!state3) return fail(c, SWRT_ERR_ARG, "state3 is NULL");
  if (nx < 8 || nx > 4096 || !is_pow2(nx)) return fail(c, SWRT_ERR_ARG, "nx must be a power of two, 8..4096");
  if (!(f != 0.0) || !std::isfinite(f) || !std::isfinite(Cg) || !(L > 0))
    return fail(c, SWRT_ERR_ARG, "f must be nonzero and finite, L > 0");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_twiddles(c, (int)nx))) return rc;
  if ((rc = xka_nodes_for(c, nx))) return rc;
  const int n = (int)nx;
  const int64_t nn = nx * nx;
  const size_t zb = sizeof(double2) * nn;
  // Z: 4 spectra | T: 4 transforms | planes: 7 real (the 3 state planes first)
  if ((rc = ensure_scratch(c, 8 * zb + sizeof(double) * 7 * nn))) return rc;
  char* base = (char*)c->scratch.get();
  double2* Z = (double2*)base;
  double2* T = (double2*)(base + 4 * zb);
  double* planes = (double*)(base + 8 * zb);
  HIPCHK(c, hipMemcpyAsync(planes, state3, sizeof(double) * 3 * nn, hipMemcpyHostToDevice, c->stream));
  // g2k.m:8 fft2 of u, v, eta (raytrace_sw.m:26-28)
  hipLaunchKernelGGL(real_to_complex_kernel, dim3(nblocks(3 * nn, 256)), dim3(256), 0, c->stream, planes, Z, 3 * nn);
  HIPCHK(c, hipGetLastError());
  if ((rc = transform_2d(c, Z, T, n, 3, 0))) return rc;
  // projection + gradients + fulspec (raytrace_sw.m:25-41), then 4 inverse transforms
  hipLaunchKernelGGL(rsw_spectra_kernel, dim3(nblocks(nn, 256)), dim3(256), 0, c->stream, T, n, f, Cg * Cg,
                     (2.0 * M_PI) / L, Z);
  HIPCHK(c, hipGetLastError());
  if ((rc = inverse_2d(c, Z, T, n, 4))) return rc;
  hipLaunchKernelGGL(rsw_unpack_kernel, dim3(nblocks(nn, 256)), dim3(256), 0, c->stream, T, nn, planes);
  HIPCHK(c, hipGetLastError());
  if ((rc = xka_pack(c, planes, nx))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->xka.dx = L / (double)nx;
  c->xka.dy = L / (double)nx;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_xka_get_fields(swrt_ctx* c, double* fields7_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!fields7_out) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  if (!c->xka.nodes) return fail(c, SWRT_ERR_STATE, "call swrt_xka_set_fields or swrt_xka_set_rsw first");
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t nx = c->xka.nx, nn = nx * nx;
  int rc;
  if ((rc = ensure_scratch(c, sizeof(double) * 7 * nn))) return rc;
  hipLaunchKernelGGL(unpack_xka_kernel, dim3(nblocks(nn, 256)), dim3(256), 0, c->stream, c->xka.nodes.get(), (int)nx,
                     (int)(nx + kPadTot), (double*)c->scratch.get());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(fields7_out, c->scratch.get(), sizeof(double) * 7 * nn, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int64_t swrt_xka_grid(const swrt_ctx* c) { return c ? c->xka.nx : -1; }

int64_t swrt_field_grid(const swrt_ctx* c, int slot) {
  if (!c || slot < 0 || slot >= SWRT_MAX_SLOTS || !c->slot[slot].set) return -1;
  return c->slot[slot].nx;
}

int64_t swrt_qg_grid(const swrt_ctx* c, int* nlayers_out) {
  if (nlayers_out) *nlayers_out = (c && c->qg.init) ? c->qg.g.nl : 0;
  if (!c || !c->qg.init) return -1;
  return c->qg.g.n;
}

int swrt_xka_step(swrt_ctx* c, double* state5, int64_t n, double C0, double f, double dt, int64_t nsteps,
                  int64_t save_every, double* hist5) {
  if (!c) return SWRT_ERR_ARG;
  HIPCHK_RC(tangent_refuse(c, "swrt_xka_step"));
  GUARD_BEGIN
  if (!c->xka.nodes) return fail(c, SWRT_ERR_STATE, "call swrt_xka_set_fields first");
  if (n < 0 || nsteps < 0 || save_every < 0) return fail(c, SWRT_ERR_ARG, "negative size");
  if (n == 0 || nsteps == 0) return SWRT_OK;  // nothing to advance: state5 unchanged, no frames
  if (!state5) return fail(c, SWRT_ERR_ARG, "state is NULL");
  if (hist5 && save_every > 0 && nsteps % save_every)
    return fail(c, SWRT_ERR_ARG, "nsteps must be a multiple of save_every");
  HIPCHK(c, hipSetDevice(c->device));
  if (n > c->xka.cap) {
    c->xka.cap = 0;
    HIPCHK(c, c->xka.state.alloc(5 * n));
    HIPCHK(c, c->xka.state2.alloc(5 * n));
    for (DevBuf<int>* b : {&c->xka.keys, &c->xka.src, &c->xka.src2, &c->xka.perm2}) HIPCHK(c, b->alloc(n));
    c->xka.cap = n;
  }
  if (!c->xka.bins) HIPCHK(c, c->xka.bins.alloc(3 * kMaxBins + 1));
  const int64_t frames = (hist5 && save_every > 0) ? nsteps / save_every : 0;
  if (frames * 5 * n > c->xka.hcap) {
    c->xka.hcap = 0;
    HIPCHK(c, c->xka.hist.alloc(frames * 5 * n));
    c->xka.hcap = frames * 5 * n;
  }
  HIPCHK(c, hipMemcpyAsync(c->xka.state.get(), state5, sizeof(double) * 5 * n, hipMemcpyHostToDevice, c->stream));
  XkaArgs a;
  a.nodes = c->xka.nodes.get();
  a.nx = (int)c->xka.nx;
  a.npad = (int)(c->xka.nx + kPadTot);
  a.dx = c->xka.dx;
  a.dy = c->xka.dy;
  a.inv_dx = 1.0 / a.dx;
  a.inv_dy = 1.0 / a.dy;
  a.px = a.py = (double)c->xka.nx;
  a.inv_px = a.inv_py = 1.0 / (double)c->xka.nx;
  a.C0sq = C0 * C0;
  a.f = f;
  a.f2 = f * f;
  a.dt = dt;
  a.bump = 1e-13;  // ray_trace_sw/interpolate.m:13
  a.st = c->xka.state.get();
  a.n = n;
  a.save_every = save_every > 0 ? save_every : 1;
  a.hist = frames ? c->xka.hist.get() : nullptr;
  a.perm = nullptr;
  a.st_in = a.st;
  a.src = nullptr;
  a.perm_out = nullptr;
  // larger ensembles: step the packets in spatially binned order (8 x 8-cell
  // tiles, counting sort by index) with the LDS-tiled kernel (one workgroup
  // per tile, xka_tile_kernel), re-binned every rebin_every steps (the
  // context's locality setting) so the packets stay inside their tile's
  // window; the permutation to the caller's order is composed across
  // re-binnings and history frames are written through it
  const bool binned = n >= 4096 && c->rebin_every > 0;
  BinGeom g;
  g.dx = a.dx; g.px = a.px; g.py = a.py; g.inv_px = a.inv_px; g.inv_py = a.inv_py; g.inv_dx = a.inv_dx;
  g.nx = a.nx;
  g.tile = 8;
  while ((a.nx + g.tile - 1) / g.tile > 64) g.tile *= 2;
  g.ntx = (a.nx + g.tile - 1) / g.tile;
  const int nbins = g.ntx * g.ntx;
  const bool tiled = binned && a.nx % g.tile == 0 && g.ntx >= 2 && (g.tile == 8 || g.tile == 16);
  const unsigned bgrid = nblocks(n, 256 * kBinPerThread);
  // Binning is index-only: the scatter writes the source slot of every binned
  // slot and the launch that follows reads its packets through it into the
  // other state buffer, composing the permutation to the caller's order
  double* cur = c->xka.state.get();   // the state the next launch reads
  double* other = c->xka.state2.get();
  int* perm = nullptr;          // cur's slot -> caller's packet (nullptr: identity)
  int* perm_other = c->xka.perm2.get();
  const int* src = nullptr;     // pending re-binning (cur's slots, binned order)
  auto rebin_xka = [&]() -> int {
    HIPCHK(c, hipMemsetAsync(c->xka.bins.get(), 0, sizeof(int) * nbins, c->stream));
    hipLaunchKernelGGL(bin_count_kernel, dim3(bgrid), dim3(256), sizeof(int) * nbins, c->stream, g, cur, n, nbins,
                       c->xka.keys.get(), c->xka.bins.get());
    hipLaunchKernelGGL(bin_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->xka.bins.get(), nbins,
                       c->xka.bins.get() + kMaxBins, c->xka.bins.get() + 2 * kMaxBins, n, c->dev_err.dev(), nullptr,
                       kTileThreads);
    hipLaunchKernelGGL(bin_scatter_kernel<true>, dim3(bgrid), dim3(256), 2 * sizeof(int) * nbins, c->stream, cur, cur,
                       nullptr, c->xka.keys.get(), n, nbins, c->xka.bins.get() + kMaxBins, nullptr, nullptr, nullptr,
                       c->xka.src2.get());
    HIPCHK(c, hipGetLastError());
    src = c->xka.src2.get();
    return SWRT_OK;
  };
  int rc;
  if (binned && (rc = rebin_xka())) return rc;
  const int64_t per_launch = tiled ? std::min<int64_t>(kMaxStepsPerLaunch, c->rebin_every) : kMaxStepsPerLaunch;
  for (int64_t s0 = 0; s0 < nsteps; s0 += per_launch) {
    if (tiled && s0 > 0 && (rc = rebin_xka())) return rc;
    a.st_in = cur;
    a.src = src;
    a.perm = perm;
    if (src) {  // out of place: into the other buffer, with the composed permutation
      int* pout = perm == nullptr ? c->xka.src.get() : perm_other;
      a.st = other;
      a.perm_out = pout;
    } else {
      a.st = cur;
      a.perm_out = nullptr;
    }
    a.nsteps = (int)std::min<int64_t>(per_launch, nsteps - s0);
    a.step0 = s0;
    if (tiled)
      hipLaunchKernelGGL(xka_tile_kernel_of(g.tile), dim3(nbins), dim3(256), 0, c->stream, a,
                         (const int*)(c->xka.bins.get() + 2 * kMaxBins), g.ntx);
    else
      hipLaunchKernelGGL(xka_kernel, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    if (src) {
      std::swap(cur, other);
      if (perm == nullptr) {
        perm = c->xka.src.get();
      } else {
        std::swap(perm, perm_other);
      }
      src = nullptr;
    }
  }
  if (binned) {
    hipLaunchKernelGGL(xka_scatter_back_kernel, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, cur, perm, n, other);
    HIPCHK(c, hipGetLastError());
    cur = other;
  }
  HIPCHK(c, hipMemcpyAsync(state5, cur, sizeof(double) * 5 * n, hipMemcpyDeviceToHost, c->stream));
  if (frames)
    HIPCHK(c, hipMemcpyAsync(hist5, c->xka.hist.get(), sizeof(double) * frames * 5 * n, hipMemcpyDeviceToHost,
                             c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_spectral_set_modes(swrt_ctx* c, const double* C, int64_t nkx, int64_t nky, double kx0, double ky0,
                            double s) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!C) return fail(c, SWRT_ERR_ARG, "C is NULL");
  if (nkx <= 0 || nky <= 0 || nkx * nky > (int64_t)1 << 28) return fail(c, SWRT_ERR_ARG, "bad mode grid");
  HIPCHK(c, hipSetDevice(c->device));
  if (nkx * nky > c->spec.cap) {
    c->spec.cap = 0;
    HIPCHK(c, c->spec.modes.alloc(nkx * nky));
    c->spec.cap = nkx * nky;
  }
  if (nky > c->spec.rows_cap) {
    c->spec.rows_cap = 0;
    HIPCHK(c, c->spec.rows.alloc(nky));
    c->spec.rows_cap = nky;
  }
  // nonzero span of each row (the kernel skips zero head/tail segments)
  std::vector<int2> rows(nky);
  for (int64_t j = 0; j < nky; ++j) {
    int lo = 0, hi = (int)nkx;
    while (lo < hi && C[2 * (j * nkx + lo)] == 0.0 && C[2 * (j * nkx + lo) + 1] == 0.0) ++lo;
    while (hi > lo && C[2 * (j * nkx + hi - 1)] == 0.0 && C[2 * (j * nkx + hi - 1) + 1] == 0.0) --hi;
    rows[j] = make_int2(lo, hi);
  }
  // fp32 packed-pair copy of the spans (ModeGrid::Cf): groups of 4 modes as
  // two float4 {re_m, re_m+1, im_m, im_m+1}, zero past the span end
  std::vector<int> frow(nky);
  int64_t nf = 0;
  for (int64_t j = 0; j < nky; ++j) {
    frow[j] = (int)nf;
    nf += 2 * (((int64_t)rows[j].y - rows[j].x + kSpecChains - 1) / kSpecChains);
  }
  // + zero slots: the LDS stream's chunk prefetch reads up to two chunks past
  // the last group (SpecStream; 16-B slots in both precisions)
  std::vector<float4> cf((size_t)(nf + 2 * kSpecChunk), make_float4(0.f, 0.f, 0.f, 0.f));
  for (int64_t j = 0; j < nky; ++j) {
    for (int m = rows[j].x; m < rows[j].y; ++m) {
      const int64_t r = m - rows[j].x, q = frow[j] + 2 * (r / kSpecChains) + (r % kSpecChains) / 2;
      const int h = (int)(r & 1);
      float* v = reinterpret_cast<float*>(&cf[q]);
      v[h] = (float)C[2 * (j * nkx + m)];
      v[2 + h] = (float)C[2 * (j * nkx + m) + 1];
    }
  }
  // the same groups in fp64: kSpecChains double2 per group (Cd_row = 2 * Cf_row)
  std::vector<double2> cd((size_t)(2 * nf + 2 * kSpecChunk), make_double2(0.0, 0.0));
  std::vector<int> drow(nky);
  for (int64_t j = 0; j < nky; ++j) {
    drow[j] = 2 * frow[j];
    for (int m = rows[j].x; m < rows[j].y; ++m)
      cd[(size_t)drow[j] + (m - rows[j].x)] = make_double2(C[2 * (j * nkx + m)], C[2 * (j * nkx + m) + 1]);
  }
  if ((int64_t)cd.size() > c->spec.modes_f_cap) {
    c->spec.modes_f_cap = 0;
    HIPCHK(c, c->spec.modes_f.alloc(cd.size()));
    HIPCHK(c, c->spec.modes_d.alloc(cd.size()));
    c->spec.modes_f_cap = (int64_t)cd.size();
  }
  if (nky > c->spec.modes_f_rcap) {
    c->spec.modes_f_rcap = 0;
    HIPCHK(c, c->spec.modes_f_row.alloc(nky));
    HIPCHK(c, c->spec.modes_d_row.alloc(nky));
    c->spec.modes_f_rcap = nky;
  }
  HIPCHK(c, hipMemcpyAsync(c->spec.modes_d.get(), cd.data(), sizeof(double2) * cd.size(), hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, hipMemcpyAsync(c->spec.modes_d_row.get(), drow.data(), sizeof(int) * nky, hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, hipMemcpyAsync(c->spec.modes.get(), C, sizeof(double2) * nkx * nky, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->spec.rows.get(), rows.data(), sizeof(int2) * nky, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->spec.modes_f.get(), cf.data(), sizeof(float4) * cf.size(), hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, hipMemcpyAsync(c->spec.modes_f_row.get(), frow.data(), sizeof(int) * nky, hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->spec.mg.Cd = c->spec.modes_d.get();
  c->spec.mg.Cd_row = c->spec.modes_d_row.get();
  c->spec.mg.Cf = c->spec.modes_f.get();
  c->spec.mg.Cf_row = c->spec.modes_f_row.get();
  int64_t active = 0;
  for (auto& r : rows) active += r.y - r.x;
  c->spec.active = active;
  c->spec.mg.rows = c->spec.rows.get();
  c->spec.mg.C = c->spec.modes.get();
  c->spec.mg.nkx = (int)nkx;
  c->spec.mg.nky = (int)nky;
  c->spec.mg.kx0 = kx0;
  c->spec.mg.ky0 = ky0;
  c->spec.mg.s = s;
  c->spec.set = true;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_spectral_eval(swrt_ctx* c, const double* x, const double* y, int64_t n, int precision, double* out6) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!c->spec.set) return fail(c, SWRT_ERR_STATE, "call swrt_spectral_set_modes first");
  if (precision != 64 && precision != 32) return fail(c, SWRT_ERR_ARG, "precision must be 64 or 32");
  if (n < 0) return fail(c, SWRT_ERR_ARG, "n < 0");
  if (n == 0) return SWRT_OK;
  if (!x || !y || !out6) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_scratch(c, sizeof(double) * 8 * n))) return rc;
  double* dxp = (double*)c->scratch.get();
  double* dyp = dxp + n;
  double* dout = dyp + n;
  HIPCHK(c, hipMemcpyAsync(dxp, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dyp, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(spectral_eval_kernel_of(precision), dim3(nblocks(n, kSpecThreads)), dim3(kSpecThreads), 0,
                     c->stream, c->spec.mg, dxp, dyp, n, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out6, dout, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_spectral_leapfrog(swrt_ctx* c, double* x, double* k, int64_t n, double dt, int64_t nsteps, double f,
                           double gH, int precision) {
  if (!c) return SWRT_ERR_ARG;
  HIPCHK_RC(tangent_refuse(c, "swrt_spectral_leapfrog"));
  GUARD_BEGIN
  if (!c->spec.set) return fail(c, SWRT_ERR_STATE, "call swrt_spectral_set_modes first");
  if (precision != 64 && precision != 32) return fail(c, SWRT_ERR_ARG, "precision must be 64 or 32");
  if (n < 0 || nsteps < 0) return fail(c, SWRT_ERR_ARG, "negative size");
  if (n == 0 || nsteps == 0) return SWRT_OK;
  if (!x || !k) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_scratch(c, sizeof(double) * 4 * n))) return rc;
  double* dxp = (double*)c->scratch.get();
  double* dkp = dxp + 2 * n;
  HIPCHK(c, hipMemcpyAsync(dxp, x, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dkp, k, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
  for (int64_t s0 = 0; s0 < nsteps; s0 += kMaxStepsPerLaunch) {
    const int ns = (int)std::min<int64_t>(kMaxStepsPerLaunch, nsteps - s0);
    hipLaunchKernelGGL(spectral_leapfrog_kernel_of(precision), dim3(nblocks(n, kSpecThreads)), dim3(kSpecThreads), 0,
                       c->stream, c->spec.mg, dxp, dkp, n, dt, ns, f * f, gH);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(x, dxp, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(k, dkp, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_omega_histogram(swrt_ctx* c, double f, double Cg, const double* edges, int64_t nbins,
                         int64_t* counts_inout, double* mean_omega_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (nbins <= 0 || nbins > kMaxHistBins) return fail(c, SWRT_ERR_ARG, "nbins must be 1..4096");
  if (!edges || !counts_inout) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  for (int64_t i = 0; i < nbins; ++i)
    if (!(edges[i] < edges[i + 1])) return fail(c, SWRT_ERR_ARG, "edges must increase");
  HIPCHK(c, hipSetDevice(c->device));
  const int nblk = 1024;
  const size_t bytes = sizeof(double) * (nbins + 1) + sizeof(unsigned long long) * nbins +
                       sizeof(double) * (nblk + 1);
  int rc;
  if ((rc = ensure_scratch(c, bytes))) return rc;
  double* dedges = (double*)c->scratch.get();
  unsigned long long* dcounts = (unsigned long long*)(dedges + nbins + 1);
  double* partial = (double*)(dcounts + nbins);
  HIPCHK(c, hipMemcpyAsync(dedges, edges, sizeof(double) * (nbins + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(dcounts, 0, sizeof(unsigned long long) * nbins, c->stream));
  double mean = 0.0;
  if (c->n > 0) {
    hipLaunchKernelGGL(omega_hist_kernel, dim3(nblk), dim3(kHistThreads), 0, c->stream, c->pk.cur.k.get(), c->n, f * f,
                       Cg * Cg, dedges, (int)nbins, dcounts, partial);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(omega_sum_kernel, dim3(1), dim3(64), 0, c->stream, partial, nblk, partial + nblk);
    HIPCHK(c, hipGetLastError());
  }
  std::vector<unsigned long long> hc(nbins, 0ull);
  double sum = 0.0;
  HIPCHK(c, hipMemcpyAsync(hc.data(), dcounts, sizeof(unsigned long long) * nbins, hipMemcpyDeviceToHost, c->stream));
  if (c->n > 0)
    HIPCHK(c, hipMemcpyAsync(&sum, partial + nblk, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int64_t i = 0; i < nbins; ++i) counts_inout[i] += (int64_t)hc[i];
  if (c->n > 0) mean = sum / (double)c->n;
  if (mean_omega_out) *mean_omega_out = mean;
  return SWRT_OK;
  GUARD_END(c)
}

// ---- ray diagnostics (swrt_raydiag.hpp, swrt_host_diag.hpp) ----
int swrt_raydiag_mark(swrt_ctx* c, double f, double gH, int nslots, double alpha, double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c);
  HIPCHK_RC(raydiag_check(c, nslots));
  HIPCHK(c, hipSetDevice(c->device));
  RayDiagState& rd = c->rd;
  rd.marked = false;
  HIPCHK_RC(raydiag_reserve(c, 1));
  HIPCHK_RC(raydiag_launch(c, true, f, gH, nslots, alpha, bump, nullptr, nullptr));
  rd.marked = true;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_raydiag_sample(swrt_ctx* c, double f, double gH, int nslots, double alpha, double bump,
                        double* sample4_out, double* frame8_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c);
  HIPCHK_RC(raydiag_check(c, nslots));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(raydiag_reserve(c, 0));
  double* dsample = nullptr;
  if (sample4_out) {
    HIPCHK_RC(ensure_scratch(c, sizeof(double) * 4 * c->n));
    dsample = (double*)c->scratch.get();
  }
  double* dframe = c->rd.partial.get() + kRayDiagStats * kRayDiagBlocks;
  HIPCHK_RC(raydiag_launch(c, false, f, gH, nslots, alpha, bump, dsample, dframe));
  if (sample4_out)
    HIPCHK(c, hipMemcpyAsync(sample4_out, dsample, sizeof(double) * 4 * c->n, hipMemcpyDeviceToHost, c->stream));
  if (frame8_out)
    HIPCHK(c, hipMemcpyAsync(frame8_out, dframe, sizeof(double) * kRayDiagFrame, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return dev_err_check(c);
  GUARD_END(c)
}

int swrt_raydiag_record(swrt_ctx* c, double f, double gH, int nslots, double alpha, double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c);
  HIPCHK_RC(raydiag_check(c, nslots));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(raydiag_reserve(c, 1));
  return raydiag_record_frame(c, f, gH, nslots, alpha, bump);
  GUARD_END(c)
}

int swrt_raydiag_record_history(swrt_ctx* c, int64_t first, int64_t count, double f, double gH, int nslots,
                                const double* alphas, double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c);
  HIPCHK_RC(raydiag_check(c, nslots));
  HIPCHK_RC(frame_range_check(c, c->hist.ext, first, count, "history frame range out of bounds"));
  if (nslots == 2 && !alphas && count > 0) return fail(c, SWRT_ERR_ARG, "NULL buffer (alphas, two snapshots)");
  if (count == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(raydiag_reserve(c, count));
  for (int64_t i = 0; i < count; ++i) {
    const int64_t off = (first + i) * 2 * c->n;
    HIPCHK_RC(raydiag_record_frame(c, f, gH, nslots, alphas ? alphas[i] : 0.0, bump, c->hist.a.get() + off,
                                   c->hist.b.get() + off));
  }
  return SWRT_OK;
  GUARD_END(c)
}

int64_t swrt_raydiag_frames(const swrt_ctx* c) { return c ? c->rd.series.ext.frames() : -1; }

int swrt_raydiag_series_get(swrt_ctx* c, int64_t first, int64_t count, double* frames8_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return series_get(c, c->rd.series, kRayDiagFrame, 0, first, count, frames8_out, nullptr, "frame range out of bounds");
  GUARD_END(c)
}

int swrt_raydiag_series_reset(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  c->rd.series.ext.cleared();
  return SWRT_OK;
}

// ---- the spectrum series (swrt_diag.hpp, swrt_host_diag.hpp) ----
int swrt_omega_series_begin(swrt_ctx* c, double f, double Cg, const double* edges, int64_t nbins) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(omega_edges_check(c, edges, nbins));
  HIPCHK(c, hipSetDevice(c->device));
  OmegaSeriesState& om = c->om;
  HIPCHK_RC(series_release(c, om.series));
  om.open = false;
  HIPCHK(c, om.edges.alloc(nbins + 1));
  HIPCHK(c, hipMemcpyAsync(om.edges.get(), edges, sizeof(double) * (nbins + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  om.nb = (int)nbins;
  om.f2 = f * f;
  om.Cg2 = Cg * Cg;
  om.open = true;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_omega_series_record(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(omega_series_check(c));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(omega_reserve(c, 1, true));
  OmegaSeriesState& om = c->om;
  hipLaunchKernelGGL(omega_scatter_kernel, dim3(nblocks(c->n, kOmegaThreads)), dim3(kOmegaThreads), 0, c->stream,
                     c->pk.cur.k.get(), c->pk.cur.perm.get(), c->n, om.f2, om.Cg2, om.w.get(),
                     om.series.end_a(om.row()), om.nb + 2);
  HIPCHK(c, hipGetLastError());
  return omega_frames_launch(c, false, om.w.get(), 0, 1);
  GUARD_END(c)
}

int swrt_omega_series_record_history(swrt_ctx* c, int64_t first, int64_t count) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(omega_series_check(c));
  HIPCHK_RC(frame_range_check(c, c->hist.ext, first, count, "history frame range out of bounds"));
  if (count == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(omega_reserve(c, count, false));
  OmegaSeriesState& om = c->om;
  HIPCHK(c, hipMemsetAsync(om.series.end_a(om.row()), 0, sizeof(unsigned long long) * om.row() * count, c->stream));
  for (int64_t i = 0; i < count; i += kOmegaHistoryChunk) {
    const int64_t m = std::min<int64_t>(kOmegaHistoryChunk, count - i);
    HIPCHK_RC(omega_frames_launch(c, true, c->hist.b.get() + (first + i) * 2 * c->n, 2 * c->n, m));
  }
  return SWRT_OK;
  GUARD_END(c)
}

int64_t swrt_omega_series_frames(const swrt_ctx* c) { return c ? c->om.series.ext.frames() : -1; }

int64_t swrt_omega_series_bins(const swrt_ctx* c) { return c ? (c->om.open ? c->om.nb : 0) : -1; }

int swrt_omega_series_get(swrt_ctx* c, int64_t first, int64_t count, int64_t* counts_out, double* stats4_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return series_get(c, c->om.series, c->om.row(), kOmegaStats, first, count, counts_out, stats4_out,
                    "frame range out of bounds");
  GUARD_END(c)
}

int swrt_omega_series_reset(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (as swrt_raydiag_series_reset)
  c->om.series.ext.cleared();
  return SWRT_OK;
}

int swrt_omega_ideal(swrt_ctx* c, int slot, const double* ring_k, int64_t m, double omega0, const double* edges,
                     int64_t nbins, int64_t* counts_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c);
  if (slot < 0 || slot >= SWRT_MAX_SLOTS || !c->slot[slot].set) return fail(c, SWRT_ERR_ARG, "field slot not set");
  if (m < 1 || m > (1 << 20)) return fail(c, SWRT_ERR_ARG, "m must be 1..2^20");
  HIPCHK_RC(omega_edges_check(c, edges, nbins));
  if (!ring_k || !counts_out) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  const Slot& s = c->slot[slot];
  const size_t nslot = (size_t)nbins + 2;
  HIPCHK_RC(ensure_scratch(c, sizeof(double) * (nbins + 1 + 2 * m) + sizeof(unsigned long long) * nslot));
  double* dedges = (double*)c->scratch.get();
  double* dring = dedges + nbins + 1;
  unsigned long long* drow = (unsigned long long*)(dring + 2 * m);
  HIPCHK(c, hipMemcpyAsync(dedges, edges, sizeof(double) * (nbins + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dring, ring_k, sizeof(double) * 2 * m, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(drow, 0, sizeof(unsigned long long) * nslot, c->stream));
  const int64_t total = s.nx * s.nx * m;
  const int nblk = (int)std::min<int64_t>(kOmegaBlocks, nblocks(total, kOmegaThreads));
  hipLaunchKernelGGL(omega_ideal_kernel, dim3(nblk), dim3(kOmegaThreads), omega_lds_bytes((int)nbins), c->stream,
                     s.nodes.get(), (int)s.nx, (int)s.npad, dring, m, omega0, dedges, (int)nbins, drow);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(counts_out, drow, sizeof(int64_t) * nslot, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

// ---- the map series (swrt_map.hpp, swrt_host_diag.hpp) ----
int swrt_map_series_begin(swrt_ctx* c, double L, int64_t m, double f, double Cg, int frac_bits) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (m < 1 || m > kMapMaxCells) return fail(c, SWRT_ERR_ARG, "m must be 1..4096");
  if (!(L > 0.0) || !std::isfinite(L)) return fail(c, SWRT_ERR_ARG, "L must be positive and finite");
  if (frac_bits < 0 || frac_bits > kMapMaxFracBits) return fail(c, SWRT_ERR_ARG, "frac_bits must be 0..32");
  if (c->n > kMapMaxPackets) return fail(c, SWRT_ERR_ARG, "a map frame takes at most 2^24 packets");
  HIPCHK(c, hipSetDevice(c->device));
  MapSeriesState& ms = c->map;
  HIPCHK_RC(series_release(c, ms.series));
  ms.open = false;
  if (!ms.strays) {
    HIPCHK(c, ms.strays.alloc(1));
    HIPCHK(c, hipMemsetAsync(ms.strays.get(), 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  ms.m = (int)m;
  ms.frac_bits = frac_bits;
  ms.L = L;
  ms.f2 = f * f;
  ms.Cg2 = Cg * Cg;
  ms.open = true;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_map_series_record(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(map_series_check(c));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(map_reserve_zeroed(c, 1));
  if (!map_tiled(c)) return map_general_launch(c, c->pk.cur.x.get(), c->pk.cur.k.get(), 0, 1);
  return map_tile_launch(c);
  GUARD_END(c)
}

int swrt_map_series_record_history(swrt_ctx* c, int64_t first, int64_t count) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(map_series_check(c));
  HIPCHK_RC(frame_range_check(c, c->hist.ext, first, count, "history frame range out of bounds"));
  if (count == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(map_reserve_zeroed(c, count));
  return history_chunks(c, first, count, kMapHistoryChunk, [&](int64_t, int64_t off, int64_t nf) {
    return map_general_launch(c, c->hist.a.get() + off, c->hist.b.get() + off, 2 * c->n, nf);
  });
  GUARD_END(c)
}

int64_t swrt_map_series_frames(const swrt_ctx* c) { return c ? c->map.series.ext.frames() : -1; }

int64_t swrt_map_series_cells(const swrt_ctx* c) { return c ? (c->map.open ? c->map.m : 0) : -1; }

int swrt_map_series_get(swrt_ctx* c, int64_t first, int64_t count, int64_t* planes4_out, int64_t* stats2_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return series_get(c, c->map.series, c->map.frame(), kMapStats, first, count, planes4_out, stats2_out,
                    "frame range out of bounds");
  GUARD_END(c)
}

int swrt_map_series_reset(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (as swrt_raydiag_series_reset)
  c->map.series.ext.cleared();
  return SWRT_OK;
}

// ---- the wave-vector plane series (swrt_kmap.hpp, swrt_host_diag.hpp) ----
int swrt_kmap_series_begin(swrt_ctx* c, double K, int64_t m, int frac_bits) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!(K > 0.0) || !std::isfinite(K)) return fail(c, SWRT_ERR_ARG, "K must be positive and finite");
  if (m < 1 || m > kKmapMaxCells) return fail(c, SWRT_ERR_ARG, "m must be 1..4096");
  if (frac_bits < 0 || frac_bits > kKmapMaxFracBits) return fail(c, SWRT_ERR_ARG, "frac_bits must be 0..32");
  if (c->n > kKmapMaxPackets) return fail(c, SWRT_ERR_ARG, "a k-plane frame takes at most 2^24 packets");
  HIPCHK(c, hipSetDevice(c->device));
  KmapSeriesState& ks = c->kmap;
  HIPCHK_RC(series_release(c, ks.series));
  ks.m = (int)m;
  ks.frac_bits = frac_bits;
  ks.K = K;
  ks.s = (double)m / (2.0 * K);
  ks.open = true;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_kmap_series_record(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(kmap_series_check(c));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(kmap_reserve_zeroed(c, 1));
  return kmap_launch(c, c->pk.cur.k.get(), 0, 1);
  GUARD_END(c)
}

int swrt_kmap_series_record_history(swrt_ctx* c, int64_t first, int64_t count) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(kmap_series_check(c));
  HIPCHK_RC(frame_range_check(c, c->hist.ext, first, count, "history frame range out of bounds"));
  if (count == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(kmap_reserve_zeroed(c, count));
  return history_chunks(c, first, count, kKmapHistoryChunk, [&](int64_t, int64_t off, int64_t nf) {
    return kmap_launch(c, c->hist.b.get() + off, 2 * c->n, nf);
  });
  GUARD_END(c)
}

int64_t swrt_kmap_series_frames(const swrt_ctx* c) { return c ? c->kmap.series.ext.frames() : -1; }

int64_t swrt_kmap_series_cells(const swrt_ctx* c) { return c ? (c->kmap.open ? c->kmap.m : 0) : -1; }

int swrt_kmap_series_get(swrt_ctx* c, int64_t first, int64_t count, int64_t* plane_out, int64_t* stats8_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return kmap_series_get(c, first, count, plane_out, stats8_out);
  GUARD_END(c)
}

int swrt_kmap_series_reset(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (as swrt_raydiag_series_reset)
  c->kmap.series.ext.cleared();
  return SWRT_OK;
}

// ---- the track series (swrt_track.hpp, swrt_host_diag.hpp) ----
int swrt_track_begin(swrt_ctx* c, const int64_t* ids, int64_t m) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(packets_check(c));
  if (m < 1 || m > c->n || m > kTrackMax) return fail(c, SWRT_ERR_ARG, "m must be 1..min(N, 2^20)");
  if (!ids) return fail(c, SWRT_ERR_ARG, "NULL buffer (ids)");
  std::vector<int> table((size_t)c->n, -1), dense((size_t)m);
  for (int64_t j = 0; j < m; ++j) {
    if (ids[j] < 0 || ids[j] >= c->n)
      return fail(c, SWRT_ERR_ARG, "track id " + std::to_string(ids[j]) + " out of range (0..N-1)");
    if (table[ids[j]] >= 0) return fail(c, SWRT_ERR_ARG, "track id " + std::to_string(ids[j]) + " given twice");
    table[ids[j]] = (int)j;
    dense[j] = (int)ids[j];
  }
  HIPCHK(c, hipSetDevice(c->device));
  TrackState& tr = c->trk;
  HIPCHK_RC(series_release(c, tr.series));  // (waits: queued records read the old tables too)
  tr.drop();
  HIPCHK(c, tr.slot_of.alloc(c->n));
  HIPCHK(c, tr.dids.alloc(m));
  HIPCHK(c, hipMemcpyAsync(tr.slot_of.get(), table.data(), sizeof(int) * c->n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(tr.dids.get(), dense.data(), sizeof(int) * m, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  tr.ids.assign(ids, ids + m);
  tr.m = m;
  tr.open = true;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_track_record(swrt_ctx* c, double f, double gH, int nslots, double alpha, double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c, false, track_slot_mask(nslots));
  HIPCHK_RC(track_check(c, nslots));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(track_reserve(c, 1));
  return track_record_frame(c, f, gH, nslots, alpha, bump);
  GUARD_END(c)
}

int swrt_track_record_history(swrt_ctx* c, int64_t first, int64_t count, double f, double gH, int nslots,
                              const double* alphas, double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c, false, track_slot_mask(nslots));
  HIPCHK_RC(track_check(c, nslots));
  HIPCHK_RC(frame_range_check(c, c->hist.ext, first, count, "history frame range out of bounds"));
  if (nslots == 2 && !alphas && count > 0) return fail(c, SWRT_ERR_ARG, "NULL buffer (alphas, two snapshots)");
  if (count == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(track_reserve(c, count));
  for (int64_t i = 0; i < count; ++i) {
    const int64_t off = (first + i) * 2 * c->n;
    HIPCHK_RC(track_record_frame(c, f, gH, nslots, alphas ? alphas[i] : 0.0, bump, c->hist.a.get() + off,
                                 c->hist.b.get() + off));
  }
  return SWRT_OK;
  GUARD_END(c)
}

int64_t swrt_track_frames(const swrt_ctx* c) { return c ? c->trk.series.ext.frames() : -1; }

int64_t swrt_track_count(const swrt_ctx* c) { return c ? (c->trk.open ? c->trk.m : 0) : -1; }

int swrt_track_ids(const swrt_ctx* c, int64_t* ids_out) {
  if (!c) return SWRT_ERR_ARG;
  if (!c->trk.open) return SWRT_ERR_STATE;
  if (!ids_out) return SWRT_ERR_ARG;
  std::copy(c->trk.ids.begin(), c->trk.ids.end(), ids_out);
  return SWRT_OK;
}

int swrt_track_get(swrt_ctx* c, int64_t first, int64_t count, double* frames_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return series_get(c, c->trk.series, c->trk.frame(), 0, first, count, frames_out, nullptr,
                    "frame range out of bounds");
  GUARD_END(c)
}

int swrt_track_reset(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (as swrt_raydiag_series_reset)
  c->trk.series.ext.cleared();
  return SWRT_OK;
}

// ---- the flow spectrum series (swrt_flowspec.hpp, swrt_host_diag.hpp) ----
// Every call runs on the QG stream (OnQGStream) and none touches the packets.
int swrt_flow_spectrum_begin(swrt_ctx* c, int64_t nx, double k_scale, double K_d2) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  if (nx < 8 || nx > 4096 || !is_pow2(nx)) return fail(c, SWRT_ERR_ARG, "nx must be a power of two, 8..4096");
  if (!(k_scale > 0.0) || !std::isfinite(k_scale)) return fail(c, SWRT_ERR_ARG, "k_scale must be positive and finite");
  if (!(K_d2 >= 0.0) || !std::isfinite(K_d2)) return fail(c, SWRT_ERR_ARG, "K_d2 must be finite and not negative");
  HIPCHK(c, hipSetDevice(c->device));
  FlowSpecState& fs = c->flow;
  HIPCHK_RC(series_release(c, fs.series));  // (waits: a queued record_qk may still read the staged plane)
  fs.stage.reset();
  fs.nx = (int)nx;
  fs.nshell = flow_shells((int)nx);
  fs.k_scale = k_scale;
  fs.K_d2 = K_d2;
  fs.open = true;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_flow_spectrum_record_qg(swrt_ctx* c, int layer) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  const QGState& q = c->qg;
  if (!c->flow.open) return fail(c, SWRT_ERR_STATE, "call swrt_flow_spectrum_begin first");
  if (!q.init) return fail(c, SWRT_ERR_STATE, "swrt_qg_init not called");
  if (q.g.n != c->flow.nx) return fail(c, SWRT_ERR_STATE, "the QG state's nx differs from the series'");
  if (layer < 0 || layer >= q.g.nl) return fail(c, SWRT_ERR_ARG, "layer out of range");
  HIPCHK(c, hipSetDevice(c->device));
  // (a pending speculative step writes the spare buffers only, as for swrt_qg_export)
  const int kmax = q.g.n / 2 - 1;
  return flow_spectrum_record_frame(c, q.qk.get() + layer * q.nhalf, kmax + 1, 1, q.t);
  GUARD_END(c)
}

int swrt_flow_spectrum_record_qk(swrt_ctx* c, const double* qk_interleaved, int64_t nx, double t) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  FlowSpecState& fs = c->flow;
  if (!fs.open) return fail(c, SWRT_ERR_STATE, "call swrt_flow_spectrum_begin first");
  if (nx != fs.nx) return fail(c, SWRT_ERR_STATE, "nx differs from the series'");
  if (!qk_interleaved) return fail(c, SWRT_ERR_ARG, "NULL buffer (qk_interleaved)");
  HIPCHK(c, hipSetDevice(c->device));
  const int kmax = fs.nx / 2 - 1;
  const size_t nhalf = (size_t)(2 * kmax + 1) * (kmax + 1);
  if (!fs.stage) HIPCHK(c, fs.stage.alloc(nhalf));
  HIPCHK(c, hipMemcpyAsync(fs.stage.get(), qk_interleaved, sizeof(double2) * nhalf, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's host buffer is free on return
  return flow_spectrum_record_frame(c, fs.stage.get(), 1, 2 * kmax + 1, t);
  GUARD_END(c)
}

int64_t swrt_flow_spectrum_frames(const swrt_ctx* c) { return c ? c->flow.series.ext.frames() : -1; }

int64_t swrt_flow_spectrum_shells(const swrt_ctx* c) { return c ? (c->flow.open ? c->flow.nshell : 0) : -1; }

int swrt_flow_spectrum_get(swrt_ctx* c, int64_t first, int64_t count, double* spectra_out, double* stats4_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  return flow_spectrum_get(c, first, count, spectra_out, stats4_out);
  GUARD_END(c)
}

int swrt_flow_spectrum_reset(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  c->flow.series.ext.cleared();
  return SWRT_OK;
}

// ---- the conditional spectrum series (swrt_cond.hpp, swrt_host_diag.hpp) ----
int swrt_cond_series_begin(swrt_ctx* c, double f, double Cg, const double* omega_edges, int64_t nw, int which,
                           const double* q_edges, int64_t nq, int frac_bits) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  const char* which_err = which < 0 || which > 2 ? "which must be 0 (zeta), 1 (sigma) or 2 (D)" : nullptr;
  HIPCHK_RC(plane_series_begin(c, c->cond, f, Cg, omega_edges, nw, q_edges, nq, frac_bits,
                               "(nq + 2) * (nw + 2) must be at most 65536", which_err, [] {}));
  c->cond.which = which;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_cond_series_record(swrt_ctx* c, int nslots, double alpha, double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c, false, track_slot_mask(nslots));
  HIPCHK_RC(cond_series_check(c, nslots));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(plane_reserve_zeroed(c, c->cond, 1));
  return cond_launch(c, nslots, alpha, nullptr, bump, c->pk.cur.x.get(), c->pk.cur.k.get(), 0, 1);
  GUARD_END(c)
}

int swrt_cond_series_record_history(swrt_ctx* c, int64_t first, int64_t count, int nslots, const double* alphas,
                                    double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c, false, track_slot_mask(nslots));
  HIPCHK_RC(cond_series_check(c, nslots));
  return plane_record_history(c, c->cond, first, count, nslots == 2, alphas, kCondHistoryChunk,
                              [&](const double* dalphas, const double* x, const double* k, int64_t nf) {
                                return cond_launch(c, nslots, 0.0, dalphas, bump, x, k, 2 * c->n, nf);
                              });
  GUARD_END(c)
}

int64_t swrt_cond_series_frames(const swrt_ctx* c) { return plane_series_frames(c, &swrt_ctx::cond); }

int swrt_cond_series_bins(const swrt_ctx* c, int64_t* nw_out, int64_t* nq_out) {
  return plane_series_bins(c, &swrt_ctx::cond, nw_out, nq_out);
}

int swrt_cond_series_get(swrt_ctx* c, int64_t first, int64_t count, int64_t* counts_out, int64_t* sums_out,
                         int64_t* stats2_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return plane_series_get(c, c->cond, first, count, counts_out, sums_out, stats2_out);
  GUARD_END(c)
}

int swrt_cond_series_reset(swrt_ctx* c) { return plane_series_reset(c, &swrt_ctx::cond); }

// ---- the transition series (swrt_trans.hpp, swrt_host_diag.hpp) ----
int swrt_trans_series_begin(swrt_ctx* c, double f, double Cg, const double* omega_edges, int64_t nw,
                            const double* src_edges, int64_t ns, int frac_bits) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  TransSeriesState& ts = c->trans;
  return plane_series_begin(c, ts, f, Cg, omega_edges, nw, src_edges, ns, frac_bits,
                            "(ns + 2) * (nw + 2) must be at most 65536", nullptr, [&ts] {
                              ts.marked = false;  // (a mark of omega belongs to the f and Cg it was taken with)
                              ts.serial = 0;
                            });
  GUARD_END(c)
}

int swrt_trans_series_mark(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(trans_series_check(c, false));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(trans_src_reserve(c));
  TransSeriesState& ts = c->trans;
  hipLaunchKernelGGL(trans_mark_kernel, dim3(nblocks(c->n, kTransThreads)), dim3(kTransThreads), 0, c->stream,
                     c->pk.cur.k.get(), c->pk.cur.perm.get(), c->n, ts.f2, ts.Cg2, ts.src.get());
  HIPCHK(c, hipGetLastError());
  ++ts.serial;
  ts.marked = true;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_trans_series_mark_values(swrt_ctx* c, const double* v, int64_t n) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(trans_series_check(c, false));
  if (n != c->n) return fail(c, SWRT_ERR_ARG, "one source value per packet: n must equal the packet count");
  if (!v) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(trans_src_reserve(c));
  TransSeriesState& ts = c->trans;
  // (the stream orders the upload after the queued records that read the old mark)
  HIPCHK(c, hipMemcpyAsync(ts.src.get(), v, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's buffer is free on return
  ++ts.serial;
  ts.marked = true;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_trans_series_record(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(trans_series_check(c, true));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(plane_reserve_zeroed(c, c->trans, 1));
  return trans_launch(c, c->pk.cur.k.get(), c->pk.cur.perm.get(), 0, 1);
  GUARD_END(c)
}

int swrt_trans_series_record_history(swrt_ctx* c, int64_t first, int64_t count) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(trans_series_check(c, true));
  return plane_record_history(c, c->trans, first, count, false, nullptr, kTransHistoryChunk,
                              [&](const double*, const double*, const double* k, int64_t nf) {
                                return trans_launch(c, k, nullptr, 2 * c->n, nf);
                              });
  GUARD_END(c)
}

int64_t swrt_trans_series_frames(const swrt_ctx* c) { return plane_series_frames(c, &swrt_ctx::trans); }

int swrt_trans_series_bins(const swrt_ctx* c, int64_t* nw_out, int64_t* ns_out) {
  return plane_series_bins(c, &swrt_ctx::trans, nw_out, ns_out);
}

int swrt_trans_series_get(swrt_ctx* c, int64_t first, int64_t count, int64_t* counts_out, int64_t* sums_out,
                          int64_t* stats3_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return plane_series_get(c, c->trans, first, count, counts_out, sums_out, stats3_out);
  GUARD_END(c)
}

int swrt_trans_series_reset(swrt_ctx* c) { return plane_series_reset(c, &swrt_ctx::trans); }

// ---- packet recycling (swrt_recycle.hpp, swrt_host_diag.hpp) ----
int swrt_recycle_begin(swrt_ctx* c, double f, double Cg, double omega_cut, double L, uint64_t seed, int64_t index_base,
                       int frac_bits, const double* home_k) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!std::isfinite(f) || !std::isfinite(Cg) || !std::isfinite(omega_cut))
    return fail(c, SWRT_ERR_ARG, "f, Cg and omega_cut must be finite");
  if (!std::isfinite(L) || !(L > 0.0)) return fail(c, SWRT_ERR_ARG, "L must be finite and positive");
  if (!(omega_cut > std::fabs(f))) return fail(c, SWRT_ERR_ARG, "omega_cut must be above |f|: no wave lies below it");
  if (frac_bits < 0 || frac_bits > kRecycleMaxFracBits) return fail(c, SWRT_ERR_ARG, "frac_bits must be 0..32");
  HIPCHK_RC(packets_check(c));
  HIPCHK(c, hipSetDevice(c->device));
  RecycleState& rs = c->recycle;
  HIPCHK_RC(series_release(c, rs.series));  // (waits: queued events use the old state too)
  rs.open = rs.live = false;
  rs.n = 0;
  const int64_t n = c->n;
  HIPCHK(c, rs.home.alloc(2 * n));
  HIPCHK(c, rs.marks.alloc(2 * n));
  if (!rs.bad) HIPCHK(c, rs.bad.alloc(1));
  rs.n = n;
  if (c->hz.on) {
    c->hz.name(rs.home.get(), "recycle home wavevectors");
    c->hz.name(rs.gen(), "recycle generation and birth marks");
  }
  const dim3 grid(nblocks(n, kRecycleThreads)), block(kRecycleThreads);
  if (home_k) {
    HIPCHK(c, hipMemcpyAsync(rs.home.get(), home_k, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
  } else {
    hipLaunchKernelGGL(recycle_home_kernel, grid, block, 0, c->stream, c->pk.cur.k.get(), c->pk.cur.perm.get(), n,
                       rs.home.get());
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemsetAsync(rs.marks.get(), 0, sizeof(int) * 2 * n, c->stream));
  HIPCHK(c, hipMemsetAsync(rs.bad.get(), 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(recycle_home_check_kernel, grid, block, 0, c->stream, rs.home.get(), n, f * f, Cg * Cg, omega_cut,
                     std::ldexp(1.0, frac_bits), rs.bad.get());
  HIPCHK(c, hipGetLastError());
  int bad = 0;
  HIPCHK(c, hipMemcpyAsync(&bad, rs.bad.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the one read-back; the caller's home_k is free on return
  hz_synced(c);
  if (bad)
    return fail(c, SWRT_ERR_ARG,
                "a home wavevector's omega is at or above omega_cut, or too large for the frame: its packet would be "
                "absorbed at every event");
  rs.f2 = f * f;
  rs.Cg2 = Cg * Cg;
  rs.cut = omega_cut;
  rs.L = L;
  rs.seed = seed;
  rs.base = index_base;
  rs.frac_bits = frac_bits;
  rs.serial = 0;
  rs.open = rs.live = true;
  return dev_err_check(c);
  GUARD_END(c)
}

int swrt_recycle_apply(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  HIPCHK_RC(tangent_refuse(c, "swrt_recycle_apply"));
  GUARD_BEGIN
  HIPCHK_RC(recycle_check(c));
  HIPCHK(c, hipSetDevice(c->device));
  return recycle_launch(c);
  GUARD_END(c)
}

int64_t swrt_recycle_frames(const swrt_ctx* c) { return c ? c->recycle.series.ext.frames() : -1; }

int swrt_recycle_get(swrt_ctx* c, int64_t first, int64_t count, int64_t* stats8_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!c->recycle.open) return fail(c, SWRT_ERR_STATE, "call swrt_recycle_begin first");
  return series_get(c, c->recycle.series, kRecycleFrame, 0, first, count, stats8_out, nullptr,
                    "frame range out of bounds");
  GUARD_END(c)
}

int swrt_recycle_state(swrt_ctx* c, int32_t* gen_out, int32_t* born_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(recycle_check(c));
  HIPCHK(c, hipSetDevice(c->device));
  const RecycleState& rs = c->recycle;
  if (gen_out)
    HIPCHK(c, hipMemcpyAsync(gen_out, rs.gen(), sizeof(int32_t) * rs.n, hipMemcpyDeviceToHost, c->stream));
  if (born_out)
    HIPCHK(c, hipMemcpyAsync(born_out, rs.born(), sizeof(int32_t) * rs.n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return dev_err_check(c);
  GUARD_END(c)
}

int swrt_recycle_reset(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN  // (the packets stay as they are)
  RecycleState& rs = c->recycle;
  rs.series.ext.cleared();
  rs.serial = 0;
  if (rs.live) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(rs.marks.get(), 0, sizeof(int) * 2 * rs.n, c->stream));
  }
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_recycle_end(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  RecycleState& rs = c->recycle;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(series_release(c, rs.series));  // (waits: nothing queued uses the buffers below any more)
  rs.open = rs.live = false;
  rs.serial = 0;
  rs.n = 0;
  rs.home.reset();
  rs.marks.reset();
  return SWRT_OK;
  GUARD_END(c)
}

// ---- the refraction series (swrt_refr.hpp, swrt_host_diag.hpp) ----
int swrt_refr_series_begin(swrt_ctx* c, double f, double Cg, const double* omega_edges, int64_t nw,
                           const double* a_edges, int64_t na, int frac_bits) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return plane_series_begin(c, c->refr, f, Cg, omega_edges, nw, a_edges, na, frac_bits,
                            "(na + 2) * (nw + 2) must be at most 65536", nullptr, [] {});
  GUARD_END(c)
}

int swrt_refr_series_record(swrt_ctx* c, int nslots, double alpha, double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c, false, track_slot_mask(nslots));
  HIPCHK_RC(refr_series_check(c, nslots));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(plane_reserve_zeroed(c, c->refr, 1));
  return refr_launch(c, nslots, alpha, nullptr, bump, c->pk.cur.x.get(), c->pk.cur.k.get(), 0, 1);
  GUARD_END(c)
}

int swrt_refr_series_record_history(swrt_ctx* c, int64_t first, int64_t count, int nslots, const double* alphas,
                                    double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c, false, track_slot_mask(nslots));
  HIPCHK_RC(refr_series_check(c, nslots));
  return plane_record_history(c, c->refr, first, count, nslots == 2, alphas, kRefrHistoryChunk,
                              [&](const double* dalphas, const double* x, const double* k, int64_t nf) {
                                return refr_launch(c, nslots, 0.0, dalphas, bump, x, k, 2 * c->n, nf);
                              });
  GUARD_END(c)
}

int64_t swrt_refr_series_frames(const swrt_ctx* c) { return plane_series_frames(c, &swrt_ctx::refr); }

int swrt_refr_series_bins(const swrt_ctx* c, int64_t* nw_out, int64_t* na_out) {
  return plane_series_bins(c, &swrt_ctx::refr, nw_out, na_out);
}

int swrt_refr_series_get(swrt_ctx* c, int64_t first, int64_t count, int64_t* counts_out, int64_t* sums_out,
                         int64_t* stats2_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return plane_series_get(c, c->refr, first, count, counts_out, sums_out, stats2_out);
  GUARD_END(c)
}

int swrt_refr_series_reset(swrt_ctx* c) { return plane_series_reset(c, &swrt_ctx::refr); }

// ---- the absolute-frequency series (swrt_absfreq.hpp, swrt_host_diag.hpp) ----
int swrt_absfreq_series_begin(swrt_ctx* c, double f, double Cg, const double* omega_edges, int64_t nw,
                              const double* abs_edges, int64_t no, int frac_bits) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return plane_series_begin(c, c->absfreq, f, Cg, omega_edges, nw, abs_edges, no, frac_bits,
                            "(no + 2) * (nw + 2) must be at most 65536", nullptr, [] {});
  GUARD_END(c)
}

int swrt_absfreq_series_record(swrt_ctx* c, int slot_a, int slot_b, double alpha, double tau, double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c, false, absfreq_slot_mask(slot_a, slot_b));
  HIPCHK_RC(absfreq_series_check(c, slot_a, slot_b, tau));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(plane_reserve_zeroed(c, c->absfreq, 1));
  return absfreq_launch(c, slot_a, slot_b, alpha, nullptr, tau, bump, c->pk.cur.x.get(), c->pk.cur.k.get(), 0, 1);
  GUARD_END(c)
}

int swrt_absfreq_series_record_history(swrt_ctx* c, int64_t first, int64_t count, int slot_a, int slot_b,
                                       const double* alphas, double tau, double bump) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  SlotUse slot_use(c, false, absfreq_slot_mask(slot_a, slot_b));
  HIPCHK_RC(absfreq_series_check(c, slot_a, slot_b, tau));
  return plane_record_history(c, c->absfreq, first, count, slot_b >= 0, alphas, kAbsfreqHistoryChunk,
                              [&](const double* dalphas, const double* x, const double* k, int64_t nf) {
                                return absfreq_launch(c, slot_a, slot_b, 0.0, dalphas, tau, bump, x, k, 2 * c->n, nf);
                              });
  GUARD_END(c)
}

int64_t swrt_absfreq_series_frames(const swrt_ctx* c) { return plane_series_frames(c, &swrt_ctx::absfreq); }

int swrt_absfreq_series_bins(const swrt_ctx* c, int64_t* nw_out, int64_t* no_out) {
  return plane_series_bins(c, &swrt_ctx::absfreq, nw_out, no_out);
}

int swrt_absfreq_series_get(swrt_ctx* c, int64_t first, int64_t count, int64_t* counts_out, int64_t* sums_out,
                            int64_t* stats2_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return plane_series_get(c, c->absfreq, first, count, counts_out, sums_out, stats2_out);
  GUARD_END(c)
}

int swrt_absfreq_series_reset(swrt_ctx* c) { return plane_series_reset(c, &swrt_ctx::absfreq); }

// ---- the tangent map (swrt_tangent.hpp, swrt_host_packets.hpp, swrt_host_diag.hpp) ----
int swrt_tangent_begin(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(packets_check(c));
  HIPCHK(c, hipSetDevice(c->device));
  TangentState& ts = c->tan;
  ts.live = false;
  if (c->n != ts.n || !ts.M) {  // (releasing the old buffers waits for their queued users)
    if (c->hz.on) {
      c->hz.bufs.erase(ts.M.get());
      c->hz.bufs.erase(ts.caustics.get());
    }
    ts.n = 0;
    HIPCHK(c, ts.M.alloc((size_t)kTanM * c->n));
    HIPCHK(c, ts.caustics.alloc(c->n));
    ts.n = c->n;
    if (c->hz.on) {
      c->hz.name(ts.M.get(), "tangent maps");
      c->hz.name(ts.caustics.get(), "caustic counters");
    }
  }
  ts.serial = 0;
  HIPCHK_RC(tangent_mark_queue(c));  // serial 1
  ts.live = true;
  c->bin.invalidate();  // the per-packet route's binning from here on
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_tangent_mark(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(tangent_check(c));
  HIPCHK(c, hipSetDevice(c->device));
  return tangent_mark_queue(c);
  GUARD_END(c)
}

int swrt_tangent_get(swrt_ctx* c, double* M16_out, int32_t* caustics_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  HIPCHK_RC(tangent_check(c));
  HIPCHK(c, hipSetDevice(c->device));
  const TangentState& ts = c->tan;
  if (M16_out)
    HIPCHK(c, hipMemcpyAsync(M16_out, ts.M.get(), sizeof(double) * kTanM * ts.n, hipMemcpyDeviceToHost, c->stream));
  if (caustics_out)
    HIPCHK(c, hipMemcpyAsync(caustics_out, ts.caustics.get(), sizeof(int32_t) * ts.n, hipMemcpyDeviceToHost,
                             c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return dev_err_check(c);
  GUARD_END(c)
}

int swrt_tangent_end(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  TangentState& ts = c->tan;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // nothing queued uses the buffers below any more
  hz_synced(c);
  if (c->hz.on) {
    c->hz.bufs.erase(ts.M.get());
    c->hz.bufs.erase(ts.caustics.get());
  }
  ts.live = false;
  ts.n = 0;
  ts.serial = 0;
  ts.M.reset();
  ts.caustics.reset();
  c->bin.invalidate();  // back to the route the settings name
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_tangent_live(const swrt_ctx* c) { return c ? (c->tan.live ? 1 : 0) : -1; }

int64_t swrt_tangent_serial(const swrt_ctx* c) { return c ? (c->tan.live ? c->tan.serial : 0) : -1; }

int swrt_tangent_series_begin(swrt_ctx* c, double f, double Cg, const double* omega_edges, int64_t nw,
                              const double* growth_edges, int64_t ns) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return plane_series_begin(c, c->tan, f, Cg, omega_edges, nw, growth_edges, ns, 0,
                            "(ns + 2) * (nw + 2) must be at most 65536", nullptr, [] {});
  GUARD_END(c)
}

int swrt_tangent_series_record(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (!c->tan.open) return fail(c, SWRT_ERR_STATE, "call swrt_tangent_series_begin first");
  HIPCHK_RC(tangent_check(c));
  if (c->n > kTanMaxPackets) return fail(c, SWRT_ERR_ARG, "a tangent frame takes at most 2^24 packets");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(plane_reserve_zeroed(c, c->tan, 1));
  return tangent_record_launch(c);
  GUARD_END(c)
}

int64_t swrt_tangent_series_frames(const swrt_ctx* c) { return plane_series_frames(c, &swrt_ctx::tan); }

int swrt_tangent_series_bins(const swrt_ctx* c, int64_t* nw_out, int64_t* ns_out) {
  return plane_series_bins(c, &swrt_ctx::tan, nw_out, ns_out);
}

int swrt_tangent_series_get(swrt_ctx* c, int64_t first, int64_t count, int64_t* counts_out, int64_t* sums_out,
                            int64_t* stats3_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  return plane_series_get(c, c->tan, first, count, counts_out, sums_out, stats3_out);
  GUARD_END(c)
}

int swrt_tangent_series_reset(swrt_ctx* c) { return plane_series_reset(c, &swrt_ctx::tan); }

int swrt_check_arith(swrt_ctx* c, int64_t n, uint64_t seed, int64_t* mismatches3) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN
  if (n <= 0 || !mismatches3) return fail(c, SWRT_ERR_ARG, "n must be > 0, mismatches3 non-NULL");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_scratch(c, 3 * sizeof(unsigned long long)))) return rc;
  unsigned long long* d = (unsigned long long*)c->scratch.get();
  HIPCHK(c, hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(check_arith_kernel, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, seed, d);
  HIPCHK(c, hipGetLastError());
  unsigned long long h[3];
  HIPCHK(c, hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int q = 0; q < 3; ++q) mismatches3[q] = (int64_t)h[q];
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_synchronize(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sync_sx(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->qstream.get()));
  if (c->hz.on) c->hz.sync_all();
  return dev_err_check(c);
}

int swrt_debug_set(swrt_ctx* c, int key, int64_t value) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (int rc = chain_drop(c)) return rc;
  switch (key) {
    case SWRT_DEBUG_HAZARD_CHECK:
      if (value != 0 && value != 1) return fail(c, SWRT_ERR_ARG, "hazard check must be 0 or 1");
      if (value && !c->hz.on) {
        // start from a quiet device: nothing queued before is tracked
        if (int rc = swrt_synchronize(c)) return rc;
        c->hz = HazardChecker();
      }
      c->hz.on = value != 0;
      if (!c->hz.on) c->dbg.share_skew = false;
      return SWRT_OK;
    case SWRT_DEBUG_SPIN_US:
      if (value < 0 || value > 100000) return fail(c, SWRT_ERR_ARG, "spin must be 0..100000 us");
      c->dbg.spin_us = (int)value;
      return SWRT_OK;
    case SWRT_DEBUG_LEGACY_PARK:
      if (value != 0 && value != 1) return fail(c, SWRT_ERR_ARG, "legacy park must be 0 or 1");
      c->dbg.legacy_park = value != 0;
      return SWRT_OK;
    case SWRT_DEBUG_SHARE_SKEW:
      if (value != 0 && value != 1) return fail(c, SWRT_ERR_ARG, "share skew must be 0 or 1");
      if (value && !c->hz.on) return fail(c, SWRT_ERR_STATE, "the skewed share runs only under the hazard checker");
      c->dbg.share_skew = value != 0;
      return SWRT_OK;
    case SWRT_DEBUG_CORRUPT_COUNT:
      if (value < -1000000 || value > 1000000) return fail(c, SWRT_ERR_ARG, "count corruption out of range");
      c->dbg.corrupt_count = (int)value;
      c->bin.invalidate();  // the next call re-bins (and meets the corrupted count)
      return SWRT_OK;
    case SWRT_DEBUG_ODE23_DENSE_REBIN:
      if (value < 0 || value > 1000000) return fail(c, SWRT_ERR_ARG, "ode23 run_at re-binning cadence out of range");
      c->o23.dense_rebin = value;
      return SWRT_OK;
    case SWRT_DEBUG_KMAP_GLOBAL:
      if (value < 0 || value > 3) return fail(c, SWRT_ERR_ARG, "k-plane path must be 0..3");
      c->dbg.kmap_path = (int)value;
      return SWRT_OK;
    case SWRT_DEBUG_COND_GLOBAL:
      if (value != 0 && value != 1) return fail(c, SWRT_ERR_ARG, "conditional spectrum path must be 0 or 1");
      c->dbg.cond_global = value != 0;
      return SWRT_OK;
    case SWRT_DEBUG_TRANS_GLOBAL:
      if (value != 0 && value != 1) return fail(c, SWRT_ERR_ARG, "transition series path must be 0 or 1");
      c->dbg.trans_global = value != 0;
      return SWRT_OK;
    case SWRT_DEBUG_REFR_GLOBAL:
      if (value != 0 && value != 1) return fail(c, SWRT_ERR_ARG, "refraction series path must be 0 or 1");
      c->dbg.refr_global = value != 0;
      return SWRT_OK;
    case SWRT_DEBUG_ABSFREQ_GLOBAL:
      if (value != 0 && value != 1) return fail(c, SWRT_ERR_ARG, "absolute-frequency series path must be 0 or 1");
      c->dbg.absfreq_global = value != 0;
      return SWRT_OK;
    case SWRT_DEBUG_TANGENT_GLOBAL:
      if (value != 0 && value != 1) return fail(c, SWRT_ERR_ARG, "tangent series path must be 0 or 1");
      c->dbg.tangent_global = value != 0;
      return SWRT_OK;
    case SWRT_DEBUG_QG_UPDATE_COLS:
      if (value != 0 && value != 1) return fail(c, SWRT_ERR_ARG, "QG update/column-pass fusion must be 0 or 1");
      if (c->qg.spec) return fail(c, SWRT_ERR_STATE, "a speculative QG step is pending (swrt_qg_resolve first)");
      c->qg_update_cols = (int)value;
      c->qg.post_valid = false;
      return SWRT_OK;
    case SWRT_DEBUG_QG_JFUSE:
      if (value != 0 && value != 1) return fail(c, SWRT_ERR_ARG, "QG column/Jacobian fusion must be 0 or 1");
      if (c->qg.spec) return fail(c, SWRT_ERR_STATE, "a speculative QG step is pending (swrt_qg_resolve first)");
      c->qg_jfuse = (int)value;
      c->qg.post_valid = false;
      c->qg.post_inv_valid = false;
      return SWRT_OK;
    default:
      return fail(c, SWRT_ERR_ARG, "unknown debug key");
  }
}

int swrt_debug_get(swrt_ctx* c, int key, int64_t* value_out) {
  if (!c || !value_out) return SWRT_ERR_ARG;
  switch (key) {
    case SWRT_DEBUG_HAZARD_CHECK: *value_out = c->hz.on ? 1 : 0; return SWRT_OK;
    case SWRT_DEBUG_SPIN_US: *value_out = c->dbg.spin_us; return SWRT_OK;
    case SWRT_DEBUG_LEGACY_PARK: *value_out = c->dbg.legacy_park ? 1 : 0; return SWRT_OK;
    case SWRT_DEBUG_HAZARD_CHECKS: *value_out = c->hz.checks; return SWRT_OK;
    case SWRT_DEBUG_QG_JFUSE: *value_out = c->qg_jfuse; return SWRT_OK;
    case SWRT_DEBUG_SHARE_SKEW: *value_out = c->dbg.share_skew ? 1 : 0; return SWRT_OK;
    case SWRT_DEBUG_CORRUPT_COUNT: *value_out = c->dbg.corrupt_count; return SWRT_OK;
    case SWRT_DEBUG_QG_UPDATE_COLS: *value_out = c->qg_update_cols; return SWRT_OK;
    case SWRT_DEBUG_ODE23_CHAINED: *value_out = c->o23.chain.taken; return SWRT_OK;
    case SWRT_DEBUG_ODE23_FIRST_TAKEN: *value_out = c->o23.first_taken; return SWRT_OK;
    case SWRT_DEBUG_ODE23_GUESSES_TAKEN: *value_out = c->o23.guesses_taken; return SWRT_OK;
    case SWRT_DEBUG_ODE23_SPLIT_RUNS: *value_out = c->o23.split_runs; return SWRT_OK;
    case SWRT_DEBUG_ODE23_FIRST_CHAINED: *value_out = c->o23.chain.first_taken; return SWRT_OK;
    case SWRT_DEBUG_ODE23_DENSE_REBIN: *value_out = c->o23.dense_rebin; return SWRT_OK;
    case SWRT_DEBUG_ODE23_DENSE_REBINS: *value_out = c->o23.dense_rebins; return SWRT_OK;
    case SWRT_DEBUG_MAP_TILED_FRAMES: *value_out = c->map.tiled_frames; return SWRT_OK;
    case SWRT_DEBUG_KMAP_GLOBAL: *value_out = c->dbg.kmap_path; return SWRT_OK;
    case SWRT_DEBUG_COND_GLOBAL: *value_out = c->dbg.cond_global ? 1 : 0; return SWRT_OK;
    case SWRT_DEBUG_TRANS_GLOBAL: *value_out = c->dbg.trans_global ? 1 : 0; return SWRT_OK;
    case SWRT_DEBUG_REFR_GLOBAL: *value_out = c->dbg.refr_global ? 1 : 0; return SWRT_OK;
    case SWRT_DEBUG_ABSFREQ_GLOBAL: *value_out = c->dbg.absfreq_global ? 1 : 0; return SWRT_OK;
    case SWRT_DEBUG_TANGENT_GLOBAL: *value_out = c->dbg.tangent_global ? 1 : 0; return SWRT_OK;
    case SWRT_DEBUG_MAP_STRAYS: {  // the device's counter: waits for the queued records
      unsigned long long v = 0;
      if (c->map.strays) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipMemcpyAsync(&v, c->map.strays.get(), sizeof(v), hipMemcpyDeviceToHost, c->stream0.get()));
        HIPCHK(c, hipStreamSynchronize(c->stream0.get()));
      }
      *value_out = (int64_t)v;
      return SWRT_OK;
    }
    default: return fail(c, SWRT_ERR_ARG, "unknown debug key");
  }
}

int swrt_qg_set_fused(swrt_ctx* c, int on) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (c->qg.spec) return fail(c, SWRT_ERR_STATE, "a speculative QG step is pending (swrt_qg_resolve first)");
  if (on != 0 && on != 1) return fail(c, SWRT_ERR_ARG, "on must be 0 or 1");
  int rc = swrt_synchronize(c);
  if (rc) return rc;
  c->qg_fused = on != 0;
  c->qg.post_valid = false;
  c->qg.post_inv_valid = false;
  return SWRT_OK;
}

int swrt_qg_set_stream(swrt_ctx* c, int separate) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (c->qg.spec) return fail(c, SWRT_ERR_STATE, "a speculative QG step is pending (swrt_qg_resolve first)");
  if (separate != 0 && separate != 1) return fail(c, SWRT_ERR_ARG, "separate must be 0 or 1");
  int rc = swrt_synchronize(c);
  if (rc) return rc;
  c->qg_sep = separate != 0;
  return SWRT_OK;
}

int swrt_get_stream(swrt_ctx* c, void** out) {
  if (!c || !out) return SWRT_ERR_ARG;
  if (int rc = join_b(c)) return rc;  // work queued on it by the caller sees every packet
  c->s0_dirty = true;                   // ... and the next split launch follows that work
  *out = (void*)c->stream;
  return SWRT_OK;
}

int swrt_kernel_time(swrt_ctx* c, int reset, double* total_ms, int64_t* launches) {
  if (!c) return SWRT_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  for (const Stream& s : c->sx)  // stop events of split launches
    if (s) HIPCHK(c, hipStreamSynchronize(s.get()));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double tot = c->timing.folded_ms;
  for (size_t i = 0; i + 1 < c->timing.used; i += 2) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->timing.ev[i].get(), c->timing.ev[i + 1].get()));
    tot += ms;
  }
  HIPCHK_RC(dev_err_check(c));
  if (total_ms) *total_ms = tot;
  if (launches) *launches = c->timing.folded_n + (int64_t)(c->timing.used / 2);
  if (reset) {
    c->timing.used = 0;
    c->timing.folded_ms = 0.0;
    c->timing.folded_n = 0;
  }
  return SWRT_OK;
}

int swrt_clock_stamp(swrt_ctx* c, int which) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN  // join_b: the stamp follows every packet launch queued on any packet stream
  if (which != 0 && which != 1) return fail(c, SWRT_ERR_ARG, "which must be 0 (start) or 1 (end)");
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->clk) HIPCHK(c, c->clk.alloc(2 * kClockWaves * 3));
  hipLaunchKernelGGL(clock_stamp_kernel, dim3(kClockWaves), dim3(64), 0, c->stream,
                     c->clk.get() + which * kClockWaves * 3);
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_clock_ghz(swrt_ctx* c, double* ghz_out, double* spread_out) {
  if (!c || !ghz_out) return SWRT_ERR_ARG;
  if (!c->clk) return fail(c, SWRT_ERR_STATE, "no clock stamps (swrt_clock_stamp 0 and 1 first)");
  GUARD_BEGIN_KEEP_CHAIN
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<uint64_t> h(2 * kClockWaves * 3);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->clk.get(), sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  hz_synced(c);
  // the pairing and median (swrt_clock.cpp, host-only, tested on synthetic stamps)
  const int rc = swrt_clock_ghz_stamps(h.data(), kClockWaves, kRealTimeHz, ghz_out, spread_out);
  if (rc == SWRT_ERR_STATE) return fail(c, rc, "no CU with both a start and an end stamp");
  if (rc) return fail(c, rc, "swrt_clock_ghz_stamps");
  return SWRT_OK;
  GUARD_END(c)
}

// ---------------------------------------------------------------------------
// QG PDE stepper (swrt_qg.hpp)
// ---------------------------------------------------------------------------
int swrt_qg_init(swrt_ctx* c, const swrt_qg_params* p, int64_t nx, const double* qk_in) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  if (!p || !qk_in) return fail(c, SWRT_ERR_ARG, "NULL argument");
  if (p->nlayers != 1 && p->nlayers != 2) return fail(c, SWRT_ERR_ARG, "nlayers must be 1 or 2");
  if (nx < 8 || nx > 4096 || !is_pow2(nx)) return fail(c, SWRT_ERR_ARG, "nx must be a power of two, 8..4096");
  if (!(p->L > 0)) return fail(c, SWRT_ERR_ARG, "L must be > 0");
  HIPCHK(c, hipSetDevice(c->device));
  QGState& q = c->qg;
  q = QGState{};  // (releases the previous state's buffers and events)
  const int n = (int)nx, kmax = n / 2 - 1;
  q.nhalf = (int64_t)(2 * kmax + 1) * (kmax + 1);
  q.nn = nx * nx;
  QGDev& g = q.g;
  g.n = n;
  g.nl = p->nlayers;
  g.kscale = 2.0 * 3.14159265358979323846 / p->L;
  if (p->nlayers == 1) g.kscale = 1.0;  // qgsw_raytrace.m:13-20: L = 2*pi, integer k
  g.dx = p->L / (double)n;
  g.K_d2 = p->K_d2;
  g.beta = p->beta;
  g.r_drag = p->r_drag;
  g.force_strength = p->force_strength;
  g.f = p->f;
  g.Cg = p->Cg;
  g.filter = p->filter;
  g.shear = p->nlayers == 2 ? p->shear : 0.0;
  g.nu = p->nu;
  g.hyper = p->hyper_order;
  g.r = p->r;
  const size_t hb = sizeof(double2) * q.nhalf * g.nl;
  for (DevBuf<double2>* b : {&q.qk, &q.qk_prev, &q.Qm1, &q.Qm2}) HIPCHK(c, b->alloc(q.nhalf * g.nl));
  HIPCHK(c, q.Z.alloc(q.nn * std::max(2 * g.nl, 3)));
  HIPCHK(c, q.T.alloc(q.nn * std::max(2 * g.nl, 3)));
  HIPCHK(c, q.dmax.alloc(1));
  HIPCHK(c, q.hmax.alloc(2));
  HIPCHK(c, q.ev.create());
  HIPCHK(c, q.ev_b.create());
  if (g.nl == 2) {
    HIPCHK(c, q.E1.alloc(4 * q.nhalf));
    HIPCHK(c, q.E2.alloc(4 * q.nhalf));
  }
  // host column-major (kx fastest) -> device ky-fastest, via qk_prev as staging
  HIPCHK(c, hipMemcpyAsync(q.qk_prev.get(), qk_in, hb, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(halfplane_relayout_kernel, dim3(nblocks(q.nhalf * g.nl, 256)), dim3(256), 0, c->stream,
                     q.qk_prev.get(), q.qk.get(), 2 * kmax + 1, kmax + 1, 1, g.nl);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemsetAsync(q.Qm1.get(), 0, hb, c->stream));
  HIPCHK(c, hipMemsetAsync(q.Qm2.get(), 0, hb, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  q.init = true;
  if (c->qg_sep) mark_slots_used(c, on_qg.saved);  // (the context stream's work so far)
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_qg_step(swrt_ctx* c, double dt, int64_t nsteps) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  QGState& q = c->qg;
  if (!q.init) return fail(c, SWRT_ERR_STATE, "swrt_qg_init not called");
  if (c->qg.spec) return fail(c, SWRT_ERR_STATE, "a speculative QG step is pending (swrt_qg_resolve first)");
  if (!(dt > 0) || nsteps < 0) return fail(c, SWRT_ERR_ARG, "dt must be > 0, nsteps >= 0");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  const int n = q.g.n, nl = q.g.nl;
  if ((rc = ensure_twiddles(c, n))) return rc;
  for (int64_t s = 0; s < nsteps; ++s) {
    if (nl == 2 && dt != q.exp_dt) {
      hipLaunchKernelGGL(qg2_exp_kernel, dim3(nblocks(q.nhalf, 256)), dim3(256), 0, c->stream, q.g, dt, q.E1.get(),
                         q.E2.get());
      HIPCHK(c, hipGetLastError());
      q.exp_dt = dt;
    }
    const int abstep = q.steps == 0 ? 1 : (q.steps == 1 ? 2 : 3);
    if (c->qg_fused) {
      if ((rc = qg_post(c))) return rc;
      if (q.Fj_rows) {
        // the tendency over Qm2 (read first by the same lane), then renamed:
        // Qm2 <- Qm1, Qm1 <- Qn
        if ((rc = qg_update_cols_launch(c, dt, abstep, q.Fj, q.qk_prev.get(), q.Qm2.get()))) return rc;
        std::swap(q.Qm1, q.Qm2);
      } else {
        rc = qg_update_launch(c, dt, abstep, q.Fj, q.qk_prev.get(), q.Qm1.get(), q.Qm2.get());
      }
    } else {
      rc = qg_step_launches(c, dt, abstep);
    }
    if (rc) return rc;
    q.post_valid = false;
    q.post_inv_valid = false;
    std::swap(q.qk, q.qk_prev);
    q.steps += 1;
    q.t = q.t + dt;
    q.has_prev = true;
  }
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_qg_step_speculative(swrt_ctx* c, double dt) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  QGState& q = c->qg;
  if (!q.init) return fail(c, SWRT_ERR_STATE, "swrt_qg_init not called");
  if (q.spec) return fail(c, SWRT_ERR_STATE, "a speculative QG step is already pending");
  if (!c->qg_fused) return fail(c, SWRT_ERR_STATE, "speculative steps need the fused post-step transforms");
  if (!(dt > 0)) return fail(c, SWRT_ERR_ARG, "dt must be > 0");
  if (q.g.nl == 2 && dt != q.exp_dt)
    return fail(c, SWRT_ERR_STATE, "a speculative step takes the dt of the exponential propagators in place");
  if (q.sp_count >= 2) return fail(c, SWRT_ERR_STATE, "two CFL read-backs already pending");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_twiddles(c, q.g.n))) return rc;
  for (DevBuf<double2>* b : {&q.qk_spare, &q.Qm1_spare, &q.Qm2_spare})
    if (!*b) HIPCHK(c, b->alloc((size_t)q.g.nl * (size_t)q.nhalf));
  const int abstep = q.steps == 0 ? 1 : (q.steps == 1 ? 2 : 3);
  if ((rc = qg_post(c))) return rc;  // of the committed qk (valid when the caller read its speed)
  q.spec_rot = q.Fj_rows;
  if (q.spec_rot)  // the tendency only; the committed Qm1 becomes Qm2 on acceptance
    rc = qg_update_cols_launch(c, dt, abstep, q.Fj, q.qk_spare.get(), q.Qm1_spare.get());
  else
    rc = qg_update_launch(c, dt, abstep, q.Fj, q.qk_spare.get(), q.Qm1_spare.get(), q.Qm2_spare.get());
  if (rc) return rc;
  // the post-step transforms and CFL read-back of the speculative qk
  std::swap(q.qk, q.qk_spare);  // (the spare as the current qk for the launches below only)
  const int rb_slot = q.sp_head;
  rc = qg_speed_launch(c);
  std::swap(q.qk, q.qk_spare);
  if (rc) return rc;
  q.spec_rb = true;
  q.spec_rb_slot = rb_slot;
  q.spec = true;
  q.spec_dt = dt;
  q.spec_steps = q.steps + 1;
  q.spec_t = q.t + dt;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_qg_resolve(swrt_ctx* c, int accept) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  QGState& q = c->qg;
  if (!q.spec) return fail(c, SWRT_ERR_STATE, "no speculative QG step pending");
  if (accept) {
    // the committed qk becomes the previous one, the speculative one current
    std::swap(q.qk_prev, q.qk);   // (prev, qk, spare) <- (qk, spare, prev)
    std::swap(q.qk, q.qk_spare);
    if (q.spec_rot) {
      // Qm2 <- the committed Qm1, Qm1 <- the speculative tendency; the old
      // Qm2 is the next spare
      std::swap(q.Qm2, q.Qm1);        // (Qm2, Qm1, spare) <- (Qm1, spare, Qm2)
      std::swap(q.Qm1, q.Qm1_spare);
    } else {
      std::swap(q.Qm1, q.Qm1_spare);
      std::swap(q.Qm2, q.Qm2_spare);
    }
    q.steps = q.spec_steps;
    q.t = q.spec_t;
    q.has_prev = true;
  } else {
    // its CFL read-back (the newest pending) is dropped unless the caller
    // already popped it; PZ/PT hold its post-step transforms, so the
    // committed qk's are recomputed on use
    if (q.spec_rb) {
      q.sp_head ^= 1;
      q.sp_count -= 1;
    }
  }
  q.spec = false;
  q.spec_rb = false;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_qg_max_speed(swrt_ctx* c, double* U0_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  QGState& q = c->qg;
  if (!q.init) return fail(c, SWRT_ERR_STATE, "swrt_qg_init not called");
  if (!U0_out) return fail(c, SWRT_ERR_ARG, "NULL output");
  if (c->qg.spec) return fail(c, SWRT_ERR_STATE, "a speculative QG step is pending (swrt_qg_resolve first)");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = qg_speed_launch(c))) return rc;
  while (q.sp_count > 0)  // the last one popped is this call's (earlier pending ones are superseded)
    if ((rc = qg_speed_wait(c, U0_out))) return rc;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_qg_max_speed_async(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  if (!c->qg.init) return fail(c, SWRT_ERR_STATE, "swrt_qg_init not called");
  if (c->qg.spec) return fail(c, SWRT_ERR_STATE, "a speculative QG step is pending (swrt_qg_resolve first)");
  HIPCHK(c, hipSetDevice(c->device));
  return qg_speed_launch(c);
  GUARD_END(c)
}

int swrt_qg_max_speed_result(swrt_ctx* c, double* U0_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  if (c->qg.sp_count == 0) return fail(c, SWRT_ERR_STATE, "no swrt_qg_max_speed_async pending");
  if (!U0_out) return fail(c, SWRT_ERR_ARG, "NULL output");
  return qg_speed_wait(c, U0_out);
  GUARD_END(c)
}

int swrt_qg_get(swrt_ctx* c, double* qk_out, double* t_out, int64_t* steps_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  QGState& q = c->qg;
  if (!q.init) return fail(c, SWRT_ERR_STATE, "swrt_qg_init not called");
  HIPCHK(c, hipSetDevice(c->device));
  if (qk_out) {
    const int kmax = q.g.n / 2 - 1;
    double2* tmp = q.Z.get();  // relayout to the host's kx-fastest order
    hipLaunchKernelGGL(halfplane_relayout_kernel, dim3(nblocks(q.nhalf * q.g.nl, 256)), dim3(256), 0, c->stream,
                       q.qk.get(), tmp, 2 * kmax + 1, kmax + 1, 0, q.g.nl);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(qk_out, tmp, sizeof(double2) * q.nhalf * q.g.nl, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (t_out) *t_out = q.t;
  if (steps_out) *steps_out = q.steps;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_qg_get_q(swrt_ctx* c, double* q_out) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  QGState& q = c->qg;
  if (!q.init) return fail(c, SWRT_ERR_STATE, "swrt_qg_init not called");
  if (!q_out) return fail(c, SWRT_ERR_ARG, "NULL output");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  const int n = q.g.n, nl = q.g.nl;
  if ((rc = ensure_twiddles(c, n))) return rc;
  for (int l = 0; l < nl; ++l) {
    hipLaunchKernelGGL(fulspec_kernel, dim3(nblocks(q.nn, 256)), dim3(256), 0, c->stream, q.qk.get() + l * q.nhalf, n,
                       q.Z.get() + l * q.nn, n / 2, 1);
    HIPCHK(c, hipGetLastError());
  }
  if ((rc = inverse_2d(c, q.Z.get(), q.T.get(), n, nl))) return rc;
  double* planes = reinterpret_cast<double*>(q.Z.get());
  hipLaunchKernelGGL(real_part_kernel, dim3(nblocks(q.nn * nl, 256)), dim3(256), 0, c->stream, q.T.get(), planes,
                     q.nn * nl);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(q_out, planes, sizeof(double) * q.nn * nl, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_qg_snapshot(swrt_ctx* c, int slot, int which, int layer, int64_t ny_period) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  return qg_snapshot_impl(c, slot, which, layer, ny_period, false);
  GUARD_END(c)
}

int swrt_qg_snapshot_speculative(swrt_ctx* c, int slot, int64_t ny_period) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  return qg_snapshot_impl(c, slot, 0, 0, ny_period, true);
  GUARD_END(c)
}

// ---------------------------------------------------------------------------
// Owner-driver hand-off: one rank steps the PDE, the others build their
// snapshots from the top layer's spectral PV it sends (qg2layersw_raytrace.m
// :186-188 reads layer 1 only)
// ---------------------------------------------------------------------------

int swrt_qg_export(swrt_ctx* c, int which, int layer, double* dst, int dst_mode, void* stream, double tail) {
  if (!c) return SWRT_ERR_ARG;
  GUARD_BEGIN_KEEP_CHAIN
  OnQGStream on_qg(c);
  QGState& q = c->qg;
  if (!q.init) return fail(c, SWRT_ERR_STATE, "swrt_qg_init not called");
  // (a pending speculative step writes the spare buffers only: the committed
  // qk and prev_qk stay as they are until swrt_qg_resolve)
  if (!dst) return fail(c, SWRT_ERR_ARG, "dst is NULL");
  if (which != 0 && which != 1) return fail(c, SWRT_ERR_ARG, "which must be 0 (current) or 1 (previous)");
  if (which == 1 && !q.has_prev) return fail(c, SWRT_ERR_STATE, "no previous qk before the first step");
  if (layer < 0 || layer >= q.g.nl) return fail(c, SWRT_ERR_ARG, "layer out of range");
  HIPCHK(c, hipSetDevice(c->device));
  const double2* src = (which == 0 ? q.qk.get() : q.qk_prev.get()) + layer * q.nhalf;
  const size_t bytes = sizeof(double2) * q.nhalf;
  if (dst_mode != 0 && dst_mode != 1 && dst_mode != 2) return fail(c, SWRT_ERR_ARG, "dst_mode must be 0, 1 or 2");
  if (dst_mode) {
    const hipStream_t ext = stream ? (hipStream_t)stream : on_qg.saved;
    if (dst_mode == 1) HIPCHK_RC(stream_order(c, ext, c->stream, 0));  // the caller's last read of dst
    hipLaunchKernelGGL(export_half_kernel, dim3(nblocks(q.nhalf + 1, 256)), dim3(256), 0, c->stream, src, dst,
                       q.nhalf, tail);
    HIPCHK(c, hipGetLastError());
    HIPCHK_RC(stream_order(c, c->stream, ext, 1));  // the caller's next use of dst
  } else {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    dst[2 * q.nhalf] = tail;
  }
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_snapshot_qk(swrt_ctx* c, int slot, const double* qk, int src_on_device, void* stream, int64_t nx,
                     double L, double K_d2, double shear, double k_scale, int64_t ny_period) {
  int rc = check_slot_args(c, slot, nx);
  if (rc) return rc;
  GUARD_BEGIN_KEEP_CHAIN
  if (!qk) return fail(c, SWRT_ERR_ARG, "qk is NULL");
  if (!is_pow2(nx)) return fail(c, SWRT_ERR_ARG, "nx must be a power of two for the GPU FFT");
  if (!(L > 0)) return fail(c, SWRT_ERR_ARG, "L must be > 0");
  if (ny_period == 0) ny_period = nx;
  if (ny_period % nx) return fail(c, SWRT_ERR_ARG, "ny_period must be a multiple of nx");
  if (c->qg.init && c->qg.g.n != nx) return fail(c, SWRT_ERR_ARG, "nx differs from the QG state's");
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t pk = c->stream;  // the packet stream
  if (!c->xq.init && !c->qg.init && c->qg_sep) mark_slots_used(c, pk);  // (as swrt_qg_init)
  c->xq.init = true;
  OnQGStream on_qg(c);
  const int n = (int)nx, kmax = n / 2 - 1;
  const int64_t nn = nx * nx, nhalf = (int64_t)(2 * kmax + 1) * (kmax + 1);
  if (c->xq.nx != nx) {
    HIPCHK(c, hipStreamSynchronize(c->stream));  // a queued snapshot may still use them
    c->xq.nx = 0;
    HIPCHK(c, c->xq.Z.alloc(3 * nn));
    HIPCHK(c, c->xq.T.alloc(3 * nn));
    HIPCHK(c, c->xq.fk.alloc(nhalf));
    c->xq.nx = nx;
  }
  if ((rc = ensure_twiddles(c, n))) return rc;
  if ((rc = qg_slot_acquire(c, slot))) return rc;
  if ((rc = ensure_slot(c, slot, nx))) return rc;
  const hipStream_t ext = stream ? (hipStream_t)stream : pk;
  const double2* fk = (const double2*)qk;
  if (src_on_device) {
    HIPCHK_RC(stream_order(c, ext, c->stream, 0));  // the caller's fill of qk (e.g. a broadcast)
  } else {
    HIPCHK(c, hipMemcpyAsync(c->xq.fk.get(), qk, sizeof(double2) * nhalf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's host buffer is free on return
    fk = c->xq.fk.get();
  }
  // grid_U of the half plane in the QG state's order (ky fastest): the
  // unfused path of swrt_qg_snapshot, bit for bit
  if ((rc = fields_from_halfplane(c, slot, fk, n, 1, K_d2, k_scale, shear, 0, c->xq.Z.get(), c->xq.T.get(), n / 2, 1)))
    return rc;
  if (src_on_device) HIPCHK_RC(stream_order(c, c->stream, ext, 1));  // qk read: the caller may refill it
  Slot& s = c->slot[slot];
  s.L = L;
  s.ny_period = ny_period;
  return qg_slot_written(c, slot);
  GUARD_END(c)
}

int swrt_swap_slots(swrt_ctx* c, int a, int b) {
  if (!c) return SWRT_ERR_ARG;
  if (a < 0 || a >= SWRT_MAX_SLOTS || b < 0 || b >= SWRT_MAX_SLOTS) return fail(c, SWRT_ERR_ARG, "slot out of range");
  std::swap(c->slot[a], c->slot[b]);
  return SWRT_OK;
}

// ---------------------------------------------------------------------------
// ode23 device stages (swrt_ode23.hpp)
// ---------------------------------------------------------------------------

int swrt_ode23_f1(swrt_ctx* c, double t, double tmax, double f, double Cg, int nslots, double thr, double bump,
                  double* rh_raw_out) {
  if (!c) return SWRT_ERR_ARG;
  HIPCHK_RC(tangent_refuse(c, "swrt_ode23_f1"));
  GUARD_BEGIN
  HIPCHK_RC(lost_check(c));
  SlotUse slot_use(c, false, kSlots01);
  int rc;
  if ((rc = ode23_f1_queue(c, t, tmax, f, Cg, nslots, thr, bump))) return rc;
  return read_max(c, rh_raw_out);
  GUARD_END(c)
}

int swrt_ode23_attempt(swrt_ctx* c, double t, double h, double tnew, double tmax, double f, double Cg,
                       int nslots, double thr, double bump, double* err_raw_out) {
  if (!c) return SWRT_ERR_ARG;
  HIPCHK_RC(tangent_refuse(c, "swrt_ode23_attempt"));
  GUARD_BEGIN
  HIPCHK_RC(lost_check(c));
  SlotUse slot_use(c, false, kSlots01);
  HIPCHK(c, hipSetDevice(c->device));
  // (swrt_ode23_set_dense: the tile kernel also stores F2 and F3)
  return ode23_attempt(c, t, h, tnew, tmax, f, Cg, nslots, thr, bump, c->o23.dense, err_raw_out);
  GUARD_END(c)
}

int swrt_ode23_accept(swrt_ctx* c) {
  if (!c) return SWRT_ERR_ARG;
  HIPCHK_RC(tangent_refuse(c, "swrt_ode23_accept"));
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (c->in_hook) return fail(c, SWRT_ERR_STATE, "this call may touch the packets: not allowed inside an ode23 hook");
  HIPCHK_RC(lost_check(c));
  HIPCHK_RC(chain_drop(c));
  if (!c->o23.ynx) return fail(c, SWRT_ERR_STATE, "no ode23 step attempted");
  ode23_accept_sets(c);
  return SWRT_OK;
}

int swrt_ode23_set_dense(swrt_ctx* c, int on) {
  if (!c) return SWRT_ERR_ARG;
  c->s0_dirty = true;  // (conservative: settings and syncs may precede packet-stream work)
  if (on != 0 && on != 1) return fail(c, SWRT_ERR_ARG, "dense must be 0 or 1");
  c->o23.dense = on != 0;
  c->o23.dense_ready = false;
  return SWRT_OK;
}

int swrt_ode23_ntrp(swrt_ctx* c, double t, double tnew, const double* tout, int64_t nout) {
  if (!c) return SWRT_ERR_ARG;
  HIPCHK_RC(tangent_refuse(c, "swrt_ode23_ntrp"));
  HOOK_REFUSE
  // (reads the packets and the stage buffers only: whatever dropped the chain
  // since the attempt also ended the attempt's validity)
  GUARD_BEGIN_KEEP_CHAIN
  HIPCHK_RC(lost_check(c));
  if (nout < 0) return fail(c, SWRT_ERR_ARG, "nout < 0");
  if (nout > 0 && !tout) return fail(c, SWRT_ERR_ARG, "NULL buffer");
  if (!c->o23.dense_ready)
    return fail(c, SWRT_ERR_STATE,
                "ode23 ntrp: no dense attempt in the stage buffers (swrt_ode23_set_dense 1, then "
                "swrt_ode23_attempt; valid until swrt_ode23_accept or any other packet call)");
  const double tdir = std::copysign(1.0, tnew - t);
  if (!(tnew != t) || !std::isfinite(t) || !std::isfinite(tnew)) return fail(c, SWRT_ERR_ARG, "ode23 ntrp: empty step");
  for (int64_t i = 0; i < nout; ++i)
    if (!(tdir * (tout[i] - t) >= 0 && tdir * (tnew - tout[i]) >= 0))
      return fail(c, SWRT_ERR_ARG, "ode23 ntrp: an output time lies outside the step");
  if (nout == 0) return SWRT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK_RC(ensure_history(c, nout));
  return ode23_ntrp_queue(c, t, tnew, tout, nout);
  GUARD_END(c)
}

int swrt_ode23_run_at(swrt_ctx* c, const double* tspan, int64_t nt, double tmax, double f, double Cg, int nslots,
                      double rtol, double atol, double bump, double* ts_out, int64_t ts_cap, int64_t* nts_out,
                      int64_t* stats3_out) {
  if (!c) return SWRT_ERR_ARG;
  HIPCHK_RC(tangent_refuse(c, "swrt_ode23_run_at"));
  if (!tspan) return fail(c, SWRT_ERR_ARG, "tspan is NULL");
  if (nt < 2) return fail(c, SWRT_ERR_ARG, "tspan needs at least two times");
  if (!ts_out || ts_cap < 1 || !nts_out) return fail(c, SWRT_ERR_ARG, "ts_out / ts_cap / nts_out");
  for (int64_t i = 0; i < nt; ++i)
    if (!std::isfinite(tspan[i])) return fail(c, SWRT_ERR_ARG, "tspan must be finite");
  {
    const double tdir = std::copysign(1.0, tspan[nt - 1] - tspan[0]);
    for (int64_t i = 1; i < nt; ++i)
      if (!(tdir * (tspan[i] - tspan[i - 1]) > 0))
        return fail(c, SWRT_ERR_ARG, "tspan must be strictly increasing or strictly decreasing");
  }
  GUARD_BEGIN
  HIPCHK_RC(lost_check(c));
  SlotUse slot_use(c, false, kSlots01);
  O23Stats st;
  int64_t nts = 0;
  const int rc = ode23_run_at(c, tspan, nt, tmax, f, Cg, nslots, rtol, atol, bump, ts_out, ts_cap, &nts, &st);
  if (rc == kO23BelowHmin) return fail(c, SWRT_ERR_STATE, "ode23: step size below hmin");
  if (rc) return rc;
  *nts_out = nts;
  if (stats3_out) {
    stats3_out[0] = st.steps;
    stats3_out[1] = st.failed;
    stats3_out[2] = st.attempts;
  }
  c->o23.last = st;
  return SWRT_OK;
  GUARD_END(c)
}

int swrt_ode23_chain_next(swrt_ctx* c, int slot_a, int slot_b) {
  if (!c) return SWRT_ERR_ARG;
  if (slot_a < 0 || slot_a >= SWRT_MAX_SLOTS || slot_b < 0 || slot_b >= SWRT_MAX_SLOTS || slot_a == slot_b)
    return fail(c, SWRT_ERR_ARG, "chain slots out of range or equal");
  c->o23.chain.want = true;
  c->o23.chain.sa = slot_a;
  c->o23.chain.sb = slot_b;
  return SWRT_OK;
}

int swrt_ode23_run(swrt_ctx* c, double t0, double tfinal, double tmax, double f, double Cg, int nslots,
                   double rtol, double atol, double bump, double* ts_out, int64_t ts_cap, int64_t* nts_out,
                   int64_t* stats3_out) {
  return swrt_ode23_run_hooked(c, t0, tfinal, tmax, f, Cg, nslots, rtol, atol, bump, ts_out, ts_cap, nts_out,
                               stats3_out, nullptr, nullptr);
}

int swrt_ode23_run_hooked(swrt_ctx* c, double t0, double tfinal, double tmax, double f, double Cg, int nslots,
                          double rtol, double atol, double bump, double* ts_out, int64_t ts_cap, int64_t* nts_out,
                          int64_t* stats3_out, void (*hook)(void*), void* hook_user) {
  return swrt_ode23_run_sharded(c, t0, tfinal, tmax, f, Cg, nslots, rtol, atol, bump, ts_out, ts_cap, nts_out,
                                stats3_out, hook, hook_user, nullptr, nullptr);
}

int swrt_ode23_run_sharded(swrt_ctx* c, double t0, double tfinal, double tmax, double f, double Cg, int nslots,
                           double rtol, double atol, double bump, double* ts_out, int64_t ts_cap, int64_t* nts_out,
                           int64_t* stats3_out, void (*hook)(void*), void* hook_user,
                           int (*reduce)(double*, void*), void* reduce_user) {
  if (!c) return SWRT_ERR_ARG;
  HIPCHK_RC(tangent_refuse(c, "swrt_ode23_run_sharded"));
  if (!ts_out || ts_cap < 1 || !nts_out) return fail(c, SWRT_ERR_ARG, "ts_out / ts_cap / nts_out");
  if (c->in_hook) return fail(c, SWRT_ERR_STATE, "an ode23 hook may not start another ode23 call");
  GUARD_BEGIN_KEEP_CHAIN
  HIPCHK_RC(lost_check(c));
  SlotUse slot_use(c, false, kSlots01);
  const double rtol_c = std::max(rtol, 100 * 2.220446049250313e-16);
  const double thr = atol / rtol_c;
  const double htspan = std::fabs(tfinal - t0);
  const double hmax = 0.1 * htspan;
  const double c0 = 0.8 * std::pow(rtol_c, 1.0 / 3.0);
  int rc;
  // stage 1 (with this call's re-binning and in-tile sort), its max in slot
  // sl_f1: queued by the previous call when it was chained to this one
  int sl_f1;
  // the chained first attempt is a candidate if this call asks for the first
  // attempt it assumed; anything else joins its part 1 before touching the packets
  Ode23State::O23Chain& ch = c->o23.chain;
  const bool first_cand = ch.first_q && same_bits(t0, 0.0) && same_bits(tfinal, ch.tfinal) &&
                          same_bits(tmax, ch.tmax) && same_bits(rtol, ch.rtol);
  ch.first_q = false;
  const bool taken = ode23_chain_take(c, t0, tmax, f, Cg, nslots, thr, bump);
  if (!(taken && first_cand)) HIPCHK_RC(chain_join(c));
  if (taken) {
    sl_f1 = ch.dmax_slot;
    ++ch.taken;
  } else {
    if ((rc = ode23_f1_queue(c, t0, tmax, f, Cg, nslots, thr, bump))) return rc;
    sl_f1 = c->o23.dmax_cur;
    c->o23.dmax_cur = (sl_f1 + 1) % 3;
  }
  Ode23Args base;
  if ((rc = ode23_prepare(c, nslots, base, tmax, f, Cg, thr, bump))) return rc;
  // The first attempt's step size on the device (ode23_first_step_kernel,
  // the host's own operations), so the attempt is queued behind stage 1
  // without a host round trip; the controller then computes the same and
  // checks it against the kernel's mapped copy (the tile path only: its
  // attempt kernel reads device coefficients).
  // (not in a sharded run: the device would take the first step size from
  // this rank's stage-1 max, the controller takes it from every rank's)
  const bool dev_first = !reduce && tile_binned(c);
  // Two part launches per attempt when the binning allows.
  const bool split = ode23_split_ok(c);
  const bool first_chained = taken && first_cand && dev_first && split == ch.split;
  uint64_t ticket = 0;  // the first-step launch's (dev_first)
  if (first_chained) {
    ticket = ch.first_ticket;
    // queued by the previous call: stage 1, the first step (and stage 1's
    // event after it), the fork and the first attempt, whose part 1 is now
    // this call's pending split
    c->o23.chain_b = false;
    if (split) c->b_pending = 1;
    ++ch.first_taken;
  } else {
    HIPCHK_RC(chain_join(c));
    if (dev_first) {
      HIPCHK_RC(ode23_first_step_queue(c, sl_f1, c0, hmax, htspan, t0, tfinal, split, &ticket));
    } else {
      HIPCHK(c, hipMemcpyAsync(c->o23.hmax.get() + sl_f1, c->o23.dmax.get() + sl_f1, sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipEventRecord(c->o23.ev[sl_f1].get(), c->stream));
    }
    if (split) {
      // the fork is stage 1's own event (one marker in front of the first attempt, not two)
      HIPCHK(c, hipStreamWaitEvent(c->sx[0].get(), c->o23.ev[sl_f1].get(), 0));
      if (c->hz.on) {
        c->hz.record(c->o23.ev[sl_f1].get(), 0);
        c->hz.wait(1, c->o23.ev[sl_f1].get());
      }
      c->b_pending = 1;  // joined into the packet stream before anything else reads the packets (join_b)
    }
  }
  DeviceExec ex(c, base, split, dev_first, sl_f1, hook, hook_user, reduce, reduce_user);
  ex.expect_ticket(ticket);
  // the first attempt from the device's coefficients, queued now (or by the
  // previous call); the caller's hook then runs (host work that overlaps
  // stage 1 and this attempt)
  if (first_chained)
    ex.adopt_first(ch.first_slot, ch.first_wg);
  else if (dev_first && (rc = ex.queue_first()))
    return rc;
  O23Stats st;
  int64_t nts = 0;
  rc = ode23_control(ex, t0, tfinal, rtol, atol, ts_out, ts_cap, &nts, &st);
  if (rc == kO23BelowHmin) return fail(c, SWRT_ERR_STATE, "ode23: step size below hmin");
  if (rc) return rc;
  if ((rc = ode23_chain_queue(c, tmax, f, Cg, nslots, thr, bump, rtol, reduce == nullptr))) return rc;
  *nts_out = nts;
  if (stats3_out) {
    stats3_out[0] = st.steps;
    stats3_out[1] = st.failed;
    stats3_out[2] = st.attempts;
  }
  c->o23.last = st;
  c->o23.first_taken += st.first_taken;
  c->o23.guesses_taken += st.guesses_taken[0] + st.guesses_taken[1] + st.guesses_taken[2];
  c->o23.split_runs += split ? 1 : 0;
  return SWRT_OK;
  GUARD_END(c)
}

#ifdef SWRT_PHASE_TIMING
// diagnostic build only (not in include/swrt.h): copy out / clear the tile
// kernel's per-workgroup phase stamps (8 u64 per tile).
int swrt_debug_phases(unsigned long long* out, int ntiles, int clear) {
  if (hipDeviceSynchronize() != hipSuccess) return SWRT_ERR_HIP;
  const size_t bytes = (size_t)ntiles * 8 * sizeof(unsigned long long);
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(swrt::swrt_phase_dbg), bytes, 0, hipMemcpyDeviceToHost) != hipSuccess)
    return SWRT_ERR_HIP;
  if (clear) {
    static unsigned long long zeros[16384 * 8];
    if (hipMemcpyToSymbol(HIP_SYMBOL(swrt::swrt_phase_dbg), zeros, sizeof(zeros), 0,
                          hipMemcpyHostToDevice) != hipSuccess)
      return SWRT_ERR_HIP;
  }
  return SWRT_OK;
}
#endif

}  // extern "C"
