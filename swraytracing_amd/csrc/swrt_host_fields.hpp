// swrt_host_fields.hpp — host side of the background fields: the context's
// scratch, twiddle and slot buffers, the FFT and 2-D transform launches, and
// the half-plane -> node-record path shared by the field setters and the QG
// snapshots; the wave-action (xka) node array.
#pragma once
#include <vector>

#include "swrt_ctx.hpp"
#include "swrt_fft.hpp"
#include "swrt_kernels.hpp"
#include "swrt_xka.hpp"

namespace {

int ensure_scratch(swrt_ctx* c, size_t bytes) {
  if (c->scratch_bytes >= bytes) return SWRT_OK;
  c->scratch_bytes = 0;
  HIPCHK(c, c->scratch.alloc(bytes));
  c->scratch_bytes = bytes;
  return SWRT_OK;
}

int ensure_twiddles(swrt_ctx* c, int n) {
  if (c->tw_n == n) return SWRT_OK;
  if (c->tw) HIPCHK(c, hipDeviceSynchronize());  // the other stream may still read them
  std::vector<double2> h(n);  // k < n: the radix-4 stages read w^(3*p*s) < w^(3n/4)
  for (int k = 0; k < n; ++k) {
    // exp(-2*pi*i*k/n); long double for the argument reduction
    const long double th = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
    h[k] = make_double2((double)cosl(th), (double)sinl(th));
  }
  HIPCHK(c, c->tw.alloc(n));
  HIPCHK(c, hipMemcpyAsync(c->tw.get(), h.data(), sizeof(double2) * n, hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->tw_n = n;
  return SWRT_OK;
}

int ensure_slot(swrt_ctx* c, int slot, int64_t nx) {
  Slot& s = c->slot[slot];
  const int64_t npad = nx + kPadTot;
  if (s.nodes.get() && s.nx == nx) return SWRT_OK;
  if (s.nodes) HIPCHK(c, hipDeviceSynchronize());  // a queued launch on either stream may read it
  s.psi.reset();
  s.set = false;
  HIPCHK(c, s.nodes.alloc(kRec * npad * npad));
  s.nx = nx;
  s.npad = npad;
  return SWRT_OK;
}

int check_slot_args(swrt_ctx* c, int slot, int64_t nx) {
  if (!c) return SWRT_ERR_ARG;
  if (slot < 0 || slot >= SWRT_MAX_SLOTS) return fail(c, SWRT_ERR_ARG, "slot out of range");
  if (nx < 8 || nx > 4096 || (nx & 1)) return fail(c, SWRT_ERR_ARG, "nx must be even, 8..4096");
  return SWRT_OK;
}

FieldView view_of(const Slot& s) {
  FieldView v;
  v.nodes = s.nodes.get();
  v.nx = (int)s.nx;
  v.npad = (int)s.npad;
  v.dx = s.L / (double)s.nx;
  v.px = (double)s.nx;
  v.py = (double)s.ny_period;
  v.inv_px = 1.0 / v.px;
  v.inv_py = 1.0 / v.py;
  v.ipx = (int)s.nx;
  v.ipy = (int)s.ny_period;
  v.inv_dx = 1.0 / v.dx;
  const auto pow2 = [](int p) { return p > 0 && (p & (p - 1)) == 0; };
  v.inv_exact = pow2(v.ipx) && pow2(v.ipy);
  v.ywrap1 = v.ipy == v.nx;
  return v;
}

// Pack 6 device planes (already in scratch) into the slot's node array.
int pack_slot(swrt_ctx* c, int slot, const double* dplanes, double shear) {
  Slot& s = c->slot[slot];
  const int64_t tot = s.npad * s.npad;
  hipLaunchKernelGGL(pack_nodes_kernel, dim3(nblocks(tot, 256)), dim3(256), 0, c->stream, dplanes,
                     (int)s.nx, (int)s.npad, shear, s.nodes.get());
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}

// FFT kernel variant (swrt_fft.hpp): radix 4 in one LDS buffer with n/4
// lanes for n <= 1024, else radix 4 ping-pong with 128 lanes.  At 512^2 x 2
// layers (8-vector inverse + 1-vector forward 2-D transforms per step) the
// one-buffer form takes the PDE step from 0.078 (radix 2, 256 lanes) / 0.077
// (radix 4 ping-pong) to 0.073 ms (profiles/r02_v21_fft_mode_ab.log).
// Vectors per workgroup of the one-buffer form (rows per workgroup of the
// Jacobian pass): two when the transforms run alone (the PDE step 0.080 vs
// 0.081 ms with four and 0.083 with one), one while packet launches run
// beside them on their own stream (driver step 0.288 vs 0.293 ms with two and
// 0.295 with four: small workgroups fit the slots packet workgroups free,
// profiles/r03_v4_qg/README.md).  Batches that do not divide fall back to one.
int fft_group(const swrt_ctx* c, int n, int nvec, bool tin) {
  const int C = (c->qg_sep && c->n > 0) ? 1 : 2;
  if (C * (n / 4) > 1024 || nvec % (tin ? 8 * C : C) != 0) return 1;
  return C;
}

template <bool TIN>
void launch_fft(swrt_ctx* c, const double2* in, double2* out, int n, int logn, int nvec, int inverse) {
  if (n <= 1024) {
    const int C = fft_group(c, n, nvec, TIN);
    hipLaunchKernelGGL((fft_vec_kernel<TIN, 2>), dim3((unsigned)(nvec / C)), dim3(C * n / 4),
                       sizeof(double2) * C * (n + 1), c->stream, in, out, n, logn, c->tw.get(), inverse, nvec);
  } else
    hipLaunchKernelGGL((fft_vec_kernel<TIN, 1>), dim3((unsigned)nvec), dim3(128), sizeof(double2) * 2 * n, c->stream,
                       in, out, n, logn, c->tw.get(), inverse, nvec);
}

int run_fft_pass(swrt_ctx* c, double2* Z, int n, int nb, int inverse) {
  const int logn = ilog2(n);
  const int64_t nvec = (int64_t)n * nb;
  launch_fft<false>(c, Z, Z, n, logn, (int)nvec, inverse);
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}

int run_transpose(swrt_ctx* c, const double2* in, double2* out, int n, int nb) {
  dim3 grid((n + 31) / 32, (n + 31) / 32, nb);
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(32, 8), 0, c->stream, in, out, n);
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}

// 2-D transform of nb n x n blocks: a pass along the contiguous index of Z (in
// place), then a pass along the other index reading Z's columns and writing
// `out` transposed ([r + n*c] for Z in [c + n*r]).  Z keeps the first pass.
int transform_2d(swrt_ctx* c, double2* Z, double2* out, int n, int nb, int inverse) {
  int rc;
  if ((rc = run_fft_pass(c, Z, n, nb, inverse))) return rc;
  const int64_t nvec = (int64_t)n * nb;
  if (nvec % 8) {  // tiny grids: the XCD mapping needs 8 | nvec
    if ((rc = run_transpose(c, Z, out, n, nb))) return rc;
    return run_fft_pass(c, out, n, nb, inverse);
  }
  const int logn = ilog2(n);
  launch_fft<true>(c, Z, out, n, logn, (int)nvec, inverse);
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}

// Inverse 2-D transform of nb spectra in layout [c + n*r] (ky contiguous);
// result in layout [r + n*c] (x contiguous) in `out`.
int inverse_2d(swrt_ctx* c, double2* Z, double2* out, int n, int nb) { return transform_2d(c, Z, out, n, nb, 1); }

// Shared tail of set_field_psi / set_field_qk / swrt_qg_snapshot: fk half
// plane in device memory, read at fk[(kx + kmax)*sx + ky*sy].
int fields_from_halfplane(swrt_ctx* c, int slot, const double2* dfk, int n, int mode, double K_d2,
                          double kscale, double shear, int with_psi, double2* Z, double2* T, int sx, int sy) {
  int rc;
  const int64_t nn = (int64_t)n * n;
  const int nb = with_psi ? 4 : 3;
  Slot& s0 = c->slot[slot];
  if (!with_psi && n % 16 == 0 && 3 * 2 * n / 4 <= 1024 && (n / 2) % 8 == 0) {
    // the spectra built by the row pass (spectra_rows_kernel), the column
    // pass fused with the pack into the node records (fft_cols_pack_kernel):
    // two launches, the values of the four below
    const int logn = ilog2(n);
    hipLaunchKernelGGL(spectra_rows_kernel, dim3((unsigned)n), dim3(3 * n / 4), sizeof(double2) * 3 * n, c->stream,
                       dfk, n, mode, K_d2, kscale, 0, sx, sy, logn, (const double2*)c->tw.get(), Z);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(fft_cols_pack_kernel<2>, dim3((unsigned)(n / 2)), dim3(3 * 2 * n / 4),
                       sizeof(double2) * 3 * 2 * (n + 1), c->stream, (const double2*)Z, n, logn,
                       (const double2*)c->tw.get(), (int)s0.npad, shear, s0.nodes.get());
    HIPCHK(c, hipGetLastError());
    s0.has_psi = false;
    s0.div_free = true;  // v_y = -u_x, as pack_pairs_kernel
    return SWRT_OK;
  }
  if (nb * n / 4 <= 1024 && ((int64_t)n * nb) % 8 == 0) {
    // the spectra built row by row in LDS by the first inverse pass
    // (spectra_rows_kernel: the same values as the separate launches below,
    // one 12.6 MB round trip less at 512^2), then the column pass
    const int logn = ilog2(n);
    hipLaunchKernelGGL(spectra_rows_kernel, dim3((unsigned)n), dim3(nb * n / 4), sizeof(double2) * nb * n, c->stream,
                       dfk, n, mode, K_d2, kscale, with_psi, sx, sy, logn, (const double2*)c->tw.get(), Z);
    HIPCHK(c, hipGetLastError());
    launch_fft<true>(c, Z, T, n, logn, n * nb, 1);
    HIPCHK(c, hipGetLastError());
  } else {
    hipLaunchKernelGGL(spectra_kernel, dim3(nblocks(nn, 256)), dim3(256), 0, c->stream, dfk, n, mode,
                       K_d2, kscale, with_psi, Z, sx, sy);
    HIPCHK(c, hipGetLastError());
    if ((rc = inverse_2d(c, Z, T, n, nb))) return rc;
  }
  // T now holds the packed fields in [x + n*y]
  Slot& s = c->slot[slot];
  if (with_psi && !s.psi) HIPCHK(c, s.psi.alloc(nn));
  if (n % 16 == 0) {
    hipLaunchKernelGGL(pack_pairs_kernel, dim3(n / 16, n / 16), dim3(256), 0, c->stream, T, n, (int)s.npad, shear,
                       s.nodes.get());
    HIPCHK(c, hipGetLastError());
    if (with_psi) {
      hipLaunchKernelGGL(psi_plane_kernel, dim3(nblocks(nn, 256)), dim3(256), 0, c->stream, T + 3 * nn, s.psi.get(),
                         nn);
      HIPCHK(c, hipGetLastError());
    }
  } else {  // tiny grids: unpair into planes (reuse Z), then pack
    double* planes = reinterpret_cast<double*>(Z);
    hipLaunchKernelGGL(unpair_kernel, dim3(nblocks(nn, 256)), dim3(256), 0, c->stream, T, n, with_psi,
                       planes, with_psi ? s.psi.get() : nullptr);
    HIPCHK(c, hipGetLastError());
    if ((rc = pack_slot(c, slot, planes, shear))) return rc;
  }
  s.has_psi = with_psi != 0;
  s.div_free = true;  // pack_pairs_kernel / unpair_kernel write v_y = -u_x
  return SWRT_OK;
}

// the context scratch carved for a field transform: Z | T (zb bytes each) | fk (nhalf complex) | raw (a real plane)
struct FftScratch {
  double2 *Z, *T, *fk;
  double* raw;
};
FftScratch fft_scratch(swrt_ctx* c, size_t zb, int64_t nhalf) {
  char* base = c->scratch.get();
  return {(double2*)base, (double2*)(base + zb), (double2*)(base + 2 * zb),
          (double*)(base + 2 * zb + sizeof(double2) * nhalf)};
}

// g2k on the device (g2k.m:8-9): forward FFT2 of the real n x n grid `raw`
// (layout [r + n*c], r = x index) along x, then y (T: [c + n*r]), cropped to
// the half plane fk
int g2k_launches(swrt_ctx* c, const double* raw, double2* Z, double2* T, double2* fk, int n) {
  const int64_t nn = (int64_t)n * n, nhalf = (int64_t)(n - 1) * (n / 2);
  hipLaunchKernelGGL(real_to_complex_kernel, dim3(nblocks(nn, 256)), dim3(256), 0, c->stream, raw, Z, nn);
  HIPCHK(c, hipGetLastError());
  if (int rc = transform_2d(c, Z, T, n, 1, 0)) return rc;
  hipLaunchKernelGGL(crop_half_kernel, dim3(nblocks(nhalf, 256)), dim3(256), 0, c->stream, T, n, fk);
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}

// a field setter's end: the slot's writes complete, its geometry and a new write generation
int slot_set_done(swrt_ctx* c, int slot, double L, int64_t ny_period) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  Slot& s = c->slot[slot];
  s.L = L;
  s.ny_period = ny_period;
  s.set = true;
  s.wgen = ++c->slot_wgen;
  return SWRT_OK;
}

// (Re)allocate the xka node array for an nx grid.
int xka_nodes_for(swrt_ctx* c, int64_t nx) {
  const int64_t npad = nx + kPadTot;
  if (c->xka.nx != nx) {
    c->xka.nx = 0;
    HIPCHK(c, c->xka.nodes.alloc(kXkaRec * npad * npad));
    c->xka.nx = nx;
  }
  return SWRT_OK;
}

// 7 device planes -> padded node records
int xka_pack(swrt_ctx* c, const double* dplanes, int64_t nx) {
  const int64_t npad = nx + kPadTot;
  hipLaunchKernelGGL(pack_xka_kernel, dim3(nblocks(npad * npad, 256)), dim3(256), 0, c->stream, dplanes, (int)nx,
                     (int)npad, c->xka.nodes.get());
  HIPCHK(c, hipGetLastError());
  return SWRT_OK;
}
}  // namespace
