// swrt_mex.cpp — MATLAB MEX gateway over the swrt C ABI (include/swrt.h).
//
// The reference-side binding a maintainer adds to ndefilippis/SWRaytracing so
// that SpectralScheme / ode_symplectic / interpolate_U / ode23 callers run on
// the MI355X.  Deliberately thin: argument marshalling only, every error is
// raised with mexErrMsgIdAndTxt AFTER the C call has returned (never from HIP
// code).
//
// Contexts are handles: h = swrt_mex('create', device) opens one library
// context (its own field slots, packets and streams) and every other command
// takes h as its second argument, so independent objects — two
// SpectralSchemeGPU instances, a scheme and a QG run — never share fields
// (each SpectralScheme owns its fields, SpectralScheme.m:28-35).
// Build (MATLAB R2018a+, interleaved complex):
//   mex -R2018a -I../include swrt_mex.cpp -L../swraytracing_amd -lswrt
// Usage (see SpectralSchemeGPU.m, ode_symplectic_gpu.m, ode23_packets_gpu.m):
//   h = swrt_mex('create', device);   swrt_mex('destroy', h)    % through SwrtContext (a handle class)
//   n = swrt_mex('live')                                        % open contexts
//   swrt_mex('set_field_psi', h, slot, psi_grid, L)           % SpectralScheme ctor
//   swrt_mex('set_field_qk', h, slot, qk, L, K_d2, shear, kscale, ny_period)   % grid_U
//   swrt_mex('set_field_grid', h, slot, u, v, ux, uy, vx, vy, L, ny_period)
//   swrt_mex('set_field_q', h, slot, q_grid, L, K_d2, shear, kscale, ny_period)   % grid_U(g2k(q)), read_field frame
//   swrt_mex('advance_intervals', h, dts, nsub, f, gH, alpha0, dalpha, bump)       % slots 0..numel(dts)
//   swrt_mex('set_locality', h, rebin_every, tile)
//   F6  = swrt_mex('get_fields', h, slot, nx)                 % nx x nx x 6: u v u_x u_y v_x v_y
//   psi = swrt_mex('get_psi', h, slot, nx)                    % k2g(g2k(psi)) of set_field_psi
//   out = swrt_mex('eval', h, x, y, nslots, alpha, bump)      % n x 6 (U, grad U per column)
//   FI  = swrt_mex('interpolate', h, x, y, F, dx, dy, bump)   % interpolate.m
//   [x, k, hx, hk] = swrt_mex('leapfrog', h, x0, k0, dt, nsteps, f, gH, nslots, alpha0, dalpha, bump, save_every)
//   fk = swrt_mex('g2k', h, fg);  fg = swrt_mex('k2g', h, fk);
//   swrt_mex('packets_set', h, x, k);  [x, k] = swrt_mex('packets_get', h);
//   swrt_mex('advance', h, dt, nsteps, f, gH, nslots, alpha0, dalpha, bump)
//   rh  = swrt_mex('ode23_f1', h, t, tmax, f, Cg, nslots, thr, bump)       % ode23_packets_gpu.m
//   err = swrt_mex('ode23_attempt', h, t, hstep, tnew, tmax, f, Cg, nslots, thr, bump)
//   swrt_mex('ode23_accept', h)
//   swrt_mex('ode23_set_dense', h, on)                        % ode23_attempt keeps F2, F3 (vector tspan)
//   swrt_mex('ode23_ntrp', h, t, tnew, tout)                  % history frames at tout inside the step
//   [hx, hk] = swrt_mex('history', h);  swrt_mex('history_reset', h)   % N x 2 x frames each
//   swrt_mex('qg_init', h, params_struct, qk)   % qk (2kmax+1) x (kmax+1) [x 2], complex
//   swrt_mex('qg_step', h, dt, nsteps);  U0 = swrt_mex('qg_max_speed', h);
//   [qk, t, steps] = swrt_mex('qg_get', h, nx, nlayers);  q = swrt_mex('qg_get_q', h, nx, nlayers);
//   swrt_mex('qg_snapshot', h, slot, which, layer, ny_period);  swrt_mex('swap_slots', h, a, b)
//   tf = swrt_mex('field_div_free', h, slot)   % v_y == -u_x exactly (five-sum kernels)
//   swrt_mex('omega_series_begin', h, f, Cg, edges)           % load_data.m:33-52,63 on the device
//   swrt_mex('omega_series_record', h);  swrt_mex('omega_series_record_history', h, first, count)
//   [counts, stats] = swrt_mex('omega_series_get', h)         % (nbins+2) x frames, 4 x frames
//   swrt_mex('omega_series_reset', h)
//   counts = swrt_mex('omega_ideal', h, slot, ring, omega0, edges)   % ideal_omega_distribution.m:3-11
//   swrt_mex('map_series_begin', h, L, m, f, Cg[, frac_bits])  % packet density / wave-energy maps on the device
//   swrt_mex('map_series_record', h);  swrt_mex('map_series_record_history', h, first, count)
//   [planes, stats] = swrt_mex('map_series_get', h)           % m x m x 4 x frames, 2 x frames
//   swrt_mex('map_series_reset', h)
//   swrt_mex('kmap_series_begin', h, K, m[, frac_bits])       % (k, l)-plane counts and wavevector moments on the device
//   swrt_mex('kmap_series_record', h);  swrt_mex('kmap_series_record_history', h, first, count)
//   n = swrt_mex('kmap_series_frames', h)
//   [planes, stats] = swrt_mex('kmap_series_get', h)          % int64 m x m x frames, int64 8 x frames
//   swrt_mex('kmap_series_reset', h)
//   swrt_mex('cond_series_begin', h, f, Cg, omega_edges, which, q_edges[, frac_bits])   % omega classes by zeta/sigma/D classes
//   swrt_mex('cond_series_record', h, nslots, alpha, bump)
//   swrt_mex('cond_series_record_history', h, first, count, nslots, alphas, bump)   % alphas [] when nslots < 2
//   n = swrt_mex('cond_series_frames', h)
//   [counts, sums, stats] = swrt_mex('cond_series_get', h)    % int64 (nw+2) x (nq+2) x frames, (nq+2) x frames, 2 x frames
//   swrt_mex('cond_series_reset', h)
//   swrt_mex('trans_series_begin', h, f, Cg, omega_edges, src_edges[, frac_bits])   % omega classes by a per-packet source value's classes
//   swrt_mex('trans_series_mark', h)                          % source := the packets' omega now
//   swrt_mex('trans_series_mark_values', h, v)                % source := v, one per packet in the original order
//   swrt_mex('trans_series_record', h)
//   swrt_mex('trans_series_record_history', h, first, count)
//   n = swrt_mex('trans_series_frames', h)
//   [counts, sums, stats] = swrt_mex('trans_series_get', h)   % int64 (nw+2) x (ns+2) x frames, 3 x (ns+2) x frames, 3 x frames
//   swrt_mex('trans_series_reset', h)
//   swrt_mex('recycle_begin', h, f, Cg, omega_cut, L[, seed, index_base, frac_bits, home_k])   % absorb at omega_cut, re-inject at home; home_k n x 2 ([]: the packets' k now)
//   swrt_mex('recycle_apply', h)                              % one event on the packets, in place; its frame appended
//   n = swrt_mex('recycle_frames', h)
//   stats = swrt_mex('recycle_get', h)                        % int64 8 x frames: n, absorbed, rejected, sum q(omega_out), sum q(omega_home), sum age, max age, serial
//   [gen, born] = swrt_mex('recycle_state', h)                % int64 n x 1 each, original order
//   swrt_mex('recycle_reset', h)
//   swrt_mex('recycle_end', h)
//   swrt_mex('refr_series_begin', h, f, Cg, omega_edges, a_edges[, frac_bits])   % omega classes by strain-alignment classes; omega-dot, omega-dot^2, gamma sums
//   swrt_mex('refr_series_record', h, nslots, alpha, bump)
//   swrt_mex('refr_series_record_history', h, first, count, nslots, alphas, bump)   % alphas [] when nslots < 2
//   n = swrt_mex('refr_series_frames', h)
//   [counts, sums, stats] = swrt_mex('refr_series_get', h)    % int64 (nw+2) x (na+2) x frames, (3(nw+2)+(na+2)) x frames, 2 x frames
//   swrt_mex('refr_series_reset', h)
//   swrt_mex('absfreq_series_begin', h, f, Cg, omega_edges, abs_edges[, frac_bits])   % omega classes by classes of Omega = omega + U.k; Omega-dot, Omega-dot^2, U.k sums
//   swrt_mex('absfreq_series_record', h, slot_a, slot_b, alpha, tau, bump)   % slots 0-based; slot_b -1: one snapshot
//   swrt_mex('absfreq_series_record_history', h, first, count, slot_a, slot_b, alphas, tau, bump)   % alphas [] when slot_b < 0
//   n = swrt_mex('absfreq_series_frames', h)
//   [counts, sums, stats] = swrt_mex('absfreq_series_get', h)    % int64 (nw+2) x (no+2) x frames, (3(nw+2)+2(no+2)) x frames, 2 x frames
//   swrt_mex('absfreq_series_reset', h)
//   swrt_mex('tangent_begin', h)                              % carry M = d(x,k)/d(x0,k0) of the discrete step: M = I, caustic counters 0
//   swrt_mex('tangent_mark', h)                               % a new window: M = I, counters 0
//   [M, caustics] = swrt_mex('tangent_get', h)                % 16 x n (column i: packet i's M, row-major), int64 n x 1; original order
//   swrt_mex('tangent_end', h)
//   swrt_mex('tangent_series_begin', h, f, Cg, omega_edges, growth_edges)   % classes of |M|_F^2/4 by omega classes
//   swrt_mex('tangent_series_record', h)
//   n = swrt_mex('tangent_series_frames', h)
//   [counts, sums, stats] = swrt_mex('tangent_series_get', h)    % int64 (nw+2) x (ns+2) x frames, (3(nw+2)+(ns+2)) x frames, 3 x frames
//   swrt_mex('tangent_series_reset', h)
//   swrt_mex('track_begin', h, ids)                         % trajectories of chosen packets; ids 0-based doubles
//   swrt_mex('track_record', h, f, gH, nslots, alpha, bump)   % nslots 0: no flow, Omega..D are NaN
//   swrt_mex('track_record_history', h, first, count, f, gH, nslots, alphas, bump)   % alphas [] when nslots < 2
//   frames = swrt_mex('track_get', h)                         % m x 8 x frames [x y k l Omega zeta sigma D]
//   swrt_mex('track_reset', h)
//   swrt_mex('flow_spectrum_begin', h, nx, k_scale, K_d2)     % shell spectra of the background flow on the device
//   swrt_mex('flow_spectrum_record_qg', h[, layer]);  swrt_mex('flow_spectrum_record_qk', h, qk, t)
//   n = swrt_mex('flow_spectrum_frames', h);  ns = swrt_mex('flow_spectrum_shells', h)
//   [spectra, stats] = swrt_mex('flow_spectrum_get', h)       % nshell x 3 x frames [E Z Q], 4 x frames [t; sums]
//   swrt_mex('flow_spectrum_reset', h)
#include <cstring>
#include <string>
#include <vector>

#include "mex.h"
#if defined(__has_include)
#if __has_include("mex_int64.h")
#include "mex_int64.h"  // a test build against tests/mex_shim: its mex.h declares no int64 arrays
#endif
#endif
#include "swrt.h"

static std::vector<swrt_ctx*> g_ctx;  // handle h = index + 1; closed handles hold nullptr

static void cleanup() {
  for (swrt_ctx*& c : g_ctx)
    if (c) {
      swrt_destroy(c);
      c = nullptr;
    }
  g_ctx.clear();
}

static size_t live_contexts() {
  size_t n = 0;
  for (swrt_ctx* c : g_ctx) n += c != nullptr;
  return n;
}

static double scalar(const mxArray* a) { return mxGetScalar(a); }

static swrt_ctx* handle(int nrhs, const mxArray* prhs[]) {
  if (nrhs < 2 || mxGetNumberOfElements(prhs[1]) != 1)
    mexErrMsgIdAndTxt("swrt:arg", "second argument: the context handle from swrt_mex('create', device)");
  const double h = scalar(prhs[1]);
  const size_t i = (size_t)h;
  if (h < 1 || (double)i != h || i > g_ctx.size() || g_ctx[i - 1] == nullptr)
    mexErrMsgIdAndTxt("swrt:state", "invalid or closed context handle %g", h);
  return g_ctx[i - 1];
}

static void check(swrt_ctx* c, int rc, const char* what) {
  if (rc != SWRT_OK) {
    const std::string msg = std::string(what) + ": " + swrt_last_error(c);
    mexErrMsgIdAndTxt("swrt:call", "%s (code %d)", msg.c_str(), rc);
  }
}

static const double* reals(const mxArray* a, const char* name) {
  if (!mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("swrt:arg", "%s must be real double", name);
  return mxGetDoubles(a);
}

static const double* complexes(const mxArray* a, const char* name) {
  if (!mxIsDouble(a) || !mxIsComplex(a)) mexErrMsgIdAndTxt("swrt:arg", "%s must be complex double", name);
  return (const double*)mxGetComplexDoubles(a);  // interleaved re, im (R2018a API)
}

static void need(int nrhs, int n, const char* cmd) {
  if (nrhs < n) mexErrMsgIdAndTxt("swrt:arg", "%s: expected %d arguments after the command", cmd, n - 1);
}

// The library's own grid sizes size every output (a caller's nx that does not
// match is an error, never a buffer size).
static int64_t slot_grid(swrt_ctx* c, int slot, int64_t nx_arg) {
  const int64_t nx = swrt_field_grid(c, slot);
  if (nx < 0) mexErrMsgIdAndTxt("swrt:state", "field slot %d is not set", slot);
  if (nx_arg != nx) mexErrMsgIdAndTxt("swrt:arg", "slot %d holds a %lld^2 grid, not %lld^2", slot, (long long)nx,
                                      (long long)nx_arg);
  return nx;
}

static int64_t qg_grid(swrt_ctx* c, int64_t nx_arg, int nl_arg, int* nl) {
  const int64_t nx = swrt_qg_grid(c, nl);
  if (nx < 0) mexErrMsgIdAndTxt("swrt:state", "swrt_qg_init not called");
  if (nx_arg != nx || nl_arg != *nl)
    mexErrMsgIdAndTxt("swrt:arg", "the QG state is %lld x %lld x %d, not %lld x %lld x %d", (long long)nx,
                      (long long)nx, *nl, (long long)nx_arg, (long long)nx_arg, nl_arg);
  return nx;
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  if (nrhs < 1 || !mxIsChar(prhs[0])) mexErrMsgIdAndTxt("swrt:arg", "first argument: command");
  char cmd[64];
  mxGetString(prhs[0], cmd, sizeof(cmd));

  if (!strcmp(cmd, "create")) {  // (device) -> h
    const int dev = nrhs > 1 ? (int)scalar(prhs[1]) : 0;
    swrt_ctx* c = nullptr;
    const int rc = swrt_create(dev, &c);
    if (rc != SWRT_OK) mexErrMsgIdAndTxt("swrt:create", "swrt_create failed (code %d)", rc);
    if (g_ctx.empty()) mexAtExit(cleanup);
    if (live_contexts() == 0) mexLock();  // stay loaded while a context is open
    g_ctx.push_back(c);  // handles are never reused: a stale copy of a closed one fails, never aliases
    plhs[0] = mxCreateDoubleScalar((double)g_ctx.size());
    return;
  }
  if (!strcmp(cmd, "live")) {  // () -> number of open contexts (SwrtContext lifetime tests)
    plhs[0] = mxCreateDoubleScalar((double)live_contexts());
    return;
  }
  if (!strcmp(cmd, "integrator_weights")) {  // (composition 0|1|2) -> [w 1 x S, off 1 x S]; no context
    if (nrhs < 2) mexErrMsgIdAndTxt("swrt:arg", "integrator_weights: composition");
    double w[5], off[5];
    int S = 0;
    if (swrt_integrator_weights((int)scalar(prhs[1]), w, off, &S) != SWRT_OK)
      mexErrMsgIdAndTxt("swrt:arg", "integrator_weights: composition must be 0 (none), 1 (Yoshida) or 2 (Suzuki)");
    plhs[0] = mxCreateDoubleMatrix(1, (mwSize)S, mxREAL);
    memcpy(mxGetDoubles(plhs[0]), w, sizeof(double) * (size_t)S);
    if (nlhs > 1) {
      plhs[1] = mxCreateDoubleMatrix(1, (mwSize)S, mxREAL);
      memcpy(mxGetDoubles(plhs[1]), off, sizeof(double) * (size_t)S);
    }
    return;
  }
  swrt_ctx* c = handle(nrhs, prhs);
  const mxArray** a = prhs + 1;  // a[1] = first argument after the handle
  const int na = nrhs - 1;

  if (!strcmp(cmd, "destroy")) {  // SwrtContext.delete: the last reference to a context is gone
    swrt_destroy(c);
    g_ctx[(size_t)scalar(prhs[1]) - 1] = nullptr;
    if (live_contexts() == 0) mexUnlock();  // `clear mex` may unload the gateway again
    return;
  }
  if (!strcmp(cmd, "set_field_psi")) {  // (slot, psi, L)
    need(na, 4, cmd);
    const int64_t nx = (int64_t)mxGetM(a[2]);
    check(c, swrt_set_field_psi(c, (int)scalar(a[1]), reals(a[2], "psi"), nx, scalar(a[3])), "swrt_set_field_psi");
    return;
  }
  if (!strcmp(cmd, "set_field_qk")) {  // (slot, qk, L, K_d2, shear, kscale, ny_period)
    need(na, 8, cmd);
    const int64_t nx = (int64_t)mxGetM(a[2]) + 1;
    check(c, swrt_set_field_qk(c, (int)scalar(a[1]), complexes(a[2], "qk"), nx, scalar(a[3]), scalar(a[4]),
                               scalar(a[5]), scalar(a[6]), (int64_t)scalar(a[7])),
          "swrt_set_field_qk");
    return;
  }
  if (!strcmp(cmd, "set_field_q")) {  // (slot, q nx x nx, L, K_d2, shear, kscale, ny_period)
    need(na, 8, cmd);
    const int64_t nx = (int64_t)mxGetM(a[2]);
    if ((int64_t)mxGetN(a[2]) != nx) mexErrMsgIdAndTxt("swrt:arg", "q must be an nx x nx frame");
    check(c, swrt_set_field_q(c, (int)scalar(a[1]), reals(a[2], "q"), nx, scalar(a[3]), scalar(a[4]), scalar(a[5]),
                              scalar(a[6]), (int64_t)scalar(a[7])),
          "swrt_set_field_q");
    return;
  }
  if (!strcmp(cmd, "set_field_grid")) {  // (slot, u, v, ux, uy, vx, vy, L, ny_period)
    need(na, 10, cmd);
    const int64_t nx = (int64_t)mxGetM(a[2]);
    const size_t plane = (size_t)(nx * nx);
    for (int f = 0; f < 6; ++f)
      if (mxGetNumberOfElements(a[2 + f]) != plane) mexErrMsgIdAndTxt("swrt:arg", "fields must all be nx x nx");
    mxArray* tmp = mxCreateDoubleMatrix(plane, 6, mxREAL);  // 6 planes, MATLAB-owned scratch
    double* d = mxGetDoubles(tmp);
    for (int f = 0; f < 6; ++f) memcpy(d + f * plane, reals(a[2 + f], "field"), plane * sizeof(double));
    const int rc = swrt_set_field_grid(c, (int)scalar(a[1]), d, nx, scalar(a[8]), (int64_t)scalar(a[9]));
    mxDestroyArray(tmp);
    check(c, rc, "swrt_set_field_grid");
    return;
  }
  if (!strcmp(cmd, "get_fields")) {  // (slot, nx) -> nx x nx x 6
    need(na, 3, cmd);
    const int64_t nx = slot_grid(c, (int)scalar(a[1]), (int64_t)scalar(a[2]));
    const mwSize dims[3] = {(mwSize)nx, (mwSize)nx, 6};
    plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    check(c, swrt_get_field_grid(c, (int)scalar(a[1]), mxGetDoubles(plhs[0])), "swrt_get_field_grid");
    return;
  }
  if (!strcmp(cmd, "get_psi")) {  // (slot, nx) -> nx x nx
    need(na, 3, cmd);
    const int64_t nx = slot_grid(c, (int)scalar(a[1]), (int64_t)scalar(a[2]));
    plhs[0] = mxCreateDoubleMatrix((mwSize)nx, (mwSize)nx, mxREAL);
    check(c, swrt_get_psi_grid(c, (int)scalar(a[1]), mxGetDoubles(plhs[0])), "swrt_get_psi_grid");
    return;
  }
  if (!strcmp(cmd, "eval")) {  // (x, y, nslots, alpha, bump) -> n x 6
    need(na, 6, cmd);
    const size_t n = mxGetNumberOfElements(a[1]);
    if (mxGetNumberOfElements(a[2]) != n) mexErrMsgIdAndTxt("swrt:arg", "x and y must have the same size");
    plhs[0] = mxCreateDoubleMatrix(n, 6, mxREAL);  // 6 x n row blocks == n x 6 column-major
    check(c, swrt_eval(c, reals(a[1], "x"), reals(a[2], "y"), (int64_t)n, (int)scalar(a[3]), scalar(a[4]),
                       scalar(a[5]), mxGetDoubles(plhs[0])),
          "swrt_eval");
    return;
  }
  if (!strcmp(cmd, "interpolate")) {  // (x, y, F, dx, dy, bump)
    need(na, 7, cmd);
    const mxArray* F = a[3];
    const int64_t nx = (int64_t)mxGetM(F);
    const int64_t nyF = (int64_t)(mxGetNumberOfElements(F) / mxGetM(F));
    const size_t n = mxGetNumberOfElements(a[1]);
    plhs[0] = mxCreateNumericArray(mxGetNumberOfDimensions(a[1]), mxGetDimensions(a[1]), mxDOUBLE_CLASS, mxREAL);
    check(c, swrt_interpolate(c, reals(F, "F"), nx, nyF, scalar(a[4]), scalar(a[5]), scalar(a[6]),
                              reals(a[1], "x"), reals(a[2], "y"), (int64_t)n, mxGetDoubles(plhs[0])),
          "swrt_interpolate");
    return;
  }
  if (!strcmp(cmd, "leapfrog")) {
    // (x0 Nx2, k0 Nx2, dt, nsteps, f, gH, nslots, alpha0, dalpha, bump, save_every)
    need(na, 11, cmd);
    const int64_t n = (int64_t)mxGetM(a[1]);
    if (mxGetN(a[1]) != 2 || mxGetM(a[2]) != (size_t)n || mxGetN(a[2]) != 2)
      mexErrMsgIdAndTxt("swrt:arg", "x0 and k0 must be N x 2");
    const int64_t nsteps = (int64_t)scalar(a[4]);
    const int64_t save_every = na > 11 ? (int64_t)scalar(a[11]) : 0;
    plhs[0] = mxDuplicateArray(a[1]);
    plhs[1] = mxDuplicateArray(a[2]);
    double *hx = nullptr, *hk = nullptr;
    if (nlhs > 2 && save_every > 0) {
      const mwSize dims[3] = {(mwSize)n, 2, (mwSize)(nsteps / save_every)};  // frames of N x 2
      plhs[2] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
      plhs[3] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
      hx = mxGetDoubles(plhs[2]);
      hk = mxGetDoubles(plhs[3]);
    }
    check(c, swrt_leapfrog(c, mxGetDoubles(plhs[0]), mxGetDoubles(plhs[1]), n, scalar(a[3]), nsteps, scalar(a[5]),
                           scalar(a[6]), (int)scalar(a[7]), scalar(a[8]), scalar(a[9]), scalar(a[10]),
                           hx ? save_every : 0, hx, hk),
          "swrt_leapfrog");
    return;
  }
  if (!strcmp(cmd, "g2k")) {
    need(na, 2, cmd);
    const int64_t nx = (int64_t)mxGetM(a[1]);
    const int64_t kmax = nx / 2 - 1;
    plhs[0] = mxCreateDoubleMatrix(2 * kmax + 1, kmax + 1, mxCOMPLEX);
    check(c, swrt_g2k(c, reals(a[1], "fg"), nx, (double*)mxGetComplexDoubles(plhs[0])), "swrt_g2k");
    return;
  }
  if (!strcmp(cmd, "k2g")) {
    need(na, 2, cmd);
    const int64_t nx = (int64_t)mxGetM(a[1]) + 1;
    const double* fk = complexes(a[1], "fk");
    plhs[0] = mxCreateDoubleMatrix(nx, nx, mxREAL);
    check(c, swrt_k2g(c, fk, nx, mxGetDoubles(plhs[0])), "swrt_k2g");
    return;
  }
  if (!strcmp(cmd, "packets_set")) {  // (x Nx2, k Nx2)
    need(na, 3, cmd);
    check(c, swrt_packets_set(c, reals(a[1], "x"), reals(a[2], "k"), (int64_t)mxGetM(a[1])), "swrt_packets_set");
    return;
  }
  if (!strcmp(cmd, "packets_get")) {
    const int64_t n = swrt_packets_count(c);
    plhs[0] = mxCreateDoubleMatrix((mwSize)n, 2, mxREAL);
    plhs[1] = mxCreateDoubleMatrix((mwSize)n, 2, mxREAL);
    check(c, swrt_packets_get(c, mxGetDoubles(plhs[0]), mxGetDoubles(plhs[1])), "swrt_packets_get");
    return;
  }
  if (!strcmp(cmd, "advance")) {  // (dt, nsteps, f, gH, nslots, alpha0, dalpha, bump)
    need(na, 9, cmd);
    check(c, swrt_advance(c, scalar(a[1]), (int64_t)scalar(a[2]), scalar(a[3]), scalar(a[4]), (int)scalar(a[5]),
                          scalar(a[6]), scalar(a[7]), scalar(a[8]), 0),
          "swrt_advance");
    return;
  }
  if (!strcmp(cmd, "advance_intervals")) {  // (dts, nsub, f, gH, alpha0, dalpha, bump)
    need(na, 8, cmd);
    const int nint = (int)mxGetNumberOfElements(a[1]);
    check(c, swrt_advance_intervals(c, nint, reals(a[1], "dts"), (int64_t)scalar(a[2]), scalar(a[3]), scalar(a[4]),
                                    scalar(a[5]), scalar(a[6]), scalar(a[7]), 0),
          "swrt_advance_intervals");
    return;
  }
  if (!strcmp(cmd, "set_locality")) {  // (rebin_every, tile)
    need(na, 3, cmd);
    check(c, swrt_set_locality(c, (int64_t)scalar(a[1]), (int64_t)scalar(a[2])), "swrt_set_locality");
    return;
  }
  if (!strcmp(cmd, "set_integrator")) {  // (kick, iterations, composition): the packet step of leapfrog / advance*
    need(na, 4, cmd);
    check(c, swrt_set_integrator(c, (int)scalar(a[1]), (int)scalar(a[2]), (int)scalar(a[3])), "swrt_set_integrator");
    return;
  }
  if (!strcmp(cmd, "get_integrator")) {  // () -> [kick iterations composition]
    int kick = 0, it = 0, comp = 0;
    check(c, swrt_get_integrator(c, &kick, &it, &comp), "swrt_get_integrator");
    plhs[0] = mxCreateDoubleMatrix(1, 3, mxREAL);
    double* d = mxGetDoubles(plhs[0]);
    d[0] = kick; d[1] = it; d[2] = comp;
    return;
  }
  if (!strcmp(cmd, "ode23_f1")) {  // (t, tmax, f, Cg, nslots, thr, bump) -> rh_raw
    need(na, 8, cmd);
    double r = 0.0;
    check(c, swrt_ode23_f1(c, scalar(a[1]), scalar(a[2]), scalar(a[3]), scalar(a[4]), (int)scalar(a[5]),
                           scalar(a[6]), scalar(a[7]), &r),
          "swrt_ode23_f1");
    plhs[0] = mxCreateDoubleScalar(r);
    return;
  }
  if (!strcmp(cmd, "ode23_attempt")) {  // (t, h, tnew, tmax, f, Cg, nslots, thr, bump) -> err_raw
    need(na, 10, cmd);
    double r = 0.0;
    check(c, swrt_ode23_attempt(c, scalar(a[1]), scalar(a[2]), scalar(a[3]), scalar(a[4]), scalar(a[5]),
                                scalar(a[6]), (int)scalar(a[7]), scalar(a[8]), scalar(a[9]), &r),
          "swrt_ode23_attempt");
    plhs[0] = mxCreateDoubleScalar(r);
    return;
  }
  if (!strcmp(cmd, "ode23_accept")) {
    check(c, swrt_ode23_accept(c), "swrt_ode23_accept");
    return;
  }
  if (!strcmp(cmd, "ode23_set_dense")) {  // (on)
    need(na, 2, cmd);
    check(c, swrt_ode23_set_dense(c, (int)scalar(a[1])), "swrt_ode23_set_dense");
    return;
  }
  if (!strcmp(cmd, "ode23_ntrp")) {  // (t, tnew, tout): one history frame per time in tout
    need(na, 4, cmd);
    check(c, swrt_ode23_ntrp(c, scalar(a[1]), scalar(a[2]), reals(a[3], "tout"),
                             (int64_t)mxGetNumberOfElements(a[3])),
          "swrt_ode23_ntrp");
    return;
  }
  if (!strcmp(cmd, "history")) {  // -> hx, hk: N x 2 x frames
    const int64_t n = swrt_packets_count(c), nf = swrt_history_frames(c);
    const mwSize dims[3] = {(mwSize)n, 2, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    plhs[1] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    check(c, swrt_history_get(c, 0, nf, mxGetDoubles(plhs[0]), mxGetDoubles(plhs[1])), "swrt_history_get");
    return;
  }
  if (!strcmp(cmd, "history_reset")) {
    check(c, swrt_history_reset(c), "swrt_history_reset");
    return;
  }
  if (!strcmp(cmd, "qg_init")) {  // (params struct, qk complex (2kmax+1) x (kmax+1) [x nlayers])
    need(na, 3, cmd);
    const mxArray* s = a[1];
    auto fld = [&](const char* name, double dflt) {
      const mxArray* v = mxGetField(s, 0, name);
      return v ? mxGetScalar(v) : dflt;
    };
    swrt_qg_params p;
    p.nlayers = (int)fld("nlayers", 1);
    p.filter = (int)fld("filter", 1);
    p.L = fld("L", 6.283185307179586);
    p.K_d2 = fld("K_d2", 1.0);
    p.beta = fld("beta", 0.0);
    p.r_drag = fld("r_drag", 0.0);
    p.force_strength = fld("force_strength", 0.0);
    p.f = fld("f", 1.0);
    p.Cg = fld("Cg", 1.0);
    p.shear = fld("shear", 0.0);
    p.nu = fld("nu", 0.0);
    p.hyper_order = fld("hyper_order", 4.0);
    p.r = fld("r", 0.0);
    const int64_t nx = (int64_t)mxGetM(a[2]) + 1;
    check(c, swrt_qg_init(c, &p, nx, complexes(a[2], "qk")), "swrt_qg_init");
    return;
  }
  if (!strcmp(cmd, "qg_step")) {  // (dt, nsteps)
    need(na, 2, cmd);
    check(c, swrt_qg_step(c, scalar(a[1]), na > 2 ? (int64_t)scalar(a[2]) : 1), "swrt_qg_step");
    return;
  }
  if (!strcmp(cmd, "qg_max_speed")) {
    double u = 0.0;
    check(c, swrt_qg_max_speed(c, &u), "swrt_qg_max_speed");
    plhs[0] = mxCreateDoubleScalar(u);
    return;
  }
  if (!strcmp(cmd, "qg_get")) {  // (nx, nlayers) -> qk, t, steps
    need(na, 3, cmd);
    double t = 0.0;
    int64_t steps = 0;
    int nl = 0;
    const int64_t nx = qg_grid(c, (int64_t)scalar(a[1]), (int)scalar(a[2]), &nl);
    const mwSize dims[3] = {(mwSize)(nx - 1), (mwSize)(nx / 2), (mwSize)nl};
    plhs[0] = mxCreateNumericArray(nl > 1 ? 3 : 2, dims, mxDOUBLE_CLASS, mxCOMPLEX);
    check(c, swrt_qg_get(c, (double*)mxGetComplexDoubles(plhs[0]), &t, &steps), "swrt_qg_get");
    if (nlhs > 1) plhs[1] = mxCreateDoubleScalar(t);
    if (nlhs > 2) plhs[2] = mxCreateDoubleScalar((double)steps);
    return;
  }
  if (!strcmp(cmd, "qg_get_q")) {  // (nx, nlayers) -> q nx x nx [x nlayers]
    need(na, 3, cmd);
    int nl = 0;
    const int64_t nx = qg_grid(c, (int64_t)scalar(a[1]), (int)scalar(a[2]), &nl);
    const mwSize dims[3] = {(mwSize)nx, (mwSize)nx, (mwSize)nl};
    plhs[0] = mxCreateNumericArray(nl > 1 ? 3 : 2, dims, mxDOUBLE_CLASS, mxREAL);
    check(c, swrt_qg_get_q(c, mxGetDoubles(plhs[0])), "swrt_qg_get_q");
    return;
  }
  if (!strcmp(cmd, "qg_snapshot")) {  // (slot, which, layer, ny_period)
    need(na, 5, cmd);
    check(c, swrt_qg_snapshot(c, (int)scalar(a[1]), (int)scalar(a[2]), (int)scalar(a[3]), (int64_t)scalar(a[4])),
          "swrt_qg_snapshot");
    return;
  }
  if (!strcmp(cmd, "swap_slots")) {
    need(na, 3, cmd);
    check(c, swrt_swap_slots(c, (int)scalar(a[1]), (int)scalar(a[2])), "swrt_swap_slots");
    return;
  }
  if (!strcmp(cmd, "field_div_free")) {
    need(na, 2, cmd);
    const int rc = swrt_field_div_free(c, (int)scalar(a[1]));
    if (rc < 0) check(c, rc, "swrt_field_div_free");
    plhs[0] = mxCreateDoubleScalar(rc == 1 ? 1.0 : 0.0);
    return;
  }
  if (!strcmp(cmd, "omega_series_begin")) {  // (f, Cg, edges)
    need(na, 4, cmd);
    check(c, swrt_omega_series_begin(c, scalar(a[1]), scalar(a[2]), reals(a[3], "edges"),
                                     (int64_t)mxGetNumberOfElements(a[3]) - 1),
          "swrt_omega_series_begin");
    return;
  }
  if (!strcmp(cmd, "omega_series_record")) {
    check(c, swrt_omega_series_record(c), "swrt_omega_series_record");
    return;
  }
  if (!strcmp(cmd, "omega_series_record_history")) {  // (first, count): 0-based history frames
    need(na, 3, cmd);
    check(c, swrt_omega_series_record_history(c, (int64_t)scalar(a[1]), (int64_t)scalar(a[2])),
          "swrt_omega_series_record_history");
    return;
  }
  if (!strcmp(cmd, "omega_series_get")) {  // -> counts (nbins+2) x frames (double, exact), stats 4 x frames
    const int64_t nf = swrt_omega_series_frames(c), ns = swrt_omega_series_bins(c) + 2;
    std::vector<int64_t> counts((size_t)(nf * ns));
    plhs[0] = mxCreateDoubleMatrix((mwSize)ns, (mwSize)nf, mxREAL);
    mxArray* stats = mxCreateDoubleMatrix(4, (mwSize)nf, mxREAL);
    check(c, swrt_omega_series_get(c, 0, nf, counts.data(), mxGetDoubles(stats)), "swrt_omega_series_get");
    double* d = mxGetDoubles(plhs[0]);
    for (size_t i = 0; i < counts.size(); ++i) d[i] = (double)counts[i];
    if (nlhs > 1) plhs[1] = stats; else mxDestroyArray(stats);
    return;
  }
  if (!strcmp(cmd, "omega_series_reset")) {
    check(c, swrt_omega_series_reset(c), "swrt_omega_series_reset");
    return;
  }
  if (!strcmp(cmd, "omega_ideal")) {  // (slot, ring m x 2, omega0, edges) -> counts (nbins+2) x 1
    need(na, 5, cmd);
    if (mxGetN(a[2]) != 2) mexErrMsgIdAndTxt("swrt:arg", "ring must be m x 2");
    const int64_t nb = (int64_t)mxGetNumberOfElements(a[4]) - 1;
    std::vector<int64_t> counts((size_t)(nb > 0 ? nb + 2 : 2));
    check(c, swrt_omega_ideal(c, (int)scalar(a[1]), reals(a[2], "ring"), (int64_t)mxGetM(a[2]), scalar(a[3]),
                              reals(a[4], "edges"), nb, counts.data()),
          "swrt_omega_ideal");
    plhs[0] = mxCreateDoubleMatrix((mwSize)counts.size(), 1, mxREAL);
    for (size_t i = 0; i < counts.size(); ++i) mxGetDoubles(plhs[0])[i] = (double)counts[i];
    return;
  }
  if (!strcmp(cmd, "map_series_begin")) {  // (L, m, f, Cg[, frac_bits = 20])
    need(na, 5, cmd);
    check(c, swrt_map_series_begin(c, scalar(a[1]), (int64_t)scalar(a[2]), scalar(a[3]), scalar(a[4]),
                                   na > 5 ? (int)scalar(a[5]) : 20),
          "swrt_map_series_begin");
    return;
  }
  if (!strcmp(cmd, "map_series_record")) {
    check(c, swrt_map_series_record(c), "swrt_map_series_record");
    return;
  }
  if (!strcmp(cmd, "map_series_record_history")) {  // (first, count): 0-based history frames
    need(na, 3, cmd);
    check(c, swrt_map_series_record_history(c, (int64_t)scalar(a[1]), (int64_t)scalar(a[2])),
          "swrt_map_series_record_history");
    return;
  }
  if (!strcmp(cmd, "map_series_get")) {  // -> planes m x m x 4 x frames (double, exact), stats 2 x frames
    const int64_t nf = swrt_map_series_frames(c), m = swrt_map_series_cells(c);
    std::vector<int64_t> planes((size_t)(nf * 4 * m * m)), st((size_t)(nf * 2));
    const mwSize dims[4] = {(mwSize)m, (mwSize)m, 4, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(4, dims, mxDOUBLE_CLASS, mxREAL);
    mxArray* stats = mxCreateDoubleMatrix(2, (mwSize)nf, mxREAL);
    check(c, swrt_map_series_get(c, 0, nf, planes.data(), st.data()), "swrt_map_series_get");
    double* d = mxGetDoubles(plhs[0]);
    for (size_t i = 0; i < planes.size(); ++i) d[i] = (double)planes[i];
    for (size_t i = 0; i < st.size(); ++i) mxGetDoubles(stats)[i] = (double)st[i];
    if (nlhs > 1) plhs[1] = stats; else mxDestroyArray(stats);
    return;
  }
  if (!strcmp(cmd, "map_series_reset")) {
    check(c, swrt_map_series_reset(c), "swrt_map_series_reset");
    return;
  }
  if (!strcmp(cmd, "kmap_series_begin")) {  // (K, m[, frac_bits = 16])
    need(na, 3, cmd);
    check(c, swrt_kmap_series_begin(c, scalar(a[1]), (int64_t)scalar(a[2]), na > 3 ? (int)scalar(a[3]) : 16),
          "swrt_kmap_series_begin");
    return;
  }
  if (!strcmp(cmd, "kmap_series_record")) {
    check(c, swrt_kmap_series_record(c), "swrt_kmap_series_record");
    return;
  }
  if (!strcmp(cmd, "kmap_series_record_history")) {  // (first, count): 0-based history frames
    need(na, 3, cmd);
    check(c, swrt_kmap_series_record_history(c, (int64_t)scalar(a[1]), (int64_t)scalar(a[2])),
          "swrt_kmap_series_record_history");
    return;
  }
  if (!strcmp(cmd, "kmap_series_frames")) {
    plhs[0] = mxCreateDoubleScalar((double)swrt_kmap_series_frames(c));
    return;
  }
  if (!strcmp(cmd, "kmap_series_get")) {  // -> planes m x m x frames (int64), stats 8 x frames (int64)
    const int64_t nf = swrt_kmap_series_frames(c), m = swrt_kmap_series_cells(c);
    const mwSize dims[3] = {(mwSize)m, (mwSize)m, (mwSize)nf}, sdims[2] = {8, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(3, dims, mxINT64_CLASS, mxREAL);
    mxArray* stats = mxCreateNumericArray(2, sdims, mxINT64_CLASS, mxREAL);
    if (nf > 0)
      check(c, swrt_kmap_series_get(c, 0, nf, (int64_t*)mxGetInt64s(plhs[0]), (int64_t*)mxGetInt64s(stats)),
            "swrt_kmap_series_get");
    if (nlhs > 1) plhs[1] = stats; else mxDestroyArray(stats);
    return;
  }
  if (!strcmp(cmd, "kmap_series_reset")) {
    check(c, swrt_kmap_series_reset(c), "swrt_kmap_series_reset");
    return;
  }
  if (!strcmp(cmd, "cond_series_begin")) {  // (f, Cg, omega_edges, which, q_edges[, frac_bits = 20])
    need(na, 6, cmd);
    const size_t ne = mxGetNumberOfElements(a[3]), nqe = mxGetNumberOfElements(a[5]);
    check(c, swrt_cond_series_begin(c, scalar(a[1]), scalar(a[2]), reals(a[3], "omega_edges"), (int64_t)ne - 1,
                                    (int)scalar(a[4]), reals(a[5], "q_edges"), (int64_t)nqe - 1,
                                    na > 6 ? (int)scalar(a[6]) : 20),
          "swrt_cond_series_begin");
    return;
  }
  if (!strcmp(cmd, "cond_series_record")) {  // (nslots, alpha, bump)
    need(na, 4, cmd);
    check(c, swrt_cond_series_record(c, (int)scalar(a[1]), scalar(a[2]), scalar(a[3])), "swrt_cond_series_record");
    return;
  }
  if (!strcmp(cmd, "cond_series_record_history")) {  // (first, count, nslots, alphas, bump): [] alphas = none
    need(na, 6, cmd);
    const int64_t count = (int64_t)scalar(a[2]);
    const size_t nal = mxGetNumberOfElements(a[4]);
    if (nal != 0 && (int64_t)nal != count) mexErrMsgIdAndTxt("swrt:arg", "alphas must hold one value per frame");
    check(c, swrt_cond_series_record_history(c, (int64_t)scalar(a[1]), count, (int)scalar(a[3]),
                                             nal ? reals(a[4], "alphas") : nullptr, scalar(a[5])),
          "swrt_cond_series_record_history");
    return;
  }
  if (!strcmp(cmd, "cond_series_frames")) {
    plhs[0] = mxCreateDoubleScalar((double)swrt_cond_series_frames(c));
    return;
  }
  if (!strcmp(cmd, "cond_series_get")) {  // -> counts (nw+2) x (nq+2) x frames, sums (nq+2) x frames, stats 2 x frames
    const int64_t nf = swrt_cond_series_frames(c);
    int64_t nw = 0, nq = 0;
    check(c, swrt_cond_series_bins(c, &nw, &nq), "swrt_cond_series_bins");
    const mwSize dims[3] = {(mwSize)(nw + 2), (mwSize)(nq + 2), (mwSize)nf}, udims[2] = {(mwSize)(nq + 2), (mwSize)nf},
                 sdims[2] = {2, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(3, dims, mxINT64_CLASS, mxREAL);
    mxArray* sums = mxCreateNumericArray(2, udims, mxINT64_CLASS, mxREAL);
    mxArray* stats = mxCreateNumericArray(2, sdims, mxINT64_CLASS, mxREAL);
    if (nf > 0)
      check(c, swrt_cond_series_get(c, 0, nf, (int64_t*)mxGetInt64s(plhs[0]), (int64_t*)mxGetInt64s(sums),
                                    (int64_t*)mxGetInt64s(stats)),
            "swrt_cond_series_get");
    if (nlhs > 1) plhs[1] = sums; else mxDestroyArray(sums);
    if (nlhs > 2) plhs[2] = stats; else mxDestroyArray(stats);
    return;
  }
  if (!strcmp(cmd, "cond_series_reset")) {
    check(c, swrt_cond_series_reset(c), "swrt_cond_series_reset");
    return;
  }
  if (!strcmp(cmd, "trans_series_begin")) {  // (f, Cg, omega_edges, src_edges[, frac_bits = 20])
    need(na, 5, cmd);
    const size_t ne = mxGetNumberOfElements(a[3]), nse = mxGetNumberOfElements(a[4]);
    check(c, swrt_trans_series_begin(c, scalar(a[1]), scalar(a[2]), reals(a[3], "omega_edges"), (int64_t)ne - 1,
                                     reals(a[4], "src_edges"), (int64_t)nse - 1, na > 5 ? (int)scalar(a[5]) : 20),
          "swrt_trans_series_begin");
    return;
  }
  if (!strcmp(cmd, "trans_series_mark")) {
    check(c, swrt_trans_series_mark(c), "swrt_trans_series_mark");
    return;
  }
  if (!strcmp(cmd, "trans_series_mark_values")) {  // (v): one value per packet, original order
    need(na, 2, cmd);
    check(c, swrt_trans_series_mark_values(c, reals(a[1], "v"), (int64_t)mxGetNumberOfElements(a[1])),
          "swrt_trans_series_mark_values");
    return;
  }
  if (!strcmp(cmd, "trans_series_record")) {
    check(c, swrt_trans_series_record(c), "swrt_trans_series_record");
    return;
  }
  if (!strcmp(cmd, "trans_series_record_history")) {  // (first, count)
    need(na, 3, cmd);
    check(c, swrt_trans_series_record_history(c, (int64_t)scalar(a[1]), (int64_t)scalar(a[2])),
          "swrt_trans_series_record_history");
    return;
  }
  if (!strcmp(cmd, "trans_series_frames")) {
    plhs[0] = mxCreateDoubleScalar((double)swrt_trans_series_frames(c));
    return;
  }
  if (!strcmp(cmd, "trans_series_get")) {  // -> counts (nw+2) x (ns+2) x frames, sums 3 x (ns+2) x frames, stats 3 x frames
    const int64_t nf = swrt_trans_series_frames(c);
    int64_t nw = 0, ns = 0;
    check(c, swrt_trans_series_bins(c, &nw, &ns), "swrt_trans_series_bins");
    const mwSize dims[3] = {(mwSize)(nw + 2), (mwSize)(ns + 2), (mwSize)nf},
                 udims[3] = {3, (mwSize)(ns + 2), (mwSize)nf}, sdims[2] = {3, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(3, dims, mxINT64_CLASS, mxREAL);
    mxArray* sums = mxCreateNumericArray(3, udims, mxINT64_CLASS, mxREAL);
    mxArray* stats = mxCreateNumericArray(2, sdims, mxINT64_CLASS, mxREAL);
    if (nf > 0)
      check(c, swrt_trans_series_get(c, 0, nf, (int64_t*)mxGetInt64s(plhs[0]), (int64_t*)mxGetInt64s(sums),
                                     (int64_t*)mxGetInt64s(stats)),
            "swrt_trans_series_get");
    if (nlhs > 1) plhs[1] = sums; else mxDestroyArray(sums);
    if (nlhs > 2) plhs[2] = stats; else mxDestroyArray(stats);
    return;
  }
  if (!strcmp(cmd, "trans_series_reset")) {
    check(c, swrt_trans_series_reset(c), "swrt_trans_series_reset");
    return;
  }
  if (!strcmp(cmd, "refr_series_begin")) {  // (f, Cg, omega_edges, a_edges[, frac_bits = 20])
    need(na, 5, cmd);
    const size_t ne = mxGetNumberOfElements(a[3]), nae = mxGetNumberOfElements(a[4]);
    check(c, swrt_refr_series_begin(c, scalar(a[1]), scalar(a[2]), reals(a[3], "omega_edges"), (int64_t)ne - 1,
                                    reals(a[4], "a_edges"), (int64_t)nae - 1, na > 5 ? (int)scalar(a[5]) : 20),
          "swrt_refr_series_begin");
    return;
  }
  if (!strcmp(cmd, "refr_series_record")) {  // (nslots, alpha, bump)
    need(na, 4, cmd);
    check(c, swrt_refr_series_record(c, (int)scalar(a[1]), scalar(a[2]), scalar(a[3])), "swrt_refr_series_record");
    return;
  }
  if (!strcmp(cmd, "refr_series_record_history")) {  // (first, count, nslots, alphas, bump): [] alphas = none
    need(na, 6, cmd);
    const int64_t count = (int64_t)scalar(a[2]);
    const size_t nal = mxGetNumberOfElements(a[4]);
    if (nal != 0 && (int64_t)nal != count) mexErrMsgIdAndTxt("swrt:arg", "alphas must hold one value per frame");
    check(c, swrt_refr_series_record_history(c, (int64_t)scalar(a[1]), count, (int)scalar(a[3]),
                                             nal ? reals(a[4], "alphas") : nullptr, scalar(a[5])),
          "swrt_refr_series_record_history");
    return;
  }
  if (!strcmp(cmd, "refr_series_frames")) {
    plhs[0] = mxCreateDoubleScalar((double)swrt_refr_series_frames(c));
    return;
  }
  if (!strcmp(cmd, "refr_series_get")) {  // -> counts (nw+2) x (na+2) x frames, sums (3(nw+2)+(na+2)) x frames, stats 2 x frames
    const int64_t nf = swrt_refr_series_frames(c);
    int64_t nw = 0, nal = 0;
    check(c, swrt_refr_series_bins(c, &nw, &nal), "swrt_refr_series_bins");
    const mwSize dims[3] = {(mwSize)(nw + 2), (mwSize)(nal + 2), (mwSize)nf},
                 udims[2] = {(mwSize)(3 * (nw + 2) + nal + 2), (mwSize)nf}, sdims[2] = {2, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(3, dims, mxINT64_CLASS, mxREAL);
    mxArray* sums = mxCreateNumericArray(2, udims, mxINT64_CLASS, mxREAL);
    mxArray* stats = mxCreateNumericArray(2, sdims, mxINT64_CLASS, mxREAL);
    if (nf > 0)
      check(c, swrt_refr_series_get(c, 0, nf, (int64_t*)mxGetInt64s(plhs[0]), (int64_t*)mxGetInt64s(sums),
                                    (int64_t*)mxGetInt64s(stats)),
            "swrt_refr_series_get");
    if (nlhs > 1) plhs[1] = sums; else mxDestroyArray(sums);
    if (nlhs > 2) plhs[2] = stats; else mxDestroyArray(stats);
    return;
  }
  if (!strcmp(cmd, "refr_series_reset")) {
    check(c, swrt_refr_series_reset(c), "swrt_refr_series_reset");
    return;
  }
  if (!strcmp(cmd, "absfreq_series_begin")) {  // (f, Cg, omega_edges, abs_edges[, frac_bits = 20])
    need(na, 5, cmd);
    const size_t ne = mxGetNumberOfElements(a[3]), noe = mxGetNumberOfElements(a[4]);
    check(c, swrt_absfreq_series_begin(c, scalar(a[1]), scalar(a[2]), reals(a[3], "omega_edges"), (int64_t)ne - 1,
                                       reals(a[4], "abs_edges"), (int64_t)noe - 1, na > 5 ? (int)scalar(a[5]) : 20),
          "swrt_absfreq_series_begin");
    return;
  }
  if (!strcmp(cmd, "absfreq_series_record")) {  // (slot_a, slot_b, alpha, tau, bump)
    need(na, 6, cmd);
    check(c, swrt_absfreq_series_record(c, (int)scalar(a[1]), (int)scalar(a[2]), scalar(a[3]), scalar(a[4]),
                                        scalar(a[5])),
          "swrt_absfreq_series_record");
    return;
  }
  if (!strcmp(cmd, "absfreq_series_record_history")) {  // (first, count, slot_a, slot_b, alphas, tau, bump): [] alphas = none
    need(na, 8, cmd);
    const int64_t count = (int64_t)scalar(a[2]);
    const size_t nal = mxGetNumberOfElements(a[5]);
    if (nal != 0 && (int64_t)nal != count) mexErrMsgIdAndTxt("swrt:arg", "alphas must hold one value per frame");
    check(c, swrt_absfreq_series_record_history(c, (int64_t)scalar(a[1]), count, (int)scalar(a[3]), (int)scalar(a[4]),
                                                nal ? reals(a[5], "alphas") : nullptr, scalar(a[6]), scalar(a[7])),
          "swrt_absfreq_series_record_history");
    return;
  }
  if (!strcmp(cmd, "absfreq_series_frames")) {
    plhs[0] = mxCreateDoubleScalar((double)swrt_absfreq_series_frames(c));
    return;
  }
  if (!strcmp(cmd, "absfreq_series_get")) {  // -> counts (nw+2) x (no+2) x frames, sums (3(nw+2)+2(no+2)) x frames, stats 2 x frames
    const int64_t nf = swrt_absfreq_series_frames(c);
    int64_t nw = 0, nol = 0;
    check(c, swrt_absfreq_series_bins(c, &nw, &nol), "swrt_absfreq_series_bins");
    const mwSize dims[3] = {(mwSize)(nw + 2), (mwSize)(nol + 2), (mwSize)nf},
                 udims[2] = {(mwSize)(3 * (nw + 2) + 2 * (nol + 2)), (mwSize)nf}, sdims[2] = {2, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(3, dims, mxINT64_CLASS, mxREAL);
    mxArray* sums = mxCreateNumericArray(2, udims, mxINT64_CLASS, mxREAL);
    mxArray* stats = mxCreateNumericArray(2, sdims, mxINT64_CLASS, mxREAL);
    if (nf > 0)
      check(c, swrt_absfreq_series_get(c, 0, nf, (int64_t*)mxGetInt64s(plhs[0]), (int64_t*)mxGetInt64s(sums),
                                       (int64_t*)mxGetInt64s(stats)),
            "swrt_absfreq_series_get");
    if (nlhs > 1) plhs[1] = sums; else mxDestroyArray(sums);
    if (nlhs > 2) plhs[2] = stats; else mxDestroyArray(stats);
    return;
  }
  if (!strcmp(cmd, "absfreq_series_reset")) {
    check(c, swrt_absfreq_series_reset(c), "swrt_absfreq_series_reset");
    return;
  }
  if (!strcmp(cmd, "tangent_begin")) {
    check(c, swrt_tangent_begin(c), "swrt_tangent_begin");
    return;
  }
  if (!strcmp(cmd, "tangent_mark")) {
    check(c, swrt_tangent_mark(c), "swrt_tangent_mark");
    return;
  }
  if (!strcmp(cmd, "tangent_get")) {  // -> M 16 x n (double), caustics n x 1 (int64), original order
    const int64_t n = swrt_packets_count(c);
    std::vector<int32_t> caus((size_t)n);
    plhs[0] = mxCreateDoubleMatrix(16, (mwSize)n, mxREAL);
    check(c, swrt_tangent_get(c, mxGetDoubles(plhs[0]), caus.data()), "swrt_tangent_get");
    const mwSize dims[2] = {(mwSize)n, 1};
    mxArray* b = mxCreateNumericArray(2, dims, mxINT64_CLASS, mxREAL);
    int64_t* pb = (int64_t*)mxGetInt64s(b);
    for (int64_t i = 0; i < n; ++i) pb[i] = caus[(size_t)i];
    if (nlhs > 1) plhs[1] = b; else mxDestroyArray(b);
    return;
  }
  if (!strcmp(cmd, "tangent_end")) {
    check(c, swrt_tangent_end(c), "swrt_tangent_end");
    return;
  }
  if (!strcmp(cmd, "tangent_series_begin")) {  // (f, Cg, omega_edges, growth_edges)
    need(na, 5, cmd);
    const size_t ne = mxGetNumberOfElements(a[3]), nge = mxGetNumberOfElements(a[4]);
    check(c, swrt_tangent_series_begin(c, scalar(a[1]), scalar(a[2]), reals(a[3], "omega_edges"), (int64_t)ne - 1,
                                       reals(a[4], "growth_edges"), (int64_t)nge - 1),
          "swrt_tangent_series_begin");
    return;
  }
  if (!strcmp(cmd, "tangent_series_record")) {
    check(c, swrt_tangent_series_record(c), "swrt_tangent_series_record");
    return;
  }
  if (!strcmp(cmd, "tangent_series_frames")) {
    plhs[0] = mxCreateDoubleScalar((double)swrt_tangent_series_frames(c));
    return;
  }
  if (!strcmp(cmd, "tangent_series_get")) {  // -> counts (nw+2) x (ns+2) x frames, sums (3(nw+2)+(ns+2)) x frames, stats 3 x frames
    const int64_t nf = swrt_tangent_series_frames(c);
    int64_t nw = 0, ns = 0;
    check(c, swrt_tangent_series_bins(c, &nw, &ns), "swrt_tangent_series_bins");
    const mwSize dims[3] = {(mwSize)(nw + 2), (mwSize)(ns + 2), (mwSize)nf},
                 udims[2] = {(mwSize)(3 * (nw + 2) + (ns + 2)), (mwSize)nf}, sdims[2] = {3, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(3, dims, mxINT64_CLASS, mxREAL);
    mxArray* sums = mxCreateNumericArray(2, udims, mxINT64_CLASS, mxREAL);
    mxArray* stats = mxCreateNumericArray(2, sdims, mxINT64_CLASS, mxREAL);
    if (nf > 0)
      check(c, swrt_tangent_series_get(c, 0, nf, (int64_t*)mxGetInt64s(plhs[0]), (int64_t*)mxGetInt64s(sums),
                                       (int64_t*)mxGetInt64s(stats)),
            "swrt_tangent_series_get");
    if (nlhs > 1) plhs[1] = sums; else mxDestroyArray(sums);
    if (nlhs > 2) plhs[2] = stats; else mxDestroyArray(stats);
    return;
  }
  if (!strcmp(cmd, "tangent_series_reset")) {
    check(c, swrt_tangent_series_reset(c), "swrt_tangent_series_reset");
    return;
  }
  if (!strcmp(cmd, "recycle_begin")) {  // (f, Cg, omega_cut, L[, seed = 0, index_base = 0, frac_bits = 20, home_k = []])
    need(na, 5, cmd);
    const double* home = nullptr;
    if (na > 8 && mxGetNumberOfElements(a[8]) > 0) {
      if ((int64_t)mxGetNumberOfElements(a[8]) != 2 * swrt_packets_count(c))
        mexErrMsgIdAndTxt("swrt:arg", "home_k must be n x 2, one home wavevector per packet");
      home = reals(a[8], "home_k");
    }
    check(c, swrt_recycle_begin(c, scalar(a[1]), scalar(a[2]), scalar(a[3]), scalar(a[4]),
                                na > 5 ? (uint64_t)scalar(a[5]) : 0, na > 6 ? (int64_t)scalar(a[6]) : 0,
                                na > 7 ? (int)scalar(a[7]) : 20, home),
          "swrt_recycle_begin");
    return;
  }
  if (!strcmp(cmd, "recycle_apply")) {
    check(c, swrt_recycle_apply(c), "swrt_recycle_apply");
    return;
  }
  if (!strcmp(cmd, "recycle_frames")) {
    plhs[0] = mxCreateDoubleScalar((double)swrt_recycle_frames(c));
    return;
  }
  if (!strcmp(cmd, "recycle_get")) {  // -> stats 8 x frames (int64)
    const int64_t nf = swrt_recycle_frames(c);
    const mwSize dims[2] = {8, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(2, dims, mxINT64_CLASS, mxREAL);
    // (with no frame the call still runs: before begin it is an error)
    check(c, swrt_recycle_get(c, 0, nf, (int64_t*)mxGetInt64s(plhs[0])), "swrt_recycle_get");
    return;
  }
  if (!strcmp(cmd, "recycle_state")) {  // -> gen, born n x 1 (int64), original order
    const int64_t n = swrt_packets_count(c);
    std::vector<int32_t> gen((size_t)n), born((size_t)n);
    check(c, swrt_recycle_state(c, gen.data(), born.data()), "swrt_recycle_state");
    const mwSize dims[2] = {(mwSize)n, 1};
    plhs[0] = mxCreateNumericArray(2, dims, mxINT64_CLASS, mxREAL);
    mxArray* b = mxCreateNumericArray(2, dims, mxINT64_CLASS, mxREAL);
    int64_t *pg = (int64_t*)mxGetInt64s(plhs[0]), *pb = (int64_t*)mxGetInt64s(b);
    for (int64_t i = 0; i < n; ++i) pg[i] = gen[(size_t)i], pb[i] = born[(size_t)i];
    if (nlhs > 1) plhs[1] = b; else mxDestroyArray(b);
    return;
  }
  if (!strcmp(cmd, "recycle_reset")) {
    check(c, swrt_recycle_reset(c), "swrt_recycle_reset");
    return;
  }
  if (!strcmp(cmd, "recycle_end")) {
    check(c, swrt_recycle_end(c), "swrt_recycle_end");
    return;
  }
  if (!strcmp(cmd, "track_begin")) {  // (ids): 0-based original packet indices, as doubles
    need(na, 2, cmd);
    const double* v = reals(a[1], "ids");
    std::vector<int64_t> ids(mxGetNumberOfElements(a[1]));
    for (size_t i = 0; i < ids.size(); ++i) {
      if (!(v[i] >= -9.0e15 && v[i] <= 9.0e15) || (double)(int64_t)v[i] != v[i])
        mexErrMsgIdAndTxt("swrt:arg", "ids must be whole numbers");
      ids[i] = (int64_t)v[i];
    }
    check(c, swrt_track_begin(c, ids.data(), (int64_t)ids.size()), "swrt_track_begin");
    return;
  }
  if (!strcmp(cmd, "track_record")) {  // (f, gH, nslots, alpha, bump)
    need(na, 6, cmd);
    check(c, swrt_track_record(c, scalar(a[1]), scalar(a[2]), (int)scalar(a[3]), scalar(a[4]), scalar(a[5])),
          "swrt_track_record");
    return;
  }
  if (!strcmp(cmd, "track_record_history")) {  // (first, count, f, gH, nslots, alphas, bump): [] alphas = none
    need(na, 8, cmd);
    const int64_t count = (int64_t)scalar(a[2]);
    const size_t nal = mxGetNumberOfElements(a[6]);
    if (nal != 0 && (int64_t)nal != count) mexErrMsgIdAndTxt("swrt:arg", "alphas must hold one value per frame");
    check(c, swrt_track_record_history(c, (int64_t)scalar(a[1]), count, scalar(a[3]), scalar(a[4]), (int)scalar(a[5]),
                                       nal ? reals(a[6], "alphas") : nullptr, scalar(a[7])),
          "swrt_track_record_history");
    return;
  }
  if (!strcmp(cmd, "track_get")) {  // -> m x 8 x frames [x y k l Omega zeta sigma D]
    const int64_t nf = swrt_track_frames(c), m = swrt_track_count(c);
    const mwSize dims[3] = {(mwSize)m, 8, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    check(c, swrt_track_get(c, 0, nf, mxGetDoubles(plhs[0])), "swrt_track_get");
    return;
  }
  if (!strcmp(cmd, "track_reset")) {
    check(c, swrt_track_reset(c), "swrt_track_reset");
    return;
  }
  if (!strcmp(cmd, "flow_spectrum_begin")) {  // (nx, k_scale, K_d2)
    need(na, 4, cmd);
    check(c, swrt_flow_spectrum_begin(c, (int64_t)scalar(a[1]), scalar(a[2]), scalar(a[3])),
          "swrt_flow_spectrum_begin");
    return;
  }
  if (!strcmp(cmd, "flow_spectrum_record_qg")) {  // ([layer = 0]): 0-based layer of the QG state
    check(c, swrt_flow_spectrum_record_qg(c, na > 1 ? (int)scalar(a[1]) : 0), "swrt_flow_spectrum_record_qg");
    return;
  }
  if (!strcmp(cmd, "flow_spectrum_record_qk")) {  // (qk complex (2kmax+1) x (kmax+1), t)
    need(na, 3, cmd);
    const double* qk = complexes(a[1], "qk");
    const int64_t nx = (int64_t)mxGetM(a[1]) + 1;
    if ((int64_t)mxGetN(a[1]) * 2 != nx) mexErrMsgIdAndTxt("swrt:arg", "qk must be (2kmax+1) x (kmax+1)");
    check(c, swrt_flow_spectrum_record_qk(c, qk, nx, scalar(a[2])), "swrt_flow_spectrum_record_qk");
    return;
  }
  if (!strcmp(cmd, "flow_spectrum_frames")) {
    plhs[0] = mxCreateDoubleScalar((double)swrt_flow_spectrum_frames(c));
    return;
  }
  if (!strcmp(cmd, "flow_spectrum_shells")) {
    plhs[0] = mxCreateDoubleScalar((double)swrt_flow_spectrum_shells(c));
    return;
  }
  if (!strcmp(cmd, "flow_spectrum_get")) {  // -> spectra nshell x 3 x frames [E Z Q], stats 4 x frames [t; sums]
    const int64_t nf = swrt_flow_spectrum_frames(c), ns = swrt_flow_spectrum_shells(c);
    const mwSize dims[3] = {(mwSize)ns, 3, (mwSize)nf};
    plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    mxArray* stats = mxCreateDoubleMatrix(4, (mwSize)nf, mxREAL);
    if (nf > 0)
      check(c, swrt_flow_spectrum_get(c, 0, nf, mxGetDoubles(plhs[0]), mxGetDoubles(stats)), "swrt_flow_spectrum_get");
    if (nlhs > 1) plhs[1] = stats; else mxDestroyArray(stats);
    return;
  }
  if (!strcmp(cmd, "flow_spectrum_reset")) {
    check(c, swrt_flow_spectrum_reset(c), "swrt_flow_spectrum_reset");
    return;
  }
  mexErrMsgIdAndTxt("swrt:arg", "unknown command '%s'", cmd);
}
