/*
 * swrt.h — C ABI of the MI355X-native wave-packet ray-tracing hot path
 * (ndefilippis/SWRaytracing, qg_flow_ray_trace hot loop).
 *
 * The reference is MATLAB and has no native interface; each entry point below
 * names the MATLAB function (file:line, paths relative to the reference root)
 * whose behaviour it replaces.  A MEX gateway (matlab/swrt_mex.cpp) and the
 * Python ctypes front-end (swraytracing_amd/) bind exactly these symbols.
 *
 * Conventions
 *  - Every function returns an int status: SWRT_OK (0) or a SWRT_ERR_* code;
 *    swrt_last_error(ctx) returns a message for the last failure on ctx.
 *    No C++ exception or longjmp crosses this ABI.
 *  - Host buffers are caller-owned, fp64, MATLAB column-major, and are never
 *    retained after a call returns.  The context owns all device memory.
 *  - Packet arrays are N x 2 column-major: x(:,1) (all x) then x(:,2) (all y),
 *    the layout of packet_x / packet_k in qgsw_raytrace.m:54-55 and of one
 *    frame of packet_x.bin (write_field.m:38).
 *  - Gridded fields are nx x nx column-major, first index = x: F(ig, jg) at
 *    x = (ig-1)*dx, y = (jg-1)*dx (k2g.m / interpolate.m conventions).
 *  - One context per host thread; calls are synchronous with respect to the
 *    host (stream-ordered internally); not re-entrant on the same context.
 */
#ifndef SWRT_H
#define SWRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWRT_OK 0
#define SWRT_ERR_ARG 1   /* invalid argument (shape, slot, null pointer) */
#define SWRT_ERR_HIP 2   /* HIP runtime error */
#define SWRT_ERR_STATE 3 /* call out of order (e.g. field not set) */
#define SWRT_ERR_ALLOC 4 /* allocation failure */

#define SWRT_MAX_SLOTS 5 /* snapshot slots: 0 = flow1 / steady, 1 = flow2; 2..4 the later
                            snapshots of swrt_advance_intervals */

typedef struct swrt_ctx swrt_ctx;

/* ABI version (major*10000 + minor*100 + patch). */
int swrt_version(void);

/* Create a context bound to HIP device `device` (one process per GPU). */
int swrt_create(int device, swrt_ctx** out);
void swrt_destroy(swrt_ctx* ctx);
const char* swrt_last_error(const swrt_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Background flow (L1/L2: field preparation, once per snapshot)
 * ------------------------------------------------------------------------ */

/* Six gridded fields (u, v, u_x, u_y, v_x, v_y), each nx*nx column-major,
 * concatenated.  Replaces holding SpectralScheme.U_field / GradU_field
 * (SpectralScheme.m:29-35) or a grid_U output struct (grid_U.m:11-17).
 * ny_period: the y-period of interpolate.m's mod (interpolate.m:15,22): nx for
 * a single layer, nlayers*nx for the 2-layer call (qg2layersw_raytrace.m:187-188)
 * where F is nx x nx x 2 and only layer 1 is read.  0 means nx.
 * If v_y == -u_x bit for bit at every node (a streamfunction flow stored that
 * way) the slot is marked divergence-free and the packet kernels carry five
 * stencil sums instead of six (v_y's is the exact negation of u_x's), with
 * unchanged results. */
int swrt_set_field_grid(swrt_ctx* ctx, int slot, const double* fields6, int64_t nx, double L,
                        int64_t ny_period);

/* 1 if slot's v_y is exactly -u_x at every node (always so for fields the
 * library derives from psi / qk: it stores v_y as -u_x, see
 * swrt_set_field_psi), 0 if not, < 0 on error. */
int swrt_field_div_free(swrt_ctx* ctx, int slot);

/* SpectralScheme(L, nx, psi_field) constructor (SpectralScheme.m:6-36):
 * psik = g2k(psi); u = k2g(-i ky psik), v = k2g(i kx psik), gradients by
 * i kx / i ky; integer wavenumbers regardless of L.  FFTs run on the GPU.
 * The filtered psi grid k2g(g2k(psi)) is kept for swrt_get_psi_grid.
 * v_y is stored as -u_x (bit-exact negation): SpectralScheme.m / grid_U.m
 * transform i ky vk separately, which equals -(i kx uk) up to the FFT's
 * roundoff (the identity u_x + v_y = 0 of a streamfunction flow); the same
 * holds for swrt_set_field_qk and swrt_qg_snapshot. */
int swrt_set_field_psi(swrt_ctx* ctx, int slot, const double* psi_grid, int64_t nx, double L);

/* grid_U(qk, K_d2, K2, kx_, ky_, shear_strength) (grid_U.m:1-18) for one
 * layer: psik = -qk./(K_d2+K2), six derivative spectra, k2g on the GPU,
 * u += shear.  qk: (2kmax+1) x (kmax+1) complex, column-major, interleaved
 * (re, im) (MATLAB -R2018a interleaved complex).  k_scale multiplies the
 * integer wavenumbers (1 for qgsw_raytrace.m:19, 2*pi/L for
 * qg2layersw_raytrace.m:20-21).  ny_period as in swrt_set_field_grid. */
int swrt_set_field_qk(swrt_ctx* ctx, int slot, const double* qk_interleaved, int64_t nx, double L,
                      double K_d2, double shear, double k_scale, int64_t ny_period);

/* grid_U(g2k(q)) into `slot` from a gridded PV frame q (nx x nx fp64,
 * column-major): the stored-field consumer's read_field -> g2k -> grid_U
 * (symplectic_full_fourier.m:18-20, read_field.m:37-98, g2k.m:8-9,
 * grid_U.m:1-18) with both transforms on the device — the same result as
 * swrt_g2k followed by swrt_set_field_qk, without the spectrum's round
 * trip through host memory.  Arguments as swrt_set_field_qk. */
int swrt_set_field_q(swrt_ctx* ctx, int slot, const double* q_grid, int64_t nx, double L, double K_d2,
                     double shear, double k_scale, int64_t ny_period);

/* g2k(fg) (g2k.m:5-9): nx x nx real grid (column-major) -> the
 * (2kmax+1) x (kmax+1) half-plane spectrum fftshift(fft2(fg))/nx^2 cropped,
 * interleaved complex, column-major.  GPU FFT. */
int swrt_g2k(swrt_ctx* ctx, const double* fg, int64_t nx, double* fk_interleaved_out);
/* k2g(fk) (k2g.m:5-6 + fulspec.m): half-plane spectrum -> nx x nx real grid
 * nx^2*ifft2(ifftshift(fulspec(fk))) (real part), column-major.  GPU FFT. */
int swrt_k2g(swrt_ctx* ctx, const double* fk_interleaved, int64_t nx, double* fg_out);

/* Download slot's six fields (nx*nx column-major each) — for checks/plots. */
int swrt_get_field_grid(swrt_ctx* ctx, int slot, double* fields6_out);
/* Download the filtered psi grid of the last swrt_set_field_psi (nx*nx). */
int swrt_get_psi_grid(swrt_ctx* ctx, int slot, double* psi_out);

/* nx of the grid held by field slot `slot` (the size swrt_get_field_grid /
 * swrt_get_psi_grid write: 6 / 1 planes of nx x nx); -1 when the slot is
 * unset or the index is out of range.  Front-ends size their outputs from
 * this, never from a caller's argument. */
int64_t swrt_field_grid(const swrt_ctx* ctx, int slot);

/* ---------------------------------------------------------------------------
 * Point evaluation (L2 boundary API)
 * ------------------------------------------------------------------------ */

/* interpolate(x, y, F, dx, dy) (interpolate.m:1-50) of an arbitrary nx x nyF
 * grid field F (only the first nx columns are read when nyF > nx, as MATLAB's
 * 2-subscript F(ig,jg) does), with the given bump (1e-10:
 * qg_flow_ray_trace/interpolate.m:13; 1e-13: ray_trace_sw/interpolate.m:13). */
int swrt_interpolate(swrt_ctx* ctx, const double* F, int64_t nx, int64_t nyF, double dx, double dy,
                     double bump, const double* x, const double* y, int64_t n, double* out);

/* U and grad U at n points from the slot fields: out is 6 x n row-major
 * (u, v, u_x, u_y, v_x, v_y).  nslots = 1: slot 0 only (SpectralScheme.U /
 * grad_U, SpectralScheme.m:45-68).  nslots = 2: interpolate_U's blend
 * (1-alpha)*slot0 + alpha*slot1 (interpolate_U.m:5-23). */
int swrt_eval(swrt_ctx* ctx, const double* x, const double* y, int64_t n, int nslots, double alpha,
              double bump, double* out6);

/* ---------------------------------------------------------------------------
 * Packets and the fused symplectic integrator (L3)
 * ------------------------------------------------------------------------ */

/* Upload / download packet state (N x 2 column-major x and k). */
int swrt_packets_set(swrt_ctx* ctx, const double* x, const double* k, int64_t n);
int swrt_packets_get(swrt_ctx* ctx, double* x, double* k);
/* The same state in the original packet order into DEVICE buffers of this
 * context's GPU: x_dev[i + j*ld], k_dev[i + j*ld] (N x 2 column-major with
 * leading dimension ld >= N), enqueued on the packet stream (swrt_get_stream)
 * without a host synchronisation — the input of a device-side gather of
 * sharded trajectories (RCCL all_gather, swraytracing_amd/dist.py). */
int swrt_packets_get_device(swrt_ctx* ctx, double* x_dev, double* k_dev, int64_t ld);
int64_t swrt_packets_count(const swrt_ctx* ctx);

/* Locality tuning: the packets are kept counting-sorted by spatial tile
 * (tile x tile cells of slot 0's grid) and re-binned every `rebin_every`
 * steps (0 disables binning; tile 0 picks a size automatically).  Binning
 * changes only the device-side order: results, downloads and history frames
 * are identical and in the original packet order. */
int swrt_set_locality(swrt_ctx* ctx, int64_t rebin_every, int64_t tile);

/* Packet-kernel variant (same results, bit for bit): 0 = automatic (the
 * LDS-tiled kernel whenever binning is on and nx >= 32), 1 = one lane per
 * packet gathering from the global node array, 2 = LDS-tiled kernel (16x16-
 * cell tiles, field window staged in LDS, in-tile cell sort). */
int swrt_set_kernel(swrt_ctx* ctx, int variant);

/* Opt-in stencil arithmetic of the LDS-tiled packet kernel for fields with
 * v_y == -u_x (every field the library derives from psi / qk): 1 = each
 * tap's wij*F added by one fused multiply-add (and the snapshot blend as
 * (1-alpha)*I1 + alpha*I2 with one FMA), which drops ~350 of the ~1,100 VALU
 * instructions of a packet-step; the sums keep interpolate.m:43-49's order
 * but round once per tap instead of twice, so results agree with the
 * reference to tolerance (per step ~1e-15 relative), not bit for bit.
 * 0 (default) = mul then add, bit-identical to the reference's arithmetic.
 * Other kernels (host-given six-field windows, the per-packet kernel, ode23,
 * xka) always use mul then add. */
int swrt_set_gather_mode(swrt_ctx* ctx, int mode);

/* Launch shape of the LDS-tiled two-snapshot launches (fields with v_y ==
 * -u_x) when tiles hold few packets: 256-thread workgroups with a 256-VGPR
 * budget whose stencil gather issues each tap's LDS reads three taps ahead
 * (instead of 512 threads, 128 VGPRs, one tap ahead), so the one busy wave a
 * SIMD has at ~120 packets per tile waits less on the LDS.  0 (default) =
 * below SWRT_SPARSE_BELOW packets per 16x16 tile on average (build default
 * 192: the 8-GPU shard of the 1e6 bench, whose driver step it shortens by
 * 2.5 % beside the PDE), 1 = never, 2 = always.  Same arithmetic in the same
 * order: bit-identical for any setting. */
int swrt_set_sparse_tiles(swrt_ctx* ctx, int mode);

/* The packet step of swrt_advance, swrt_advance_intervals and swrt_leapfrog.
 *
 * The reference's step (ode_symplectic.m:13-37) is drift dt/2, kick dt, drift
 * dt/2, and its kick phi2 (ode_symplectic.m:18-21) moves x by dt*U(x1) and k
 * by -dt*(grad U(x1))^T k1: one explicit Euler step of the sub-flow of
 * H2 = U(x).k.  That sub-flow is not integrable, so the Euler step is neither
 * its exact flow nor symmetric, and the splitting around it is FIRST order
 * (the conserved frequency drifts as O(dt)), whatever the file names of the
 * reference's error plots say.  Its yoshida (ode_symplectic.m:39-53) computes
 * triple-jump weights and never applies them (and its w0 lacks the minus
 * sign that makes 2*w1 + w0 = 1).
 *
 *   kick 0 (default)  the reference's Euler kick.                   Order 1.
 *   kick 1            the implicit midpoint rule of the same sub-flow:
 *                     xm = x1 + (h/2)*U(xm) by `iterations` (1..4) fixed-
 *                     point passes from xm = x1 (each one gather of u and
 *                     v), U and grad U once at xm, x2 = x1 + h*U, and
 *                     (1 + (h/2)A) k2 = (1 - (h/2)A) k1, A = (grad U)^T,
 *                     by Cramer's rule.  Symmetric.                 Order 2.
 *   composition 0     one stage of size dt.
 *   composition 1     Yoshida's triple jump, stage sizes w*dt with
 *                     w = {w1, 1 - 2*w1, w1}, w1 = 1/(2 - 2^(1/3)).
 *                     Over kick 1: order 4.  Over kick 0 (a base that is
 *                     not symmetric): order 1, worse than the plain step.
 *   composition 2     Suzuki's five stages, w = {s, s, 1 - 4*s, s, s},
 *                     s = 1/(4 - 4^(1/3)).  Over kick 1: order 4.
 *
 * A stage is drift(h/2), kick(h), drift(h/2) with its own blend value
 * a_j = (alpha0 + s*dalpha) + off_j*dalpha (the stage's midpoint within the
 * step), so a composite step is, bit for bit, its stages as single-step
 * swrt_advance(w_j*dt, 1, .., alpha0 = a_j, dalpha = 0, ..) calls under the
 * same kick.  History frames, save_every and the re-binning cadence count
 * composite steps.  iterations is ignored for kick 0.  The default is
 * (0, 1, 0): the reference's arithmetic, bit for bit.  Setting it does not
 * invalidate the binning.  A non-default integrator with
 * swrt_set_gather_mode(1) makes the advance calls fail with SWRT_ERR_ARG: the
 * FMA gather has the leapfrog step only.  ode23, xka and
 * swrt_spectral_leapfrog are not affected. */
int swrt_set_integrator(swrt_ctx* ctx, int kick, int iterations, int composition);
int swrt_get_integrator(const swrt_ctx* ctx, int* kick, int* iterations, int* composition);

/* The stage weights and blend offsets of a composition (0, 1 or 2), as the
 * exact doubles the device uses: w5[0..nstages-1], off5[0..nstages-1] (the
 * rest 0).  No context and no GPU call. */
int swrt_integrator_weights(int composition, double* w5, double* off5, int* nstages);

/* Packet streams of the LDS-tiled leapfrog: 2 (default) or 1.  With 2 every
 * launch runs as two part launches — the even and the odd band positions of
 * each XCD band's tiles (the mapping: swraytracing_amd/csrc/swrt_share.hpp)
 * — on the context's packet stream and a second stream.
 * Between re-binnings the parts advance disjoint packet ranges, so one
 * stream's launch k overlaps the other's launch k+1: one part's tail runs
 * under the other's body instead of leaving CUs idle at every launch
 * boundary.  The launch after a re-binning's sort launch (which gathers its
 * input from any slot) and any call that reads the packets (or re-bins them)
 * first order the second stream's work before their own; swrt_synchronize
 * waits for both.  Results are bit-identical for either setting.  Ensembles
 * under 65,536 packets always use one stream (the split costs more than it
 * returns there). */
int swrt_set_packet_streams(swrt_ctx* ctx, int streams);

/* Advance the device-resident packets by nsteps leapfrog steps
 * (ode_symplectic.m:13-37: drift dt/2 with gH*k/omega, kick dt with U(x1)
 * and (grad U(x1))^T k1 (RaytracingScheme.m:9-16), drift dt/2).  The kick of
 * step s uses alpha = alpha0 + s*dalpha when nslots == 2.  bump: Lagrange
 * bump.  If save_every > 0 a frame (N x 2 x, then N x 2 k) is recorded on the
 * device after every save_every steps (frames appended to the history
 * buffer, see swrt_history_*). */
int swrt_advance(swrt_ctx* ctx, double dt, int64_t nsteps, double f, double gH, int nslots,
                 double alpha0, double dalpha, double bump, int64_t save_every);

/* nintervals consecutive PDE intervals in one call: interval i advances the
 * packets nsub leapfrog steps of size dts[i], blending slots i and i+1 with
 * alpha = alpha0 + s*dalpha (s = step within the interval) — exactly
 * nintervals swrt_advance(dts[i], nsub, ..., nslots 2) calls with slots
 * (i, i+1) moved to (0, 1) in turn, bit for bit.  Slots 0..nintervals must
 * be set on one grid; nintervals <= SWRT_MAX_SLOTS - 1; save_every (0 = no
 * history) divides nsub.  With the LDS-tiled kernel and re-binning every
 * multiple of nsub steps, up to 4 intervals run in ONE launch (each
 * workgroup re-stages its window between them), so the launch's tail and the
 * in-tile sort are paid once per 4 intervals instead of once per interval.
 * (The drivers' packet branch over several PDE steps: qgsw_raytrace.m:140-151,
 * qg2layersw_raytrace.m:185-197 with the snapshots of the PDE run ahead.) */
int swrt_advance_intervals(swrt_ctx* ctx, int nintervals, const double* dts, int64_t nsub, double f, double gH,
                           double alpha0, double dalpha, double bump, int64_t save_every);

/* History frames recorded by swrt_advance since the last swrt_history_reset. */
int64_t swrt_history_frames(const swrt_ctx* ctx);
int swrt_history_get(swrt_ctx* ctx, int64_t first, int64_t count, double* hist_x, double* hist_k);
int swrt_history_reset(swrt_ctx* ctx);

/* Host convenience = packets_set + advance + packets_get (+ history): the
 * drop-in for ode_symplectic(x0,k0,dt,T,f,gH,scheme) (ode_symplectic.m:1-31).
 * hist_x / hist_k may be NULL; otherwise they receive nsteps/save_every frames
 * of N x 2 each. */
int swrt_leapfrog(swrt_ctx* ctx, double* x, double* k, int64_t n, double dt, int64_t nsteps,
                  double f, double gH, int nslots, double alpha0, double dalpha, double bump,
                  int64_t save_every, double* hist_x, double* hist_k);

/* ---------------------------------------------------------------------------
 * Wave-action packets over an RSW background (ray_trace_sw/step_packet_xka.m)
 * ------------------------------------------------------------------------ */

/* Background of step_packet_xka(P, U, GradU, H, C0, f, dx, dy, dt)
 * (step_packet_xka.m:1): seven nx x nx column-major planes concatenated in the
 * order U.u, U.v, GradU.u_x, GradU.u_y, GradU.v_x, GradU.v_y, H. */
int swrt_xka_set_fields(swrt_ctx* ctx, const double* fields7, int64_t nx, double dx, double dy);

/* The same background built on the GPU from an RSW state, as
 * ray_trace_sw/raytrace_sw.m:16-52 does: state3 = S(:,:,1:3) = [u v eta]
 * (nx x nx x 3 column-major, :12), g2k of each (:26-28), the geostrophic
 * projection etagk = (f*etak - zetak).*f./(f^2 + gH0*K2) with gH0 = Cg^2
 * (:22-31), ug/vg and their i*k gradients (:34-41), seven k2g and
 * H = 1 + etag (:44-52).  Integer wavenumbers (L = 2*pi, :84); L sets
 * dx = dy = L/nx.  nx a power of two. */
int swrt_xka_set_rsw(swrt_ctx* ctx, const double* state3, int64_t nx, double f, double Cg, double L);

/* Download the current xka background as the seven planes of
 * swrt_xka_set_fields (U.u, U.v, GradU.u_x, u_y, v_x, v_y, H); nx x nx each
 * with nx = swrt_xka_grid(ctx). */
int swrt_xka_get_fields(swrt_ctx* ctx, double* fields7_out);
int64_t swrt_xka_grid(const swrt_ctx* ctx);

/* nsteps of Pout = step_packet_xka(P, ...) for n packets (step_packet_xka.m:
 * 38-91 with cg_sw.m:15-32 evaluated per stencil tap; interpolate of
 * ray_trace_sw, bump 1e-13).  state5 (in/out): n x 5 column-major
 * [P.x P.y P.k P.l P.a].  hist5 (may be NULL): nsteps/save_every frames of
 * n x 5 after every save_every steps. */
int swrt_xka_step(swrt_ctx* ctx, double* state5, int64_t n, double C0, double f, double dt,
                  int64_t nsteps, int64_t save_every, double* hist5);

/* ---------------------------------------------------------------------------
 * Exact spectral evaluator (scratch/fourier_interpolate_test.m:92-136)
 * ------------------------------------------------------------------------ */

/* psi(x,y) = sum_{i,j} Re(C[i,j] exp(1i*(kx_i x + ky_j y))), kx_i = (kx0+i)*s,
 * ky_j = (ky0+j)*s; C nkx x nky column-major interleaved complex.  The
 * half-plane spectrum of g2k maps to C = 2*psik (ky = 0, kx < 0 zeroed, DC
 * real, kx0 = -kmax, ky0 = 0); the scratch test's amp/phase field to
 * C = amp.*exp(1i*phase) (kx0 = ky0 = -n, s = 1). */
int swrt_spectral_set_modes(swrt_ctx* ctx, const double* C_interleaved, int64_t nkx, int64_t nky,
                            double kx0, double ky0, double s);
/* Exact U and grad U (6 x n, as swrt_eval) by the direct mode sum;
 * precision 64 (fp64) or 32 (fp32 sums, the config-5 tolerance study). */
int swrt_spectral_eval(swrt_ctx* ctx, const double* x, const double* y, int64_t n, int precision,
                       double* out6);
/* Leapfrog (ode_symplectic.m:13-37) with the exact spectral kick
 * (fourier_interpolate_test.m:73-114); x, k N x 2 column-major, in/out. */
int swrt_spectral_leapfrog(swrt_ctx* ctx, double* x, double* k, int64_t n, double dt, int64_t nsteps,
                           double f, double gH, int precision);

/* ---------------------------------------------------------------------------
 * Diagnostics (analysis/load_data.m)
 * ------------------------------------------------------------------------ */

/* Energy-vs-omega input of load_data.m:33-52 for the device-resident packets:
 * omega = sqrt(f^2 + Cg^2*|k|^2) per packet, histcounts over `edges`
 * (nbins + 1 increasing values; last bin closed) ADDED to counts_inout (so a
 * window of frames accumulates), and the ensemble mean omega of this frame
 * (load_data.m:63; deterministic block-ordered sum). */
int swrt_omega_histogram(swrt_ctx* ctx, double f, double Cg, const double* edges, int64_t nbins,
                         int64_t* counts_inout, double* mean_omega_out);

/* The energy-vs-omega series of a run, kept on the device: what load_data.m
 * computes from every saved packet frame (load_data.m:33-52,63), without the
 * frames.  omega = sqrt(f^2 + Cg^2*(k*k + l*l)) in that operation order, as
 * swrt_omega_histogram.  A frame is
 *   a row of nbins + 2 int64 counts [below, bin 0 .. bin nbins-1, above]:
 *     bin i holds edges[i] <= omega < edges[i+1], the last bin also omega ==
 *     edges[nbins] (histcounts, load_data.m:47); below counts omega <
 *     edges[0], above omega > edges[nbins]; a NaN omega is counted nowhere, so
 *     n - sum(row) is the number of NaN packets;
 *   four doubles [n, sum omega, min omega, max omega]: the mean of
 *     load_data.m:63 and the value load_data.m:39 builds its edges from.  min
 *     and max ignore NaN (+inf and -inf if there is nothing else); the sum is
 *     a plain sum.
 * A frame depends on the packets alone: counts, min and max by nature, and
 * the sum runs over the original packet index (the set's perm; per-workgroup
 * partials of a fixed grid, combined in an order their number fixes).  Two
 * contexts holding the same packets, a re-binning between two records, or
 * swrt_advance against swrt_advance_intervals all give the same bits.  Frames
 * are self-contained: swrt_packets_set with another N keeps the series. */

/* Open a series: 1 <= nbins <= 4096, nbins + 1 finite increasing edges
 * (SWRT_ERR_ARG otherwise).  Uploads the edges, keeps f^2 and Cg^2, empties
 * the series.  The edges of load_data.m:39-40. */
int swrt_omega_series_begin(swrt_ctx* ctx, double f, double Cg, const double* edges, int64_t nbins);

/* Append the frame of the current packets (one iteration of load_data.m:44-50
 * with a window of one frame): queued on the packet stream after whatever last
 * wrote the packets (both packet streams, the ode23 attempts); the host does
 * not wait.  Reads no field slot.  Capacity: 4096 frames, doubled when full,
 * and only a growing call may wait for the stream.  SWRT_ERR_STATE before
 * swrt_omega_series_begin, SWRT_ERR_ARG without packets. */
int swrt_omega_series_record(swrt_ctx* ctx);

/* One frame per history frame in [first, first + count) (the frames of
 * swrt_advance(save_every) or swrt_ode23_run_at): load_data.m:33's omega of
 * the stored frames without a download.  The same bits as
 * swrt_omega_series_record on packets set to that frame.  A range out of
 * bounds: SWRT_ERR_ARG. */
int swrt_omega_series_record_history(swrt_ctx* ctx, int64_t first, int64_t count);

/* Frames recorded since begin or the last reset (the frame count of
 * load_data.m:32); nbins of the open series, 0 if none. */
int64_t swrt_omega_series_frames(const swrt_ctx* ctx);
int64_t swrt_omega_series_bins(const swrt_ctx* ctx);

/* Frames [first, first + count): counts_out count x (nbins + 2) and stats4_out
 * count x 4 (may be NULL), frame-major.  Waits for them.  The rows
 * load_data.m:45-49 sums over its window, and load_data.m:63's sum and n. */
int swrt_omega_series_get(swrt_ctx* ctx, int64_t first, int64_t count, int64_t* counts_out,
                          double* stats4_out);

/* Empty the series; f, Cg and the edges stay (load_data.m:44, a new window). */
int swrt_omega_series_reset(swrt_ctx* ctx);

/* ideal_omega_distribution.m:3-11: Omega = omega0 + (u_g*kx_j + v_g*ky_j), in
 * that operation order, for every node g of slot's nx x nx grid (layer 1 of a
 * slot with a 2*nx y-period) and every ring vector j, binned into counts_out
 * [below, bins, above] (nbins + 2) over `edges` by the rule above: nx^2*m
 * samples.  ring_k: m x 2 column-major, k_0*[cos t, sin t]
 * (ideal_omega_distribution.m:3-5); omega0 = sqrt(f^2 + Cg^2*k_0^2) (:9).
 * Synchronous.  An unset slot, m < 1 or bad edges: SWRT_ERR_ARG. */
int swrt_omega_ideal(swrt_ctx* ctx, int slot, const double* ring_k, int64_t m, double omega0,
                     const double* edges, int64_t nbins, int64_t* counts_out);

/* The packet density and wave-energy maps of a run, kept on the device: where
 * the ensemble sits, which generate_image.m:9-34 and raytracing_figures.m:6-24
 * draw packet by packet.  The map has m x m cells over the periodic square of
 * side L.  The cell of a packet is interpolate.m:21-31's with dxm = L/m:
 * i = floor(mod(x/dxm, m)), then i mod m (mod may round up to m), the same for
 * y; cell (i, j) covers x in [i*dxm, (i+1)*dxm) and sits at plane[i + m*j]
 * (first index x, column-major: with m = nx the layout of a pv.bin frame).
 * Every packet has three moments, omega = sqrt(f^2 + Cg^2*(k*k + l*l)) in
 * load_data.m:33's operation order, k and l, each quantised once per packet:
 * q = rint(v * 2^frac_bits), round half even.  A packet is rejected — it adds
 * to no cell — when x, y, k, l or omega is not finite or any
 * |v * 2^frac_bits| >= 2^38.  A frame is
 *   four m x m planes of int64 [count, sum q(omega), sum q(k), sum q(l)];
 *   two int64 stats [n, rejected].
 * With n <= 2^24 every sum stays below 2^62: integer addition is exact and
 * order-free, so a frame is a function of the packet set alone (not of the
 * storage order, the binning, the launch shape or a shard split), and the
 * frame of a sharded ensemble is the element-wise sum of the shards' frames.
 * Energy per cell at unit action per packet (load_data.m:49) is
 * sum q(omega) * 2^-frac_bits; the mean wavevector sum q(k) / count *
 * 2^-frac_bits. */

/* Open a series: 1 <= m <= 4096, L > 0, 0 <= frac_bits <= 32, at most 2^24
 * packets set (SWRT_ERR_ARG otherwise).  Empties the series. */
int swrt_map_series_begin(swrt_ctx* ctx, double L, int64_t m, double f, double Cg, int frac_bits);

/* Append the frame of the current packets: queued on the packet stream after
 * whatever last wrote the packets (both packet streams, the ode23 attempts);
 * the host does not wait.  Capacity: 64 MiB of frames (at least one, at most
 * 4096), doubled when full; only a growing call may wait for the stream, and
 * a failed allocation is an error return.  When the packets are binned for
 * the LDS tile kernel, L is slot 0's and a map cell is c x c field cells with
 * c dividing the tile side, one workgroup per tile accumulates in LDS; any
 * other case adds per packet through global memory: the same integers.
 * SWRT_ERR_STATE before swrt_map_series_begin, SWRT_ERR_ARG without packets
 * or with more than 2^24. */
int swrt_map_series_record(swrt_ctx* ctx);

/* One frame per history frame in [first, first + count): the same bits as
 * swrt_map_series_record on packets set to that frame.  A range out of
 * bounds: SWRT_ERR_ARG. */
int swrt_map_series_record_history(swrt_ctx* ctx, int64_t first, int64_t count);

/* Frames recorded since begin or the last reset; m of the open series, 0 if none. */
int64_t swrt_map_series_frames(const swrt_ctx* ctx);
int64_t swrt_map_series_cells(const swrt_ctx* ctx);

/* Frames [first, first + count): planes4_out count x 4 x m x m and stats2_out
 * count x 2 (may be NULL), frame-major.  Waits for them. */
int swrt_map_series_get(swrt_ctx* ctx, int64_t first, int64_t count, int64_t* planes4_out,
                        int64_t* stats2_out);

/* Empty the series; L, m, f, Cg and frac_bits stay. */
int swrt_map_series_reset(swrt_ctx* ctx);

/* The wave-vector plane of a run, kept on the device: the density of the
 * ensemble over (k, l) and the moments of the wavevector, which
 * raytracing_figures.m:19-26,76-83, SW_zero_background_raytracing.m:103-104
 * and qgflow_animation.m:59-63 draw packet by packet.  The plane has m x m
 * cells over [-K, K) in both components; the host computes s = m / (2.0*K)
 * once, in double.  A record reads only the packets' k and l: no positions and
 * no field slot.  Every packet has five values in this operation order, k, l,
 * k*k, l*l, k*l (each product one double multiplication), each quantised once
 * per packet: q = rint(v * 2^frac_bits), round half even.  A packet is
 * rejected when k or l is not finite or any |v * 2^frac_bits| >= 2^38; it then
 * adds to nothing but `rejected`.  A packet is inside iff -K <= k < K and
 * -K <= l < K, tested on k and l themselves; its index is
 * i = min((int)floor((k + K) * s), m - 1) (one add, then one multiply, never
 * contracted; the product can round up to exactly m for the last double below
 * K), j the same for l, and cell (i, j) sits at plane[i + m*j] (first index
 * k).  A packet that is not rejected but not inside counts as `outside` and
 * still adds to the moments.  A frame is
 *   one m x m plane of int64 counts;
 *   eight int64 stats [n, rejected, outside, sum q(k), sum q(l), sum q(k*k),
 *   sum q(l*l), sum q(k*l)].
 * With n <= 2^24 every sum stays below 2^62: integer addition is exact and
 * order-free, so a frame is a function of the packet set alone (not of the
 * storage order, the binning, the launch shape or a shard split), and the
 * frame of a sharded ensemble is the element-wise sum of the shards' frames.
 * Negative sums wrap in two's complement and are read back as int64.  With
 * n_used = n - rejected the mean wavevector is sum q(k) / n_used *
 * 2^-frac_bits, and the covariance follows from the second moments. */

/* Open a series: K > 0 finite, 1 <= m <= 4096, 0 <= frac_bits <= 32, at most
 * 2^24 packets set (SWRT_ERR_ARG with a message otherwise).  Empties the
 * series. */
int swrt_kmap_series_begin(swrt_ctx* ctx, double K, int64_t m, int frac_bits);

/* Append the frame of the current packets: queued on the packet stream after
 * whatever last wrote the packets (both packet streams, the ode23 attempts, a
 * re-binning's parked set); the host does not wait.  Capacity: 64 MiB of
 * frames (at least one, at most 4096), doubled when full; only a growing call
 * may wait for the stream, and a failed allocation is an error return.  Up to
 * m = 128 every workgroup counts into a private plane in LDS and adds its
 * non-zero cells to the frame; beyond, every packet adds through global
 * memory: the same integers.  SWRT_ERR_STATE before swrt_kmap_series_begin,
 * SWRT_ERR_ARG without packets or with more than 2^24. */
int swrt_kmap_series_record(swrt_ctx* ctx);

/* One frame per history frame in [first, first + count): the same bits as
 * swrt_kmap_series_record on packets set to that frame.  A range out of
 * bounds: SWRT_ERR_ARG. */
int swrt_kmap_series_record_history(swrt_ctx* ctx, int64_t first, int64_t count);

/* Frames recorded since begin or the last reset; m of the open series, 0 if none. */
int64_t swrt_kmap_series_frames(const swrt_ctx* ctx);
int64_t swrt_kmap_series_cells(const swrt_ctx* ctx);

/* Frames [first, first + count): plane_out count x m x m and stats8_out
 * count x 8, frame-major.  Either may be NULL, not both (SWRT_ERR_ARG).
 * Waits for the frames. */
int swrt_kmap_series_get(swrt_ctx* ctx, int64_t first, int64_t count, int64_t* plane_out,
                         int64_t* stats8_out);

/* Empty the series; K, m and frac_bits stay. */
int swrt_kmap_series_reset(swrt_ctx* ctx);

/* The trajectories of a chosen few packets, kept on the device: what
 * images/QG_spread*.png, the (k, l) paths of raytracing_figures.m:76-83 and
 * the Omega time series draw per packet, and analysis/load_data.m:29-33 reads
 * as packet_x.bin / packet_k.bin, for m packets out of an ensemble too large
 * to download every frame.  A frame is m x 8 doubles, column-major: row j is
 * packet ids[j], in the order the ids were given, the columns
 *   [x, y, k, l, Omega, zeta, sigma, D].
 * x, y, k, l are the bits swrt_packets_get returns for that packet (positions
 * unwrapped).  Omega, zeta, sigma and D are the bits swrt_raydiag_sample's
 * sample4_out holds for it with the same (f, gH, nslots, alpha, bump): the
 * formulas and operation order of the ray-diagnostics section below, through
 * the same device code.  With nslots == 0 no flow is read and columns 4..7
 * hold the quiet NaN 0x7ff8000000000000. */

/* Name the packets to track by their original index: 1 <= m <= N, m <= 2^20,
 * 0 <= ids[j] < N, all distinct, ids not NULL, packets set (SWRT_ERR_ARG with
 * a message otherwise).  Empties the series and writes the N-entry device
 * table the records look the ids up in; waits for the stream.
 * swrt_packets_set with a different N closes the series (the ids name packets
 * of the old ensemble); the same N keeps it. */
int swrt_track_begin(swrt_ctx* ctx, const int64_t* ids, int64_t m);

/* Append the frame of the current state: queued on the packet stream after
 * whatever last wrote the packets (both packet streams, the ode23 attempts, a
 * re-binning's parked set) and after the snapshot writes of the slots it
 * reads; the host does not wait.  nslots is 0, 1 or 2; with 1 or 2 the checks
 * of swrt_raydiag_record apply.  One lane per stored packet finds the tracked
 * ones through the table: 8 bytes read per packet, then m gathers.  Capacity:
 * 64 MiB of frames (at least one, at most 4096), doubled when full; only a
 * growing call may wait for the stream, and a failed allocation is an error
 * return.  SWRT_ERR_STATE before swrt_track_begin. */
int swrt_track_record(swrt_ctx* ctx, double f, double gH, int nslots, double alpha, double bump);

/* One frame per history frame in [first, first + count), frame i with the
 * snapshot blend alphas[i] (alphas may be NULL when nslots < 2): the same
 * bits as swrt_track_record on packets set to that frame.  A range out of
 * bounds: SWRT_ERR_ARG. */
int swrt_track_record_history(swrt_ctx* ctx, int64_t first, int64_t count, double f, double gH, int nslots,
                              const double* alphas, double bump);

/* Frames recorded since begin or the last reset; m of the open series, 0 if
 * none; its ids into ids_out (m values; SWRT_ERR_STATE if none is open). */
int64_t swrt_track_frames(const swrt_ctx* ctx);
int64_t swrt_track_count(const swrt_ctx* ctx);
int swrt_track_ids(const swrt_ctx* ctx, int64_t* ids_out);

/* Frames [first, first + count) into frames_out: count x 8 x m, frame-major
 * (each frame m x 8 column-major).  Waits for them. */
int swrt_track_get(swrt_ctx* ctx, int64_t first, int64_t count, double* frames_out);

/* Empty the series; the ids stay. */
int swrt_track_reset(swrt_ctx* ctx);

/* The background flow's shell spectra, kept on the device: what the
 * reference's analysis computes from a PV frame (scratch/energy_spectrum.m:3-13:
 * psik = -qk./(K_d2 + K2), KE = K2.*|psik|^2 summed over the shells
 * (j - 1/2)^2 <= K^2 < (j + 1/2)^2; rsw/isospectrum.m:14-21 writes the rule
 * floor(K + .5) == j), from one layer's spectral PV, at the packet frames'
 * times and without a download.  The one series on the PDE side: its work runs
 * on the QG stream (the context's stream when swrt_qg_set_stream(ctx, 0)).
 *
 * Geometry.  nx is a power of two, kmax = nx/2 - 1; the half plane is
 * kx in [-kmax, kmax], ky in [0, kmax]; k_scale = 2*pi/L as a double (the
 * one-layer model passes exactly 1); K_d2 >= 0.
 * Shell.  The shell of (kx, ky) is the integer j >= 0 with
 * (2j-1)^2 <= 4(kx^2 + ky^2) < (2j+1)^2, and j = 0 for the mean mode alone:
 * floor(K + .5) on index wavenumbers, in integers.  nshell =
 * shell(kmax, kmax) + 1 (11 at nx = 16, 45 at 64, 362 at 512): the corner
 * shells beyond kmax are kept.
 * Modes.  Those with ky = 0 and kx < 0 are skipped, whatever they hold
 * (fulspec.m:16 overwrites them).  The mean mode has weight w = 0.5, every
 * other w = 1: a shell sum is half the full-plane sum.
 * Per mode, every operation one IEEE double operation, never contracted, in
 * the order of grid_U's inversion:
 *   kxs = (double)kx * k_scale;  kys = (double)ky * k_scale
 *   K2  = kxs*kxs + kys*kys
 *   den = K_d2 + K2
 *   pr  = -qr/den;  pi = -qi/den          (both 0 when den == 0)
 *   a   = pr*pr + pi*pi
 *   E   = w * (K2 * a)
 *   Z   = w * ((K2*K2) * a)
 *   Q   = w * (qr*qr + qi*qi)
 * Summation.  For each quantity and shell there are nx slots: slot kx + kmax
 * holds the sum of row kx's modes in that shell, in ascending ky from +0.0;
 * slots 2kmax+1 .. nx-1 are +0.0.  The slots are folded by halving: for
 * h = nx/2, nx/4, ..., 1, P[i] = P[i] + P[i+h] for i < h; the shell's value
 * is P[0].  A frame is
 *   3 x nshell doubles [E(0..J), Z(0..J), Q(0..J)];
 *   four stats doubles [t, sum E, sum Z, sum Q], each total summed in
 *   ascending j from +0.0.
 * The order is defined on (kx, ky), not on memory: a frame is a function of
 * the values of qk alone.  sum E = mean(u^2 + v^2)/2 of grid_U's velocity
 * without the shear offset, sum Z = mean((v_x - u_y)^2)/2, sum Q =
 * mean(q^2)/2 with q = k2g(qk), the mean included.  The two-layer PDE's own
 * inversion (the B matrix; barotropic and baroclinic energies) is not
 * computed: every layer goes through the one-layer inversion above, which is
 * what the packets' snapshots use. */

/* Open a series and empty it.  SWRT_ERR_ARG with a message unless nx is a
 * power of two in 8..4096 (swrt_qg_init's range), k_scale positive and finite,
 * K_d2 finite and >= 0.  Waits for the series' stream. */
int swrt_flow_spectrum_begin(swrt_ctx* ctx, int64_t nx, double k_scale, double K_d2);

/* Append the frame of layer `layer` of the QG state's committed current qk
 * (swrt_qg_export's view: a pending speculative step is neither waited for
 * nor included), t the state's model time: queued on the QG stream behind the
 * step that made that qk; the host does not wait and no packet launch does.
 * One workgroup per shell gathers the shell's modes, each read once; nothing
 * is added through memory.  Capacity: 64 MiB of frames (at least one, at most
 * 4096), doubled when full; only a growing call may wait for the stream, and
 * a failed allocation is an error return.  SWRT_ERR_STATE before
 * swrt_flow_spectrum_begin, before swrt_qg_init, or when the state's nx
 * differs from the series'; SWRT_ERR_ARG for a layer the state does not have. */
int swrt_flow_spectrum_record_qg(swrt_ctx* ctx, int layer);

/* The same from a host half plane in swrt_set_field_qk's layout (column-major
 * (2kmax+1) x (kmax+1), kx fastest, interleaved complex), stamped with t: the
 * bits swrt_flow_spectrum_record_qg gives for the same values.  Returns once
 * the plane is copied (qk_interleaved is free); the frame itself is queued.
 * SWRT_ERR_STATE before begin or when nx differs from the series'. */
int swrt_flow_spectrum_record_qk(swrt_ctx* ctx, const double* qk_interleaved, int64_t nx, double t);

/* Frames recorded since begin or the last reset; nshell of the open series, 0 if none. */
int64_t swrt_flow_spectrum_frames(const swrt_ctx* ctx);
int64_t swrt_flow_spectrum_shells(const swrt_ctx* ctx);

/* Frames [first, first + count): spectra_out count x 3 x nshell and stats4_out
 * count x 4, frame-major.  Either may be NULL, not both (SWRT_ERR_ARG).  Waits
 * for the series' stream up to these frames, never for the packet streams. */
int swrt_flow_spectrum_get(swrt_ctx* ctx, int64_t first, int64_t count, double* spectra_out, double* stats4_out);

/* Empty the series; nx, k_scale and K_d2 stay. */
int swrt_flow_spectrum_reset(swrt_ctx* ctx);

/* ---------------------------------------------------------------------------
 * The conditional spectrum series: the energy-vs-omega distribution of the
 * packets (analysis/load_data.m:33-52) split by a scalar of the flow at each
 * packet (RaytracingScheme.m:18-31), kept on the device as integers.
 *
 * Per packet, with which = 0 (zeta), 1 (sigma) or 2 (D):
 *   omega = sqrt(f^2 + Cg^2 (k k + l l)), the operation order of the spectrum
 *           series (load_data.m:33);
 *   q     = that scalar, the bits swrt_raydiag_sample returns for the same
 *           (nslots, alpha, bump).
 * The omega class is the spectrum series' rule over omega_edges (a row
 * [below, bin 0 .. bin nw-1, above], the last bin closed); the q class is the
 * same rule over q_edges with nq bins.  A frame holds
 *   counts  (nq + 2) x (nw + 2) int64, q class major: counts[qc * (nw + 2) + wc];
 *   sums    nq + 2 int64: per q class the sum of rint(omega * 2^frac_bits)
 *           (round half even) over the packets counted there, so that
 *           sums / counts is the conditional mean omega, exact to the quantum;
 *   stats   2 int64 [n, rejected].
 * A packet whose omega or q is NaN, or with |omega * 2^frac_bits| >= 2^38, is
 * rejected and counted nowhere: the counts of a frame sum to n - rejected.
 * The marginal over the q classes is the spectrum series' row of the accepted
 * packets.  Integer addition is exact and order-free: a frame depends on the
 * packet set alone (two contexts, a re-binning between two records, either
 * advance call and either packet-stream setting give the same bits), and the
 * frames of shards combine by adding.  Positions must be finite, as for every
 * gather of the library.
 * ------------------------------------------------------------------------- */

/* Open a series: 1 <= nw, nq <= 4096 with (nq + 2) * (nw + 2) <= 65536 cells
 * (512 KB a frame), both edge arrays finite and increasing, which 0..2,
 * 0 <= frac_bits <= 32 (SWRT_ERR_ARG with a message otherwise).  Empties the
 * series. */
int swrt_cond_series_begin(swrt_ctx* ctx, double f, double Cg, const double* omega_edges, int64_t nw, int which,
                           const double* q_edges, int64_t nq, int frac_bits);

/* Append the frame of the current packets in the flow of slot 0 (nslots 1) or
 * of slots 0 and 1 blended at alpha (nslots 2): queued on the packet stream
 * after whatever last wrote the packets and after the snapshot writes of the
 * slots it reads, no host wait (growing the series past its capacity, which
 * doubles, may wait for the stream).  Up to 16384 cells every workgroup
 * counts into a private plane in LDS and adds its non-zero cells to the frame;
 * beyond, every packet adds through global memory: the same integers.
 * SWRT_ERR_STATE before swrt_cond_series_begin; SWRT_ERR_ARG as for
 * swrt_raydiag_record (nslots, an unset slot, two grids, no packets) and with
 * more than 2^24 packets. */
int swrt_cond_series_record(swrt_ctx* ctx, int nslots, double alpha, double bump);

/* One frame per history frame in [first, first + count), frame i in the flow
 * at alphas[i] (alphas may be NULL with one snapshot, as for
 * swrt_raydiag_record_history): the same bits as swrt_cond_series_record on
 * packets set to that frame.  With two snapshots the call waits for the
 * stream once, before its launches, while alphas goes to the device.  A
 * range out of bounds: SWRT_ERR_ARG. */
int swrt_cond_series_record_history(swrt_ctx* ctx, int64_t first, int64_t count, int nslots, const double* alphas,
                                    double bump);

/* Frames recorded since begin or the last reset; nw and nq of the open
 * series, 0 if none (either pointer may be NULL). */
int64_t swrt_cond_series_frames(const swrt_ctx* ctx);
int swrt_cond_series_bins(const swrt_ctx* ctx, int64_t* nw_out, int64_t* nq_out);

/* Frames [first, first + count): counts_out count x (nq + 2) x (nw + 2),
 * sums_out count x (nq + 2) and stats2_out count x 2, frame-major.  Each may
 * be NULL.  Waits for the frames. */
int swrt_cond_series_get(swrt_ctx* ctx, int64_t first, int64_t count, int64_t* counts_out, int64_t* sums_out,
                         int64_t* stats2_out);

/* Empty the series; the edges, which and frac_bits stay. */
int swrt_cond_series_reset(swrt_ctx* ctx);

/* ---------------------------------------------------------------------------
 * The transition series: the energy-vs-omega distribution of the packets
 * (analysis/load_data.m:33-52, the Energy_versus_omega_* figures) split by a
 * source value the device keeps per packet, by ORIGINAL packet index: the
 * packet's omega at an earlier mark (how energy moves along the omega axis,
 * a two-time statistic) or any value the caller gives, such as the ring a
 * packet started on (parameters.txt's near_inertial_factor sweep in one run).
 *
 * Per packet, with scale = 2^frac_bits:
 *   omega = sqrt(f^2 + Cg^2 (k k + l l)), the spectrum series' bits;
 *   s     = the source value of the packet;
 *   d     = omega - s (one subtraction), d2 = d * d (one multiplication).
 * A packet is rejected, and counted nowhere else, if omega, s or d is NaN or
 * any of |omega * scale|, |d * scale|, |d2 * scale| is not below 2^38.
 * Otherwise its source class is the spectrum series' rule over src_edges (a
 * row [below, bin 0 .. bin ns-1, above], the last bin closed) and its omega
 * class the same rule over omega_edges.  A frame holds
 *   counts  (ns + 2) x (nw + 2) int64, source class major:
 *           counts[sc * (nw + 2) + wc];
 *   sums    (ns + 2) x 3 int64: per source class the sums of
 *           rint(omega * scale), rint(d * scale) and rint(d2 * scale) (round
 *           half even; signed sums in two's complement), so that the drift
 *           <d> / tau and the diffusivity <d2> / (2 tau) follow per source
 *           class, exact to the quantum;
 *   stats   3 int64 [n, rejected, mark serial]; the serial counts the marks
 *           since swrt_trans_series_begin.
 * With n <= 2^24 every sum stays below 2^62.  Integer addition is exact and
 * order-free: a frame depends on the packet set and the source values alone
 * (a re-binning between the mark and the record, either advance call and
 * either packet-stream setting give the same bits), and the frames of shards
 * that marked together combine by adding.
 * ------------------------------------------------------------------------- */

/* Open a series: 1 <= nw, ns <= 4096 with (ns + 2) * (nw + 2) <= 65536 cells,
 * both edge arrays finite and increasing, 0 <= frac_bits <= 32 (SWRT_ERR_ARG
 * with a message otherwise).  Empties the series, drops the mark and sets the
 * mark serial to 0. */
int swrt_trans_series_begin(swrt_ctx* ctx, double f, double Cg, const double* omega_edges, int64_t nw,
                            const double* src_edges, int64_t ns, int frac_bits);

/* The source of every packet := its current omega (begin's f and Cg): queued
 * on the packet stream after whatever last wrote the packets, no host wait
 * (the first mark, or one for more packets, allocates).  The mark belongs to
 * the packet set: swrt_packets_set drops it.  SWRT_ERR_STATE before begin;
 * SWRT_ERR_ARG without packets or with more than 2^24. */
int swrt_trans_series_mark(swrt_ctx* ctx);

/* The source of the packet with original index i := v[i]; n must equal the
 * packet count (SWRT_ERR_ARG).  NaN values are allowed: those packets are
 * rejected at every record.  v is free on return. */
int swrt_trans_series_mark_values(swrt_ctx* ctx, const double* v, int64_t n);

/* Append the frame of the current packets against the mark: queued on the
 * packet stream after whatever last wrote the packets, no host wait (growing
 * the series past its capacity, which doubles, may wait for the stream).  Up
 * to 16384 cells every workgroup counts into a private plane in LDS and adds
 * its non-zero cells to the frame; beyond, every packet adds through global
 * memory: the same integers.  SWRT_ERR_STATE before begin or without a valid
 * mark; SWRT_ERR_ARG without packets or with more than 2^24. */
int swrt_trans_series_record(swrt_ctx* ctx);

/* One frame per history frame in [first, first + count), each joined to the
 * current mark: the same bits as swrt_trans_series_record on packets set to
 * that frame and marked alike.  A range out of bounds: SWRT_ERR_ARG. */
int swrt_trans_series_record_history(swrt_ctx* ctx, int64_t first, int64_t count);

/* Frames recorded since begin or the last reset; nw and ns of the open
 * series, 0 if none (either pointer may be NULL). */
int64_t swrt_trans_series_frames(const swrt_ctx* ctx);
int swrt_trans_series_bins(const swrt_ctx* ctx, int64_t* nw_out, int64_t* ns_out);

/* Frames [first, first + count): counts_out count x (ns + 2) x (nw + 2),
 * sums_out count x (ns + 2) x 3 and stats3_out count x 3, frame-major.  Each
 * may be NULL.  Waits for the frames. */
int swrt_trans_series_get(swrt_ctx* ctx, int64_t first, int64_t count, int64_t* counts_out, int64_t* sums_out,
                          int64_t* stats3_out);

/* Empty the series; the mark, its serial, the edges and frac_bits stay. */
int swrt_trans_series_reset(swrt_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Packet recycling: at chosen moments every packet whose omega has reached
 * omega_cut is absorbed and re-injected in the same slot, with its own home
 * wavevector and a fresh uniform position.  N stays fixed, so a long run holds
 * a source at omega_0, a sink at omega_cut and a flux between them, and each
 * event's tally is kept as an integer frame on the device.
 *
 * State per packet, by ORIGINAL index (as the transition series keeps its
 * source): home (2 doubles), gen (int32, the re-injections so far) and born
 * (int32, the serial of the event that last injected it; 0 at begin).
 *
 * One event (swrt_recycle_apply), its serial counting from 1 since begin or
 * reset.  Per packet p in storage order, o its original index,
 *   w = sqrt(f^2 + Cg^2 (k k + l l)), the spectrum series' bits:
 *   1. rejected when w is not finite or w * 2^frac_bits >= 2^38: counted and
 *      left untouched, as the other series reject such packets (a blow-up
 *      stays visible);
 *   2. otherwise absorbed when w >= omega_cut: the frame tallies
 *      rint(w * 2^fb), rint(omega(home[o]) * 2^fb) and age = serial - born[o];
 *      then gen[o] += 1, born[o] = serial, (k, l) = home[o],
 *      x = (u1 - 0.5) * L, y = (u2 - 0.5) * L;
 *   3. otherwise untouched.
 * The position comes from a counter-based hash, a function of (seed, global
 * id, generation) only (uint64, wrapping):
 *   mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z>>30)) * 0xBF58476D1CE4E5B9;
 *           z = (z ^ (z>>27)) * 0x94D049BB133111EB; return z ^ (z>>31)
 *   h1 = mix(mix(seed ^ mix(index_base + o)) + gen_after_increment)
 *   h2 = mix(h1);   u = (h >> 11) * 2^-53
 * (mix(0) = 0xE220A8397B1DCDAF, mix(0x9E3779B97F4A7C15) = 0x6E789E6AA1B965F4).
 *
 * A frame is 8 int64: [n, absorbed, rejected, sum rint(w * 2^fb) of the
 * absorbed, sum rint(omega(home) * 2^fb) of the absorbed, sum age, max age,
 * serial].  Integer sums and a max are order-free: a frame, and the packets
 * after it, depend on the packet set alone, whatever the storage order, and
 * the frames of shards with index_base = the shard's first global id combine
 * by adding (the max age by the max).
 *
 * The marks of other subsystems are not touched: a re-injected packet keeps
 * its ray-diagnostics Omega_0 and its transition source value.
 * ------------------------------------------------------------------------- */

/* Begin recycling the current packets.  home_k: n x 2 column-major home
 * wavevectors in the original order, or NULL for the packets' k now.  Sets
 * gen = born = 0, the serial to 0 and empties the frames.  SWRT_ERR_ARG with
 * a message: L not finite and positive; f, Cg or omega_cut not finite;
 * omega_cut <= |f|; frac_bits outside 0..32; no packets; a home wavevector
 * whose omega is >= omega_cut or would be rejected (its packet would be
 * absorbed at every event: checked on the device, one read-back of a flag,
 * the call's only host wait). */
int swrt_recycle_begin(swrt_ctx* ctx, double f, double Cg, double omega_cut, double L, uint64_t seed,
                       int64_t index_base, int frac_bits, const double* home_k);

/* One event on the current packets, in place, and its frame appended: queued
 * on the packet stream after whatever last wrote the packets, no host wait
 * (growing the frame buffer past its capacity, which doubles, may wait).  A
 * queued ode23 chain is dropped, and the packet binning is invalidated:
 * re-injected packets jump across tiles, so the next packet call re-bins.
 * SWRT_ERR_STATE before begin, after a swrt_packets_set (which drops the
 * recycle state as it drops the transition mark) or inside an ode23 hook. */
int swrt_recycle_apply(swrt_ctx* ctx);

/* Frames recorded since begin or the last reset. */
int64_t swrt_recycle_frames(const swrt_ctx* ctx);

/* Frames [first, first + count) -> stats8_out, count x 8, frame-major.  Waits
 * for the frames.  A range out of bounds: SWRT_ERR_ARG; SWRT_ERR_STATE before
 * begin. */
int swrt_recycle_get(swrt_ctx* ctx, int64_t first, int64_t count, int64_t* stats8_out);

/* gen and born of every packet in the original order (n values each; either
 * pointer may be NULL).  Waits.  SWRT_ERR_STATE as swrt_recycle_apply. */
int swrt_recycle_state(swrt_ctx* ctx, int32_t* gen_out, int32_t* born_out);

/* Drop the frames, set the serial to 0 and gen and born to 0; home, the cut
 * and the seed stay: the next event equals a fresh begin's. */
int swrt_recycle_reset(swrt_ctx* ctx);

/* Release the recycle state and its frames. */
int swrt_recycle_end(swrt_ctx* ctx);

/* ---------------------------------------------------------------------------
 * The refraction series: how fast the flow's gradients carry each packet along
 * the omega axis right now, and how its wavevector lies in the local strain,
 * reduced per class and kept on the device as integers.  The rate is the
 * kick's, kdot = -(grad U)^T k (RaytracingScheme.m:9-16); summed per omega
 * class, omega-dot is the instantaneous flux density of the cascade that
 * analysis/load_data.m:33-52 plots, the lag-0 counterpart of the transition
 * series' drift.
 *
 * Per packet.  The state is (x, y, k1, k2); the flow record is
 * I[0..5] = (u, v, u_x, u_y, v_x, v_y), the bits swrt_eval and
 * swrt_raydiag_sample give for the same (nslots, alpha, bump).  Every
 * operation below is rounded on its own (no fused multiply-add):
 *   kk  = k1*k1 + k2*k2
 *   w   = sqrt(f2 + Cg2*kk)                  the spectrum series' omega (load_data.m:33)
 *   kd  = -(I[2]*k1 + I[4]*k2)               RaytracingScheme.m:14, the kick's sum
 *   ld  = -(I[3]*k1 + I[5]*k2)               RaytracingScheme.m:15
 *   g   = k1*kd + k2*ld
 *   wd  = (Cg2*g)/w                          omega-dot
 *   gam = g/kk                               d ln|k| / dt
 *   s1  = I[2]-I[5];  s2 = I[4]+I[3];  sig = sqrt(s1*s1 + s2*s2)   the strain (RaytracingScheme.m:25)
 *   c   = (gam+gam)/sig                      alignment
 * with f2 = f*f and Cg2 = Cg*Cg.  For a non-divergent flow c = -cos 2 theta,
 * theta the angle between k and the extension axis of the local strain: c = +1
 * has k on the compression axis, |k| growing at the largest rate the flow
 * allows (wave capture); c = -1 has k on the extension axis.  With
 * S = 2^frac_bits: qd = rint(wd*S), qd2 = rint((wd*wd)*S), qg = rint(gam*S),
 * round half even.
 *
 * Classes.  wc is the spectrum series' rule over omega_edges (a row [below,
 * bin 0 .. bin nw-1, above], the last bin closed) and ac the same rule for c
 * over a_edges with na bins.  In a flow that is not exactly non-divergent, or
 * by rounding, |c| may exceed 1: such packets land in below or above of
 * whatever edges the caller gave, which is no error.
 *
 * Rejected, adding to stats[1] and to nothing else, is a packet with any of
 *   !(fabs(w*S) < 2^38);
 *   c NaN (a NaN anywhere in the gradients or in k, kk = 0, sig = 0 with
 *   gam = 0);
 *   !(fabs(wd*S) < 2^38);  !((wd*wd)*S < 2^38);  !(fabs(gam*S) < 2^38).
 *
 * A frame holds
 *   counts  (na + 2) x (nw + 2) int64, alignment class major:
 *           counts[ac * (nw + 2) + wc];
 *   sums    3 (nw + 2) + (na + 2) int64, signed sums in two's complement:
 *           sums[0 * (nw + 2) + wc] += qd,  sums[1 * (nw + 2) + wc] += qd2,
 *           sums[2 * (nw + 2) + wc] += qg,  sums[3 * (nw + 2) + ac] += qd
 *           (the omega flux each alignment class carries, which the joint
 *           counts cannot give because omega-dot also depends on sig);
 *   stats   2 int64 [n, rejected].
 * The counts of a frame sum to n - rejected, and their marginal over the
 * alignment classes is the spectrum series' row of the accepted packets.  With
 * n <= 2^24 every sum stays below 2^62.  Integer addition is exact and
 * order-free: a frame depends on the packet set alone (two contexts, a
 * re-binning between two records, either advance call and either
 * packet-stream setting give the same bits), and the frames of shards combine
 * by adding.  Positions must be finite, as for every gather of the library.
 * ------------------------------------------------------------------------- */

/* Open a series: 1 <= nw, na <= 4096 with (na + 2) * (nw + 2) <= 65536 cells
 * (512 KB a frame), both edge arrays finite and increasing,
 * 0 <= frac_bits <= 32 (SWRT_ERR_ARG with a message otherwise).  Empties the
 * series. */
int swrt_refr_series_begin(swrt_ctx* ctx, double f, double Cg, const double* omega_edges, int64_t nw,
                           const double* a_edges, int64_t na, int frac_bits);

/* Append the frame of the current packets in the flow of slot 0 (nslots 1) or
 * of slots 0 and 1 blended at alpha (nslots 2): queued on the packet stream
 * after whatever last wrote the packets and after the snapshot writes of the
 * slots it reads, no host wait (growing the series past its capacity, which
 * doubles, may wait for the stream).  While the count plane has at most 16384
 * cells and fits a workgroup's LDS share beside the sums, every workgroup
 * counts into a private plane in LDS and adds its non-zero cells to the frame;
 * beyond, every packet adds through global memory: the same integers.
 * SWRT_ERR_STATE before swrt_refr_series_begin; SWRT_ERR_ARG as for
 * swrt_raydiag_record (nslots, an unset slot, two grids, no packets) and with
 * more than 2^24 packets. */
int swrt_refr_series_record(swrt_ctx* ctx, int nslots, double alpha, double bump);

/* One frame per history frame in [first, first + count), frame i in the flow
 * at alphas[i] (alphas may be NULL with one snapshot, as for
 * swrt_raydiag_record_history): the same bits as swrt_refr_series_record on
 * packets set to that frame.  With two snapshots the call waits for the
 * stream once, before its launches, while alphas goes to the device.  A
 * range out of bounds: SWRT_ERR_ARG. */
int swrt_refr_series_record_history(swrt_ctx* ctx, int64_t first, int64_t count, int nslots, const double* alphas,
                                    double bump);

/* Frames recorded since begin or the last reset; nw and na of the open
 * series, 0 if none (either pointer may be NULL). */
int64_t swrt_refr_series_frames(const swrt_ctx* ctx);
int swrt_refr_series_bins(const swrt_ctx* ctx, int64_t* nw_out, int64_t* na_out);

/* Frames [first, first + count): counts_out count x (na + 2) x (nw + 2),
 * sums_out count x (3 (nw + 2) + (na + 2)) and stats2_out count x 2,
 * frame-major.  Each may be NULL.  Waits for the frames. */
int swrt_refr_series_get(swrt_ctx* ctx, int64_t first, int64_t count, int64_t* counts_out, int64_t* sums_out,
                         int64_t* stats2_out);

/* Empty the series; the edges and frac_bits stay. */
int swrt_refr_series_reset(swrt_ctx* ctx);

/* ---------------------------------------------------------------------------
 * The absolute-frequency series: the distribution of the ray Hamiltonian
 * Omega = omega(k) + U(x,t).k over the packets beside that of omega, and its
 * rate along the rays, dOmega/dt = k . dU/dt, reduced per class and kept on
 * the device as integers.  In a steady flow Omega is conserved per packet and
 * omega only wanders inside the Doppler band |U.k| around it; only the
 * unsteadiness of the flow diffuses Omega, which is what lets the
 * energy-vs-omega spectrum of analysis/load_data.m:33-52 keep spreading.  The
 * reference watches Omega (symplectic_full_fourier.m:41,54-57,
 * SW_zero_background_raytracing.m:57,85-87); swrt_raydiag_* gives moments of
 * its relative change, this series its distribution and its rate.
 *
 * The flow is linear in time between two snapshots (interpolate_U.m:19-23),
 * so for the ODE the packets solve dU/dt = (U2 - U1)/tau exactly, tau the time
 * between the snapshots.  The records name their two slots: slot_a holds the
 * flow at alpha = 0, slot_b the flow at alpha = 1.
 *
 * Per packet.  The state is (x, y, k1, k2); A[0..1] and B[0..1] are (u, v) of
 * slot_a and slot_b at (x, y), the bits swrt_eval(nslots = 1) gives with that
 * slot in place 0 and the same bump.  Every operation below is rounded on its
 * own (no fused multiply-add):
 *   two snapshots:  oma = 1 - alpha
 *                   u   = oma*A[0] + alpha*B[0]    swrt_eval's blend (nslots = 2)
 *                   v   = oma*A[1] + alpha*B[1]
 *                   ut  = (B[0] - A[0]) / tau
 *                   vt  = (B[1] - A[1]) / tau
 *   one snapshot:   u = A[0];  v = A[1];  Od below is the literal 0.0
 *   kk  = k1*k1 + k2*k2
 *   w   = sqrt(f2 + Cg2*kk)                the spectrum series' omega (load_data.m:33)
 *   D   = u*k1 + v*k2                      the Doppler shift, swrt_raydiag's dot(U, k)
 *   Om  = w + D                            swrt_raydiag_sample's Omega when gH == Cg*Cg
 *   Od  = ut*k1 + vt*k2                    dOmega/dt along the ray
 * with f2 = f*f and Cg2 = Cg*Cg.  With S = 2^frac_bits: qO = rint(Od*S),
 * qO2 = rint((Od*Od)*S), qD = rint(D*S), round half even.
 *
 * Classes.  wc is the spectrum series' rule over omega_edges (a row [below,
 * bin 0 .. bin nw-1, above], the last bin closed) and oc the same rule for Om
 * over abs_edges with no bins.
 *
 * Rejected, adding to stats[1] and to nothing else, is a packet with any of
 *   Om or Od NaN;
 *   !(fabs(w*S) < 2^38);  !(fabs(Om*S) < 2^38);  !(fabs(D*S) < 2^38);
 *   !(fabs(Od*S) < 2^38);  !((Od*Od)*S < 2^38).
 * A packet with k = 0 is accepted: w = f, D = 0.
 *
 * A frame holds
 *   counts  (no + 2) x (nw + 2) int64, Omega class major:
 *           counts[oc * (nw + 2) + wc];
 *   sums    3 (nw + 2) + 2 (no + 2) int64, signed sums in two's complement:
 *           sums[0 * (nw + 2) + wc] += qO,  sums[1 * (nw + 2) + wc] += qO2,
 *           sums[2 * (nw + 2) + wc] += qD,
 *           sums[3 * (nw + 2) + oc] += qO,  sums[3 * (nw + 2) + (no + 2) + oc] += qO2;
 *   stats   2 int64 [n, rejected].
 * The counts of a frame sum to n - rejected, and their marginal over the
 * Omega classes is the spectrum series' row of the accepted packets.  With
 * n <= 2^24 every sum stays below 2^62.  Integer addition is exact and
 * order-free: a frame depends on the packet set and the two snapshots alone
 * (two contexts, a re-binning between two records, either advance call and
 * either packet-stream setting give the same bits), and the frames of shards
 * combine by adding.  Positions must be finite, as for every gather of the
 * library.  swrt_packets_set with another N empties the series.
 * ------------------------------------------------------------------------- */

/* Open a series: 1 <= nw, no <= 4096 with (no + 2) * (nw + 2) <= 65536 cells
 * (512 KB a frame), both edge arrays finite and increasing,
 * 0 <= frac_bits <= 32 (SWRT_ERR_ARG with a message otherwise).  Empties the
 * series. */
int swrt_absfreq_series_begin(swrt_ctx* ctx, double f, double Cg, const double* omega_edges, int64_t nw,
                              const double* abs_edges, int64_t no, int frac_bits);

/* Append the frame of the current packets in the flow of slot_a (alpha = 0)
 * and slot_b (alpha = 1), both in 0..SWRT_MAX_SLOTS-1, blended at alpha, the
 * snapshots tau apart; slot_b = -1: one snapshot, alpha and tau are ignored
 * and the rates are zero.  Queued on the packet stream after whatever last
 * wrote the packets and after the snapshot writes of both slots, no host wait
 * (growing the series past its capacity, which doubles, may wait for the
 * stream); a later snapshot into either slot waits for the record.  While the
 * count plane has at most 16384 cells and fits a workgroup's LDS share beside
 * the sums, every workgroup counts into a private plane in LDS and adds its
 * non-zero cells to the frame; beyond, every packet adds through global
 * memory: the same integers.  SWRT_ERR_STATE before
 * swrt_absfreq_series_begin; SWRT_ERR_ARG with a slot out of range,
 * slot_a == slot_b, an unset slot, two grids, with two snapshots a tau that
 * is zero or not finite (a negative tau is allowed), no packets, and with
 * more than 2^24 packets. */
int swrt_absfreq_series_record(swrt_ctx* ctx, int slot_a, int slot_b, double alpha, double tau, double bump);

/* One frame per history frame in [first, first + count), frame i in the flow
 * at alphas[i] (alphas may be NULL with one snapshot): the same bits as
 * swrt_absfreq_series_record on packets set to that frame.  With two
 * snapshots the call waits for the stream once, before its launches, while
 * alphas goes to the device.  A range out of bounds: SWRT_ERR_ARG. */
int swrt_absfreq_series_record_history(swrt_ctx* ctx, int64_t first, int64_t count, int slot_a, int slot_b,
                                       const double* alphas, double tau, double bump);

/* Frames recorded since begin or the last reset; nw and no of the open
 * series, 0 if none (either pointer may be NULL). */
int64_t swrt_absfreq_series_frames(const swrt_ctx* ctx);
int swrt_absfreq_series_bins(const swrt_ctx* ctx, int64_t* nw_out, int64_t* no_out);

/* Frames [first, first + count): counts_out count x (no + 2) x (nw + 2),
 * sums_out count x (3 (nw + 2) + 2 (no + 2)) and stats2_out count x 2,
 * frame-major.  Each may be NULL.  Waits for the frames. */
int swrt_absfreq_series_get(swrt_ctx* ctx, int64_t first, int64_t count, int64_t* counts_out, int64_t* sums_out,
                            int64_t* stats2_out);

/* Empty the series; the edges and frac_bits stay. */
int swrt_absfreq_series_reset(swrt_ctx* ctx);

/* ---------------------------------------------------------------------------
 * The ray-tube tangent map (no reference counterpart: its interpolate has no
 * derivative)
 * ------------------------------------------------------------------------ */

/* Per packet M = d(x, y, k, l) / d(x0, y0, k0, l0) since the last mark: the
 * exact derivative of the DISCRETE leapfrog step (drift, Euler kick, drift),
 * 4 x 4 row-major, carried along every ray on the device, and an int32
 * caustic counter: the sign changes of J = M00 M11 - M01 M10 from step to
 * step (J = 1 at a mark; 1/|J| scales the wave-action density of a packet
 * launched as a plane wave).  M is the Jacobian of the map, not of the ray
 * equations' flow: det M != 1 measures the scheme, and M overflows after some
 * thousands of steps without a mark.  The operation order is stated in
 * swrt_tangent.hpp and restated in numpy by tests/tangent_ref.py; results are
 * bit-reproducible and do not depend on re-binning or on how the steps are
 * split over calls.
 *
 * swrt_tangent_begin allocates the set for the current packets (M = I,
 * counters 0, mark serial 1); it is live until swrt_tangent_end.  While it is
 * live
 *   - swrt_advance, swrt_advance_intervals and swrt_leapfrog take the
 *     per-packet route (as swrt_set_kernel 1: re-binning moves the packets,
 *     intervals run one at a time, history frames are written as ever) and
 *     launch the tangent kernel on the current set in place; x and k keep the
 *     bits of every other route;
 *   - a non-default integrator (swrt_set_integrator) or the FMA gather
 *     (swrt_set_gather_mode 1) makes those calls fail with SWRT_ERR_ARG;
 *   - swrt_ode23_*, swrt_xka_step, swrt_spectral_leapfrog and
 *     swrt_recycle_apply fail with SWRT_ERR_STATE: they would move packets
 *     without their M;
 *   - swrt_packets_set with another N drops the set (as it drops the raydiag
 *     mark), with the same N it marks.
 * Everything is queued on the packet stream in call order, with the raydiag
 * calls' guarantees for streams and slots: a record or a get sees the M of
 * every advance queued before it.  Without a live set nothing changes.
 * swrt_tangent_mark: M = I, counters 0, ++serial (a new window).
 * swrt_tangent_get: M (N x 16) and the counters (N) in the original packet
 * order; either may be NULL.  Waits. */
int swrt_tangent_begin(swrt_ctx* ctx);
int swrt_tangent_mark(swrt_ctx* ctx);
int swrt_tangent_get(swrt_ctx* ctx, double* M16_out, int32_t* caustics_out);
int swrt_tangent_end(swrt_ctx* ctx);
/* 1 while a set is live, else 0 (-1: NULL context); the mark serial (0: none). */
int swrt_tangent_live(const swrt_ctx* ctx);
int64_t swrt_tangent_serial(const swrt_ctx* ctx);

/* The tangent series: class-plane frames of the live set.  Per packet omega =
 * sqrt(f^2 + Cg^2 |k|^2) in the spectrum series' bits, s = (sum of M_ij^2,
 * row-major) / 4 and J; e(v) = frexp exponent - 1 = floor(log2 v), exact.  A
 * frame is
 *   counts  (ns + 2) x (nw + 2) 64-bit counts, cell gc * (nw + 2) + wc: the
 *           class of s over growth_edges by the class of omega over
 *           omega_edges ([below, bins, above], comparisons only);
 *   sums    per omega class the sums of e(s), e(|J|) and the caustic counters
 *           (three rows of nw + 2, two's complement), then per growth class
 *           the sum of the caustic counters (ns + 2);
 *   stats   [n, rejected, mark serial].
 * A packet is rejected, and adds to nothing else, if omega, s or J is not
 * finite or J == 0.  Integer sums: frames of shards add.  At most 2^24
 * packets a frame, 1..4096 classes an axis, (ns + 2) * (nw + 2) <= 65536.
 * begin empties the series (it needs no live set); record needs one
 * (SWRT_ERR_STATE otherwise) and is queued without a host wait. */
int swrt_tangent_series_begin(swrt_ctx* ctx, double f, double Cg, const double* omega_edges, int64_t nw,
                              const double* growth_edges, int64_t ns);
int swrt_tangent_series_record(swrt_ctx* ctx);
int64_t swrt_tangent_series_frames(const swrt_ctx* ctx);
int swrt_tangent_series_bins(const swrt_ctx* ctx, int64_t* nw_out, int64_t* ns_out);
/* Frames [first, first + count): counts_out count x (ns + 2) x (nw + 2),
 * sums_out count x (3 (nw + 2) + (ns + 2)) and stats3_out count x 3,
 * frame-major.  Each may be NULL.  Waits for the frames. */
int swrt_tangent_series_get(swrt_ctx* ctx, int64_t first, int64_t count, int64_t* counts_out, int64_t* sums_out,
                            int64_t* stats3_out);
/* Empty the series; the edges stay. */
int swrt_tangent_series_reset(swrt_ctx* ctx);

/* ---------------------------------------------------------------------------
 * The invariant and the flow along the rays (symplectic_full_fourier.m:41,54-57,
 * SW_zero_background_raytracing.m:57,85-87, RaytracingScheme.m:18-31)
 * ------------------------------------------------------------------------ */

/* One pass over the device-resident packets, no trajectory download.  Per
 * packet, with U and grad U at x the bits swrt_eval gives there (slot 0, or
 * (1-alpha)*slot 0 + alpha*slot 1 when nslots == 2; bump: Lagrange bump), in
 * this operation order:
 *   Omega = sqrt(f^2 + gH*(k*k + l*l)) + (u*k + v*l)   omega(k) + dot(U, k)
 *                                                     (symplectic_full_fourier.m:41,55)
 *   zeta  = v_x - u_y                                  (RaytracingScheme.m:20)
 *   sigma = sqrt((u_x - v_y)^2 + (v_x + u_y)^2)        (RaytracingScheme.m:25)
 *   D     = v_y^2 + v_x*u_y                            (RaytracingScheme.m:30, as written there)
 * Both square roots are IEEE correctly rounded for every argument, zero and
 * subnormals included.
 * A frame is eight doubles [n, max|r|, sum r, sum r^2, sum omega, sum zeta,
 * sum sigma, sum D], omega = sqrt(f^2 + gH*|k|^2) and r = (Omega - Omega_0) /
 * Omega_0 (symplectic_full_fourier.m:56): sums, not means, so the frames of
 * shards combine by adding the sums and taking the max of entry 1.  Omega_0
 * and everything a packet leaves are kept by the original packet index, and
 * the sums run over that index (per-workgroup partials of a fixed grid,
 * combined in block order): a frame depends on the packets alone, not on the
 * binning's storage order, so two calls on the same state, two contexts
 * holding the same packets, or a re-binning between the mark and a sample
 * all give the same bits.
 * Every call is ordered after whatever last wrote the packets (both packet
 * streams, the ode23 attempts) and after the snapshot writes of the slots it
 * reads.  Errors: nslots not 1 or 2, an unset slot, two grids, no packets, a
 * NULL buffer where one is required: SWRT_ERR_ARG with a message.
 * swrt_packets_set with a different N drops the mark and the series. */

/* Omega_0 of every packet at the current state (Omega_0 of
 * symplectic_full_fourier.m:41, SW_zero_background_raytracing.m:57).  Queued on
 * the packet stream; reserves the buffers the later calls use. */
int swrt_raydiag_mark(swrt_ctx* ctx, double f, double gH, int nslots, double alpha, double bump);

/* Sample the current state, synchronously.  sample4_out (may be NULL): N x 4
 * column-major [Omega zeta sigma D] in the original packet order.  frame8_out
 * (may be NULL): the frame.  Without a mark r and frame entries 1..3 are 0. */
int swrt_raydiag_sample(swrt_ctx* ctx, double f, double gH, int nslots, double alpha, double bump,
                        double* sample4_out, double* frame8_out);

/* Append the frame of the current state to a series kept on the device
 * (solver_error against time, symplectic_full_fourier.m:54-57): queued on the
 * packet stream, the host does not wait for it.  Capacity: swrt_raydiag_mark
 * (or the first record of an ensemble without one) reserves the per-packet
 * buffers and 4096 frames; a record that finds the series full doubles it,
 * and only those calls may wait for the stream. */
int swrt_raydiag_record(swrt_ctx* ctx, double f, double gH, int nslots, double alpha, double bump);

/* swrt_raydiag_record for history frames [first, first + count) instead of
 * the current state (the frames of swrt_advance or swrt_ode23_run_at): one
 * series frame per history frame, frame i with the snapshot blend alphas[i]
 * (alphas may be NULL when nslots == 1) — solver_error at every output time
 * (SW_zero_background_raytracing.m:85-87) without a download.  The same bits
 * as swrt_raydiag_sample on packets set to that frame. */
int swrt_raydiag_record_history(swrt_ctx* ctx, int64_t first, int64_t count, double f, double gH, int nslots,
                                const double* alphas, double bump);

/* Frames recorded since the last reset; frames [first, first + count) into
 * frames8_out (8 doubles each, frame-major; waits for them); empty the series.
 * As swrt_history_frames / _get / _reset. */
int64_t swrt_raydiag_frames(const swrt_ctx* ctx);
int swrt_raydiag_series_get(swrt_ctx* ctx, int64_t first, int64_t count, double* frames8_out);
int swrt_raydiag_series_reset(swrt_ctx* ctx);

/* ---------------------------------------------------------------------------
 * ode23 packet integrator (the drivers' integrator)
 * ------------------------------------------------------------------------ */

/* Device stages of MATLAB's ode23 (Bogacki-Shampine 3(2), FSAL) over the
 * device-resident packets as ONE 4N-vector ODE (qgsw_raytrace.m:143-150 with
 * odefun :259-265: dx/dt = U + Cg*k/sqrt(f^2 + Cg^2|k|^2), dk/dt =
 * -(grad U)^T k, U from interpolate_U(slot 0, slot 1, t/tmax) — nslots = 1
 * reads slot 0 only).  The step-size controller (a global decision over the
 * max-norm error) runs on the host; thr = AbsTol/RelTol.
 * swrt_ode23_f1:     F1 = odefun(t, y);  *rh_raw = max |F1| ./ max(|y|, thr)
 * swrt_ode23_attempt: stages 2-4 of one trial step of size h ending at tnew
 *                    (ynew uses h4 = tnew - t); *err_raw = max over all
 *                    components of |F*E| ./ max(max(|y|, |ynew|), thr)
 * swrt_ode23_accept: y = ynew, F1 = F4 (FSAL). */
int swrt_ode23_f1(swrt_ctx* ctx, double t, double tmax, double f, double Cg, int nslots, double thr, double bump,
                  double* rh_raw_out);
int swrt_ode23_attempt(swrt_ctx* ctx, double t, double h, double tnew, double tmax, double f, double Cg,
                       int nslots, double thr, double bump, double* err_raw_out);
int swrt_ode23_accept(swrt_ctx* ctx);
/* Output at requested times (MATLAB ode23 with numel(tspan) > 2: the steps are
 * chosen as ever, the solution at the requested times is ntrp23 inside the
 * accepted steps).
 * swrt_ode23_set_dense: on = 1 makes swrt_ode23_attempt keep the stage
 *   derivatives F2 and F3 in device memory (the fused attempt otherwise never
 *   writes them); default 0.  swrt_ode23_run* ignore it.
 * swrt_ode23_ntrp: between such an attempt of the step from t to tnew and
 *   swrt_ode23_accept, appends nout history frames (swrt_history_*: the layout
 *   of swrt_advance's frames, original packet order), frame i the solution at
 *   tout[i], each within [t, tnew].  A time equal to tnew bit for bit gives
 *   ynew itself; any other, per component and in this operation order with
 *   h = tnew - t, s = (tout[i] - t)/h, s2 = s*s, s3 = s2*s,
 *     c1 = F1*(h*1)
 *     c2 = ((F1*(h*(-4/3)) + F2*(h*1))      + F3*(h*(4/3)))  + F4*(h*(-1))
 *     c3 = ((F1*(h*(5/9))  + F2*(h*(-2/3))) + F3*(h*(-8/9))) + F4*(h*1)
 *     yi = y + ((c1*s + c2*s2) + c3*s3)
 *   (ntrp23's BI; MATLAB's own BLAS order is unpinned, as its ode23 is).
 *   Without a dense attempt in the buffers — none made, already accepted, or
 *   another call that may touch the packets since — SWRT_ERR_STATE with a
 *   message.  Queued on the packet stream; may grow the history. */
int swrt_ode23_set_dense(swrt_ctx* ctx, int on);
int swrt_ode23_ntrp(swrt_ctx* ctx, double t, double tnew, const double* tout, int64_t nout);
/* [~, y] = ode23(odefun, [t0 tfinal], y) for the device-resident packets with
 * MATLAB's controller (RelTol rtol, AbsTol atol, MaxStep 0.1*|tfinal - t0|,
 * max-norm error, initial-step heuristic, step update) in the library: the
 * f1 / attempt / accept sequence above without a host interpreter between
 * attempts.  Writes the accepted times (t0 first) to ts_out[0 .. min(*nts_out,
 * ts_cap)): ts_cap bounds only the times recorded, the interval always
 * completes and *nts_out counts every accepted time.  {steps, failed,
 * attempts} go to stats3_out (may be NULL).  If the step size falls below
 * hmin (MATLAB's "unable to meet integration tolerances") the packets are
 * left at the last accepted time and SWRT_ERR_STATE is returned.  Single rank: a sharded ensemble needs the error norm's
 * max over the ranks (swrt_ode23_run_sharded). */
int swrt_ode23_run(swrt_ctx* ctx, double t0, double tfinal, double tmax, double f, double Cg, int nslots,
                   double rtol, double atol, double bump, double* ts_out, int64_t ts_cap, int64_t* nts_out,
                   int64_t* stats3_out);
/* [t, y] = ode23(odefun, tspan, y) for a tspan of nt >= 2 times, strictly
 * increasing or strictly decreasing (SW_zero_background_raytracing.m:69-87):
 * the whole call in the library.  t0 = tspan[0], tfinal = tspan[nt-1], MaxStep
 * 0.1*|tfinal - t0|; the first output gap |tspan[1] - tspan[0]| bounds the
 * initial step only (odearguments' htspan), and the output times influence
 * nothing else.  After each accepted step the solution at every tspan entry
 * it reaches is appended to the history (swrt_ode23_ntrp's frames): nt - 1
 * frames, for tspan[1..], their capacity reserved up front.  The packets are
 * left at y(tfinal), the last frame.  Plain launches on the packet stream, one
 * attempt at a time; the packets are re-binned every few accepted steps (stage
 * 1 recomputed at the current time gives the FSAL derivative bit for bit, so
 * the results do not depend on that cadence).  ts_out / ts_cap / nts_out /
 * stats3_out as in swrt_ode23_run.  Below hmin: SWRT_ERR_STATE, the packets at
 * the last accepted time, the frames emitted so far kept and counted.  Errors:
 * nt < 2, a tspan that is not strictly monotonic or not finite, NULL buffers:
 * SWRT_ERR_ARG with a message.  Single rank (no reduce callback). */
int swrt_ode23_run_at(swrt_ctx* ctx, const double* tspan, int64_t nt, double tmax, double f, double Cg, int nslots,
                      double rtol, double atol, double bump, double* ts_out, int64_t ts_cap, int64_t* nts_out,
                      int64_t* stats3_out);
/* swrt_ode23_run with a host hook: hook(hook_user) is called once, after
 * stage 1 and the first attempt are queued and before the host first waits
 * on the device — host work placed there (the drivers queue the next QG step,
 * qg2layersw_raytrace.m:166-181, through swrt_qg_step_speculative) overlaps
 * the interval's first launches instead of the gap between intervals.  The
 * hook may call the library's QG entry points; it must not touch the packets
 * or the field slots this call reads.  hook NULL: swrt_ode23_run. */
int swrt_ode23_run_hooked(swrt_ctx* ctx, double t0, double tfinal, double tmax, double f, double Cg, int nslots,
                          double rtol, double atol, double bump, double* ts_out, int64_t ts_cap, int64_t* nts_out,
                          int64_t* stats3_out, void (*hook)(void*), void* hook_user);
/* swrt_ode23_run_hooked for packets sharded over ranks: the
 * error norm is a max over every packet of every rank, so each max this
 * rank's stages produce — stage 1's, then every attempt's the controller
 * consumes — goes through reduce(&value, reduce_user), which replaces it in
 * place with the max over the ranks (the caller's collective, e.g. an RCCL
 * all_reduce) and returns 0 (else SWRT_ERR_STATE).  Every rank then takes the
 * same steps: one reduce per stage 1 and per consumed attempt, in the same
 * order on every rank (the order swraytracing_amd.integrate's controller
 * reduces in, so a rank without packets can run that one).  The first step
 * size comes from the reduced stage-1 max, so it is not guessed on the
 * device; a device-gated guess runs only if this rank's max passes its gate,
 * which the global max passing implies.  reduce NULL: swrt_ode23_run_hooked. */
int swrt_ode23_run_sharded(swrt_ctx* ctx, double t0, double tfinal, double tmax, double f, double Cg, int nslots,
                           double rtol, double atol, double bump, double* ts_out, int64_t ts_cap, int64_t* nts_out,
                           int64_t* stats3_out, void (*hook)(void*), void* hook_user,
                           int (*reduce)(double* value, void* reduce_user), void* reduce_user);
/* Chain the next swrt_ode23_run(_hooked) to the one running (or the next to
 * run): when it ends, it queues the next call's stage 1 (re-binning when due,
 * in-tile sort, f at t = 0) on the accepted packets with slot_a / slot_b as
 * slots 0 / 1, so the device runs it while the host returns and prepares that
 * call (the drivers arm it from the hook: their next interval reads this
 * interval's end snapshot and the one the hook queued).  The next call takes
 * it only if it would compute exactly that — its slots 0 / 1 hold the same
 * nodes, not rewritten since, the same f, Cg, AbsTol/RelTol, bump and
 * alpha(t0) = 0, and no call that may touch the packets ran in between — else
 * it computes its own.  Same bits either way; one call's arming is consumed
 * by that call. */
int swrt_ode23_chain_next(swrt_ctx* ctx, int slot_a, int slot_b);
/* swrt_ode23_run's controller (MATLAB ode23's step-size logic, the library's
 * own code: swrt_ode23_ctl.cpp) replayed against a scripted error sequence
 * instead of the device stages — host only, no context, no GPU.  raw[0] is
 * stage 1's max (max |F1| ./ max(|y|, thr)), raw[1..nraw) the attempts' raw
 * error maxima in the order the controller consumes them; dev_first: a first
 * attempt is queued from the device's own step size, as on the tile path.
 * log_out: per consumed attempt {t, h, tnew, raw} (4 doubles; *nlog_out
 * counts all of them); ts_out / ts_cap / nts_out as in swrt_ode23_run;
 * stats9_out: {steps, failed, attempts, first attempts taken, guesses queued,
 * guesses taken by rule (MaxStep at MaxStep, MaxStep from 5*absh, 5*absh),
 * consumed guesses whose device gate would have skipped them (always 0)}.
 * Returns SWRT_ERR_STATE below hmin (as swrt_ode23_run), SWRT_ERR_ARG if the
 * script runs out.  Replaces nothing in the reference: it pins the library's
 * controller to swraytracing_amd/integrate.py's (qgsw_raytrace.m:149). */
int swrt_ode23_replay(double t0, double tfinal, double rtol, double atol, int dev_first, const double* raw,
                      int64_t nraw, double* log_out, int64_t log_cap, int64_t* nlog_out, double* ts_out,
                      int64_t ts_cap, int64_t* nts_out, int64_t* stats9_out);

/* ---------------------------------------------------------------------------
 * QG PDE stepper: the snapshots' producer, device-resident
 * ------------------------------------------------------------------------ */

/* Parameters of the two drivers' PDEs.  nlayers = 1: qgsw_raytrace.m
 * (L = 2*pi, integer wavenumbers; update :270-286 with beta, r_drag and the
 * inertial_ring forcing :216-220; filter :222-230 when filter = 1).
 * nlayers = 2: qg2layersw_raytrace.m (wavenumbers scaled by 2*pi/L; B
 * inversion, factor_L with shear, nu*K2^hyper_order + r diffusion and beta
 * :129-144). */
typedef struct swrt_qg_params {
  int nlayers;
  int filter;
  double L;
  double K_d2;
  double beta;
  double r_drag;
  double force_strength;
  double f;
  double Cg;
  double shear;
  double nu;
  double hyper_order;
  double r;
} swrt_qg_params;

/* Load the initial spectral PV qk (nlayers blocks of the (2kmax+1) x (kmax+1)
 * g2k half plane, interleaved complex, column-major) and reset the AB3
 * history (qgsw_raytrace.m:111-112, qg2layersw_raytrace.m:120-121). */
int swrt_qg_init(swrt_ctx* ctx, const swrt_qg_params* params, int64_t nx, const double* qk_interleaved);
/* nsteps PDE steps of size dt: AB3 (forward Euler, AB2 for the first two
 * steps), 1 layer: qgsw_raytrace.m:121-137; 2 layers: qg2layersw_raytrace.m
 * :167-181 with expLdt/expL2dt recomputed on the device whenever dt changes.
 * Before each step the previous qk is kept (prev_qk, :122 / :167). */
int swrt_qg_step(swrt_ctx* ctx, double dt, int64_t nsteps);
/* Speculative PDE step (qg2layersw_raytrace.m:152-181 with the CFL rule of
 * :156-165 decided late): queue the next step with `dt` — the step size the
 * rule will keep unless U0 of the current qk says otherwise — together with
 * its post-step transforms and its CFL read-back, before the host has read
 * the current U0 (swrt_qg_max_speed_result pops read-backs oldest first).
 * The step is computed into spare buffers; the committed state (qk, history,
 * t, steps — what swrt_qg_get reports) is untouched until swrt_qg_resolve:
 * accept (1) makes it the current step, reject (0) drops it and its read-back,
 * after which the caller steps with the rule's new dt.  An accepted step is
 * the same computation as swrt_qg_step(dt): bit-identical.  Needs the fused
 * post-step transforms and, for two layers, dt equal to the dt of the last
 * step (the exponential propagators are not recomputed).  While one is
 * pending, swrt_qg_step / _snapshot / _max_speed(_async) fail with
 * SWRT_ERR_STATE. */
int swrt_qg_step_speculative(swrt_ctx* ctx, double dt);
int swrt_qg_resolve(swrt_ctx* ctx, int accept);
/* 1 (default): the swrt_qg_* calls run on a second HIP stream of the
 * context, so the next PDE step, its CFL speed and snapshot overlap the
 * packet launch that reads the previous snapshots.  Slot reads and writes
 * are ordered across the two streams with events; a swrt_qg_snapshot into a
 * slot whose buffer a queued packet launch still reads writes a spare buffer
 * instead (renaming), so it never waits for that launch.  0: one stream.
 * Results are identical; swrt_synchronize waits for both streams. */
int swrt_qg_set_stream(swrt_ctx* ctx, int separate);
/* 1 (default): the transforms every consumer of a new qk needs — the next
 * step's Jacobian, the CFL speed (swrt_qg_max_speed*) and layer 0's grid_U
 * for swrt_qg_snapshot(which 0, layer 0) — come from ONE batched inverse
 * 2-D FFT of the current qk, computed once on first use.  0: each call runs
 * its own transforms.  The same spectra and per-vector FFTs either way:
 * results are bit-identical. */
int swrt_qg_set_fused(swrt_ctx* ctx, int on);
/* U0 = sqrt(max((u + shear)^2 + v^2)) over every layer of grid_U(qk)
 * (qg2layersw_raytrace.m:156-158; qgsw_raytrace.m:63-65 with shear 0). */
int swrt_qg_max_speed(swrt_ctx* ctx, double* U0_out);
/* The same, split: _async enqueues the speed of the CURRENT qk (read back into
 * pinned memory behind an event) and returns at once, so the caller can queue
 * the packet work of this step before _result waits for U0 — the driver's
 * CFL decision for the next step no longer stalls the GPU. */
int swrt_qg_max_speed_async(swrt_ctx* ctx);
int swrt_qg_max_speed_result(swrt_ctx* ctx, double* U0_out);
/* Copy out qk (same layout as swrt_qg_init), the model time and step count. */
int swrt_qg_get(swrt_ctx* ctx, double* qk_out, double* t_out, int64_t* steps_out);
/* q = k2g(qk) per layer: nx x nx x nlayers column-major (pv.bin frames,
 * qgsw_raytrace.m:167-170). */
int swrt_qg_get_q(swrt_ctx* ctx, double* q_out);

/* nx of the QG state and (if nlayers_out) its layer count; -1 before
 * swrt_qg_init.  swrt_qg_get writes (nx-1) x nx/2 x nlayers complex values,
 * swrt_qg_get_q nx x nx x nlayers reals. */
int64_t swrt_qg_grid(const swrt_ctx* ctx, int* nlayers_out);
/* grid_U of the current (which = 0) or previous (which = 1) qk of one layer
 * straight into packet field slot `slot` (qgsw_raytrace.m:141-142,
 * qg2layersw_raytrace.m:187-188: layer 1, u += shear_strength), no host copy.
 * ny_period as in swrt_set_field_grid (0 = nx). */
int swrt_qg_snapshot(swrt_ctx* ctx, int slot, int which, int layer, int64_t ny_period);
/* swrt_qg_snapshot(slot, which = 0, layer = 0, ny_period) of the pending
 * speculative step's qk (swrt_qg_step_speculative; fused two-layer mode):
 * the snapshot that the same call would write after swrt_qg_resolve(ctx, 1),
 * bit for bit, queued before the CFL rule has decided — a driver queues it
 * with the speculative step and discards it if the step is rejected.
 * SWRT_ERR_STATE without a pending fused speculative step. */
int swrt_qg_snapshot_speculative(swrt_ctx* ctx, int slot, int64_t ny_period);
/* Owner-driver hand-off (qg2layersw_raytrace.m:186-188: the packets read the
 * top layer only).  In a sharded run one rank steps the PDE and the others
 * build their snapshots from the top layer's spectral PV it sends them.
 * swrt_qg_export: layer `layer` of the current (which = 0) or previous (1) qk,
 * (2kmax+1)*(kmax+1) interleaved complex in the device order (ky fastest:
 * element (kx, ky) at (kx + kmax)*(kmax + 1) + ky), to dst, followed by
 * `tail` (e.g. the step's dt, so one broadcast carries both: dst holds
 * 2*(2kmax+1)*(kmax+1) + 1 doubles).  dst_mode = 1: a device buffer; the
 * copy runs on the QG stream behind the step that made qk, after `stream`'s
 * work queued so far (its last read of dst) and before `stream`'s later work
 * (stream: a hipStream_t of the caller, e.g. the one a broadcast is queued
 * on; NULL = the context's packet stream).  2: the same without the first
 * ordering — the caller guarantees dst is no longer read (a wait of the QG
 * stream on another stream's event measured ~0.1 ms per step on ROCm while
 * packet launches hold the GPU).  0: host memory, returns once copied.  The committed state is exported: a pending
 * speculative step (swrt_qg_step_speculative) is neither waited for nor
 * included. */
int swrt_qg_export(swrt_ctx* ctx, int which, int layer, double* dst, int dst_mode, void* stream, double tail);
/* grid_U (grid_U.m:1-18: psi = -q/(K_d2 + K^2), u += shear) of a half plane in
 * swrt_qg_export's order into packet slot `slot`: bit for bit the
 * swrt_qg_snapshot(slot, which, layer, ny_period) of the context that exported
 * it, given that context's K_d2, shear and k_scale (2*pi/L for two layers, 1
 * for one).  src_on_device = 1: read after `stream`'s work queued so far (the
 * broadcast that filled it) and before `stream`'s later work (its next fill);
 * 0: host memory.  Runs on the QG stream with swrt_qg_snapshot's renaming: it
 * never waits for a packet launch that still reads the slot. */
int swrt_snapshot_qk(swrt_ctx* ctx, int slot, const double* qk, int src_on_device, void* stream, int64_t nx,
                     double L, double K_d2, double shear, double k_scale, int64_t ny_period);
/* Exchange two packet field slots (the previous step's "current" snapshot
 * becomes the next step's "previous" one without recomputing it). */
int swrt_swap_slots(swrt_ctx* ctx, int a, int b);

/* ---------------------------------------------------------------------------
 * Runtime helpers
 * ------------------------------------------------------------------------ */
/* Hardware conformance check of the hot loop's short IEEE sequences
 * (swrt_kernels.hpp sqrt_rn_normal, rcp_rn_normal, drift_inc's fast path —
 * the half-step drift of ode_symplectic.m:10-16): 16*n random operands over
 * their documented ranges, compared bit for bit with the compiler's IEEE
 * sqrt and division on the device.  mismatches3 = {sqrt, 1/w, drift}; all
 * zero on a conforming device.  Diagnostic; no reference counterpart. */
int swrt_check_arith(swrt_ctx* ctx, int64_t n, uint64_t seed, int64_t* mismatches3);
int swrt_synchronize(swrt_ctx* ctx);
/* The hipStream_t all of ctx's work is ordered on (for external event timing). */
int swrt_get_stream(swrt_ctx* ctx, void** stream_out);
/* Bracket every `every`-th packet-kernel launch with HIP events (default 1;
 * 0 disables).  A timestamped event between two launches costs a few µs of
 * GPU idle, so sampled timing keeps the measurement inside the timed region
 * without perturbing it. */
int swrt_set_timing(swrt_ctx* ctx, int every);
/* Sum of HIP-event-measured durations of the packet kernel launches since the
 * last reset (synchronizes). */
int swrt_kernel_time(swrt_ctx* ctx, int reset, double* total_ms, int64_t* launches);
/* Observed shader clock over a region of the packet stream: swrt_clock_stamp
 * (ctx, 0) before it and (ctx, 1) after it each enqueue (after every queued
 * packet launch) 1024 one-wave workgroups that record the shader-cycle
 * counter (s_memtime), the 100 MHz real-time counter (s_memrealtime) and the
 * CU they ran on; swrt_clock_ghz synchronises and returns the median over
 * the CUs stamped at both ends of cycles / seconds (a CU's own counter: the
 * counters of different CUs are not aligned), and (spread_out, may be NULL)
 * the per-CU clocks' (p90 - p10) / median.  Normalises a throughput measured
 * on one box to the clock it actually ran at (the chip lowers its clock
 * under load). */
int swrt_clock_stamp(swrt_ctx* ctx, int which);
int swrt_clock_ghz(swrt_ctx* ctx, double* ghz_out, double* spread_out);
/* swrt_clock_ghz's arithmetic on given stamps (host only, no context): stamps
 * = `waves` start waves then `waves` end waves, each {shader cycles, realtime
 * ticks, CU id}; realtime_hz the realtime counter's rate (100e6 on gfx950).
 * SWRT_ERR_STATE when no CU holds both a start and an end wave. */
int swrt_clock_ghz_stamps(const uint64_t* stamps, int64_t waves, double realtime_hz, double* ghz_out,
                          double* spread_out);

/* Debug knobs (test infrastructure; no reference counterpart).
 * SWRT_DEBUG_HAZARD_CHECK 0/1: a host-side happens-before checker of the
 *   packet buffers across the packet streams (swrt_set_packet_streams): every
 *   re-binning, part launch, join and synchronisation is mirrored with one
 *   vector clock per stream, each part launch's accesses covering the tiles
 *   its workgroups actually take (the device's own mapping); a launch whose
 *   reads or writes of a packet buffer are not ordered after a conflicting
 *   access on another stream is refused before it is queued (SWRT_ERR_STATE,
 *   swrt_last_error names both accesses).  Also on when the environment has SWRT_HAZARD_CHECK=1 at
 *   swrt_create.  Turning it on synchronises the context.
 * SWRT_DEBUG_SPIN_US n: each extra packet stream runs a ~n us sleep kernel
 *   before every part launch of its own, so a call's extra-stream parts
 *   overlap the next call's packet-stream part (adversarial schedule).
 * SWRT_DEBUG_LEGACY_PARK 0/1: test-only; 1 restores the ordering before the
 *   third packet buffers (the launch after a source-gather sort launch
 *   overwrites the buffer that launch gathers from) — a known race the
 *   checker must report.
 * SWRT_DEBUG_HAZARD_CHECKS (get only): accesses the checker has compared.
 * SWRT_DEBUG_QG_JFUSE 0/1 (default 1): two-layer fused mode runs the inverse
 *   column pass fused with the Jacobian, the CFL max and J's first forward
 *   pass (one kernel); 0 = the separate column pass + Jacobian-rows kernel —
 *   the same values, kept so tests can compare them bit for bit.  Applies
 *   when no packets share the context (beside packet launches the separate
 *   passes' smaller workgroups run faster).
 * SWRT_DEBUG_QG_UPDATE_COLS 0/1 (default 1): fused mode runs the last pass of
 *   J's forward transform inside the AB3 update (one kernel; the spectrum
 *   never goes to memory); 0 = the separate column pass + update — the same
 *   values, kept so tests can compare them bit for bit.  Applies, like
 *   SWRT_DEBUG_QG_JFUSE, unless packet launches share the context beside a
 *   separate QG stream.
 * SWRT_DEBUG_SHARE_SKEW 0/1: test-only; 1 makes the launch that ends each
 *   re-binning cycle split its tiles unevenly between the two packet streams
 *   (2/3 : 1/3) — a tile-to-stream mapping that differs from the previous
 *   launch's, the race of round 4.  Accepted only while the hazard checker is
 *   on, which models the tiles each part launch takes and refuses such a
 *   launch (SWRT_ERR_STATE) before it is queued.
 * SWRT_DEBUG_CORRUPT_COUNT d: test-only; the next re-binning adds d to one
 *   tile's count before its scan.  The scan's own check (counts >= 0, summing
 *   to the packets) then leaves an empty binning — no kernel runs over a bad
 *   range — and the next host synchronisation (swrt_synchronize,
 *   swrt_packets_get, ...) returns SWRT_ERR_STATE; the packet state is lost
 *   until swrt_packets_set.
 * SWRT_DEBUG_ODE23_CHAINED (get only): ode23 calls that took the stage 1 the
 *   previous call queued (swrt_ode23_chain_next).
 * SWRT_DEBUG_ODE23_FIRST_TAKEN, SWRT_DEBUG_ODE23_GUESSES_TAKEN (get only):
 *   swrt_ode23_run calls whose first attempt was the one the device queued
 *   from its own step size, and attempts taken from a gated guess (queued
 *   before the previous attempt's error was known), summed over the calls.
 * SWRT_DEBUG_ODE23_SPLIT_RUNS (get only): swrt_ode23_run calls whose attempts
 *   ran as two part launches on the two packet streams.
 * SWRT_DEBUG_ODE23_FIRST_CHAINED (get only): ode23 calls that took the first
 *   step size and first attempt the previous call queued behind their chained
 *   stage 1 (t0 = 0, tfinal = tmax and RelTol as that call assumed).
 * SWRT_DEBUG_ODE23_DENSE_REBIN n (default 8): swrt_ode23_run_at re-bins the
 *   packets every n accepted steps (0: never inside a run); speed only, the
 *   same bits for every n.
 * SWRT_DEBUG_ODE23_DENSE_REBINS (get only): the re-binnings swrt_ode23_run_at
 *   made inside its runs.
 * SWRT_DEBUG_MAP_TILED_FRAMES (get only): map frames recorded by the tile
 *   path (swrt_map_series_record), summed over the context's life.
 * SWRT_DEBUG_MAP_STRAYS (get only): packets the tile path added through
 *   global memory because they had drifted out of their tile's LDS window,
 *   summed over those frames; reading it waits for the queued records.
 * SWRT_DEBUG_KMAP_GLOBAL 0..3 (default 0): the kernel of the k-plane series'
 *   records.  0: by m (the LDS kernel up to m = 128, the global one beyond);
 *   1: the global kernel for every m, as it ships; 2 / 3: the global kernel
 *   with / without its wave-level merge (tools/kmap_series_rate.py).  Every
 *   value gives the same integers.
 * SWRT_DEBUG_COND_GLOBAL 0 / 1 (default 0): 1 makes the conditional spectrum
 *   series' records take the global kernel for every shape
 *   (tools/cond_series_rate.py).  Both values give the same integers.
 * SWRT_DEBUG_TRANS_GLOBAL 0 / 1 (default 0): 1 makes the transition series'
 *   records take the global kernel for every shape
 *   (tools/trans_series_rate.py).  Both values give the same integers.
 * SWRT_DEBUG_REFR_GLOBAL 0 / 1 (default 0): 1 makes the refraction series'
 *   records take the global kernel for every shape
 *   (tools/refr_series_rate.py).  Both values give the same integers.
 * SWRT_DEBUG_ABSFREQ_GLOBAL 0 / 1 (default 0): 1 makes the absolute-frequency
 *   series' records take the global kernel for every shape
 *   (tools/absfreq_series_rate.py).  Both values give the same integers.
 * SWRT_DEBUG_TANGENT_GLOBAL 0 / 1 (default 0): 1 makes the tangent series'
 *   records take the global kernel for every shape.  Both values give the
 *   same integers. */
#define SWRT_DEBUG_HAZARD_CHECK 1
#define SWRT_DEBUG_SPIN_US 2
#define SWRT_DEBUG_LEGACY_PARK 3
#define SWRT_DEBUG_HAZARD_CHECKS 4
#define SWRT_DEBUG_QG_JFUSE 5
#define SWRT_DEBUG_QG_UPDATE_COLS 7
#define SWRT_DEBUG_SHARE_SKEW 8
#define SWRT_DEBUG_CORRUPT_COUNT 9
#define SWRT_DEBUG_ODE23_CHAINED 10
#define SWRT_DEBUG_ODE23_FIRST_TAKEN 11
#define SWRT_DEBUG_ODE23_GUESSES_TAKEN 12
#define SWRT_DEBUG_ODE23_SPLIT_RUNS 13
#define SWRT_DEBUG_ODE23_FIRST_CHAINED 14
#define SWRT_DEBUG_ODE23_DENSE_REBIN 15
#define SWRT_DEBUG_ODE23_DENSE_REBINS 16
#define SWRT_DEBUG_MAP_TILED_FRAMES 17
#define SWRT_DEBUG_MAP_STRAYS 18
#define SWRT_DEBUG_KMAP_GLOBAL 19
#define SWRT_DEBUG_COND_GLOBAL 20
#define SWRT_DEBUG_TRANS_GLOBAL 21
#define SWRT_DEBUG_REFR_GLOBAL 22
#define SWRT_DEBUG_ABSFREQ_GLOBAL 23
#define SWRT_DEBUG_TANGENT_GLOBAL 24
int swrt_debug_set(swrt_ctx* ctx, int key, int64_t value);
int swrt_debug_get(swrt_ctx* ctx, int key, int64_t* value_out);

#ifdef __cplusplus
}
#endif
#endif /* SWRT_H */
