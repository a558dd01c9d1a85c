"""The QG PDE steppers that produce the packets' background snapshots, with
their state resident on the GPU, and the two reference
drivers built on them.

* :class:`QGModel` — ``qgsw_raytrace.m:111-137`` (1 layer: AB3 + filter,
  ``update`` :270-286) and ``qg2layersw_raytrace.m:129-181`` (2 layers:
  exponential AB3, adaptive CFL :156-165) over ``swrt_qg_*``.
* :func:`qgsw_raytrace` / :func:`qg2layersw_raytrace` — the drivers
  (``qgsw_raytrace.m:1-180``, ``qg2layersw_raytrace.m:1-247``): PDE on the
  device, per PDE step grid_U of (prev_qk, qk) straight into the packet slots
  and the packets advanced through [t, t+dt] by the fused symplectic kernel
  (the reference's ``ode23`` is replaced by ``nsub`` leapfrog substeps with the
  interpolate_U blend), frames written in the reference's
  ``data/*.bin`` layout (``write_field.m``).
"""
from __future__ import annotations

import functools
import math
import numbers
import os

import numpy as np

from ._lib import Context, QGParams
from .integrate import PacketEnsemble, track_ids_array
from .io import write_field
from .runlog import RunLog, parameter_block
from .scheme import BUMP_QG


class QGModel:
    """Device-resident spectral QG model (``swrt_qg_init`` / ``swrt_qg_step``).

    ``qk``: the g2k half plane, (2kmax+1, kmax+1) for one layer or
    (2kmax+1, kmax+1, 2) for two."""

    def __init__(self, qk, nx, params: QGParams, ctx: Context | None = None, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.nx = int(nx)
        self.params = params
        self.nlayers = params.nlayers
        self.L = params.L
        self.dx = params.L / nx
        self.spec_pending = False  # a speculative step is queued (step_speculative) and not yet resolved
        self.ctx.qg_init(params, nx, qk)

    @classmethod
    def one_layer(cls, qk, nx, f, Cg, beta=0.0, r_drag=0.1, force_strength=0.1, use_filter=True, **kw):
        """qgsw_raytrace.m:22-27,111-137: L = 2*pi, K_d2 = f/Cg, inertial_ring forcing."""
        p = QGParams(nlayers=1, filter=1 if use_filter else 0, L=2 * math.pi, K_d2=f / Cg, beta=beta,
                     r_drag=r_drag, force_strength=force_strength, f=f, Cg=Cg, shear=0.0, nu=0.0,
                     hyper_order=0.0, r=0.0)
        return cls(qk, nx, p, **kw)

    @classmethod
    def two_layer(cls, qk, nx, f, Cg, L=20.0, beta=0.0, shear=0.5, alpha=4, r=0.4, nutune=0.1, **kw):
        """qg2layersw_raytrace.m:13-34,79,129-147."""
        dx = L / nx
        p = QGParams(nlayers=2, filter=0, L=L, K_d2=f / Cg, beta=beta, r_drag=0.0, force_strength=0.0, f=f,
                     Cg=Cg, shear=shear, nu=nutune * dx ** (2 * alpha), hyper_order=float(alpha), r=r)
        return cls(qk, nx, p, **kw)

    def settle(self):
        """Drop a pending speculative step (the model stays at the committed
        step).  The calls the library refuses while one is pending — step,
        max_speed(_async), snapshot — settle first, so code that touches the
        model after a TwoLayerLoop never meets SWRT_ERR_STATE."""
        if self.spec_pending:
            self.resolve(False)

    def step(self, dt, nsteps=1):
        self.settle()
        self.ctx.qg_step(dt, nsteps)

    def step_speculative(self, dt):
        """Queue the next step with dt and its CFL read-back before the current
        U0 is known; the committed state stays until resolve()."""
        self.ctx.qg_step_speculative(dt)
        self.spec_pending = True

    def resolve(self, accept):
        self.ctx.qg_resolve(accept)
        self.spec_pending = False

    def max_speed(self):
        """U0 = sqrt(max(u.^2 + v.^2)) of grid_U(qk) (all layers, u + shear)."""
        self.settle()
        return self.ctx.qg_max_speed()

    def cfl_rule(self, dt, U0, cfl_fraction):
        """qg2layersw_raytrace.m:159-165 given U0: returns (dt, changed)."""
        cond = cfl_fraction * self.dx / U0
        if cond < dt or dt < cond / 4:
            return cfl_fraction / 2 * self.dx / U0, True
        return dt, False

    def cfl_update(self, dt, cfl_fraction):
        """qg2layersw_raytrace.m:156-165: returns (dt, U0, changed)."""
        U0 = self.max_speed()
        dt, changed = self.cfl_rule(dt, U0, cfl_fraction)
        return dt, U0, changed

    def max_speed_async(self):
        """Enqueue U0 of the current qk; collect it with max_speed_result()
        after queueing other work (the driver queues the packets first)."""
        self.settle()
        self.ctx.qg_max_speed_async()

    def max_speed_result(self):
        return self.ctx.qg_max_speed_result()

    @property
    def qk(self):
        return self.ctx.qg_get()[0]

    @property
    def t(self):
        return self.ctx.qg_get()[1]

    @property
    def steps(self):
        return self.ctx.qg_get()[2]

    def q(self):
        """k2g(qk) per layer: (nx, nx) or (nx, nx, 2)."""
        q = self.ctx.qg_get_q()
        return q[:, :, 0] if self.nlayers == 1 else q

    def snapshot(self, slot, which=0, layer=0, ny_period=0):
        """grid_U of the current (0) / previous (1) qk into packet slot `slot`."""
        self.settle()
        self.ctx.qg_snapshot(slot, which, layer, ny_period)

    def snapshot_speculative(self, slot, ny_period=0):
        """Layer 0's grid_U of the pending speculative step into `slot`: the
        snapshot(slot) this step gives once accepted (bit for bit)."""
        self.ctx.qg_snapshot_speculative(slot, ny_period)

    # ---- the flow spectrum series (swrt_flow_spectrum_*) ----
    @property
    def kscale(self):
        """2*pi/L as the device holds it (QGDev.kscale): exactly 1 for one layer."""
        return 1.0 if self.nlayers == 1 else 2.0 * math.pi / self.L

    def begin_flow_spectrum(self, layer=0):
        """Open the device-side series of layer ``layer``'s shell spectra with
        the model's own nx, kscale and K_d2.  Empties the series."""
        if not 0 <= int(layer) < self.nlayers:
            raise ValueError(f"layer must be 0..{self.nlayers - 1}")
        self.flow_layer = int(layer)
        self.ctx.flow_spectrum_begin(self.nx, self.kscale, self.params.K_d2)

    def record_flow_spectrum(self):
        """Append the committed qk's frame (queued behind the step that made
        it, no host wait).  A pending speculative step stays pending and is
        not included."""
        self.ctx.flow_spectrum_record_qg(self.flow_layer)

    def write_flow_spectrum(self, out_dir, first_time=None):
        """Append the recorded frames to ``out_dir``/flow_spec.bin (float64,
        3*nshell per frame: E, Z, Q per shell) and flow_stats.bin ([t, sum E,
        sum Z, sum Q] per frame), and write flow_geom.bin ([nx, nshell,
        k_scale, K_d2, layer]).  ``first_time``: the label the first frame
        takes in place of the model time (the drivers label their first packet
        frame, taken before the loop, dt*(packet_step_start - 1); the flow is
        the initial one, model time 0).  Returns the number of frames."""
        spectra, stats = self.ctx.flow_spectrum_get()
        if first_time is not None and len(stats):
            stats[0, 0] = first_time
        ns = self.ctx.flow_spectrum_shells()
        for name, a in (("flow_spec.bin", spectra), ("flow_stats.bin", stats)):
            with open(os.path.join(out_dir, name), "ab") as fh:  # (frame-major: appended as write_field does)
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        with open(os.path.join(out_dir, "flow_geom.bin"), "wb") as fh:
            fh.write(np.array([self.nx, ns, self.kscale, self.params.K_d2, self.flow_layer], dtype=np.float64).tobytes())
        return len(stats)


def flow_shell_count(nx):
    """Shells of an nx^2 grid: shell(kmax, kmax) + 1 with the integer rule
    j(j-1) < kx^2 + ky^2 <= j(j+1) (include/swrt.h)."""
    kmax = int(nx) // 2 - 1
    r2 = 2 * kmax * kmax
    s = math.isqrt(r2)
    return (s if r2 <= s * (s + 1) else s + 1) + 1


def flow_shells(nx, L):
    """The shell wavenumbers j*2*pi/L, j = 0..nshell-1, of the flow spectrum series."""
    return np.arange(flow_shell_count(nx), dtype=np.float64) * (2.0 * math.pi / L)


def flow_spectrum_fields(spectra, stats, Cg=None):
    """Flow spectrum frames (Context.flow_spectrum_get, or flow_spec.bin and
    flow_stats.bin reshaped to (frames, 3*nshell) and (frames, 4)) as a dict:
    t, E, Z, Q (frames x nshell: kinetic energy, relative-vorticity enstrophy
    and PV variance per shell, each summing to half the domain mean),
    U_rms = sqrt(2 sum E), zeta_rms = sqrt(2 sum Z) and, with ``Cg``,
    Fr = U_rms / Cg."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 4)
    sp = np.asarray(spectra, dtype=np.float64).reshape(len(stats), 3, -1)
    out = dict(t=stats[:, 0].copy(), E=sp[:, 0], Z=sp[:, 1], Q=sp[:, 2],
               U_rms=np.sqrt(2.0 * stats[:, 1]), zeta_rms=np.sqrt(2.0 * stats[:, 2]))
    if Cg is not None:
        out["Fr"] = out["U_rms"] / float(Cg)
    return out


# ----------------------------------------------------------------------------
# Drivers
# ----------------------------------------------------------------------------
def initial_q(nx, L, a_g, K_d2, k_min, k_max, rng, ndgrid=False):
    """initial_q (qgsw_raytrace.m:191-214, qg2layersw_raytrace.m:258-281): a
    random-phase ring k_min < |k| <= k_max normalised to max|U| = a_g, on
    linspace(-L/2, L/2, nx) (meshgrid for 1 layer, ndgrid for 2).  numpy's
    generator replaces MATLAB's rng (its stream is not reproducible here)."""
    xs = np.linspace(-L / 2, L / 2, nx)
    X, Y = np.meshgrid(xs, xs, indexing="ij" if ndgrid else "xy")
    q = np.zeros_like(X)
    U = np.zeros_like(X)
    V = np.zeros_like(X)
    phase = 2 * np.pi * rng.random((2 * k_max + 1, 2 * k_max + 1))
    for k in range(-k_max, k_max + 1):
        for l in range(-k_max, k_max + 1):
            if k_min ** 2 < k * k + l * l <= k_max ** 2:
                wp = k * X + l * Y + phase[k + k_max, l + k_max]
                U = U - l * np.sin(wp)
                V = V + k * np.sin(wp)
                q = q - (K_d2 + k * k + l * l) * np.cos(wp)
    return a_g / np.sqrt((U ** 2 + V ** 2).max()) * q


def _ring_factors(near_inertial_factor):
    """``near_inertial_factor`` as (factors, several): a scalar is one ring on
    today's path; a sequence of R factors (parameters.txt sweeps 2, 4, 8, 16
    over one PDE) puts R rings into one run."""
    if np.ndim(near_inertial_factor) == 0:
        return [near_inertial_factor], False
    factors = [float(v) for v in np.asarray(near_inertial_factor, dtype=np.float64).ravel()]
    if not factors or not all(math.isfinite(v) and v > 1 for v in factors):
        raise ValueError("near_inertial_factor: a scalar or a non-empty sequence of finite factors above 1")
    return factors, True


def _ring_bounds(N, R):
    """Ring r of R holds the packets [r * N // R, (r + 1) * N // R)."""
    return [(r * N // R, (r + 1) * N // R) for r in range(R)]


def _ring_index(N, R):
    """The ring of every packet, as doubles (the source values of trans_by="ring")."""
    ring = np.empty(N, dtype=np.float64)
    for r, (lo, hi) in enumerate(_ring_bounds(N, R)):
        ring[lo:hi] = r
    return ring


def _packets(N, L, near_inertial_factor, f, Cg, rng):
    """qgsw_raytrace.m:54-60.  With a sequence of R factors the packets go to
    R rings in contiguous blocks (_ring_bounds), ring r with the radius of
    factor r and the angles 2 pi j / N_r, j = 1..N_r: qgsw_raytrace.m's formula
    per ring.  The positions take the same draws either way."""
    factors, several = _ring_factors(near_inertial_factor)
    if not several:
        wf = math.sqrt((near_inertial_factor ** 2 - 1) * f ** 2 / Cg ** 2)
        i = np.arange(1, N + 1, dtype=np.float64)
        k = np.stack([wf * np.cos(2 * np.pi * i / N), wf * np.sin(2 * np.pi * i / N)], axis=1)
    else:
        k = np.empty((N, 2), dtype=np.float64)
        for fac, (lo, hi) in zip(factors, _ring_bounds(N, len(factors))):
            wf = _ring_radius(fac, f, Cg)
            j = np.arange(1, hi - lo + 1, dtype=np.float64)
            k[lo:hi, 0] = wf * np.cos(2 * np.pi * j / (hi - lo))
            k[lo:hi, 1] = wf * np.sin(2 * np.pi * j / (hi - lo))
    x = L * rng.random((N, 2)) - L / 2
    return x, k


class _IntervalGroup:
    """Packet intervals deferred until `k` PDE steps have their end snapshots
    (slots 1..k; slot 0 holds the group's start), then advanced in one
    swrt_advance_intervals call — the same bits as one advance per step.  The
    PDE runs up to k steps ahead of the packets; a frame write flushes."""

    def __init__(self, ctx, ens, k, nsub, integrator="leapfrog", packet_method=None, packet_iterations=None):
        if integrator not in ("leapfrog", "ode23"):
            raise ValueError("integrator must be 'leapfrog' or 'ode23'")
        if packet_method is not None or packet_iterations is not None:  # (None: the ensemble's own setting stays)
            ens.set_method(*_packet_method_args(packet_method or "leapfrog", packet_iterations, integrator))
        self.ctx, self.ens, self.nsub, self.integrator = ctx, ens, nsub, integrator
        # ode23 (the reference's own packet integrator) takes one interval per call
        self.k = 1 if integrator == "ode23" else max(1, min(int(k), 4))
        self.dts = []
        # (slot_a, slot_b, dt) of the last completed interval after the last
        # flush's swap: the slots that hold its start and its end snapshot
        self.last = None
        # ode23 controller totals over the calls (steps, failed, attempts)
        self.ode23_stats = {"steps": 0, "failed": 0, "attempts": 0, "intervals": 0}

    def next_slot(self):
        return len(self.dts) + 1

    def add(self, dt, hook=None):
        """hook (ode23 only): run while the interval's first launches run."""
        self.dts.append(dt)
        if len(self.dts) == self.k:
            self.flush(hook)
        elif hook is not None:
            hook()

    def flush(self, hook=None):
        if self.dts:
            if self.integrator == "ode23":
                st = {}
                # ode23(ray_ode, [0, dt], y0), alpha = t/dt
                self.ens.advance_ode23(self.dts[0], stats=st, hook=hook)
                for key in ("steps", "failed", "attempts"):
                    self.ode23_stats[key] += int(st.get(key, 0))
                self.ode23_stats["intervals"] += 1
            else:
                self.ens.advance_intervals(self.dts, self.nsub)
                if hook is not None:
                    hook()
            g = len(self.dts)
            self.ctx.swap_slots(0, g)  # the last end snapshot starts the next group
            # the last interval ran from snapshot g - 1 to snapshot g: the swap
            # put snapshot g into slot 0 and the group's start into slot g, so
            # snapshot g - 1 sits in slot g - 1, or (g = 1: it is the start) in slot 1
            self.last = (g - 1 if g >= 2 else g, 0, self.dts[-1])
            self.dts = []


def _dist_info():
    """(rank, world) of an initialised torch.distributed job, else (0, 1)."""
    try:
        import torch.distributed as dist
    except ImportError:
        return 0, 1
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _fresh_outputs(out_dir, fresh):
    """write_field.m:31 appends to existing files; a driver run starting from
    t = 0 removes earlier outputs first unless fresh=False."""
    os.makedirs(out_dir, exist_ok=True)
    if not fresh:
        return
    for name in ("packet_x", "packet_k", "packet_time", "pv", "pv_time", "omega_hist", "omega_stats", "omega_edges",
                 "map_n", "map_omega", "map_k", "map_l", "map_stats", "track_x", "track_k", "track_diag", "track_time",
                 "track_ids", "kmap_n", "kmap_stats", "kmap_geom", "flow_spec", "flow_stats", "flow_geom", "cond_hist",
                 "cond_sums", "cond_stats", "cond_geom", "trans_hist", "trans_sums", "trans_stats", "trans_time",
                 "trans_geom", "recycle_stats", "recycle_time", "recycle_geom", "recycle_gen", "refr_hist", "refr_sums",
                 "refr_stats", "refr_geom", "absfreq_hist", "absfreq_sums", "absfreq_stats", "absfreq_geom", "tangent_hist",
                 "tangent_sums", "tangent_stats", "tangent_time", "tangent_geom"):
        p = os.path.join(out_dir, name + ".bin")
        if os.path.exists(p):
            os.remove(p)


def _spectrum_args(spectrum_edges, packet_files, kmap_cells=None):
    """The drivers' ``spectrum_edges`` / ``packet_files`` checked before anything runs."""
    if spectrum_edges is None:
        if not packet_files and kmap_cells is None:
            raise ValueError("packet_files=False without spectrum_edges: the run would write no packet output")
        return None
    edges = np.array(spectrum_edges, dtype=np.float64).ravel()
    if edges.size < 2 or not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0):
        raise ValueError("spectrum_edges must be at least two finite increasing values")
    return edges


def _map_args(map_cells, map_frac_bits):
    """The drivers' ``map_cells`` / ``map_frac_bits`` checked before anything runs."""
    if map_cells is None:
        return None
    if isinstance(map_cells, bool) or int(map_cells) != map_cells or not 1 <= int(map_cells) <= 4096:
        raise ValueError("map_cells must be an integer 1..4096")
    if isinstance(map_frac_bits, bool) or int(map_frac_bits) != map_frac_bits or not 0 <= int(map_frac_bits) <= 32:
        raise ValueError("map_frac_bits must be an integer 0..32")
    return int(map_cells), int(map_frac_bits)


def _kmap_args(kmap_cells, kmap_kmax, kmap_frac_bits, ring_radius=None):
    """The drivers' ``kmap_cells`` / ``kmap_kmax`` / ``kmap_frac_bits`` checked
    before anything runs: (K, m, frac_bits), or None without ``kmap_cells``.
    ``kmap_kmax=None`` stands for four times ``ring_radius``, the radius of
    the initial ring the driver computes."""
    if kmap_cells is None:
        return None

    def real(v):
        return isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_))

    def integer(v):
        return real(v) and math.isfinite(v) and int(v) == v

    if not integer(kmap_cells) or not 1 <= int(kmap_cells) <= 4096:
        raise ValueError("kmap_cells must be an integer 1..4096")
    if not integer(kmap_frac_bits) or not 0 <= int(kmap_frac_bits) <= 32:
        raise ValueError("kmap_frac_bits must be an integer 0..32")
    if kmap_kmax is None:
        if ring_radius is None:
            raise ValueError("kmap_kmax=None needs the initial ring radius")
        kmap_kmax = 4.0 * float(ring_radius)
    if not real(kmap_kmax) or not math.isfinite(kmap_kmax) or not kmap_kmax > 0:
        raise ValueError("kmap_kmax must be a positive finite number")
    return float(kmap_kmax), int(kmap_cells), int(kmap_frac_bits)


def _plane_edges(spectrum_edges, needs_msg, name, edges, missing_msg=None):
    """The first checks of a class-plane series' driver arguments: the run
    has ``spectrum_edges`` (its omega classes), and the argument ``name`` holds
    the second axis' edges, at least two finite increasing values."""
    if spectrum_edges is None:
        raise ValueError(needs_msg)
    if edges is None:
        raise ValueError(missing_msg)
    edges = np.array(edges, dtype=np.float64).ravel()
    if edges.size < 2 or not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0):
        raise ValueError(f"{name} must be at least two finite increasing values")
    return edges


def _plane_frac_bits(name, frac_bits, edges, spectrum_edges, cap_msg):
    """The last checks: the argument ``name`` an integer 0..32; at most 4096
    classes and 65536 cells a frame."""
    if isinstance(frac_bits, (bool, np.bool_)) or not isinstance(frac_bits, numbers.Real) \
            or int(frac_bits) != frac_bits or not 0 <= int(frac_bits) <= 32:
        raise ValueError(f"{name} must be an integer 0..32")
    nw = np.asarray(spectrum_edges).size - 1
    if not 1 <= edges.size - 1 <= 4096 or (edges.size + 1) * (nw + 2) > 65536:
        raise ValueError(cap_msg)
    return int(frac_bits)


def _cond_args(cond_by, cond_edges, cond_frac_bits, spectrum_edges):
    """The drivers' ``cond_by`` / ``cond_edges`` / ``cond_frac_bits`` checked
    before anything runs: (which, q edges, frac_bits), or None without
    ``cond_by``.  The omega classes are the run's ``spectrum_edges``."""
    if cond_by is None:
        return None
    if not isinstance(cond_by, str) or cond_by not in ("zeta", "sigma", "D"):
        raise ValueError('cond_by must be None, "zeta", "sigma" or "D"')
    edges = _plane_edges(spectrum_edges,
                         "cond_by needs spectrum_edges: they are the conditional spectra's omega classes",
                         "cond_edges", cond_edges, "cond_by needs cond_edges, the classes of the flow scalar")
    frac_bits = _plane_frac_bits("cond_frac_bits", cond_frac_bits, edges, spectrum_edges,
                                 "cond_edges: at most 4096 classes and (nq + 2) * (nbins + 2) <= 65536 cells a frame")
    return cond_by, edges, frac_bits


def _refr_args(refr_edges, refr_frac_bits, spectrum_edges):
    """The drivers' ``refr_edges`` / ``refr_frac_bits`` checked before anything
    runs: (alignment edges, frac_bits), or None without ``refr_edges``.  The
    omega classes are the run's ``spectrum_edges``."""
    if refr_edges is None:
        return None
    edges = _plane_edges(spectrum_edges,
                         "refr_edges needs spectrum_edges: they are the refraction series' omega classes",
                         "refr_edges", refr_edges)
    return edges, _plane_frac_bits(
        "refr_frac_bits", refr_frac_bits, edges, spectrum_edges,
        "refr_edges: at most 4096 classes and (na + 2) * (nbins + 2) <= 65536 cells a frame")


def _absfreq_args(absfreq_edges, absfreq_frac_bits, spectrum_edges):
    """The drivers' ``absfreq_edges`` / ``absfreq_frac_bits`` checked before
    anything runs: (Omega edges, frac_bits), or None without ``absfreq_edges``.
    The omega classes are the run's ``spectrum_edges``."""
    if absfreq_edges is None:
        return None
    edges = _plane_edges(spectrum_edges,
                         "absfreq_edges needs spectrum_edges: they are the absolute-frequency series' omega classes",
                         "absfreq_edges", absfreq_edges)
    return edges, _plane_frac_bits(
        "absfreq_frac_bits", absfreq_frac_bits, edges, spectrum_edges,
        "absfreq_edges: at most 4096 classes and (no + 2) * (nbins + 2) <= 65536 cells a frame")


def _tangent_args(tangent_edges, tangent_lag, spectrum_edges, integrator, packet_method, recycle_omega, Npackets):
    """The drivers' ``tangent_edges`` / ``tangent_lag`` checked before anything
    runs: (growth edges, lag), or None without ``tangent_edges``.  The omega
    classes are the run's ``spectrum_edges``; the tangent map has the leapfrog
    step only and does not follow recycled packets."""
    if tangent_edges is None:
        if tangent_lag != 1:
            raise ValueError("tangent_lag needs tangent_edges")
        return None
    edges = _plane_edges(spectrum_edges, "tangent_edges needs spectrum_edges: they are the tangent series' omega classes",
                         "tangent_edges", tangent_edges)
    _plane_frac_bits("tangent", 0, edges, spectrum_edges,
                     "tangent_edges: at most 4096 classes and (ns + 2) * (nbins + 2) <= 65536 cells a frame")
    if isinstance(tangent_lag, (bool, np.bool_)) or not isinstance(tangent_lag, numbers.Integral) or tangent_lag < 1:
        raise ValueError("tangent_lag must be an integer >= 1")
    if integrator == "ode23":
        raise ValueError('tangent_edges: the tangent map belongs to integrator="leapfrog"')
    if packet_method != "leapfrog":
        raise ValueError('tangent_edges: the tangent map has packet_method="leapfrog" only')
    if recycle_omega is not None:
        raise ValueError("tangent_edges: the tangent map does not follow recycled packets (leave recycle_omega out)")
    if Npackets <= 0:
        raise ValueError("the tangent series needs packets")
    return edges, int(tangent_lag)


def _ends_tangent(driver):
    """A driver that leaves the caller's context without a live tangent set
    when it raises in mid-run (the normal path ends it itself): the context
    would stay on the per-packet route and refuse the ode23, xka, spectral and
    recycle calls."""
    @functools.wraps(driver)
    def run(*args, ctx=None, **kw):
        try:
            return driver(*args, ctx=ctx, **kw)
        except BaseException:
            if ctx is not None and kw.get("tangent_edges") is not None:
                try:
                    if ctx.tangent_live():
                        ctx.tangent_end()
                except Exception:  # (the run's own error is the one to report)
                    pass
            raise
    return run


def _packet_method_args(packet_method, packet_iterations, integrator):
    """The drivers' ``packet_method`` / ``packet_iterations`` checked before
    anything runs: (method, iterations), the arguments of PacketEnsemble."""
    from .integrate import packet_method as check
    if integrator == "ode23" and (packet_method != "leapfrog" or packet_iterations is not None):
        raise ValueError('packet_method / packet_iterations belong to integrator="leapfrog"')
    check(packet_method, packet_iterations)
    return packet_method, packet_iterations


def _packet_method_line(method, iterations):
    """The one extra log line of a run whose packet step is not the leapfrog step."""
    from .integrate import packet_method as check
    kick, it, comp = check(method, iterations)
    return f"Packet step: {method} ({kick} kick, {it} iterations" + (f", {comp} composition)" if comp else ")")


def _absfreq_line(edges, frac_bits):
    """The one extra log line of a run with the absolute-frequency series."""
    return f"Absolute frequency: {edges.size - 1} classes over [{edges[0]:g}, {edges[-1]:g}], quantum 2^-{frac_bits}"


def _trans_args(trans_src_edges, trans_by, trans_lag, trans_frac_bits, spectrum_edges, nrings):
    """The drivers' ``trans_src_edges`` / ``trans_by`` / ``trans_lag`` /
    ``trans_frac_bits`` checked before anything runs: (by, source edges, lag,
    frac_bits), or None without the first two.  The omega classes are the
    run's ``spectrum_edges``."""
    if trans_src_edges is None and trans_by is None:
        if trans_lag is not None:
            raise ValueError("trans_lag needs trans_src_edges")
        return None
    if trans_by not in (None, "omega", "ring"):
        raise ValueError('trans_by must be None, "omega" or "ring"')
    if spectrum_edges is None:
        raise ValueError("the transition series needs spectrum_edges: they are its omega classes")
    if trans_by == "ring":
        if trans_src_edges is not None:
            raise ValueError('trans_by="ring" sets its own source edges: leave trans_src_edges out')
        if trans_lag is not None:
            raise ValueError('trans_by="ring" is never re-marked: leave trans_lag out')
        edges = np.arange(nrings + 1, dtype=np.float64) - 0.5
    else:
        edges = _plane_edges(spectrum_edges, None, "trans_src_edges", trans_src_edges,
                             'trans_by="omega" needs trans_src_edges, the classes of omega at the mark')
    if trans_lag is not None and (isinstance(trans_lag, (bool, np.bool_)) or not isinstance(trans_lag, numbers.Integral)
                                  or trans_lag < 1):
        raise ValueError("trans_lag must be None or an integer >= 1")
    frac_bits = _plane_frac_bits(
        "trans_frac_bits", trans_frac_bits, edges, spectrum_edges,
        "the transition series: at most 4096 source classes and (ns + 2) * (nbins + 2) <= 65536 cells a frame")
    return (1 if trans_by == "ring" else 0), edges, (None if trans_lag is None else int(trans_lag)), frac_bits


def _recycle_args(recycle_omega, recycle_seed, recycle_every, recycle_frac_bits, ring_factors, f, trans_src_edges,
                  Npackets):
    """The drivers' ``recycle_omega`` / ``recycle_seed`` / ``recycle_every`` /
    ``recycle_frac_bits`` checked before anything runs: (omega_cut, seed,
    every, frac_bits), or None without recycling."""
    if recycle_omega is None:
        return None
    if isinstance(recycle_omega, (bool, np.bool_)) or not isinstance(recycle_omega, numbers.Real) \
            or not math.isfinite(recycle_omega):
        raise ValueError("recycle_omega must be None or a finite number")
    omega0 = max(ring_factors) * abs(f)
    if not recycle_omega > omega0:
        raise ValueError(f"recycle_omega must be above the largest ring's omega0 ({omega0:g}): a packet re-injected at "
                         "home would be absorbed again at every event")
    if trans_src_edges is not None:
        raise ValueError('recycle_omega with trans_src_edges: the omega mark of a re-injected packet would be stale '
                         '(trans_by="ring" is allowed: home keeps the ring)')
    if Npackets <= 0:
        raise ValueError("recycle_omega needs packets")
    for name, v, lo in (("recycle_seed", recycle_seed, 0), ("recycle_every", recycle_every, 1),
                        ("recycle_frac_bits", recycle_frac_bits, 0)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral) or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo}")
    if recycle_frac_bits > 32:
        raise ValueError("recycle_frac_bits must be an integer 0..32")
    if recycle_seed >= 2 ** 64:
        raise ValueError("recycle_seed must be below 2^64")
    return float(recycle_omega), int(recycle_seed), int(recycle_every), int(recycle_frac_bits)


def _begin_trans(ens, trans_args, spectrum_edges, out_dir, t, Npackets, nrings):
    """Open the run's transition series and take its first mark, at the first
    packet frame (time t)."""
    by, edges, _, frac_bits = trans_args
    ens.begin_trans(spectrum_edges, edges, frac_bits, by=by, directory=out_dir)
    ens.mark_trans(_ring_index(Npackets, nrings) if by == 1 else None, t=t)


def _rings_line(factors, f, Cg):
    """The one extra log line of a run with several rings."""
    return "Rings: " + ", ".join(f"omega0 = {fac * f:g} (radius {_ring_radius(fac, f, Cg):g})" for fac in factors)


def _flow_args(flow_spectrum, Npackets):
    """The drivers' ``flow_spectrum`` checked before anything runs: its frames
    are the packet frames, so it needs packets."""
    if flow_spectrum and Npackets <= 0:
        raise ValueError("flow_spectrum records at the packet frames: it needs Npackets > 0")


def _ring_radius(near_inertial_factor, f, Cg):
    """|k| of _packets' initial ring (qgsw_raytrace.m:56)."""
    return math.sqrt((near_inertial_factor ** 2 - 1) * f ** 2 / Cg ** 2)


def _track_args(track_ids, track_every, Npackets, default_every):
    """The drivers' ``track_ids`` / ``track_every`` checked before anything
    runs: (ids as int64 in the caller's order, PDE steps per track frame), or
    None without ``track_ids``.  An integer K stands for K ids spread evenly,
    arange(K) * (Npackets // K)."""
    if track_every is None:
        track_every = default_every
    elif isinstance(track_every, (bool, np.bool_)) or not np.isscalar(track_every) or not np.isreal(track_every) \
            or int(track_every) != track_every or int(track_every) < 1:
        raise ValueError("track_every must be an integer >= 1 (PDE steps per track frame)")
    if track_ids is None:
        return None
    if isinstance(track_ids, (bool, np.bool_)):
        raise ValueError("track_ids must be a sequence of packet ids or an integer count")
    if np.isscalar(track_ids):
        if not np.isreal(track_ids) or int(track_ids) != track_ids:
            raise ValueError("track_ids: the count K must be an integer")
        K = int(track_ids)
        if not 1 <= K <= int(Npackets):
            raise ValueError(f"track_ids: the count K must be 1..Npackets ({int(Npackets)})")
        ids = np.arange(K, dtype=np.int64) * (int(Npackets) // K)
    else:
        ids = track_ids_array(track_ids, Npackets)
    if ids.size > 1 << 20:
        raise ValueError("track_ids: at most 2^20 packets can be tracked")
    return ids, int(track_every)


def _save_frame(ens, t, out_dir, spectrum, packet_files, maps=False, kmaps=False, conds=False, trans=None, index=0,
                refrs=False, absfreq=None, tangent=None):
    """One packet frame: its spectrum, its map, its k-plane, its conditional
    spectrum and its refraction frame (both in the flow of slot 0, the snapshot
    at the packets' time), its absolute-frequency frame (``absfreq``: the
    interval group's (slot_a, slot_b, dt) of the last completed interval, read
    at alpha = 1: the flow at the packets' time and the rate of the interval
    they just crossed) and its
    transition frame recorded on the device (queued, no host wait) whether or
    not the frame itself is written.  ``trans``: the run's lag (0: never
    re-marked); packet frame ``index`` records against the mark, and re-marks
    after the record when the lag divides its index.  ``tangent``: the tangent
    series' lag, likewise (None: no tangent series)."""
    if spectrum:
        ens.record_spectrum()
    if maps:
        ens.record_map()
    if kmaps:
        ens.record_kmap()
    if conds:
        ens.record_cond()
    if refrs:
        ens.record_refr()
    if absfreq is not None:
        ens.record_absfreq(absfreq[0], absfreq[1], 1.0, absfreq[2])
    if trans is not None:
        ens.record_trans(t)
        if trans and index % trans == 0:
            ens.mark_trans(t=t)
    if tangent is not None:
        ens.record_tangent(t)
        if index % tangent == 0:
            ens.mark_tangent(t)
    ens.write_frame(t, out_dir, packet_files)


def _owner_setup(world, pde, owner_weight, nx, Npackets, link_buffers="auto"):
    """(link, bounds) of a sharded run in the PDE-owner form, or (None, None)
    for the replicated form (every rank steps the PDE).  link_buffers: "auto"
    (device buffers with nccl, host buffers with gloo), "device" or "host"."""
    if world <= 1 or pde == "replicated":
        return None, None
    if pde != "owner":
        raise ValueError("pde must be 'owner' or 'replicated'")
    import torch.distributed as dist

    from .dist import OwnerLink, owner_bounds
    device = {"auto": None, "device": True, "host": False}[link_buffers]
    w0 = owner_weight_for(world) if owner_weight is None else owner_weight
    return OwnerLink(nx, dist.get_backend(), device=device), owner_bounds(Npackets, world, w0)


def owner_weight_for(world):
    """The PDE owner's packets per packet of a receiving rank, from the
    measured one-GPU legs of bench.py's driver_step_forecast["owner"]
    (profiles/r06_final): with 2 ranks the owner's PDE leaves room for
    packets (best w = 0.5), from 4 ranks on the receivers' share is what
    bounds the step and the owner's PDE already takes about as long as it
    (best w = 0: the owner holds no packets)."""
    return 0.5 if world <= 2 else 0.0


class TwoLayerLoop:
    """One iteration of qg2layersw_raytrace.m:152-197 on the device: the CFL
    rule (:156-165) on the current U0, the PDE step, U0 of the new qk read back
    asynchronously (collected after the packet work is queued, so the rule
    never idles the GPU), and — once t > packet_delay — grid_U of (prev_qk,
    qk) into the packet slots and the packet interval [t, t+dt].  Used by
    :func:`qg2layersw_raytrace` (which adds the frame writes) and by bench.py's
    end-to-end driver-step figure.

    With ``speculate`` (default) every step returns with the next PDE step
    queued speculatively (QGModel.spec_pending); the model's own calls drop
    it before they run (QGModel.settle), and :meth:`settle` does so explicitly.

    ``link`` (dist.OwnerLink): this rank is the PDE owner of a sharded run —
    after each PDE step it publishes the new qk's top layer and dt to the
    other ranks (:class:`ReceiverLoop`), which build their snapshots from it."""

    SPEC_SLOT = 2  # ode23 + speculate: where the next step's snapshot is packed ahead (slots 0/1: the interval's)

    def __init__(self, model, ens, dt, U0, cfl_fraction=0.25, packet_delay=0.0, nsub=5, packet_intervals=1,
                 integrator="leapfrog", log=None, speculate=True, link=None, packet_method=None,
                 packet_iterations=None):
        self.model, self.ens, self.dt, self.U0 = model, ens, dt, U0
        self.link = link
        # speculate: each step also queues the NEXT PDE step with this step's
        # dt (swrt_qg_step_speculative) before waiting for this step's U0, so
        # the QG stream never idles through the host's read-back and CFL rule;
        # the rule then accepts it, or drops it and steps with its new dt —
        # the same computation either way (bit-identical files)
        self.speculate = speculate
        self.cfl_fraction, self.packet_delay = cfl_fraction, packet_delay
        self.nx = model.nx
        self.t = 0.0
        self.steps = 0
        self.dts = []
        self.have_cur = False
        self.log = log
        self.group = _IntervalGroup(model.ctx, ens, packet_intervals, nsub, integrator, packet_method,
                                    packet_iterations) if ens is not None else None
        # ode23 with speculation: the speculative step's snapshot is packed into
        # slot SPEC_SLOT while the interval runs; an accepted step takes it by
        # a slot swap instead of a snapshot launch between the intervals
        self._spec_snap = False
        # ode23 + speculate: chain each interval's stage 1 to the previous call
        # (swrt_ode23_chain_next; SWRT_ODE23_CHAIN=0 turns it off for A/B runs)
        self.chain = os.environ.get("SWRT_ODE23_CHAIN", "1") != "0"

    def step(self):
        """Returns True when the packets advanced through this PDE step."""
        self.steps += 1
        self.dt, changed = self.model.cfl_rule(self.dt, self.U0, self.cfl_fraction)
        if changed and self.log is not None:
            self.log(f"CFL condition not met, max|u|={self.U0:f}, new dt={self.dt:f}\n")
        self.dts.append(self.dt)
        if self.model.spec_pending:
            # the step queued by the previous call with the previous dt
            self.model.resolve(not changed)
            if changed:
                self.model.step(self.dt)
                self.model.max_speed_async()
        else:
            self.model.step(self.dt)
            self.model.max_speed_async()
        self.t = self.t + self.dt
        active = self.ens is not None and self.t > self.packet_delay
        spec = self.speculate and self.model.params.nlayers == 2 and getattr(self.model.ctx, "qg_fused", True)
        # ode23 intervals of a sharded run hold collectives (the error norm's
        # allreduce per attempt): the owner publishes before its interval, as
        # the receivers need this step's qk before theirs
        publish_first = self.link is not None and self.group is not None and self.group.integrator == "ode23"
        if publish_first:
            self.link.publish(self.model.ctx, self.dt)
        if active and self.ens.n == 0:
            # an owner without packets: no snapshots; the interval still runs
            # (ode23: its error-norm collectives) with the speculative step inside
            if spec and self.group.integrator == "ode23":
                dt = self.dt
                self.group.add(dt, hook=lambda: self.model.step_speculative(dt))
                spec = False
            else:
                self.group.add(self.dt)
        elif active:
            ny = 2 * self.nx
            if not self.have_cur:
                self.model.snapshot(0, which=1, layer=0, ny_period=ny)
            if self._spec_snap and not changed and self.have_cur:
                # this (accepted) step's snapshot, packed during the last interval
                self.model.ctx.swap_slots(self.group.next_slot(), self.SPEC_SLOT)
            else:
                self.model.snapshot(self.group.next_slot(), which=0, layer=0, ny_period=ny)
            self._spec_snap = False
            self.have_cur = True
            if spec and self.group.integrator == "ode23":
                # the ode23 interval holds the host until it ends (its step-size
                # controller), so the next PDE step — and its snapshot — are
                # queued from inside it, once its first launches are queued
                # (swrt_ode23_run_hooked), and run beside its attempts; the
                # leapfrog interval only queues work and returns
                dt = self.dt

                def hook():
                    self.model.step_speculative(dt)
                    self.model.snapshot_speculative(self.SPEC_SLOT, ny_period=ny)
                    self._spec_snap = True
                    if self.chain:  # (sharded too: swrt_ode23_run_sharded takes a chained stage 1)
                        # the next interval reads this one's end snapshot (slot
                        # 1) and the one just queued: its stage 1 is queued as
                        # this interval ends (taken only if still exact)
                        self.model.ctx.ode23_chain_next(1, self.SPEC_SLOT)
                self.group.add(dt, hook=hook)
                spec = False
            else:
                self.group.add(self.dt)
        else:
            self.have_cur = False
            self._spec_snap = False
        if spec:
            self.model.step_speculative(self.dt)
        if self.link is not None and not publish_first:
            # this step's committed qk to the other ranks: queued after the
            # next (speculative) step, so its host calls are off the PDE's
            # critical path (U0 read-back -> CFL rule -> next step)
            self.link.publish(self.model.ctx, self.dt)
        self.U0 = self.model.max_speed_result()  # this step's (read-backs pop oldest first)
        return active

    def flush(self):
        if self.group is not None:
            self.group.flush()

    def settle(self):
        """Drop a pending speculative step: the model stays at the committed
        step.  Optional: QGModel's step / max_speed / snapshot settle on their
        own, so PDE calls after the loop need no explicit settle."""
        self.model.settle()


class ReceiverLoop:
    """A receiving rank's iteration of qg2layersw_raytrace.m:152-197 in the
    PDE-owner form of a sharded run: no PDE here — the owner's dt and the
    new qk's top layer arrive through ``link`` (dist.OwnerLink) each step,
    grid_U of it (and, on the first active step, of the previous qk) goes
    into the packet slots (swrt_snapshot_qk: the owner's snapshot bits), and
    this rank's packets take the interval [t, t+dt] exactly as the owner's
    TwoLayerLoop does (same t, dt sequence, active steps and frame points)."""

    def __init__(self, link, ens, dt, packet_delay=0.0, nsub=5, packet_intervals=1, integrator="leapfrog",
                 ahead=None, packet_method=None, packet_iterations=None):
        self.link, self.ens, self.dt = link, ens, dt
        self.packet_delay = packet_delay
        self.t = 0.0
        self.steps = 0
        self.dts = []
        self.have_cur = False
        self.group = _IntervalGroup(ens.ctx, ens, packet_intervals, nsub, integrator, packet_method,
                                    packet_iterations) if ens is not None else None
        # The host queues step n only once the packet work of step n - ahead
        # has finished.  Unpaced, a receiver whose packets are slower than the
        # owner's PDE queues snapshots until every spare slot buffer still
        # looks in use; the next snapshot then waits for the packet launch
        # before it and packets and snapshots run one after the other
        # (swrt_qg_snapshot's renaming decides at queue time).
        # the mark is an event recorded after every 2nd step's packet work (an
        # event between two kernels costs ~6 us of idle GPU, tools/owner_legs.py
        # traces), so the host is `ahead` to `ahead` + 1 steps ahead
        self.mark_every = 2
        nbuf = getattr(link, "nbuf", 2)
        self.ahead = (nbuf - self.mark_every - 1) if ahead is None else int(ahead)
        self._done = []  # (step, event)
        self._pk = None
        if self.ahead > 0 and ens is not None and ens.n > 0 and getattr(link, "device", False):
            import torch
            self._pk = torch.cuda.ExternalStream(ens.ctx.stream())
            self._events = [torch.cuda.Event() for _ in range(self.ahead + 2)]
            self._ev_i = 0
        # device link with pacing: the host waits for each broadcast and the
        # pacing orders the buffers' refills, so the snapshots need no
        # cross-stream events (OwnerLink.snapshot fenced): the buffer of step m
        # is read by step m's snapshot and, on a first active step, by step
        # m + 1's grid_U(prev_qk); it is refilled by receive m + nbuf, by which
        # the host has waited for the packet work of step m + nbuf - ahead -
        # mark_every or later — after both reads when that is >= m + 1
        self._fenced = self._pk is not None and self.ahead + self.mark_every + 1 <= nbuf

    def _snapshot(self, slot, which):
        e = self.ens
        self.link.snapshot(e.ctx, slot, which, e.L, e.K_d2, e.shear, e.k_scale, e.ny_period, fenced=self._fenced)

    def step(self):
        self.steps += 1
        while self._done and self._done[0][0] <= self.steps - 1 - self.ahead:
            self._done.pop(0)[1].synchronize()
        self.dt = self.link.receive(wait=self._fenced)
        self.dts.append(self.dt)
        self.t = self.t + self.dt
        active = self.ens is not None and self.t > self.packet_delay
        if active:
            if self.ens.n > 0:
                if not self.have_cur:
                    self._snapshot(0, 1)  # grid_U(prev_qk)
                self._snapshot(self.group.next_slot(), 0)  # grid_U(qk)
                self.have_cur = True
            self.group.add(self.dt)
            if self._pk is not None and self.steps % self.mark_every == 0:
                ev = self._events[self._ev_i]
                self._ev_i = (self._ev_i + 1) % len(self._events)
                ev.record(self._pk)
                self._done.append((self.steps, ev))
        else:
            self.have_cur = False
        return active

    def flush(self):
        if self.group is not None:
            self.group.flush()

    def settle(self):
        pass


@_ends_tangent
def qgsw_raytrace(nx, Npackets, near_inertial_factor, T_Fr_days, packet_delay_days, U_g, f, Cg, *,
                  out_dir="data", nsub=4, max_steps=None, seed=146, verbose=False, r_drag=0.1,
                  packet_intervals=1, integrator="leapfrog", fresh=True, ctx: Context | None = None,
                  pde="owner", owner_weight=None, link_buffers="auto", spectrum_edges=None, packet_files=True,
                  map_cells=None, map_frac_bits=20, track_ids=None, track_every=None,
                  kmap_cells=None, kmap_kmax=None, kmap_frac_bits=16, flow_spectrum=False,
                  cond_by=None, cond_edges=None, cond_frac_bits=20,
                  trans_src_edges=None, trans_by=None, trans_lag=None, trans_frac_bits=20,
                  recycle_omega=None, recycle_seed=0, recycle_every=1, recycle_frac_bits=20,
                  refr_edges=None, refr_frac_bits=20, absfreq_edges=None, absfreq_frac_bits=20,
                  tangent_edges=None, tangent_lag=1,
                  packet_method="leapfrog", packet_iterations=None):
    """qgsw_raytrace.m:1-180 with the PDE and the packets on the GPU.

    Writes ``out_dir``/packet_x.bin, packet_k.bin, packet_time.bin, pv.bin,
    pv_time.bin (frames appended, write_field.m) and run.log.  ``max_steps``
    bounds the run (None: the reference's Nsteps = ceil(T/dt)).  ``r_drag``
    (0.1 in the reference, :25) enters update as the literal `+ r_drag*K2`
    term of :285, which forces every mode and makes long runs blow up; pass
    0 to drop it.  ``packet_intervals`` (1..4): PDE steps whose packet
    intervals go to the device in one call (results identical for any
    value; 1 is faster end to end here: the PDE chain's latency, not the
    packet launch, bounds a driver step).  ``integrator``:
    "leapfrog" (``nsub`` fused symplectic substeps per PDE interval) or
    "ode23" (the reference's own ode23 over each interval, qgsw_raytrace.m:149).
    ``packet_method``, ``packet_iterations`` (leapfrog integrator only): the
    packet step, "leapfrog" (the reference's, first order), "midpoint",
    "yoshida4" or "suzuki4" (integrate.packet_method); a step other than the
    default adds one line to run.log after the parameter block.
    ``fresh``: remove earlier output files first (default) or append to
    them as write_field.m:31 does.  ``pde``, ``owner_weight``: the sharded
    forms, as in :func:`qg2layersw_raytrace`.  ``spectrum_edges`` (nbins + 1
    increasing values): every packet frame's energy-vs-omega counts and
    statistics are recorded on the device (analysis/load_data.m:33-52,63;
    swrt_omega_series_*) and written at the end as omega_hist.bin (nbins + 2
    values per frame: below, the bins, above), omega_stats.bin (n, sum omega,
    min, max per frame) and omega_edges.bin.  ``packet_files=False`` skips the
    packet_x.bin / packet_k.bin downloads and writes (packet_time.bin stays:
    the spectrum frames' times); it needs ``spectrum_edges``.  ``map_cells``
    (m, 1..4096): every packet frame's m x m packet density and wave-energy
    map over the domain is recorded on the device (swrt_map_series_*; moments
    quantised to 2^-``map_frac_bits``) and written as map_n.bin, map_omega.bin,
    map_k.bin, map_l.bin (one m x m frame each per packet frame, exact
    integers) and map_stats.bin (n, rejected, m, frac_bits per frame).
    ``track_ids`` (a sequence of distinct packet ids, or an integer K for
    arange(K) * (Npackets // K)): the trajectories of those packets are
    recorded on the device (swrt_track_*) every ``track_every`` PDE steps
    (default: the packet frames' cadence, 5) and written at the end as
    track_x.bin, track_k.bin (m x 2 per frame, the layout of packet_x.bin /
    packet_k.bin: load_data.m reads them with Npackets = m), track_diag.bin
    (m x 4: Omega, zeta, sigma, D of swrt_raydiag_sample at the packets' time;
    NaN in the first frame, written before any snapshot exists),
    track_time.bin and track_ids.bin; no other output changes.
    ``kmap_cells`` (m, 1..4096): every packet frame's m x m count plane over
    [-K, K) x [-K, K) of the (k, l) plane and the ensemble's wavevector
    moments are recorded on the device (swrt_kmap_series_*; K = ``kmap_kmax``,
    default four times the initial ring's radius; moments quantised to
    2^-``kmap_frac_bits``) and written as kmap_n.bin (int64, m x m per frame,
    cell (i, j) at i + m*j, first index k), kmap_stats.bin (8 int64 per frame:
    n, rejected, outside, sum q(k), sum q(l), sum q(k*k), sum q(l*l),
    sum q(k*l)) and kmap_geom.bin (three doubles K, m, frac_bits); the frames
    line up with packet_time.bin, and ``packet_files=False`` is allowed with
    ``kmap_cells`` alone.
    ``flow_spectrum``: at every packet frame the rank that steps the PDE
    (rank 0 when sharded, whether or not it holds packets) records the shell
    spectra of layer 0's committed qk on the device (swrt_flow_spectrum_*, on
    the QG stream, no host wait), written at the end as flow_spec.bin (float64,
    3*nshell per frame: E, Z, Q per shell), flow_stats.bin ([t, sum E, sum Z,
    sum Q] per frame; t lines up with packet_time.bin) and flow_geom.bin
    ([nx, nshell, k_scale, K_d2, layer]); no other output changes.
    ``cond_by`` ("zeta", "sigma" or "D"; needs ``spectrum_edges`` and
    ``cond_edges``, the nq + 1 increasing class edges of that scalar): beside
    every packet frame but the first (written before any snapshot exists) the
    counts of the packets over the omega classes of ``spectrum_edges`` by the
    classes of the flow's vorticity, strain or Okubo-Weiss at each packet are
    recorded on the device (swrt_cond_series_*; the snapshot at the packets'
    time) and written as cond_hist.bin (int64, (nq + 2) x (nw + 2) per frame,
    cell (qc, wc) at qc*(nw + 2) + wc), cond_sums.bin (nq + 2 int64 per frame:
    the sum of rint(omega * 2^``cond_frac_bits``) per q class), cond_stats.bin
    (n, rejected per frame) and cond_geom.bin (doubles: which, nq, nw,
    frac_bits, the q edges, the omega edges); frame i belongs to packet frame
    i + 1; no other output changes.
    ``near_inertial_factor`` may be a sequence of R factors: the packets start
    on R rings in contiguous blocks [r N // R, (r + 1) N // R), one PDE run
    carrying the reference's whole omega0 sweep (the packets do not interact);
    a scalar takes exactly the one-ring path.  The parameter block keeps the
    first ring's value and one line after it lists all rings.
    ``trans_src_edges`` (the ns + 1 increasing class edges of omega at the
    mark; needs ``spectrum_edges``) or ``trans_by="ring"`` (source = the ring
    index, edges -0.5 .. R - 0.5, never re-marked): the transition series
    (swrt_trans_series_*).  The mark is taken at the first packet frame, every
    later packet frame records the counts of the packets over (source class,
    omega class) with the per-class sums of omega, d = omega - source and d^2
    in quanta of 2^-``trans_frac_bits``, and with ``trans_lag`` = m the source
    is re-marked after the record of every packet frame whose index m divides.
    Written as trans_hist.bin (int64, (ns + 2) x (nw + 2) per frame),
    trans_sums.bin (3 (ns + 2) int64), trans_stats.bin (n, rejected, mark
    serial), trans_time.bin (doubles t, t_mark) and trans_geom.bin (doubles:
    ns, nw, frac_bits, by (0 omega / 1 ring), the source edges, the omega
    edges); frame i belongs to packet frame i + 1; no other output changes and
    ``packet_files=False`` is allowed with it.
    ``recycle_omega`` (above the largest ring's omega0; not together with
    ``trans_src_edges``, whose omega mark a re-injected packet would make
    stale, while ``trans_by="ring"`` is allowed: home keeps the ring; needs
    packets): packet recycling (swrt_recycle_*), a sink at that omega and a
    source at omega0 with N fixed.  At every packet frame after the first whose
    index ``recycle_every`` divides, after the packets reached the frame's time
    and before the frame is saved, every packet with omega >= ``recycle_omega``
    is absorbed and re-injected in place with its initial wavevector and a
    fresh uniform position from a hash of (``recycle_seed``, its global index,
    its generation): a saved frame holds no packet at or above the cut, and the
    files do not depend on the sharding.  Both integrators are allowed.
    Written as recycle_stats.bin (8 int64 per event: n, absorbed, rejected,
    sum q(omega_out), sum q(omega_home), sum age, max age, serial; sums in
    quanta of 2^-``recycle_frac_bits``, ages in events), recycle_time.bin (one
    double per event), recycle_geom.bin (doubles omega_cut, L, seed, frac_bits,
    f, Cg, every) and recycle_gen.bin (int32 per packet in the original order:
    its re-injections, written at the end); the other outputs are those of the
    recycled packets.
    ``refr_edges`` (the na + 1 increasing class edges of the alignment
    c = 2 gamma / sigma, e.g. alignment_edges(na); needs ``spectrum_edges``):
    the refraction series (swrt_refr_series_*).  Beside every packet frame but
    the first (written before any snapshot exists), after a recycle event that
    falls on the frame, the counts of the packets over (alignment class, omega
    class) and the per-class sums of omega-dot, omega-dot^2 and
    gamma = d ln|k|/dt in quanta of 2^-``refr_frac_bits`` are recorded on the
    device in the snapshot at the packets' time and written as refr_hist.bin
    (int64, (na + 2) x (nw + 2) per frame, cell (ac, wc) at ac*(nw + 2) + wc),
    refr_sums.bin (3 (nw + 2) + (na + 2) int64 per frame: omega-dot,
    omega-dot^2 and gamma per omega class, then omega-dot per alignment
    class), refr_stats.bin (n, rejected per frame) and refr_geom.bin (doubles:
    na, nw, frac_bits, the alignment edges, the omega edges); frame i belongs
    to packet frame i + 1; no other output changes and ``packet_files=False``
    is allowed with it.
    ``absfreq_edges`` (the no + 1 increasing class edges of the absolute
    frequency Omega = omega + U.k; needs ``spectrum_edges``): the
    absolute-frequency series (swrt_absfreq_series_*).  Beside every packet
    frame but the first, after a recycle event that falls on the frame, the
    counts of the packets over (Omega class, omega class) and the per-class
    sums of dOmega/dt = k.dU/dt, its square and the Doppler shift U.k in
    quanta of 2^-``absfreq_frac_bits`` are recorded on the device from the two
    snapshots that bracket the last completed PDE interval, at alpha = 1 with
    tau that interval's dt (the flow at the packets' time, the rate of the
    interval they just crossed), and written as absfreq_hist.bin (int64,
    (no + 2) x (nw + 2) per frame, cell (oc, wc) at oc*(nw + 2) + wc),
    absfreq_sums.bin (3 (nw + 2) + 2 (no + 2) int64 per frame: Omega-dot,
    Omega-dot^2 and U.k per omega class, then Omega-dot and Omega-dot^2 per
    Omega class), absfreq_stats.bin (n, rejected per frame) and
    absfreq_geom.bin (doubles: no, nw, frac_bits, the Omega edges, the omega
    edges); frame i belongs to packet frame i + 1; run.log gets one line after
    its parameter block; no other output changes and ``packet_files=False`` is
    allowed with it.
    Returns a dict of run facts (dt, Nsteps, steps run, frames written,
    final t, spectrum_frames, map_frames, track_frames, kmap_frames,
    flow_frames, cond_frames, trans_frames, recycle_events, refr_frames,
    absfreq_frames, tangent_frames).
    ``tangent_edges`` (needs ``spectrum_edges``; integrator="leapfrog",
    packet_method="leapfrog" and no ``recycle_omega``, else ValueError): the
    packets carry the tangent map M of the discrete step from the first packet
    frame on (swrt_tangent_*: the leapfrog calls take the per-packet route; x
    and k keep their bits) and every later packet frame records a tangent
    frame over the growth classes ``tangent_edges`` (of s = |M|_F^2 / 4) by
    the omega classes, then, with ``tangent_lag`` = m (default 1), re-marks
    (M = I) after every m-th frame.  Written as tangent_hist.bin,
    tangent_sums.bin, tangent_stats.bin, tangent_time.bin (t and t_mark per
    frame) and tangent_geom.bin (PacketEnsemble.write_tangents); frame i
    belongs to packet frame i + 1."""
    _flow_args(flow_spectrum, Npackets)
    spectrum_edges = _spectrum_args(spectrum_edges, packet_files, kmap_cells)
    map_args = _map_args(map_cells, map_frac_bits)
    ring_factors, several_rings = _ring_factors(near_inertial_factor)
    kmap_args = _kmap_args(kmap_cells, kmap_kmax, kmap_frac_bits,
                           _ring_radius(max(ring_factors), f, Cg) if kmap_cells is not None else None)
    track_args = _track_args(track_ids, track_every, Npackets, 5)  # (5: packet_steps_per_save below)
    cond_args = _cond_args(cond_by, cond_edges, cond_frac_bits, spectrum_edges)
    refr_args = _refr_args(refr_edges, refr_frac_bits, spectrum_edges)
    absfreq_args = _absfreq_args(absfreq_edges, absfreq_frac_bits, spectrum_edges)
    method_args = _packet_method_args(packet_method, packet_iterations, integrator)
    trans_args = _trans_args(trans_src_edges, trans_by, trans_lag, trans_frac_bits, spectrum_edges, len(ring_factors))
    tangent_args = _tangent_args(tangent_edges, tangent_lag, spectrum_edges, integrator, packet_method, recycle_omega,
                                 Npackets)
    if trans_args is not None and Npackets <= 0:
        raise ValueError("the transition series needs packets")
    recycle_args = _recycle_args(recycle_omega, recycle_seed, recycle_every, recycle_frac_bits, ring_factors, f,
                                 trans_src_edges, Npackets)
    ctx = ctx if ctx is not None else Context(0)
    timing = getattr(ctx, "timing_every", 1)
    ctx.set_timing(0)  # (no HIP-event pair around every packet launch; restored at the end)
    integ = ctx.get_integrator()  # (the ensemble sets the packet step on the context; restored at the end)
    rank, world = _dist_info()  # sharded run: packets split over the ranks
    if rank == 0:
        _fresh_outputs(out_dir, fresh)
    log = RunLog(os.path.join(out_dir, "run.log") if rank == 0 else None, verbose and rank == 0)
    L = 2 * math.pi
    dx = L / nx
    rng = np.random.default_rng(seed)
    K_d2 = f / Cg
    T_days = T_Fr_days / f
    CFL_fraction = 0.05
    steps_per_save = 50
    packet_delay = packet_delay_days / f
    packet_steps_per_save = 5
    q = initial_q(nx, L, U_g, K_d2, 5, 8, rng)
    qk = ctx.g2k(q)
    x, k = _packets(Npackets, L, near_inertial_factor, f, Cg, rng)
    model = QGModel.one_layer(qk, nx, f, Cg, r_drag=r_drag, ctx=ctx)
    link, bounds = _owner_setup(world, pde, owner_weight, nx, Npackets, link_buffers)
    if link is not None:
        link.seed(ctx)
    owner = link is None or rank == 0  # this rank steps the PDE
    if link is not None and owner:
        link.bind_owner(ctx)
    if not owner:
        ctx.qg_set_stream(False)  # (snapshots in series with the packets, as in qg2layersw_raytrace)
        ctx.set_packet_streams(1)
    U0 = model.max_speed()
    Fr = U0 / Cg
    T = T_days / Fr ** 2
    dt = CFL_fraction * dx / U0
    Nsteps = math.ceil(T / dt)
    packet_step_start = math.ceil(packet_delay / dt)
    log(parameter_block(nx, Npackets, ring_factors[0] * f, dt, T, packet_delay, steps_per_save,
                        packet_steps_per_save, f, Cg, U_g, U0, Fr, K_d2))
    if several_rings:
        log(_rings_line(ring_factors, f, Cg))
    if absfreq_args is not None:
        log(("\n" if several_rings else "") + _absfreq_line(*absfreq_args) + "\n")  # (a line of its own)
    if method_args != ("leapfrog", None):
        log(("\n" if several_rings and absfreq_args is None else "") + _packet_method_line(*method_args) + "\n")
    ens = PacketEnsemble(x, k, L, f, Cg, nx, K_d2, shear=0.0, k_scale=1.0, nlayers=1, bump=BUMP_QG, ctx=ctx,
                         shard=(rank, world), bounds=bounds, method=method_args[0], iterations=method_args[1]) \
        if Npackets > 0 else None

    def snapshot(slot, which):
        if owner:
            model.snapshot(slot, which=which)
        else:
            link.snapshot(ctx, slot, which, L, K_d2, 0.0, 1.0, 0)
    t = 0.0
    frames = 1
    spectrum = ens is not None and spectrum_edges is not None
    if spectrum:
        ens.begin_spectrum(spectrum_edges)
    maps = ens is not None and map_args is not None
    if maps:
        ens.begin_map(*map_args, directory=out_dir)
    kmaps = ens is not None and kmap_args is not None
    if kmaps:
        ens.begin_kmap(*kmap_args, directory=out_dir)
    conds = ens is not None and cond_args is not None
    if conds:  # (no frame beside the first packet frame: no snapshot exists yet)
        ens.begin_cond(spectrum_edges, cond_args[0], cond_args[1], cond_args[2], directory=out_dir)
    refrs = ens is not None and refr_args is not None
    if refrs:  # (no frame beside the first packet frame: no snapshot exists yet)
        ens.begin_refr(spectrum_edges, refr_args[0], refr_args[1], directory=out_dir)
    absfreqs = ens is not None and absfreq_args is not None
    if absfreqs:  # (no frame beside the first packet frame: no interval is complete yet)
        ens.begin_absfreq(spectrum_edges, absfreq_args[0], absfreq_args[1], directory=out_dir)
    trans = None  # (the lag, 0: never re-marked; None: no transition series)
    if ens is not None and trans_args is not None:  # (the mark beside the first packet frame; frames from the second on)
        _begin_trans(ens, trans_args, spectrum_edges, out_dir, dt * (packet_step_start - 1), Npackets,
                     len(ring_factors))
        trans = trans_args[2] or 0
    tangent = None  # (the lag; None: no tangent series)
    if ens is not None and tangent_args is not None:  # (M = I beside the first packet frame; frames from the second on)
        ens.begin_tangent(spectrum_edges, tangent_args[0], directory=out_dir, t=dt * (packet_step_start - 1))
        tangent = tangent_args[1]
    recycle = 0  # (packet frames per recycle event; 0: no recycling)
    if ens is not None and recycle_args is not None:  # (events from the second packet frame on)
        ens.begin_recycle(recycle_args[0], seed=recycle_args[1], frac_bits=recycle_args[3], directory=out_dir,
                          every=recycle_args[2])
        recycle = recycle_args[2]
    tracks = ens is not None and track_args is not None
    if tracks:
        ens.begin_tracks(track_args[0], directory=out_dir)
        ens.record_tracks(dt * (packet_step_start - 1), 0)  # (no snapshot yet: the flow columns are NaN)
    flows = bool(flow_spectrum) and rank == 0  # (rank 0 steps the PDE in both sharded forms)
    if flows:
        model.begin_flow_spectrum(0)
        model.record_flow_spectrum()
    if ens is not None:
        _save_frame(ens, dt * (packet_step_start - 1), out_dir, spectrum, packet_files, maps, kmaps)
    if rank == 0:
        write_field(model.q(), os.path.join(out_dir, "pv"))
        write_field(np.array([[t]]), os.path.join(out_dir, "pv_time"))
    nrun = Nsteps if max_steps is None else min(Nsteps, int(max_steps))
    have_cur = False
    group = _IntervalGroup(ctx, ens, packet_intervals, nsub, integrator) if ens is not None else None
    log.start()
    for step in range(1, nrun + 1):
        if owner:
            model.step(dt)
            if link is not None:
                link.publish(ctx, dt)
        else:
            link.receive()  # (the 1-layer driver's dt is fixed)
        t = t + dt
        if ens is not None and t > packet_delay:
            if ens.n > 0:
                if not have_cur:
                    snapshot(0, 1)  # grid_U(prev_qk); later groups start from the last grid_U(qk)
                snapshot(group.next_slot(), 0)  # grid_U(qk)
            have_cur = True
            group.add(dt)
            if tracks and (step - packet_step_start + 1) % track_args[1] == 0:
                group.flush()  # (slot 0 now holds the snapshot at the packets' time)
                ens.record_tracks(t, 1)
            if (step - packet_step_start + 1) % packet_steps_per_save == 0:
                group.flush()
                if recycle and frames % recycle == 0:
                    ens.recycle(t)  # (before the frame: it holds no packet at or above the cut)
                _save_frame(ens, t, out_dir, spectrum, packet_files, maps, kmaps, conds, trans, frames, refrs,
                            group.last if absfreqs else None, tangent)
                if flows:
                    model.record_flow_spectrum()
                frames += 1
        else:
            have_cur = False
        if step % steps_per_save == 0 and rank == 0:
            write_field(model.q(), os.path.join(out_dir, "pv"))
            write_field(np.array([[t]]), os.path.join(out_dir, "pv_time"))
        log.progress(step, Nsteps)
    if group is not None:
        group.flush()
    if link is not None:
        link.close()
    spectrum_frames = ens.write_spectrum(out_dir) if spectrum else 0
    map_frames = ens.write_maps(out_dir) if maps else 0
    track_frames = ens.write_tracks(out_dir) if tracks else 0
    kmap_frames = ens.write_kmaps(out_dir) if kmaps else 0
    cond_frames = ens.write_conds(out_dir) if conds else 0
    trans_frames = ens.write_trans(out_dir) if trans is not None else 0
    recycle_events = ens.write_recycle(out_dir) if recycle else 0
    refr_frames = ens.write_refrs(out_dir) if refrs else 0
    absfreq_frames = ens.write_absfreqs(out_dir) if absfreqs else 0
    tangent_frames = ens.write_tangents(out_dir) if tangent is not None else 0
    if tangent is not None:
        ens.end_tangent()  # (the context goes back to the route its settings name)
    if flows:
        model.write_flow_spectrum(out_dir, first_time=dt * (packet_step_start - 1))
    flow_frames = frames if flow_spectrum else 0
    ctx.synchronize()
    ctx.set_timing(timing)
    ctx.set_integrator(*integ)
    log.finish()
    log.close()
    return dict(dt=dt, Nsteps=Nsteps, steps=nrun, packet_frames=frames, t=t, U0=U0,
                packet_step_start=packet_step_start, spectrum_frames=spectrum_frames, map_frames=map_frames,
                track_frames=track_frames, kmap_frames=kmap_frames, flow_frames=flow_frames, cond_frames=cond_frames,
                trans_frames=trans_frames, recycle_events=recycle_events, refr_frames=refr_frames,
                absfreq_frames=absfreq_frames, tangent_frames=tangent_frames)


@_ends_tangent
def qg2layersw_raytrace(nx, Npackets, near_inertial_factor, T_Fr_days, packet_delay_Fr_days, U_g, f, Cg, *,
                        out_dir="data", nsub=5, max_steps=None, seed=5, verbose=False,
                        packet_intervals=1, integrator="leapfrog", fresh=True, ctx: Context | None = None,
                        pde="owner", owner_weight=None, link_buffers="auto", spectrum_edges=None,
                        packet_files=True, map_cells=None, map_frac_bits=20, track_ids=None, track_every=None,
                        kmap_cells=None, kmap_kmax=None, kmap_frac_bits=16, flow_spectrum=False,
                        cond_by=None, cond_edges=None, cond_frac_bits=20,
                        trans_src_edges=None, trans_by=None, trans_lag=None, trans_frac_bits=20,
                        recycle_omega=None, recycle_seed=0, recycle_every=1, recycle_frac_bits=20,
                        refr_edges=None, refr_frac_bits=20, absfreq_edges=None, absfreq_frac_bits=20,
                        tangent_edges=None, tangent_lag=1,
                        packet_method="leapfrog", packet_iterations=None):
    """qg2layersw_raytrace.m:1-247 with the PDE and the packets on the GPU
    (adaptive CFL :156-165, packets on layer 1 with u += shear_strength and
    interpolate's 2*nx y-period).  Same packet outputs as :func:`qgsw_raytrace`;
    pv.bin holds the initial nx x nx x 2 frame only, as in the reference.
    ``packet_intervals``, ``integrator``, ``packet_method``,
    ``packet_iterations``, ``fresh``, ``spectrum_edges``,
    ``packet_files``, ``map_cells``, ``map_frac_bits``, ``kmap_cells``,
    ``kmap_kmax``, ``kmap_frac_bits``, ``track_ids``,
    ``track_every`` (default: this driver's packet cadence, 25),
    ``flow_spectrum``, ``cond_by``, ``cond_edges``, ``cond_frac_bits``,
    ``trans_src_edges``, ``trans_by``, ``trans_lag``, ``trans_frac_bits``,
    ``recycle_omega``, ``recycle_seed``, ``recycle_every``,
    ``recycle_frac_bits``, ``refr_edges``, ``refr_frac_bits``,
    ``absfreq_edges``, ``absfreq_frac_bits``, ``tangent_edges``,
    ``tangent_lag`` and a
    sequence of factors as ``near_inertial_factor``: as in
    :func:`qgsw_raytrace`.

    Sharded (torch.distributed, world > 1): ``pde="owner"`` (default) — rank 0
    steps the PDE and sends each step's top-layer qk and dt to the other
    ranks, which only build snapshots and advance packets; rank 0 holds
    ``owner_weight`` packets per packet of another rank (dist.owner_bounds;
    default owner_weight_for(world)).
    ``pde="replicated"``: every rank steps the same PDE, packets split evenly.
    Both write the single-process files byte for byte.  ``link_buffers``: the
    owner link's buffers ("auto": on the device with nccl, on the host with
    gloo; "device" / "host" to force one)."""
    spectrum_edges = _spectrum_args(spectrum_edges, packet_files, kmap_cells)
    map_args = _map_args(map_cells, map_frac_bits)
    ring_factors, several_rings = _ring_factors(near_inertial_factor)
    kmap_args = _kmap_args(kmap_cells, kmap_kmax, kmap_frac_bits,
                           _ring_radius(max(ring_factors), f, Cg) if kmap_cells is not None else None)
    track_args = _track_args(track_ids, track_every, Npackets, 25)  # (25: packet_steps_per_save below)
    cond_args = _cond_args(cond_by, cond_edges, cond_frac_bits, spectrum_edges)
    refr_args = _refr_args(refr_edges, refr_frac_bits, spectrum_edges)
    absfreq_args = _absfreq_args(absfreq_edges, absfreq_frac_bits, spectrum_edges)
    method_args = _packet_method_args(packet_method, packet_iterations, integrator)
    trans_args = _trans_args(trans_src_edges, trans_by, trans_lag, trans_frac_bits, spectrum_edges, len(ring_factors))
    tangent_args = _tangent_args(tangent_edges, tangent_lag, spectrum_edges, integrator, packet_method, recycle_omega,
                                 Npackets)
    if trans_args is not None and Npackets <= 0:
        raise ValueError("the transition series needs packets")
    recycle_args = _recycle_args(recycle_omega, recycle_seed, recycle_every, recycle_frac_bits, ring_factors, f,
                                 trans_src_edges, Npackets)
    _flow_args(flow_spectrum, Npackets)
    ctx = ctx if ctx is not None else Context(0)
    timing = getattr(ctx, "timing_every", 1)
    ctx.set_timing(0)  # (no HIP-event pair around every packet launch; restored at the end)
    integ = ctx.get_integrator()  # (the ensemble sets the packet step on the context; restored at the end)
    rank, world = _dist_info()  # sharded run: packets split over the ranks
    if rank == 0:
        _fresh_outputs(out_dir, fresh)
    log = RunLog(os.path.join(out_dir, "run.log") if rank == 0 else None, verbose and rank == 0)
    L = 20.0
    dx = L / nx
    rng = np.random.default_rng(seed)
    K_d2 = f / Cg
    shear = 0.5
    T_Fr = T_Fr_days / f
    packet_delay_Fr = packet_delay_Fr_days / f
    CFL_fraction = 0.25
    steps_per_save = 10
    packet_delay_steps = packet_delay_Fr / f
    packet_steps_per_save = 25
    q1 = initial_q(nx, L, U_g, K_d2, 10, 30, rng, ndgrid=True)
    qk1 = ctx.g2k(q1)
    qk2 = ctx.g2k(-q1)
    qk = np.stack([qk1, qk2], axis=2)
    x, k = _packets(Npackets, L, near_inertial_factor, f, Cg, rng)
    model = QGModel.two_layer(qk, nx, f, Cg, L=L, shear=shear, ctx=ctx)  # (every rank: the same U0, T, dt)
    link, bounds = _owner_setup(world, pde, owner_weight, nx, Npackets, link_buffers)
    if link is not None:
        link.seed(ctx)
    U0 = model.max_speed()
    Fr = U0 / Cg
    T = T_Fr / Fr ** 2
    dt = CFL_fraction * dx / U0
    Nsteps = math.ceil(T / dt)
    packet_step_start = math.ceil(packet_delay_steps / dt)
    log(parameter_block(nx, Npackets, ring_factors[0] * f, dt, T, packet_delay_steps, steps_per_save,
                        packet_steps_per_save, f, Cg, U_g, U0, Fr, K_d2, two_layer=True))
    if several_rings:
        log(_rings_line(ring_factors, f, Cg))
    if absfreq_args is not None:
        log(("\n" if several_rings else "") + _absfreq_line(*absfreq_args) + "\n")  # (a line of its own)
    if method_args != ("leapfrog", None):
        log(("\n" if several_rings and absfreq_args is None else "") + _packet_method_line(*method_args) + "\n")
    ens = PacketEnsemble(x, k, L, f, Cg, nx, K_d2, shear=shear, k_scale=2 * math.pi / L, nlayers=2,
                         bump=BUMP_QG, ctx=ctx, shard=(rank, world), bounds=bounds, method=method_args[0],
                         iterations=method_args[1]) if Npackets > 0 else None
    t = 0.0
    frames = 1
    spectrum = ens is not None and spectrum_edges is not None
    if spectrum:
        ens.begin_spectrum(spectrum_edges)
    maps = ens is not None and map_args is not None
    if maps:
        ens.begin_map(*map_args, directory=out_dir)
    kmaps = ens is not None and kmap_args is not None
    if kmaps:
        ens.begin_kmap(*kmap_args, directory=out_dir)
    conds = ens is not None and cond_args is not None
    if conds:  # (no frame beside the first packet frame: no snapshot exists yet)
        ens.begin_cond(spectrum_edges, cond_args[0], cond_args[1], cond_args[2], directory=out_dir)
    refrs = ens is not None and refr_args is not None
    if refrs:  # (no frame beside the first packet frame: no snapshot exists yet)
        ens.begin_refr(spectrum_edges, refr_args[0], refr_args[1], directory=out_dir)
    absfreqs = ens is not None and absfreq_args is not None
    if absfreqs:  # (no frame beside the first packet frame: no interval is complete yet)
        ens.begin_absfreq(spectrum_edges, absfreq_args[0], absfreq_args[1], directory=out_dir)
    trans = None  # (the lag, 0: never re-marked; None: no transition series)
    if ens is not None and trans_args is not None:  # (the mark beside the first packet frame; frames from the second on)
        _begin_trans(ens, trans_args, spectrum_edges, out_dir, dt * (packet_step_start - 1), Npackets,
                     len(ring_factors))
        trans = trans_args[2] or 0
    tangent = None  # (the lag; None: no tangent series)
    if ens is not None and tangent_args is not None:  # (M = I beside the first packet frame; frames from the second on)
        ens.begin_tangent(spectrum_edges, tangent_args[0], directory=out_dir, t=dt * (packet_step_start - 1))
        tangent = tangent_args[1]
    recycle = 0  # (packet frames per recycle event; 0: no recycling)
    if ens is not None and recycle_args is not None:  # (events from the second packet frame on)
        ens.begin_recycle(recycle_args[0], seed=recycle_args[1], frac_bits=recycle_args[3], directory=out_dir,
                          every=recycle_args[2])
        recycle = recycle_args[2]
    tracks = ens is not None and track_args is not None
    if tracks:
        ens.begin_tracks(track_args[0], directory=out_dir)
        ens.record_tracks(dt * (packet_step_start - 1), 0)  # (no snapshot yet: the flow columns are NaN)
    flows = bool(flow_spectrum) and rank == 0  # (rank 0 steps the PDE in both sharded forms)
    if flows:
        model.begin_flow_spectrum(0)
        model.record_flow_spectrum()
    if ens is not None:
        _save_frame(ens, dt * (packet_step_start - 1), out_dir, spectrum, packet_files, maps, kmaps)
    if rank == 0:
        write_field(model.q(), os.path.join(out_dir, "pv"))
        write_field(np.array([[t]]), os.path.join(out_dir, "pv_time"))
    if link is not None and rank == 0:
        link.bind_owner(ctx)
    if link is not None and rank != 0:
        # a receiving rank runs its snapshots on the packet stream: beside its
        # packet launches the transforms run several times slower (they find
        # no free slots), so in series they cost less (bench.py owner legs)
        ctx.qg_set_stream(False)
        ctx.set_packet_streams(1)  # (the snapshot follows the whole previous launch, not beside its second part)
        loop = ReceiverLoop(link, ens, dt, packet_delay_steps, nsub, packet_intervals, integrator)
    else:
        loop = TwoLayerLoop(model, ens, dt, U0, CFL_fraction, packet_delay_steps, nsub, packet_intervals, integrator,
                            log, link=link)
    # (the reference only plots q every steps_per_save steps in this loop; its
    # pv.bin writes are commented out, qg2layersw_raytrace.m:211-239)
    log.start()
    while loop.t <= T and (max_steps is None or loop.steps < max_steps):
        active = loop.step()
        if active and tracks and (loop.steps - packet_step_start + 1) % track_args[1] == 0:
            loop.flush()  # (slot 0 now holds the snapshot at the packets' time)
            ens.record_tracks(loop.t, 1)
        if active and (loop.steps - packet_step_start + 1) % packet_steps_per_save == 0:
            loop.flush()
            if recycle and frames % recycle == 0:
                ens.recycle(loop.t)  # (before the frame: it holds no packet at or above the cut)
            _save_frame(ens, loop.t, out_dir, spectrum, packet_files, maps, kmaps, conds, trans, frames, refrs,
                        loop.group.last if absfreqs else None, tangent)
            if flows:
                model.record_flow_spectrum()  # (the committed qk at loop.t; the next step is only speculative)
            frames += 1
        log.progress(loop.steps, Nsteps)
    loop.flush()
    loop.settle()
    if link is not None:
        link.close()
    spectrum_frames = ens.write_spectrum(out_dir) if spectrum else 0
    map_frames = ens.write_maps(out_dir) if maps else 0
    track_frames = ens.write_tracks(out_dir) if tracks else 0
    kmap_frames = ens.write_kmaps(out_dir) if kmaps else 0
    cond_frames = ens.write_conds(out_dir) if conds else 0
    trans_frames = ens.write_trans(out_dir) if trans is not None else 0
    recycle_events = ens.write_recycle(out_dir) if recycle else 0
    refr_frames = ens.write_refrs(out_dir) if refrs else 0
    absfreq_frames = ens.write_absfreqs(out_dir) if absfreqs else 0
    tangent_frames = ens.write_tangents(out_dir) if tangent is not None else 0
    if tangent is not None:
        ens.end_tangent()  # (the context goes back to the route its settings name)
    if flows:
        model.write_flow_spectrum(out_dir, first_time=dt * (packet_step_start - 1))
    flow_frames = frames if flow_spectrum else 0
    ctx.synchronize()
    ctx.set_timing(timing)
    ctx.set_integrator(*integ)
    log.finish()
    log.close()
    dt, dts, step, t = loop.dt, loop.dts, loop.steps, loop.t
    U0 = getattr(loop, "U0", U0)  # (a receiving rank never sees the owner's U0)
    return dict(dt=dt, dts=dts, Nsteps=Nsteps, steps=step, packet_frames=frames, t=t, U0=U0,
                packet_step_start=packet_step_start, spectrum_frames=spectrum_frames, map_frames=map_frames,
                track_frames=track_frames, kmap_frames=kmap_frames, flow_frames=flow_frames, cond_frames=cond_frames,
                trans_frames=trans_frames, recycle_events=recycle_events, refr_frames=refr_frames,
                absfreq_frames=absfreq_frames, tangent_frames=tangent_frames)
