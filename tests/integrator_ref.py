"""Numpy restatement of the staged packet step (swrt_set_integrator) over the
oracle's interpolation and drift: a step of S stages, stage j being
drift(h_j/2), kick(h_j, a_j), drift(h_j/2) with h_j = w_j*dt and
a_j = (alpha0 + s*dalpha) + off_j*dalpha.  Every operation is rounded on its
own, in the order the device uses.  Weights and offsets are arguments (tests
take them from swrt_integrator_weights), never recomputed here.

Also the steady test case shared by the CPU and GPU order tests."""
import numpy as np

from oracle import swrt_oracle as orc

F, GH, BUMP = 3.0, 1.0, 1e-13


def grid_flow(snap0, snap1=None, bump=BUMP):
    """flow(x, alpha) -> the six blended sums (u, v, ux, uy, vx, vy) at the
    N x 2 points x, from one or two oracle GridFields."""

    def flow(x, alpha):
        if snap1 is None:
            return tuple(orc.interpolate_fields(x[:, 0], x[:, 1], snap0.fields, snap0.dx, bump, snap0.nyF))
        U, nab = orc.interpolate_U(snap0.fields, snap1.fields, alpha, x, snap0.dx, bump, snap0.nyF)
        return U[:, 0], U[:, 1], nab["u_x"], nab["u_y"], nab["v_x"], nab["v_y"]

    return flow


def scheme_flow(scheme):
    """The same from a RaytracingScheme-like object (U, grad_U), at scheme time 0."""

    def flow(x, alpha):
        U = np.asarray(scheme.U(x))
        nab = scheme.grad_U(x)
        return U[:, 0], U[:, 1], nab["u_x"], nab["u_y"], nab["v_x"], nab["v_y"]

    return flow


def _quot(k, f, gH):
    w = np.sqrt(f * f + gH * (k[:, 0] * k[:, 0] + k[:, 1] * k[:, 1]))
    return np.stack([gH * k[:, 0] / w, gH * k[:, 1] / w], axis=1)


def stage(x, k, h, alpha, f, gH, flow, kick, iters):
    """One stage: drift(h/2), kick(h) at blend alpha, drift(h/2)."""
    hh = 0.5 * h
    x1 = x + hh * _quot(k, f, gH)
    xm = x1
    if kick == 1:
        for _ in range(iters):
            u, v = flow(xm, alpha)[:2]
            xm = np.stack([x1[:, 0] + hh * u, x1[:, 1] + hh * v], axis=1)
    u, v, ux, uy, vx, vy = flow(xm, alpha)
    x2 = np.stack([x1[:, 0] + h * u, x1[:, 1] + h * v], axis=1)
    k1, l1 = k[:, 0], k[:, 1]
    if kick == 1:
        r1 = k1 - hh * (ux * k1 + vx * l1)
        r2 = l1 - hh * (uy * k1 + vy * l1)
        a11, a12, a21, a22 = 1 + hh * ux, hh * vx, hh * uy, 1 + hh * vy
        det = a11 * a22 - a12 * a21
        k2 = np.stack([(a22 * r1 - a12 * r2) / det, (a11 * r2 - a21 * r1) / det], axis=1)
    else:
        k2 = np.stack([k1 - h * (ux * k1 + vx * l1), l1 - h * (uy * k1 + vy * l1)], axis=1)
    return x2 + hh * _quot(k2, f, gH), k2


def integrate(x, k, dt, nsteps, f, gH, flow, w, off, kick=0, iters=1, alpha0=0.0, dalpha=0.0, save_every=0):
    """nsteps composite steps; returns x, k and the save_every frames."""
    x = np.array(x, dtype=np.float64)
    k = np.array(k, dtype=np.float64)
    hx, hk = [], []
    for s in range(nsteps):
        alpha_s = alpha0 + float(s) * dalpha
        for wj, oj in zip(w, off):
            x, k = stage(x, k, float(wj) * dt, alpha_s + float(oj) * dalpha, f, gH, flow, kick, iters)
        if save_every and (s + 1) % save_every == 0:
            hx.append(x.copy())
            hk.append(k.copy())
    return x, k, hx, hk


def abs_frequency(x, k, f, gH, flow):
    """Omega = omega(k) + U(x).k, conserved along rays of a steady flow."""
    u, v = flow(x, 0.0)[:2]
    return np.sqrt(f * f + gH * (k[:, 0] ** 2 + k[:, 1] ** 2)) + (u * k[:, 0] + v * k[:, 1])


def omega_error(x, k, dt, nsteps, f, gH, flow, w, off, kick, iters):
    """max over steps and packets of |Omega - Omega0| / Omega0."""
    O0 = abs_frequency(x, k, f, gH, flow)
    _, _, hx, hk = integrate(x, k, dt, nsteps, f, gH, flow, w, off, kick, iters, save_every=1)
    return max(np.max(np.abs(abs_frequency(a, b, f, gH, flow) - O0) / O0) for a, b in zip(hx, hk))


def steady_case(nx=64, npk=64):
    """The steady field of the order measurements: psi = sum a_i cos(K x + L y +
    phi_i) over four modes through spectral_scheme_fields, the six fields
    scaled to max(|u|, |v|) = 0.2; npk packets on the ring |k| = sqrt(135)."""
    L = 2 * np.pi
    rng = np.random.default_rng(146)
    g = L * np.arange(nx) / nx
    X, Y = np.meshgrid(g, g, indexing="ij")
    psi = np.zeros((nx, nx))
    for K, M in ((1, 0), (0, 1), (1, 1), (2, -1)):
        a = rng.uniform(0.5, 1)
        phi = rng.uniform(0, 2 * np.pi)
        psi = psi + a * np.cos(K * X + M * Y + phi)
    fl = orc.spectral_scheme_fields(L, nx, psi)
    psi_grid = fl.pop("psi")
    scale = 0.2 / max(np.abs(fl["u"]).max(), np.abs(fl["v"]).max())
    fields = {n: fl[n] * scale for n in orc.FIELD_ORDER}
    x0 = rng.uniform(-np.pi, np.pi, (npk, 2))
    th = 2 * np.pi * np.arange(npk) / npk
    k0 = np.sqrt(135.0) * np.stack([np.cos(th), np.sin(th)], axis=1)
    return dict(nx=nx, L=L, fields=fields, psi=psi_grid * scale, snap=orc.GridField(fields, L / nx), x0=x0, k0=k0)
