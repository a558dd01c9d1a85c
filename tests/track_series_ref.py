"""A numpy restatement of one track-series frame (include/swrt.h, the section
after the map series): for the packets ``ids`` of an ensemble (x, k), the
m x 8 array [x, y, k, l, Omega, zeta, sigma, D].

x, y, k, l are copied.  The other four come from the oracle's interpolation
(orc.interpolate_fields for one snapshot, orc.interpolate_U for the blend of
two) at the packets' positions, followed by the header's four formulas in its
operation order:

    Omega = sqrt(f^2 + gH*(k*k + l*l)) + (u*k + v*l)
    zeta  = v_x - u_y
    sigma = sqrt((u_x - v_y)^2 + (v_x + u_y)^2)
    D     = v_y^2 + v_x*u_y

Every operation is one IEEE double operation in numpy as on the device, so the
device's frame is compared with this one bit for bit.  Without a flow
(``fields`` empty) columns 4..7 are the quiet NaN 0x7ff8000000000000.
"""
import numpy as np

from oracle import swrt_oracle as orc

QUIET_NAN = np.uint64(0x7FF8000000000000)
COLUMNS = ("x", "y", "k", "l", "Omega", "zeta", "sigma", "D")


def flow_scalars(u, v, ux, uy, vx, vy, k1, k2, f, gH):
    """[Omega, zeta, sigma, D] from the flow at the packets and their (k, l)."""
    om = np.sqrt(f * f + gH * (k1 * k1 + k2 * k2))
    Om = om + (u * k1 + v * k2)
    zeta = vx - uy
    s1, s2 = ux - vy, vx + uy
    sigma = np.sqrt(s1 * s1 + s2 * s2)
    D = vy * vy + vx * uy
    return Om, zeta, sigma, D


def track_frame(x, k, ids, fields, alpha, f, gH, dx, bump, nyF=None):
    """The frame of packets ``ids`` (m x 8).  ``fields``: a sequence of 0, 1 or
    2 snapshots in the oracle's dict form (orc.FIELD_ORDER keys); with two,
    ``alpha`` blends them as interpolate_U.m does."""
    ids = np.asarray(ids, dtype=np.int64)
    xs = np.asarray(x, dtype=np.float64)[ids]
    ks = np.asarray(k, dtype=np.float64)[ids]
    out = np.empty((ids.size, 8))
    out[:, 0:2] = xs
    out[:, 2:4] = ks
    if len(fields) == 0:
        out[:, 4:8].view(np.uint64)[...] = QUIET_NAN
        return out
    if len(fields) == 1:
        u, v, ux, uy, vx, vy = orc.interpolate_fields(xs[:, 0], xs[:, 1], fields[0], dx, bump, nyF)
    else:
        U, nab = orc.interpolate_U(fields[0], fields[1], alpha, xs, dx, bump, nyF)
        u, v = U[:, 0], U[:, 1]
        ux, uy, vx, vy = nab["u_x"], nab["u_y"], nab["v_x"], nab["v_y"]
    out[:, 4], out[:, 5], out[:, 6], out[:, 7] = flow_scalars(u, v, ux, uy, vx, vy, ks[:, 0], ks[:, 1], f, gH)
    return out
