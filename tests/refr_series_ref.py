"""The refraction series' contract (include/swrt.h, swrt_refr_series_*)
restated in numpy on the oracle's interpolation, in the header's operation
order: what the device tests compare their integers with, and what
tests/test_refr_series_cpu.py checks against a packet-by-packet loop."""
import numpy as np

from oracle import swrt_oracle as orc
from tests.cond_series_ref import class_of, omega_of

LIM = 2.0 ** 38


def gradients(flows, nslots, alpha, x, dx, bump, nyF=None):
    """(u_x, u_y, v_x, v_y) at the points x (N x 2); ``flows``: one or two
    dicts of the six gridded fields."""
    x = np.asarray(x, dtype=np.float64)
    if nslots == 1:
        _, _, ux, uy, vx, vy = orc.interpolate_fields(x[:, 0], x[:, 1], flows[0], dx, bump, nyF)
    else:
        _, nab = orc.interpolate_U(flows[0], flows[1], alpha, x, dx, bump, nyF)
        ux, uy, vx, vy = nab["u_x"], nab["u_y"], nab["v_x"], nab["v_y"]
    return tuple(np.asarray(a, dtype=np.float64) for a in (ux, uy, vx, vy))


def packet_values(grads, k, f, Cg):
    """(w, wd, gam, c) per packet: every operation rounded on its own."""
    ux, uy, vx, vy = grads
    k = np.asarray(k, dtype=np.float64)
    k1, k2 = k[:, 0], k[:, 1]
    with np.errstate(all="ignore"):
        kk = k1 * k1 + k2 * k2
        w = omega_of(k, f, Cg)
        kd = -(ux * k1 + vx * k2)
        ld = -(uy * k1 + vy * k2)
        g = k1 * kd + k2 * ld
        wd = ((Cg * Cg) * g) / w
        gam = g / kk
        s1, s2 = ux - vy, vx + uy
        sig = np.sqrt(s1 * s1 + s2 * s2)
        c = (gam + gam) / sig
    return w, wd, gam, c


def refr_frame_of(w, wd, gam, c, omega_edges, a_edges, frac_bits):
    """The frame (counts (na + 2, nw + 2), sums (3 (nw + 2) + (na + 2),),
    stats [n, rejected], all int64) of packets with those values."""
    nw, na = len(omega_edges) - 1, len(a_edges) - 1
    nws = nw + 2
    S = 2.0 ** frac_bits
    with np.errstate(all="ignore"):
        sw, sd, sd2, sg = w * S, wd * S, (wd * wd) * S, gam * S
        ok = (np.abs(sw) < LIM) & ~np.isnan(c) & (np.abs(sd) < LIM) & (sd2 < LIM) & (np.abs(sg) < LIM)
    wc = class_of(w[ok], omega_edges)
    ac = class_of(c[ok], a_edges)
    counts = np.zeros((na + 2, nws), dtype=np.int64)
    np.add.at(counts, (ac, wc), 1)
    qd, qd2, qg = (np.rint(v[ok]).astype(np.int64) for v in (sd, sd2, sg))
    sums = np.zeros(3 * nws + na + 2, dtype=np.int64)
    np.add.at(sums, wc, qd)
    np.add.at(sums, nws + wc, qd2)
    np.add.at(sums, 2 * nws + wc, qg)
    np.add.at(sums, 3 * nws + ac, qd)
    return counts, sums, np.array([w.size, w.size - int(ok.sum())], dtype=np.int64)


def refr_frame(flows, nslots, alpha, x, k, dx, bump, f, Cg, omega_edges, a_edges, frac_bits, nyF=None):
    """The frame of the packets (x, k) in the flow."""
    vals = packet_values(gradients(flows, nslots, alpha, x, dx, bump, nyF), k, f, Cg)
    return refr_frame_of(*vals, omega_edges, a_edges, frac_bits)


def a_edges_of(na):
    """The tests' alignment edges: inside [-1, 1], so that below and above fill."""
    return np.linspace(-0.8, 0.8, na + 1)
