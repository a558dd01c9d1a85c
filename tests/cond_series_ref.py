"""The conditional spectrum series' contract (include/swrt.h,
swrt_cond_series_*) restated in numpy on the oracle's interpolation: what the
device tests compare their integers with, and what tests/test_cond_series_cpu.py
checks against a packet-by-packet loop."""
import numpy as np

from oracle import swrt_oracle as orc

WHICH = {"zeta": 0, "sigma": 1, "D": 2}


def flow_scalars(flows, nslots, alpha, x, dx, bump, nyF=None):
    """(zeta, sigma, D) at the points x (N x 2) in the operation order of
    swrt_raydiag.hpp (RaytracingScheme.m:20,25,30); ``flows``: one or two dicts
    of the six gridded fields."""
    x = np.asarray(x, dtype=np.float64)
    if nslots == 1:
        _, _, ux, uy, vx, vy = orc.interpolate_fields(x[:, 0], x[:, 1], flows[0], dx, bump, nyF)
    else:
        _, nab = orc.interpolate_U(flows[0], flows[1], alpha, x, dx, bump, nyF)
        ux, uy, vx, vy = nab["u_x"], nab["u_y"], nab["v_x"], nab["v_y"]
    zeta = vx - uy
    s1, s2 = ux - vy, vx + uy
    sigma = np.sqrt(s1 * s1 + s2 * s2)
    D = vy * vy + vx * uy
    return zeta, sigma, D


def omega_of(k, f, Cg):
    """load_data.m:33 in the spectrum series' operation order."""
    k = np.asarray(k, dtype=np.float64)
    k1, k2 = k[:, 0], k[:, 1]
    with np.errstate(all="ignore"):
        return np.sqrt(f * f + (Cg * Cg) * (k1 * k1 + k2 * k2))


def class_of(v, edges):
    """The class of every v in a row [below, bins, above] over ``edges``: bin i
    holds edges[i] <= v < edges[i + 1], the last bin v == edges[-1] too; -1 for
    NaN."""
    v = np.asarray(v, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    with np.errstate(invalid="ignore"):
        c = np.searchsorted(edges, v, side="right")  # edges[c - 1] <= v < edges[c]: bin c - 1, class c
        c = np.where(v == edges[nb], nb, c)
        c = np.where(v > edges[nb], nb + 1, c)
    return np.where(np.isnan(v), -1, c).astype(np.int64)


def cond_frame_of(q, w, omega_edges, q_edges, frac_bits):
    """The frame (counts (nq + 2, nw + 2), sums (nq + 2,), stats [n, rejected],
    all int64) of packets with the flow scalar q and the frequency w."""
    q = np.asarray(q, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    nw, nq = len(omega_edges) - 1, len(q_edges) - 1
    with np.errstate(all="ignore"):
        sw = w * 2.0 ** frac_bits
        ok = (np.abs(sw) < 2.0 ** 38) & ~np.isnan(q)  # (a NaN omega fails the first test)
    qc = class_of(q[ok], q_edges)
    wc = class_of(w[ok], omega_edges)
    counts = np.zeros((nq + 2, nw + 2), dtype=np.int64)
    np.add.at(counts, (qc, wc), 1)
    sums = np.zeros(nq + 2, dtype=np.int64)
    np.add.at(sums, qc, np.rint(sw[ok]).astype(np.int64))
    return counts, sums, np.array([q.size, q.size - int(ok.sum())], dtype=np.int64)


def cond_frame(flows, nslots, alpha, x, k, dx, bump, f, Cg, omega_edges, which, q_edges, frac_bits, nyF=None):
    """The frame of the packets (x, k) in the flow; ``which``: 0, 1, 2 or a name."""
    which = WHICH.get(which, which)
    q = flow_scalars(flows, nslots, alpha, x, dx, bump, nyF)[which]
    return cond_frame_of(q, omega_of(k, f, Cg), omega_edges, q_edges, frac_bits)


# ---- the tests' inputs ----
def zeta_edges(flow, nq):
    """The tests' vorticity edges: half the gridded flow's largest |zeta| either way."""
    return 0.5 * np.abs(flow["vx"] - flow["uy"]).max() * np.linspace(-1.0, 1.0, nq + 1)


def central_edges(v, nb):
    """linspace over the central 80 % of the finite values' range."""
    v = v[np.isfinite(v)]
    lo, hi = v.min(), v.max()
    return np.linspace(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), nb + 1)


def quantile_edges(v, nb):
    """linspace between the 10th and the 90th percentile of v: a tenth of the
    values on either side, also after the values shrink or move by a few per cent."""
    lo, hi = np.percentile(v[np.isfinite(v)], [10.0, 90.0])
    return np.linspace(lo, hi, nb + 1)


def assert_populated(counts, stats=None, planted=False):
    """The frame (the restatement's) fills below, above and at least half of
    the interior classes on both axes; rejected is non-zero where planted."""
    for axis in (0, 1):
        row = counts.sum(axis=axis)
        assert row[0] > 0 and row[-1] > 0, row
        assert 2 * np.count_nonzero(row[1:-1]) >= row.size - 2, row
    if planted:
        assert stats[1] > 0
