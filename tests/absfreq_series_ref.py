"""The absolute-frequency series' contract (include/swrt.h,
swrt_absfreq_series_*) restated in numpy, in the header's operation order,
taking the per-slot records as input: A = (u, v) of slot_a and B = (u, v) of
slot_b at the packets (None: one snapshot).  What the device tests compare
their integers with, and what tests/test_absfreq_series_cpu.py checks on
hand-made records."""
import numpy as np

from tests.cond_series_ref import omega_of

LIM = 2.0 ** 38


def hist_slot(v, edges):
    """The class of every v in a row [below, bins, above] over ``edges``: bin i
    holds edges[i] <= v < edges[i + 1], the last bin v == edges[-1] too; -1 for
    NaN (tests/refr_series_ref.py's rule, cond_series_ref.class_of)."""
    v = np.asarray(v, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    with np.errstate(invalid="ignore"):
        c = np.searchsorted(edges, v, side="right")  # edges[c - 1] <= v < edges[c]: bin c - 1, class c
        c = np.where(v == edges[nb], nb, c)
        c = np.where(v > edges[nb], nb + 1, c)
    return np.where(np.isnan(v), -1, c).astype(np.int64)


def packet_values(A, B, alpha, tau, k, f, Cg):
    """(w, Om, D, Od) per packet: every operation its own numpy expression."""
    k = np.asarray(k, dtype=np.float64)
    k1, k2 = k[:, 0], k[:, 1]
    a0, a1 = (np.asarray(a, dtype=np.float64) for a in A[:2])
    with np.errstate(all="ignore"):
        if B is None:
            u = a0
            v = a1
            Od = np.zeros(k1.shape)
        else:
            b0, b1 = (np.asarray(b, dtype=np.float64) for b in B[:2])
            alpha, tau = np.float64(alpha), np.float64(tau)
            oma = 1 - alpha
            t0 = oma * a0
            t1 = alpha * b0
            u = t0 + t1
            t0 = oma * a1
            t1 = alpha * b1
            v = t0 + t1
            d0 = b0 - a0
            ut = d0 / tau
            d1 = b1 - a1
            vt = d1 / tau
            t0 = ut * k1
            t1 = vt * k2
            Od = t0 + t1
        w = omega_of(k, f, Cg)
        t0 = u * k1
        t1 = v * k2
        D = t0 + t1
        Om = w + D
    return w, Om, D, Od


def absfreq_frame_of(w, Om, D, Od, omega_edges, abs_edges, frac_bits):
    """The frame (counts (no + 2, nw + 2), sums (3 (nw + 2) + 2 (no + 2),),
    stats [n, rejected], all int64) of packets with those values."""
    nw, no = len(omega_edges) - 1, len(abs_edges) - 1
    nws, nos = nw + 2, no + 2
    S = 2.0 ** frac_bits
    with np.errstate(all="ignore"):
        sw = w * S
        so = Om * S
        sD = D * S
        sd = Od * S
        od2 = Od * Od
        sd2 = od2 * S
        ok = ~np.isnan(Om) & ~np.isnan(Od) & (np.abs(sw) < LIM) & (np.abs(so) < LIM) & (np.abs(sD) < LIM) \
            & (np.abs(sd) < LIM) & (sd2 < LIM)
    wc = hist_slot(w[ok], omega_edges)
    oc = hist_slot(Om[ok], abs_edges)
    counts = np.zeros((nos, nws), dtype=np.int64)
    np.add.at(counts, (oc, wc), 1)
    qO, qO2, qD = (np.rint(v[ok]).astype(np.int64) for v in (sd, sd2, sD))
    sums = np.zeros(3 * nws + 2 * nos, dtype=np.int64)
    np.add.at(sums, wc, qO)
    np.add.at(sums, nws + wc, qO2)
    np.add.at(sums, 2 * nws + wc, qD)
    np.add.at(sums, 3 * nws + oc, qO)
    np.add.at(sums, 3 * nws + nos + oc, qO2)
    return counts, sums, np.array([w.size, w.size - int(ok.sum())], dtype=np.int64)


def absfreq_frame(A, B, alpha, tau, k, f, Cg, omega_edges, abs_edges, frac_bits):
    """The frame of packets with wavevectors k and the records A, B."""
    return absfreq_frame_of(*packet_values(A, B, alpha, tau, k, f, Cg), omega_edges, abs_edges, frac_bits)


def lds_bytes(nw, no, plane):
    """The kernel's dynamic LDS: the tail 8 (4 nw + 3 no + 13) bytes, then the
    uint32 count plane of the LDS form."""
    return 8 * (4 * nw + 3 * no + 13) + (4 * (no + 2) * (nw + 2) if plane else 0)


def lds_form(nw, no):
    """The shapes the LDS form takes: at most 16384 cells, tail and plane
    within 80 KB (swrt_absfreq.hpp)."""
    return (no + 2) * (nw + 2) <= 16384 and lds_bytes(nw, no, True) <= 80 << 10
