"""The transition series' contract (include/swrt.h, swrt_trans_series_*)
restated in numpy: what the device tests compare their integers with, and what
tests/test_trans_series_cpu.py checks against a packet-by-packet loop.  Also
the ring layout of the drivers' multi-ring initial packets."""
import math

import numpy as np

from tests.cond_series_ref import class_of, omega_of  # noqa: F401  (omega_of: re-exported for the tests)


def trans_accepted(src, w, frac_bits):
    """Which packets a frame counts: omega, source and d = omega - source not
    NaN and |omega|, |d|, |d * d| times 2^frac_bits all below 2^38."""
    src = np.asarray(src, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    scale, lim = 2.0 ** frac_bits, 2.0 ** 38
    with np.errstate(all="ignore"):
        d = w - src
        d2 = d * d
        ok = ~(np.isnan(w) | np.isnan(src) | np.isnan(d))
        ok &= (np.abs(w * scale) < lim) & (np.abs(d * scale) < lim) & (np.abs(d2 * scale) < lim)
    return ok


def trans_frame_of(src, w, omega_edges, src_edges, frac_bits, serial=1):
    """The frame (counts (ns + 2, nw + 2), sums (ns + 2, 3), stats [n,
    rejected, serial], all int64) of packets with the source value src and the
    frequency w."""
    src = np.asarray(src, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    nw, ns = len(omega_edges) - 1, len(src_edges) - 1
    ok = trans_accepted(src, w, frac_bits)
    s, v = src[ok], w[ok]
    d = v - s
    d2 = d * d
    scale = 2.0 ** frac_bits
    sc = class_of(s, src_edges)
    wc = class_of(v, omega_edges)
    counts = np.zeros((ns + 2, nw + 2), dtype=np.int64)
    np.add.at(counts, (sc, wc), 1)
    sums = np.zeros((ns + 2, 3), dtype=np.int64)
    for j, q in enumerate((v, d, d2)):
        np.add.at(sums[:, j], sc, np.rint(q * scale).astype(np.int64))  # (rint: round half even)
    return counts, sums, np.array([src.size, src.size - int(ok.sum()), serial], dtype=np.int64)


# ---- the drivers' rings ----
def ring_bounds(N, R):
    """Ring r of R holds the packets [r * N // R, (r + 1) * N // R)."""
    return [(r * N // R, (r + 1) * N // R) for r in range(R)]


def ring_radius(factor, f, Cg):
    """qgsw_raytrace.m:56: |k| of the ring with omega0 = factor * f."""
    return math.sqrt((factor ** 2 - 1) * f ** 2 / Cg ** 2)


def ring_k(N, factors, f, Cg):
    """The initial k of a run with the rings ``factors``: per ring
    qgsw_raytrace.m:57-60 with that ring's packet count, angles 2 pi j / N_r
    for j = 1..N_r."""
    k = np.empty((N, 2), dtype=np.float64)
    for fac, (lo, hi) in zip(factors, ring_bounds(N, len(factors))):
        wf = ring_radius(fac, f, Cg)
        j = np.arange(1, hi - lo + 1, dtype=np.float64)
        k[lo:hi, 0] = wf * np.cos(2 * np.pi * j / (hi - lo))
        k[lo:hi, 1] = wf * np.sin(2 * np.pi * j / (hi - lo))
    return k


def ring_of(N, R):
    """The ring index of every packet."""
    ring = np.empty(N, dtype=np.int64)
    for r, (lo, hi) in enumerate(ring_bounds(N, R)):
        ring[lo:hi] = r
    return ring
