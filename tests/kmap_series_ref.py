"""numpy restatement of the wave-vector plane series' contract (include/swrt.h,
swrt_kmap_series_*): what a frame must hold, bit for bit.

s = m / (2.0*K), one division in double.  Per packet the five values k, l, k*k,
l*l, k*l (each product one double multiplication), each quantised once,
q = np.rint(v * 2^frac_bits) (round half even).  Rejected: k or l not finite,
or any |v * 2^frac_bits| >= 2^38; a rejected packet adds to `rejected` alone.
Inside iff -K <= k < K and -K <= l < K, on k and l themselves; the index is
min(floor((k + K) * s), m - 1), one add then one multiply.  Not rejected and
not inside: `outside`, and the moments still count it.  Sums are int64
(np.add.at, np.sum): exact, order-free."""
import numpy as np

LIMIT = 2.0 ** 38


def kmap_frame(k, K, m, frac_bits=16):
    """(plane (m, m) int64, plane[i, j] the cell with k index i and l index j;
    stats (8,) int64 [n, rejected, outside, sum q(k), sum q(l), sum q(k*k),
    sum q(l*l), sum q(k*l)])."""
    k = np.asarray(k, dtype=np.float64).reshape(-1, 2)
    K = np.float64(K)
    s = np.float64(m) / (2.0 * K)
    k1, k2 = k[:, 0], k[:, 1]
    scale = 2.0 ** frac_bits
    with np.errstate(all="ignore"):
        scaled = [v * scale for v in (k1, k2, k1 * k1, k2 * k2, k1 * k2)]
        ok = np.isfinite(k1) & np.isfinite(k2)
        for v in scaled:
            ok &= np.abs(v) < LIMIT  # (False for NaN)
        inside = ok & (k1 >= -K) & (k1 < K) & (k2 >= -K) & (k2 < K)
    plane = np.zeros((m, m), dtype=np.int64)
    i = np.minimum(np.floor((k1[inside] + K) * s).astype(np.int64), m - 1)
    j = np.minimum(np.floor((k2[inside] + K) * s).astype(np.int64), m - 1)
    np.add.at(plane, (i, j), 1)
    n = k.shape[0]
    stats = np.zeros(8, dtype=np.int64)
    stats[0] = n
    stats[1] = n - int(ok.sum())
    stats[2] = int(ok.sum()) - int(inside.sum())
    for q, v in enumerate(scaled):
        stats[3 + q] = np.rint(v[ok]).astype(np.int64).sum(dtype=np.int64)
    return plane, stats


def edge_wavevectors(K):
    """Components whose fate is decided by a rounding, a sign or the limits:
    -K (cell 0), K (outside), the last double below K (cell m - 1), the first
    below -K (outside), -0.0 and 0 (the same cell), NaN, +-inf, 1e9 (rejected
    at frac_bits 16) and 600 (outside for K < 600, counted in the moments)."""
    K = np.float64(K)
    return np.array([-K, K, np.nextafter(K, -np.inf), np.nextafter(-K, -np.inf), -0.0, 0.0, np.nan, np.inf, -np.inf,
                     1e9, 600.0])
