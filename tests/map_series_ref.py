"""numpy restatement of the map series' contract (include/swrt.h,
swrt_map_series_*): what a frame must hold, bit for bit.

Cell: interpolate.m:21-31 with dxm = L/m through the oracle's _cell_and_frac
(i = floor(mod(x/dxm, m)), which may equal m after mod rounds up), then
i mod m.  Moments: omega = sqrt(f^2 + Cg^2*(k*k + l*l)) in load_data.m:33's
operation order, k, l; each q = np.rint(v * 2^frac_bits) (round half even).
A packet is rejected when x, y, k, l or omega is not finite or any
|v * 2^frac_bits| >= 2^38.  Sums are int64 np.add.at: exact, order-free."""
import numpy as np

from oracle.swrt_oracle import _cell_and_frac

LIMIT = 2.0 ** 38


def map_frame(x, k, L, m, f, Cg, frac_bits=20):
    """(planes (4, m, m) int64 [count, sum q(omega), sum q(k), sum q(l)],
    planes[p, i, j] the cell with x index i; stats (2,) int64 [n, rejected])."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    k = np.asarray(k, dtype=np.float64).reshape(-1, 2)
    k1, k2 = k[:, 0], k[:, 1]
    scale = 2.0 ** frac_bits
    with np.errstate(all="ignore"):
        w = np.sqrt(f * f + Cg * Cg * (k1 * k1 + k2 * k2))  # load_data.m:33
        scaled = [w * scale, k1 * scale, k2 * scale]
        ok = np.isfinite(x[:, 0]) & np.isfinite(x[:, 1]) & np.isfinite(k1) & np.isfinite(k2) & np.isfinite(w)
        for s in scaled:
            ok &= np.abs(s) < LIMIT  # (False for NaN)
    dxm = L / m
    planes = np.zeros((4, m, m), dtype=np.int64)
    xs, ys = x[ok, 0], x[ok, 1]
    i = _cell_and_frac(xs, dxm, m)[0] % m
    j = _cell_and_frac(ys, dxm, m)[0] % m
    np.add.at(planes[0], (i, j), 1)
    for p, s in enumerate(scaled):
        np.add.at(planes[1 + p], (i, j), np.rint(s[ok]).astype(np.int64))
    return planes, np.array([x.shape[0], x.shape[0] - int(ok.sum())], dtype=np.int64)


def edge_positions(L):
    """Positions whose cell is decided by a rounding or a sign: -0.0, 0, +-L,
    L/2, -1e-17 (raw cell m, wrapped to 0) and 3L."""
    return np.array([-0.0, 0.0, L, -L, L / 2, -1e-17, 3 * L])
