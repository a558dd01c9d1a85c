"""The flow spectrum frame (include/swrt.h, swrt_flow_spectrum_*) restated in
numpy, operation for operation: the per-mode arithmetic in IEEE doubles, the
row sums in ascending ky, the halving fold over the nx slots and the
sequential totals.  numpy evaluates each elementwise operation as one IEEE
operation and never contracts, so the frame equals the device's bit for bit.

The loop runs over ky; within one ky every (shell, slot) pair is distinct (a
row has one mode per ky), so the fancy-indexed add is the ordered row sum."""

import numpy as np


def shell_of(kx, ky):
    """The integer j with (2j-1)^2 <= 4(kx^2+ky^2) < (2j+1)^2; 0 for the mean
    mode.  Integer arrays in, integer array out."""
    r2 = np.asarray(kx, dtype=np.int64) ** 2 + np.asarray(ky, dtype=np.int64) ** 2
    s = np.floor(np.sqrt(r2.astype(np.float64))).astype(np.int64)  # a guess, made exact in integers
    s = s - (s * s > r2)
    s = s + ((s + 1) * (s + 1) <= r2)
    return np.where(r2 <= s * (s + 1), s, s + 1)


def nshells(nx):
    kmax = nx // 2 - 1
    return int(shell_of(kmax, kmax)) + 1


def flow_frame(qk, k_scale, K_d2, t=0.0):
    """qk: (2kmax+1, kmax+1) complex, row kx + kmax, column ky ->
    (spectra (3, nshell) float64 [E, Z, Q], stats (4,) [t, sum E, sum Z, sum Q])."""
    qk = np.asarray(qk, dtype=np.complex128)
    kmax = qk.shape[1] - 1
    nx = 2 * (kmax + 1)
    assert qk.shape == (2 * kmax + 1, kmax + 1)
    ns = nshells(nx)
    k_scale, K_d2 = np.float64(k_scale), np.float64(K_d2)
    kx = np.arange(-kmax, kmax + 1, dtype=np.int64)
    slot = kx + kmax
    kxs = kx.astype(np.float64) * k_scale
    P = np.zeros((3, ns, nx))
    with np.errstate(all="ignore"):
        for ky in range(kmax + 1):
            keep = kx >= 0 if ky == 0 else np.ones(kx.shape, dtype=bool)
            qr, qi = qk[:, ky].real, qk[:, ky].imag
            kys = np.float64(ky) * k_scale
            K2 = kxs * kxs + kys * kys
            den = K_d2 + K2
            zero = den == 0.0
            safe = np.where(zero, 1.0, den)
            pr = np.where(zero, 0.0, -qr / safe)
            pi = np.where(zero, 0.0, -qi / safe)
            a = pr * pr + pi * pi
            w = np.where((kx == 0) & (ky == 0), 0.5, 1.0)
            E = w * (K2 * a)
            Z = w * ((K2 * K2) * a)
            Q = w * (qr * qr + qi * qi)
            j = shell_of(kx, np.full_like(kx, ky))
            for p, v in enumerate((E, Z, Q)):
                P[p, j[keep], slot[keep]] = P[p, j[keep], slot[keep]] + v[keep]
        h = nx // 2
        while h >= 1:
            P = P[..., :h] + P[..., h:2 * h]
            h //= 2
    spectra = P[..., 0]
    stats = np.empty(4)
    stats[0] = t
    with np.errstate(all="ignore"):
        for p in range(3):
            s = np.float64(0.0)
            for v in spectra[p]:
                s = s + v
            stats[1 + p] = s
    return spectra, stats
