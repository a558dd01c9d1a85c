"""The numpy restatement of the packet recycling contract in include/swrt.h
(swrt_recycle_*): the hash, one event, and omega in the spectrum series'
operation order (tests/cond_series_ref.omega_of)."""
import numpy as np

from tests.cond_series_ref import omega_of

__all__ = ["mix", "omega_of", "recycle_event", "unit", "positions"]

_M64 = (1 << 64) - 1


def mix(z):
    """The splitmix64 finaliser on uint64 (wrapping), scalar or array."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def unit(h):
    """u = (h >> 11) * 2^-53, in [0, 1)."""
    return (np.asarray(h, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def positions(seed, gid, gen, L):
    """(x, y) of the packets with global ids ``gid`` at generation ``gen``."""
    gid = np.asarray(gid, dtype=np.int64).astype(np.uint64)  # (two's complement, as the C cast)
    g = np.asarray(gen, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        h1 = mix(mix(np.uint64(int(seed) & _M64) ^ mix(gid)) + g)
    h2 = mix(h1)
    return (unit(h1) - 0.5) * L, (unit(h2) - 0.5) * L


def recycle_event(x, k, home, gen, born, serial, f, Cg, omega_cut, L, seed, index_base, frac_bits):
    """One event on packets in the ORIGINAL order (x, k, home n x 2; gen, born
    int32): -> x, k, gen, born (new arrays) and the frame, 8 int64 [n, absorbed,
    rejected, sum q(omega_out), sum q(omega_home), sum age, max age, serial]."""
    x = np.array(x, dtype=np.float64)
    k = np.array(k, dtype=np.float64)
    home = np.asarray(home, dtype=np.float64)
    gen = np.array(gen, dtype=np.int32)
    born = np.array(born, dtype=np.int32)
    n = x.shape[0]
    scale = 2.0 ** int(frac_bits)
    w = omega_of(k, f, Cg)
    with np.errstate(all="ignore"):
        rejected = ~(w * scale < 2.0 ** 38)  # (NaN and infinity included)
    absorbed = ~rejected & (w >= omega_cut)
    idx = np.flatnonzero(absorbed)
    age = serial - born[idx].astype(np.int64)
    q_out = np.rint(w[idx] * scale).astype(np.int64)
    q_home = np.rint(omega_of(home[idx], f, Cg) * scale).astype(np.int64)
    gen[idx] += 1
    born[idx] = serial
    k[idx] = home[idx]
    px, py = positions(seed, int(index_base) + idx, gen[idx], L)
    x[idx, 0] = px
    x[idx, 1] = py
    stats = np.array([n, idx.size, np.count_nonzero(rejected), q_out.sum(), q_home.sum(), age.sum(),
                      age.max() if idx.size else 0, serial], dtype=np.int64)
    return x, k, gen, born, stats
