"""Packet integrators (L3): ode_symplectic and the qg-driver packet branch.

`ode_symplectic` keeps the reference signature (ode_symplectic.m:1).  With a
GPU-backed scheme (SpectralScheme / SnapshotPairScheme) the whole time loop
is one fused device pass (libswrt swrt_leapfrog: drift/kick/drift with the
packet in registers); any other RaytracingScheme runs the same Strang split
on the host through the scheme's U / grad_U_times_k (e.g. DifferenceScheme's
analytic callbacks).
"""
from __future__ import annotations

import math
import os

import numpy as np

from ._lib import COND_WHICH, Context, integrator_weights, PLANE_TAILS, plane_sums_shape, SwrtError
from .io import write_field
from .scheme import BUMP_QG, SnapshotPairScheme, SpectralScheme, flow_planes


def _omega(k, f, gH):
    return np.sqrt(f ** 2 + gH * np.sum(k * k, axis=1, keepdims=True))


def combine_frames(frames):
    """The frame of an ensemble from its shards' frames (swrt_raydiag_*:
    [n, max|r|, sum r, sum r^2, sum omega, sum zeta, sum sigma, sum D]): the
    sums add, entry 1 is the max.  ``frames``: a sequence of (8,) frames or of
    (T, 8) series, one per shard; a shard without packets (n = 0, all zeros)
    changes nothing."""
    fr = np.asarray(frames, dtype=np.float64)
    if fr.ndim < 2 or fr.shape[-1] != 8:
        raise ValueError("frames must be (shards, 8) or (shards, T, 8)")
    out = fr.sum(axis=0)
    out[..., 1] = fr[..., 1].max(axis=0)
    return out


def combine_spectra(parts):
    """The spectrum series of an ensemble from its shards' series
    (swrt_omega_series_*).  ``parts``: a sequence of (counts, stats) pairs, one
    per shard, counts (T, nbins + 2) int64 [below, bins, above] and stats
    (T, 4) [n, sum omega, min omega, max omega]: the counts, n and the sum add,
    min and max are taken.  A shard without packets stands as zeros with
    min = +inf and max = -inf, and changes nothing."""
    parts = list(parts)
    if not parts:
        raise ValueError("no series to combine")
    counts = np.stack([np.asarray(c, dtype=np.int64) for c, _ in parts])
    stats = np.stack([np.asarray(s, dtype=np.float64) for _, s in parts])
    if counts.ndim != 3 or stats.shape != counts.shape[:2] + (4,):
        raise ValueError("every shard must give counts (T, nbins + 2) and stats (T, 4) for the same T")
    out = np.empty(stats.shape[1:])
    out[:, 0:2] = stats[:, :, 0:2].sum(axis=0)
    out[:, 2] = stats[:, :, 2].min(axis=0)
    out[:, 3] = stats[:, :, 3].max(axis=0)
    return counts.sum(axis=0), out


def empty_spectrum(frames, nbins):
    """The series of a shard without packets, as combine_spectra takes it."""
    stats = np.zeros((frames, 4))
    stats[:, 2], stats[:, 3] = np.inf, -np.inf
    return np.zeros((frames, nbins + 2), dtype=np.int64), stats


def energy_spectrum(counts, edges, lo=0, hi=None):
    """(center, energy) of load_data.m:40,45-49 over the series frames
    [lo, hi): center = (edges[1:] + edges[:-1])/2, energy = center times the
    frames' summed counts (the nbins inner columns of ``counts``; below and
    above are outside histcounts' edges)."""
    counts = np.asarray(counts)
    edges = np.asarray(edges, dtype=np.float64).ravel()
    if counts.ndim != 2 or counts.shape[1] != edges.size + 1:
        raise ValueError("counts must be (T, nbins + 2) for nbins + 1 edges")
    center = (edges[1:] + edges[:-1]) / 2
    distribution = counts[lo:hi, 1:-1].sum(axis=0)
    return center, center * distribution


MAP_DRAIN_BYTES = 256 << 20  # record_map drains the device series into the files above this


def combine_maps(parts):
    """The map series of an ensemble from its shards' series
    (swrt_map_series_*).  ``parts``: a sequence of (planes, stats) pairs, one
    per shard, planes (T, 4, m, m) int64 and stats (T, 2) int64 [n, rejected]:
    the element-wise sum (integer, exact and order-free).  A shard without
    packets stands as zeros."""
    parts = list(parts)
    if not parts:
        raise ValueError("no series to combine")
    planes = np.stack([np.asarray(p, dtype=np.int64) for p, _ in parts])
    stats = np.stack([np.asarray(s, dtype=np.int64) for _, s in parts])
    if planes.ndim != 5 or planes.shape[2] != 4 or stats.shape != planes.shape[:2] + (2,):
        raise ValueError("every shard must give planes (T, 4, m, m) and stats (T, 2) for the same T and m")
    return planes.sum(axis=0), stats.sum(axis=0)


def map_fields(planes, frac_bits):
    """Physical fields of map planes (..., 4, m, m) int64 as fp64: ``n`` the
    packet count per cell, ``energy`` the wave energy per cell at unit action
    per packet (load_data.m:49: sum omega), ``k_mean`` and ``l_mean`` the mean
    wavevector; the last three NaN where the count is 0."""
    planes = np.asarray(planes)
    if planes.ndim < 3 or planes.shape[-3] != 4:
        raise ValueError("planes must be (..., 4, m, m)")
    if not 0 <= int(frac_bits) <= 32:
        raise ValueError("frac_bits must be 0..32")
    unit = 2.0 ** -int(frac_bits)
    n = planes[..., 0, :, :].astype(np.float64)
    empty = n == 0
    count = np.where(empty, 1.0, n)
    out = dict(n=n, energy=planes[..., 1, :, :].astype(np.float64) * unit,
               k_mean=planes[..., 2, :, :].astype(np.float64) / count * unit,
               l_mean=planes[..., 3, :, :].astype(np.float64) / count * unit)
    for name in ("energy", "k_mean", "l_mean"):
        out[name][empty] = np.nan
    return out


def combine_kmaps(parts):
    """The wave-vector plane series of an ensemble from its shards' series
    (swrt_kmap_series_*).  ``parts``: a sequence of (planes, stats) pairs, one
    per shard, planes (T, m, m) int64 and stats (T, 8) int64 [n, rejected,
    outside, sum q(k), sum q(l), sum q(k*k), sum q(l*l), sum q(k*l)]: the
    element-wise sum (integer, exact and order-free).  A shard without packets
    stands as zeros."""
    parts = list(parts)
    if not parts:
        raise ValueError("no series to combine")
    planes = np.stack([np.asarray(p, dtype=np.int64) for p, _ in parts])
    stats = np.stack([np.asarray(s, dtype=np.int64) for _, s in parts])
    if planes.ndim != 4 or planes.shape[2] != planes.shape[3] or stats.shape != planes.shape[:2] + (8,):
        raise ValueError("every shard must give planes (T, m, m) and stats (T, 8) for the same T and m")
    return planes.sum(axis=0), stats.sum(axis=0)


def kmap_moments(stats, frac_bits):
    """Moments of the wavevector from k-plane stats (..., 8) int64 as fp64:
    ``n_used`` = n - rejected, ``mean`` (..., 2) the mean (k, l), ``cov``
    (..., 2, 2) the covariance <(k - <k>)(k - <k>)^T> over the n_used packets;
    mean and cov NaN where n_used is 0."""
    stats = np.asarray(stats)
    if stats.ndim < 1 or stats.shape[-1] != 8:
        raise ValueError("stats must be (..., 8)")
    if not 0 <= int(frac_bits) <= 32:
        raise ValueError("frac_bits must be 0..32")
    unit = 2.0 ** -int(frac_bits)
    n_used = (stats[..., 0] - stats[..., 1]).astype(np.float64)
    empty = n_used == 0
    count = np.where(empty, 1.0, n_used)
    m1 = stats[..., 3:5].astype(np.float64) * unit / count[..., None]
    kk, ll, kl = (stats[..., 5 + q].astype(np.float64) * unit / count for q in range(3))
    cov = np.empty(stats.shape[:-1] + (2, 2))
    cov[..., 0, 0] = kk - m1[..., 0] * m1[..., 0]
    cov[..., 1, 1] = ll - m1[..., 1] * m1[..., 1]
    cov[..., 0, 1] = cov[..., 1, 0] = kl - m1[..., 0] * m1[..., 1]
    m1[empty] = np.nan
    cov[empty] = np.nan
    return dict(n_used=n_used, mean=m1, cov=cov)


def _stack_planes(parts, prefix, shapes_msg):
    """The shards' (counts, sums, stats) of a class-plane series stacked along
    a new first axis, their shapes checked against the series' layout
    (_lib.PLANE_TAILS) for whatever nw and n2 the counts have."""
    parts = list(parts)
    if not parts:
        raise ValueError("no series to combine")
    shapes = {tuple(np.shape(a) for a in p) for p in parts}
    if len(shapes) != 1:
        raise ValueError("every shard must give counts, sums and stats of the same shapes")
    counts, sums, stats = (np.stack([np.asarray(p[i], dtype=np.int64) for p in parts]) for i in range(3))
    if counts.ndim != 4 or stats.shape != counts.shape[:2] + (PLANE_TAILS[prefix][2],) \
            or sums.shape != counts.shape[:2] + plane_sums_shape(prefix, counts.shape[3] - 2, counts.shape[2] - 2):
        raise ValueError(shapes_msg)
    return counts, sums, stats


def combine_conds(parts):
    """The conditional spectrum series of an ensemble from its shards' series
    (swrt_cond_series_*).  ``parts``: a sequence of (counts, sums, stats)
    triples, one per shard, counts (T, nq + 2, nw + 2) int64, sums (T, nq + 2)
    int64 and stats (T, 2) int64 [n, rejected]: the element-wise sum (integer,
    exact and order-free).  A shard without packets stands as zeros."""
    return tuple(a.sum(axis=0) for a in _stack_planes(
        parts, "cond", "every shard must give counts (T, nq + 2, nw + 2), sums (T, nq + 2) and stats (T, 2)"))


def cond_spectra(counts, sums, frac_bits):
    """Conditional spectra of frames counts (..., nq + 2, nw + 2) and sums
    (..., nq + 2) int64 as fp64: ``n`` (..., nq + 2) the packets of each q
    class, ``spectrum`` (..., nq + 2, nw + 2) each class's omega row divided by
    its n, ``omega_mean`` (..., nq + 2) the class's mean omega; the last two
    NaN where the class is empty."""
    counts = np.asarray(counts)
    sums = np.asarray(sums)
    if counts.ndim < 2 or sums.shape != counts.shape[:-1]:
        raise ValueError("counts must be (..., nq + 2, nw + 2) and sums (..., nq + 2)")
    if not 0 <= int(frac_bits) <= 32:
        raise ValueError("frac_bits must be 0..32")
    n = counts.sum(axis=-1).astype(np.float64)
    empty = n == 0
    count = np.where(empty, 1.0, n)
    spectrum = counts.astype(np.float64) / count[..., None]
    omega_mean = sums.astype(np.float64) / count * 2.0 ** -int(frac_bits)
    spectrum[empty] = np.nan
    omega_mean[empty] = np.nan
    return dict(n=n, spectrum=spectrum, omega_mean=omega_mean)


def combine_refrs(parts):
    """The refraction series of an ensemble from its shards' series
    (swrt_refr_series_*).  ``parts``: a sequence of (counts, sums, stats)
    triples, one per shard, counts (T, na + 2, nw + 2) int64, sums
    (T, 3 (nw + 2) + (na + 2)) int64 and stats (T, 2) int64 [n, rejected]: the
    element-wise sum (integer, exact and order-free).  A shard without packets
    stands as zeros."""
    return tuple(a.sum(axis=0) for a in _stack_planes(
        parts, "refr", "every shard must give counts (T, na + 2, nw + 2), sums (T, 3 (nw + 2) + (na + 2)) "
                       "and stats (T, 2)"))


def alignment_edges(na):
    """``na`` equal alignment classes over [-1, 1], the range of
    c = -cos 2 theta in a non-divergent flow: na + 1 edges."""
    if isinstance(na, (bool, np.bool_)) or int(na) != na or not 1 <= int(na) <= 4096:
        raise ValueError("na must be an integer 1..4096")
    return np.linspace(-1.0, 1.0, int(na) + 1)


def refr_rates(counts, sums, frac_bits):
    """Rates of refraction frames counts (..., na + 2, nw + 2) and sums
    (..., 3 (nw + 2) + (na + 2)) int64, as fp64.  Per omega class: ``n``
    (..., nw + 2) its packets, ``omega_dot_mean``, ``omega_dot_sq_mean`` and
    ``gamma_mean`` (..., nw + 2) the means of omega-dot, omega-dot^2 and
    gamma = d ln|k|/dt (each exact to the quantum 2^-frac_bits), ``alignment``
    (..., nw + 2, na + 2) the class's alignment row divided by its n.  Per
    alignment class: ``n_align`` (..., na + 2), ``omega_dot_mean_align``
    (..., na + 2) and ``flux_share`` (..., na + 2), the class's part of the
    frame's sum of omega-dot (NaN where that sum is 0).  The means and the
    density are NaN where the class is empty."""
    counts = np.asarray(counts)
    sums = np.asarray(sums)
    if counts.ndim < 2:
        raise ValueError("counts must be (..., na + 2, nw + 2)")
    nas, nws = counts.shape[-2:]
    if sums.shape != counts.shape[:-2] + (3 * nws + nas,):
        raise ValueError("counts must be (..., na + 2, nw + 2) and sums (..., 3 (nw + 2) + (na + 2))")
    if not 0 <= int(frac_bits) <= 32:
        raise ValueError("frac_bits must be 0..32")
    unit = 2.0 ** -int(frac_bits)
    n = counts.sum(axis=-2).astype(np.float64)
    empty = n == 0
    count = np.where(empty, 1.0, n)
    wd, wd2, gam = (sums[..., j * nws:(j + 1) * nws].astype(np.float64) * unit / count for j in range(3))
    alignment = np.swapaxes(counts, -1, -2).astype(np.float64) / count[..., None]
    for a in (wd, wd2, gam, alignment):
        a[empty] = np.nan
    n_a = counts.sum(axis=-1).astype(np.float64)
    empty_a = n_a == 0
    flux_a = sums[..., 3 * nws:].astype(np.float64) * unit
    wd_a = flux_a / np.where(empty_a, 1.0, n_a)
    wd_a[empty_a] = np.nan
    total = flux_a.sum(axis=-1, keepdims=True)
    share = flux_a / np.where(total == 0, 1.0, total)
    share[np.broadcast_to(total == 0, share.shape)] = np.nan
    return dict(n=n, omega_dot_mean=wd, omega_dot_sq_mean=wd2, gamma_mean=gam, alignment=alignment,
                n_align=n_a, omega_dot_mean_align=wd_a, flux_share=share)


def combine_absfreqs(parts):
    """The absolute-frequency series of an ensemble from its shards' series
    (swrt_absfreq_series_*).  ``parts``: a sequence of (counts, sums, stats)
    triples, one per shard, counts (T, no + 2, nw + 2) int64, sums
    (T, 3 (nw + 2) + 2 (no + 2)) int64 and stats (T, 2) int64 [n, rejected]:
    the element-wise sum (integer, exact and order-free).  A shard without
    packets stands as zeros."""
    return tuple(a.sum(axis=0) for a in _stack_planes(
        parts, "absfreq", "every shard must give counts (T, no + 2, nw + 2), sums (T, 3 (nw + 2) + 2 (no + 2)) "
                          "and stats (T, 2)"))


def combine_tangents(parts):
    """The tangent series of an ensemble from its shards' series
    (swrt_tangent_series_*).  ``parts``: a sequence of (counts, sums, stats)
    triples, one per shard, counts (T, ns + 2, nw + 2) int64, sums
    (T, 3 (nw + 2) + (ns + 2)) int64 and stats (T, 3) int64 [n, rejected, mark
    serial]: counts, sums, n and rejected add (integer, exact and order-free);
    the serial is the shards' common one.  Frames whose shards marked a
    different number of times describe different windows and are refused.  A
    shard without packets stands as zeros (its serial does not count)."""
    counts, sums, stats = _stack_planes(
        parts, "tangent", "every shard must give counts (T, ns + 2, nw + 2), sums (T, 3 (nw + 2) + (ns + 2)) "
                          "and stats (T, 3)")
    holds = stats[..., 0] > 0                       # (shard, frame): the shard had packets
    serial = np.where(holds, stats[..., 2], 0).max(axis=0)
    if np.any(holds & (stats[..., 2] != serial[None, :])):
        raise ValueError("the shards' mark serials differ: their frames describe different windows")
    out = stats.sum(axis=0)
    out[..., 2] = serial
    return counts.sum(axis=0), sums.sum(axis=0), out


def tangent_growth(counts, sums, stats, tau):
    """Growth figures of tangent frames counts (..., ns + 2, nw + 2), sums
    (..., 3 (nw + 2) + (ns + 2)) and stats (..., 3) int64, as fp64; ``tau`` the
    time since the frame's mark (a scalar or (...)).  Per omega class: ``n``
    (..., nw + 2) its packets, ``log2_stretch_mean`` the mean of e(s) =
    floor(log2(|M|_F^2 / 4)), ``lyapunov`` = (ln 2 / 2) <e(s)> / tau the
    finite-time Lyapunov estimate (|M| ~ exp(lambda tau)), ``log2_amplitude_mean``
    the mean log2 of 1/|J| (the wave-action density's growth, -<e(|J|)>) and
    ``caustics_mean`` the caustic crossings per packet.  Per growth class:
    ``n_growth`` (..., ns + 2) and ``caustics_mean_growth``.  ``accepted`` (...)
    is n - rejected.  The means are NaN where the class is empty."""
    counts = np.asarray(counts)
    sums = np.asarray(sums)
    stats = np.asarray(stats)
    if counts.ndim < 2:
        raise ValueError("counts must be (..., ns + 2, nw + 2)")
    nss, nws = counts.shape[-2:]
    if sums.shape != counts.shape[:-2] + (3 * nws + nss,) or stats.shape != counts.shape[:-2] + (3,):
        raise ValueError("counts must be (..., ns + 2, nw + 2), sums (..., 3 (nw + 2) + (ns + 2)) and stats (..., 3)")
    tau = np.asarray(tau, dtype=np.float64)
    if np.any(~(tau > 0)):
        raise ValueError("tau must be positive")
    n = counts.sum(axis=-2).astype(np.float64)
    empty = n == 0
    count = np.where(empty, 1.0, n)
    es, ej, cz = (sums[..., j * nws:(j + 1) * nws].astype(np.float64) / count for j in range(3))
    lyap = (np.log(2.0) / 2.0) * es / tau[..., None]
    amp = -ej
    for a in (es, lyap, amp, cz):
        a[empty] = np.nan
    n_g = counts.sum(axis=-1).astype(np.float64)
    empty_g = n_g == 0
    cz_g = sums[..., 3 * nws:].astype(np.float64) / np.where(empty_g, 1.0, n_g)
    cz_g[empty_g] = np.nan
    return dict(n=n, log2_stretch_mean=es, lyapunov=lyap, log2_amplitude_mean=amp, caustics_mean=cz,
                n_growth=n_g, caustics_mean_growth=cz_g, accepted=(stats[..., 0] - stats[..., 1]).astype(np.float64))


def absfreq_rates(counts, sums, stats, frac_bits):
    """Rates of absolute-frequency frames counts (..., no + 2, nw + 2), sums
    (..., 3 (nw + 2) + 2 (no + 2)) and stats (..., 2) int64, as fp64.  Per
    omega class: ``n`` (..., nw + 2) its packets (the frame's omega spectrum),
    ``abs_dot_mean``, ``abs_dot_sq_mean`` and ``doppler_mean`` (..., nw + 2) the
    means of dOmega/dt = k.dU/dt, of its square and of the Doppler shift U.k
    (each exact to the quantum 2^-frac_bits).  Per Omega class: ``n_abs``
    (..., no + 2) its packets (the frame's Omega spectrum),
    ``abs_dot_mean_abs`` and ``abs_dot_sq_mean_abs`` (..., no + 2).
    ``accepted`` (...) is n - rejected of the frame, the sum of either
    spectrum.  The means are NaN where the class is empty."""
    counts = np.asarray(counts)
    sums = np.asarray(sums)
    stats = np.asarray(stats)
    if counts.ndim < 2:
        raise ValueError("counts must be (..., no + 2, nw + 2)")
    nos, nws = counts.shape[-2:]
    if sums.shape != counts.shape[:-2] + (3 * nws + 2 * nos,) or stats.shape != counts.shape[:-2] + (2,):
        raise ValueError("counts must be (..., no + 2, nw + 2), sums (..., 3 (nw + 2) + 2 (no + 2)) and stats (..., 2)")
    if not 0 <= int(frac_bits) <= 32:
        raise ValueError("frac_bits must be 0..32")
    unit = 2.0 ** -int(frac_bits)
    n = counts.sum(axis=-2).astype(np.float64)
    empty = n == 0
    count = np.where(empty, 1.0, n)
    od, od2, dop = (sums[..., j * nws:(j + 1) * nws].astype(np.float64) * unit / count for j in range(3))
    for a in (od, od2, dop):
        a[empty] = np.nan
    n_o = counts.sum(axis=-1).astype(np.float64)
    empty_o = n_o == 0
    count_o = np.where(empty_o, 1.0, n_o)
    od_o, od2_o = (sums[..., 3 * nws + j * nos:3 * nws + (j + 1) * nos].astype(np.float64) * unit / count_o
                   for j in range(2))
    for a in (od_o, od2_o):
        a[empty_o] = np.nan
    accepted = (stats[..., 0] - stats[..., 1]).astype(np.float64)
    return dict(n=n, abs_dot_mean=od, abs_dot_sq_mean=od2, doppler_mean=dop, n_abs=n_o, abs_dot_mean_abs=od_o,
                abs_dot_sq_mean_abs=od2_o, accepted=accepted)


def combine_transitions(parts):
    """The transition series of an ensemble from its shards' series
    (swrt_trans_series_*).  ``parts``: a sequence of (counts, sums, stats)
    triples, one per shard, counts (T, ns + 2, nw + 2) int64, sums
    (T, ns + 2, 3) int64 and stats (T, 3) int64 [n, rejected, mark serial]:
    counts, sums, n and rejected add (integer, exact and order-free); the
    serial is the shards' common one.  Frames whose shards marked a different
    number of times describe different lags and are refused.  A shard without
    packets stands as zeros (its serial does not count)."""
    counts, sums, stats = _stack_planes(
        parts, "trans", "every shard must give counts (T, ns + 2, nw + 2), sums (T, ns + 2, 3) and stats (T, 3)")
    holds = stats[..., 0] > 0                       # (shard, frame): the shard had packets
    serial = np.where(holds, stats[..., 2], 0).max(axis=0)
    if np.any(holds & (stats[..., 2] != serial[None, :])):
        raise ValueError("the shards' mark serials differ: their frames describe different marks")
    out = stats.sum(axis=0)
    out[..., 2] = serial
    return counts.sum(axis=0), sums.sum(axis=0), out


def trans_moments(counts, sums, frac_bits):
    """Per source class of frames counts (..., ns + 2, nw + 2) and sums
    (..., ns + 2, 3) int64, as fp64: ``n`` (..., ns + 2) the packets of the
    class, ``omega_mean``, ``delta_mean`` and ``delta_var`` (..., ns + 2) the
    means of omega and of d = omega - source and the variance <d^2> - <d>^2
    (each mean exact to the quantum 2^-frac_bits), ``spectrum``
    (..., ns + 2, nw + 2) the class's omega row divided by its n: the
    conditional spectrum, a row of the propagator.  All but ``n`` are NaN where
    the class is empty.  The drift is delta_mean / tau and the diffusivity
    (delta_var + delta_mean^2) / (2 tau) for the lag tau of the frame."""
    counts = np.asarray(counts)
    sums = np.asarray(sums)
    if counts.ndim < 2 or sums.shape != counts.shape[:-1] + (3,):
        raise ValueError("counts must be (..., ns + 2, nw + 2) and sums (..., ns + 2, 3)")
    if not 0 <= int(frac_bits) <= 32:
        raise ValueError("frac_bits must be 0..32")
    unit = 2.0 ** -int(frac_bits)
    n = counts.sum(axis=-1).astype(np.float64)
    empty = n == 0
    count = np.where(empty, 1.0, n)
    spectrum = counts.astype(np.float64) / count[..., None]
    omega_mean = sums[..., 0].astype(np.float64) * unit / count
    delta_mean = sums[..., 1].astype(np.float64) * unit / count
    delta_var = sums[..., 2].astype(np.float64) * unit / count - delta_mean * delta_mean
    for a in (spectrum, omega_mean, delta_mean, delta_var):
        a[empty] = np.nan
    return dict(n=n, omega_mean=omega_mean, delta_mean=delta_mean, delta_var=delta_var, spectrum=spectrum)


def combine_recycles(parts):
    """The recycle frames of an ensemble from its shards' (swrt_recycle_*).
    ``parts``: a sequence of (T, 8) int64 arrays [n, absorbed, rejected,
    sum q(omega_out), sum q(omega_home), sum age, max age, serial], one per
    shard: columns 0-5 add (integer, exact and order-free), the max age takes
    the max and the serial is the shards' common one.  Frames whose shards
    counted a different number of events are refused.  A shard without packets
    stands as zeros (its serial does not count)."""
    parts = [np.asarray(p, dtype=np.int64) for p in parts]
    if not parts:
        raise ValueError("no series to combine")
    if any(p.ndim != 2 or p.shape != parts[0].shape or p.shape[1] != 8 for p in parts):
        raise ValueError("every shard must give (T, 8) frames of the same length")
    stats = np.stack(parts)
    holds = stats[..., 0] > 0                       # (shard, frame): the shard had packets
    serial = np.where(holds, stats[..., 7], 0).max(axis=0)
    if np.any(holds & (stats[..., 7] != serial[None, :])):
        raise ValueError("the shards' event serials differ: their frames describe different events")
    out = stats.sum(axis=0)
    out[:, 6] = stats[..., 6].max(axis=0)
    out[:, 7] = serial
    return out


def recycle_flux(stats, times, frac_bits, t0=None):
    """Per event of frames ``stats`` (T, 8) int64 at the times ``times`` (T),
    as fp64: ``fraction`` absorbed / n, ``energy_out`` and ``energy_in`` the
    sums of omega of the absorbed packets as they left and as they came back
    (each exact to the quantum 2^-frac_bits) per unit time since the event
    before (``t0``: the time the first event's interval starts at; without it
    the first event's two rates are NaN), and ``mean_age`` the mean number of
    events an absorbed packet lived (NaN where none was absorbed).  The flux
    through the sink is energy_out - energy_in."""
    stats = np.asarray(stats, dtype=np.int64)
    times = np.asarray(times, dtype=np.float64).ravel()
    if stats.ndim != 2 or stats.shape[1] != 8 or times.size != stats.shape[0]:
        raise ValueError("stats must be (T, 8) with one time per frame")
    if not 0 <= int(frac_bits) <= 32:
        raise ValueError("frac_bits must be 0..32")
    unit = 2.0 ** -int(frac_bits)
    n = stats[:, 0].astype(np.float64)
    absorbed = stats[:, 1].astype(np.float64)
    dt = np.diff(times, prepend=np.nan if t0 is None else float(t0))
    with np.errstate(divide="ignore", invalid="ignore"):
        fraction = np.where(n > 0, absorbed / np.where(n > 0, n, 1.0), np.nan)
        mean_age = np.where(absorbed > 0, stats[:, 5] / np.where(absorbed > 0, absorbed, 1.0), np.nan)
        energy_out = stats[:, 3].astype(np.float64) * unit / dt
        energy_in = stats[:, 4].astype(np.float64) * unit / dt
    return dict(fraction=fraction, energy_out=energy_out, energy_in=energy_in, mean_age=mean_age)


def track_ids_array(ids, n_total):
    """``ids`` as a checked int64 array: a one-dimensional, non-empty sequence
    of distinct integers in 0..n_total-1 (ValueError otherwise)."""
    a = np.asarray(ids)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("track ids must be a non-empty one-dimensional sequence")
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.floating) or not np.all(a == np.floor(a)):
            raise ValueError("track ids must be integers")
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= int(n_total):
        raise ValueError(f"track ids must lie in 0..{int(n_total) - 1}")
    if np.unique(a).size != a.size:
        raise ValueError("track ids must be distinct")
    return a


def shard_track_rows(ids, lo, hi):
    """The rows of a track frame (positions in ``ids``) whose packets lie in
    the shard [lo, hi), in the order they appear in ``ids``."""
    ids = np.asarray(ids, dtype=np.int64)
    return np.nonzero((ids >= lo) & (ids < hi))[0]


def combine_tracks(parts, ids, bounds):
    """The track series of an ensemble from its shards' series
    (swrt_track_*).  ``ids``: the m global packet ids in the caller's order;
    ``bounds``: every shard's [lo, hi); ``parts``: one (T, 8, m_r) series per
    shard, its rows the ids inside the shard's bounds in the order they have
    in ``ids`` (a shard that owns none gives (T, 8, 0), or None).  Returns
    (T, 8, m): every row back at its place in ``ids``, bit for bit."""
    ids = np.asarray(ids, dtype=np.int64)
    parts, bounds = list(parts), list(bounds)
    if len(parts) != len(bounds) or not parts:
        raise ValueError("one series per shard")
    rows = [shard_track_rows(ids, lo, hi) for lo, hi in bounds]
    if sum(r.size for r in rows) != ids.size:
        raise ValueError("the shards' bounds must cover every id once")
    T = max((np.asarray(p).shape[0] for p, r in zip(parts, rows) if r.size), default=0)
    out = np.empty((T, 8, ids.size))
    for p, r in zip(parts, rows):
        if r.size == 0:
            continue
        p = np.asarray(p, dtype=np.float64)
        if p.shape != (T, 8, r.size):
            raise ValueError("every shard must give (T, 8, m_r) for the same T and its own ids")
        out.view(np.uint64)[:, :, r] = p.view(np.uint64)  # (the bits, NaN payloads included)
    return out


# method -> (kick, composition, default fixed-point iterations) of swrt_set_integrator
METHODS = {"leapfrog": ("euler", None, 1), "midpoint": ("midpoint", None, 2),
           "yoshida4": ("midpoint", "yoshida", 4), "suzuki4": ("midpoint", "suzuki", 4)}


def packet_method(method="leapfrog", iterations=None):
    """(kick, iterations, composition) of a packet-step method: "leapfrog" (the
    reference's step, first order), "midpoint" (implicit-midpoint kick, second
    order, 2 iterations) or "yoshida4" / "suzuki4" (fourth-order compositions
    of the midpoint step, 4 iterations)."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {list(METHODS)}, got {method!r}")
    kick, comp, it = METHODS[method]
    if iterations is not None:
        if method == "leapfrog":
            raise ValueError("iterations belongs to the midpoint kick (method 'midpoint', 'yoshida4', 'suzuki4')")
        it = int(iterations)
        if not 1 <= it <= 4:
            raise ValueError("iterations must be 1..4")
    return kick, it, comp


def _host_stage(xc, kc, h, f, gH, scheme, midpoint, iters):
    """One stage drift(h/2), kick(h), drift(h/2) of the generic host path on
    1 x 2 x P state (the arithmetic of swrt_set_integrator, include/swrt.h)."""

    def gv(kk):
        w = np.sqrt(f * f + gH * (kk[:, 0:1, :] * kk[:, 0:1, :] + kk[:, 1:2, :] * kk[:, 1:2, :]))
        return gH * kk / w

    hh = 0.5 * h
    x1 = xc + hh * gv(kc)
    if not midpoint:
        x2 = x1 + h * scheme.U(x1)
        k2 = kc - h * scheme.grad_U_times_k(x1, kc, 0)
        return x2 + hh * gv(k2), k2
    xm = x1
    for _ in range(iters):
        xm = x1 + hh * scheme.U(xm)
    x2 = x1 + h * scheme.U(xm)
    nab = scheme.grad_U(xm)
    shp = kc[:, 0, ...].shape
    ux, uy, vx, vy = (np.reshape(nab[n], shp, order="F") for n in ("u_x", "u_y", "v_x", "v_y"))
    k1, l1 = kc[:, 0, ...], kc[:, 1, ...]
    r1 = k1 - hh * (ux * k1 + vx * l1)
    r2 = l1 - hh * (uy * k1 + vy * l1)
    a11, a12, a21, a22 = 1 + hh * ux, hh * vx, hh * uy, 1 + hh * vy
    det = a11 * a22 - a12 * a21
    k2 = np.empty_like(kc)
    k2[:, 0, ...] = (a22 * r1 - a12 * r2) / det
    k2[:, 1, ...] = (a11 * r2 - a21 * r1) / det
    return x2 + hh * gv(k2), k2


def ode_symplectic(x0, k0, dt, T, f, gH, scheme, diagnostics=False, method="leapfrog", iterations=None,
                   tangent=False):
    """[x, k, t] = ode_symplectic(x0, k0, dt, T, f, gH, scheme).

    ``method``: "leapfrog" (default: ode_symplectic.m:13-37, whose Euler kick
    makes it first order), "midpoint" (implicit-midpoint kick, second order),
    "yoshida4" or "suzuki4" (fourth order); ``iterations``: the midpoint's
    fixed-point passes (default 2 for "midpoint", 4 for the compositions).
    GPU-backed schemes run swrt_set_integrator's kernels (the context's
    setting is restored on return); any other RaytracingScheme takes the same
    arithmetic on the host.

    x0, k0: 1 x 2 x P.  Returns x, k: Nsteps x 2 x P (row 1 = initial state)
    and t: (Nsteps,) with t(i) = (i-1)*dt (ode_symplectic.m:2-8,23-28).

    ``diagnostics`` (GPU-backed schemes): a fourth value, the (Nsteps x 8)
    series of swrt_raydiag frames — row i belongs to x[i], k[i]; row 0 is the
    initial state, where Omega_0 is marked (symplectic_full_fourier.m:41,54-57:
    solver_error against t).  The packets then advance one step per call with
    a frame recorded on the device after each; x, k and t are the same bits.

    ``tangent`` (GPU-backed schemes, method "leapfrog", not with
    ``diagnostics``): two more values, the final tangent map M (P x 4 x 4,
    d(x, y, k, l)/d(x0, y0, k0, l0) of the discrete map over all the steps) and
    the caustic counters (P,) int32 (swrt_tangent_*); x, k and t are the same
    bits."""
    x0 = np.asarray(x0, dtype=np.float64)
    k0 = np.asarray(k0, dtype=np.float64)
    if x0.ndim == 2:
        x0 = x0[None]
        k0 = k0[None]
    P = x0.shape[2]
    Nsteps = int(math.floor(T / dt))
    x = np.zeros((Nsteps, 2, P))
    k = np.zeros((Nsteps, 2, P))
    t = np.arange(Nsteps, dtype=np.float64) * dt
    gpu = isinstance(scheme, (SpectralScheme, SnapshotPairScheme))
    if diagnostics and not gpu:
        raise ValueError("diagnostics needs a GPU-backed scheme (SpectralScheme / SnapshotPairScheme)")
    if tangent and (not gpu or diagnostics or method != "leapfrog"):
        raise ValueError('tangent needs a GPU-backed scheme, method="leapfrog" and diagnostics=False')
    if Nsteps <= 1 and tangent:
        x[:Nsteps], k[:Nsteps] = x0[0], k0[0]
        return x, k, t, np.tile(np.eye(4), (P, 1, 1)), np.zeros(P, dtype=np.int32)
    if Nsteps == 0:
        return (x, k, t, np.zeros((0, 8))) if diagnostics else (x, k, t)
    x[0] = x0[0]
    k[0] = k0[0]
    if Nsteps == 1 and not diagnostics:
        return x, k, t
    kick, iters, comp = packet_method(method, iterations)
    if gpu:
        ctx = scheme.ctx
        before = ctx.get_integrator()
        ctx.set_integrator(kick, iters, comp)
        try:
            if tangent:
                return _ode_symplectic_tangent(ctx, scheme, x, k, t, x0, k0, dt, Nsteps, f, gH)
            return _ode_symplectic_gpu(ctx, scheme, x, k, t, x0, k0, dt, Nsteps, f, gH, diagnostics)
        finally:
            ctx.set_integrator(*before)
    # generic host path (arbitrary RaytracingScheme)
    w, _ = integrator_weights(comp)
    xc, kc = x0.copy(), k0.copy()
    for i in range(1, Nsteps):
        for wj in w:
            xc, kc = _host_stage(xc, kc, float(wj) * dt, f, gH, scheme, kick == "midpoint", iters)
        x[i] = xc[0]
        k[i] = kc[0]
    return x, k, t


def _ode_symplectic_tangent(ctx, scheme, x, k, t, x0, k0, dt, Nsteps, f, gH):
    """ode_symplectic with the tangent map carried beside the packets."""
    nslots = 1 if isinstance(scheme, SpectralScheme) else 2
    ctx.packets_set(np.asfortranarray(x0[0].T), np.asfortranarray(k0[0].T))  # (starts a new history)
    ctx.tangent_begin()
    try:
        ctx.advance(dt, Nsteps - 1, f, gH, nslots=nslots, alpha0=0.0, dalpha=0.0, bump=scheme.bump, save_every=1)
        x[1:], k[1:] = ctx.history()
        M, caustics = ctx.tangent_get()
    finally:
        ctx.tangent_end()
    return x, k, t, M.reshape(-1, 4, 4), caustics


def _ode_symplectic_gpu(ctx, scheme, x, k, t, x0, k0, dt, Nsteps, f, gH, diagnostics):
    """ode_symplectic on the device, under the context's integrator setting."""
    nslots = 1 if isinstance(scheme, SpectralScheme) else 2
    xs = np.asfortranarray(x0[0].T)  # P x 2
    ks = np.asfortranarray(k0[0].T)
    if not diagnostics:
        _, _, hx, hk = ctx.leapfrog(xs, ks, dt, Nsteps - 1, f, gH, nslots=nslots, alpha0=0.0,
                                    dalpha=0.0, bump=scheme.bump, save_every=1)
        x[1:] = hx
        k[1:] = hk
        return x, k, t
    phys = dict(nslots=nslots, alpha=0.0, bump=scheme.bump)
    ctx.packets_set(xs, ks)  # (starts a new history)
    ctx.raydiag_series_reset()
    ctx.raydiag_mark(f, gH, **phys)
    ctx.raydiag_record(f, gH, **phys)
    for _ in range(Nsteps - 1):
        ctx.advance(dt, 1, f, gH, nslots=nslots, alpha0=0.0, dalpha=0.0, bump=scheme.bump, save_every=1)
        ctx.raydiag_record(f, gH, **phys)
    if Nsteps > 1:
        x[1:], k[1:] = ctx.history()
    return x, k, t, ctx.raydiag_series()


def ode23_packets(ctx: Context, tspan, tmax, f, Cg, nslots=2, rtol=1e-3, atol=1e-6, bump=BUMP_QG,
                  allreduce_max=None, stats=None, controller=None, hook=None):
    """[~, y] = ode23(ray_ode, tspan, y0) for the device-resident packets
    (qgsw_raytrace.m:143-150, qg2layersw_raytrace.m:189-196): MATLAB ode23's
    Bogacki-Shampine controller (defaults RelTol 1e-3, AbsTol 1e-6, MaxStep
    0.1*|tspan|, max-norm error, its initial-step heuristic and step update)
    on the host, every per-packet stage on the GPU (swrt_ode23_*).  The error
    norm is global over all packets — with packets sharded over ranks pass
    ``allreduce_max`` (a callable max-reducing one float over the ranks, e.g.
    an RCCL all_reduce) so every rank takes the same steps.
    Parity: bit-identical to oracle ode23 (its restatement; MATLAB itself is
    unpinned).  Returns the accepted times.

    ``controller``: "library" runs this same controller inside the C library
    (swrt_ode23_run: no interpreter between attempts; with ``allreduce_max``
    swrt_ode23_run_sharded, which reduces stage 1's and every attempt's max
    through it), "python" the loop below (the one a rank without packets
    runs: the same reductions in the same order); default "library" for a
    Context.  Same steps and bits either way.

    ``hook``: a callable (QG calls only, never the packets) run once while
    the interval's first launches run — the library controller calls it
    after stage 1 and the first attempt are queued (swrt_ode23_run_hooked),
    the Python loop after stage 1.

    A ``tspan`` of more than two times (strictly monotonic) is MATLAB's
    output at requested times: the steps are chosen as for [tspan[0],
    tspan[-1]] — only the initial step is also bounded by the first gap
    |tspan[1] - tspan[0]| (odearguments' htspan) — and the solution at
    tspan[1:], ntrp23 inside the accepted steps, is appended to the context's
    history (len(tspan) - 1 frames, Context.history()).  "library" runs
    swrt_ode23_run_at, "python" the loop below with ode23_ntrp; the same
    steps and frame bits either way.  Single rank, no hook."""
    tspan = [float(v) for v in tspan]
    dense = len(tspan) > 2
    if dense:
        if allreduce_max is not None or hook is not None:
            raise ValueError("a tspan of more than two times takes neither allreduce_max nor a hook")
        d = np.diff(tspan)
        if not (np.all(d > 0) or np.all(d < 0)):
            raise ValueError("tspan must be strictly increasing or strictly decreasing")
    if controller is None:
        controller = "library" if hasattr(ctx, "ode23_run") else "python"
    if controller == "library" and dense:
        try:
            ts, st = ctx.ode23_run_at(tspan, tmax, f, Cg, nslots, rtol, atol, bump)
        except SwrtError as e:
            if "below hmin" in str(e):
                raise RuntimeError(str(e)) from e
            raise
        if stats is not None:
            stats.update(**st)
        return ts
    if controller == "library":
        try:
            ts, st = ctx.ode23_run(float(tspan[0]), float(tspan[1]), tmax, f, Cg, nslots, rtol, atol, bump,
                                   hook=hook, reduce=allreduce_max)
        except SwrtError as e:
            if "below hmin" in str(e):
                raise RuntimeError(str(e)) from e
            raise
        if stats is not None:
            stats.update(**st)
        return ts
    red = allreduce_max or (lambda v: v)
    if dense:
        ctx.ode23_set_dense(1)
        try:
            return _ode23_loop(ctx, tspan, tmax, f, Cg, nslots, rtol, atol, bump, red, stats, hook)
        finally:
            ctx.ode23_set_dense(0)
    return _ode23_loop(ctx, tspan, tmax, f, Cg, nslots, rtol, atol, bump, red, stats, hook)


def _ode23_loop(ctx, tspan, tmax, f, Cg, nslots, rtol, atol, bump, red, stats, hook):
    """ode23_packets' controller in Python (the library's ode23_control and
    swrt_ode23_run_at restate it operation for operation)."""
    t0, tfinal = tspan[0], tspan[-1]
    tdir = math.copysign(1.0, tfinal - t0)
    pw = 1.0 / 3.0
    rtol = max(rtol, 100 * np.finfo(float).eps)
    thr = atol / rtol
    htspan = abs(tspan[1] - tspan[0])  # the first output gap: bounds the initial step only
    hmax = 0.1 * abs(tfinal - t0)
    nxt = 1  # the next requested time (a tspan of more than two)
    t = t0
    rh = red(ctx.ode23_f1(t, tmax, f, Cg, nslots, thr, bump)) / (0.8 * rtol ** pw)
    if hook is not None:
        hook()
    absh = min(hmax, htspan)
    if absh * rh > 1:
        absh = 1.0 / rh
    absh = max(absh, 16 * np.spacing(t))
    ts = [t]
    done = False
    nfailed = 0
    attempts = 0
    while not done:
        hmin = 16 * np.spacing(t)
        absh = min(hmax, max(hmin, absh))
        h = tdir * absh
        if 1.1 * absh >= abs(tfinal - t):
            h = tfinal - t
            absh = abs(h)
            done = True
        nofailed = True
        while True:
            tnew = t + h * 1.0
            if done:
                tnew = tfinal
            attempts += 1
            err = absh * red(ctx.ode23_attempt(t, h, tnew, tmax, f, Cg, nslots, thr, bump))
            h = tnew - t
            if err > rtol:
                nfailed += 1
                if absh <= hmin:
                    raise RuntimeError(f"ode23: step size {absh} below hmin at t={t}")
                if nofailed:
                    nofailed = False
                    absh = max(hmin, absh * max(0.5, 0.8 * (rtol / err) ** pw))
                else:
                    absh = max(hmin, 0.5 * absh)
                h = tdir * absh
                done = False
            else:
                break
        if len(tspan) > 2:
            # every requested time this step reaches, in order (ntrp23; tnew itself: ynew)
            n0 = nxt
            while nxt < len(tspan) and tdir * (tnew - tspan[nxt]) >= 0:
                nxt += 1
            if nxt > n0:
                ctx.ode23_ntrp(t, tnew, tspan[n0:nxt])
        ctx.ode23_accept()
        t = tnew
        ts.append(t)
        if done:
            break
        if nofailed:
            temp = 1.25 * (err / rtol) ** pw
            absh = absh / temp if temp > 0.2 else 5.0 * absh
    if stats is not None:
        stats.update(steps=len(ts) - 1, failed=nfailed, attempts=attempts, accepted=len(ts))
    return np.array(ts)


def ode23_trajectory(x0, k0, t_hist, f, Cg, scheme, rtol=1e-3, atol=1e-6, diagnostics=False):
    """[t_hist, solver_y] = ode23(rayfun, t_hist, y0, opts) with the packet
    layout of ode_symplectic (SW_zero_background_raytracing.m:69-83): x0, k0
    are 1 x 2 x P, ``t_hist`` the strictly monotonic output times; returns
    (solver_x, solver_k) of shape len(t_hist) x 2 x P, row 0 the initial state
    and row i the ode23 solution at t_hist[i] (ntrp23 inside the accepted
    steps, the whole call on the device: ode23_packets with the library
    controller).

    The right-hand side is the drivers' (qgsw_raytrace.m:259-265): dx/dt =
    U + Cg*k/omega, dk/dt = -(grad U)^T k with omega = sqrt(f^2 + Cg^2|k|^2).
    SW_zero_background_raytracing.m:183 uses scheme.grad_omega instead, which
    is this one when Cg = 1.

    ``scheme``: a SpectralScheme (steady) or a SnapshotPairScheme (two
    snapshots blended at t / scheme.tmax).  ``diagnostics``: a third value,
    the (len(t_hist) x 8) swrt_raydiag series — row i belongs to row i of the
    outputs; Omega_0 is marked at the initial state, so row 0 has r = 0
    (solver_error of :85-87 against t_hist), computed on the device from the
    frames."""
    if not isinstance(scheme, (SpectralScheme, SnapshotPairScheme)):
        raise ValueError("ode23_trajectory needs a GPU-backed scheme (SpectralScheme / SnapshotPairScheme)")
    x0 = np.asarray(x0, dtype=np.float64)
    k0 = np.asarray(k0, dtype=np.float64)
    if x0.ndim == 2:
        x0 = x0[None]
        k0 = k0[None]
    t_hist = np.asarray(t_hist, dtype=np.float64).reshape(-1)
    if t_hist.size < 3:
        # (two times are MATLAB's every-step output: not this function's; ode23_packets leaves y(tfinal))
        raise ValueError("t_hist needs at least three times")
    P = x0.shape[2]
    nt = t_hist.size
    steady = isinstance(scheme, SpectralScheme)
    nslots = 1 if steady else 2
    tmax = 0.0 if steady else scheme.tmax
    ctx = scheme.ctx
    x = np.zeros((nt, 2, P))
    k = np.zeros((nt, 2, P))
    x[0] = x0[0]
    k[0] = k0[0]
    ctx.packets_set(np.asfortranarray(x0[0].T), np.asfortranarray(k0[0].T))  # (starts a new history)
    alphas = None if steady else t_hist / tmax
    if diagnostics:
        gH = float(Cg) ** 2
        ctx.raydiag_series_reset()
        ctx.raydiag_mark(f, gH, nslots=nslots, alpha=0.0 if steady else alphas[0], bump=scheme.bump)
        ctx.raydiag_record(f, gH, nslots=nslots, alpha=0.0 if steady else alphas[0], bump=scheme.bump)
    ode23_packets(ctx, t_hist, tmax, f, Cg, nslots=nslots, rtol=rtol, atol=atol, bump=scheme.bump,
                  controller="library")
    x[1:], k[1:] = ctx.history()
    if diagnostics:
        ctx.raydiag_record_history(0, nt - 1, f, gH, nslots=nslots, alphas=None if steady else alphas[1:],
                                   bump=scheme.bump)
        return x, k, ctx.raydiag_series()
    return x, k


class _EmptyShard:
    """The ode23 stages of a rank that holds no packets: every max is 0."""

    def ode23_f1(self, *a):
        return 0.0

    def ode23_attempt(self, *a):
        return 0.0

    def ode23_accept(self):
        pass


class _Recorder:
    """One drained count series of a PacketEnsemble run (the map, k-plane and
    class-plane series): the frames recorded in all, those still on the
    device (``pending``), the drained parts rank 0 keeps when there is no
    ``directory`` to append them to, and the drain itself.  A series supplies
    ``layout`` (per part of a frame its shape and dtype, the ``ndev`` parts
    the device holds first), ``frame_bytes`` for the drain threshold,
    ``get`` / ``reset`` into the context, ``combine`` (None: the shards' parts
    add, one all_reduce each; else one all_gather each and combine on rank
    0), ``append`` and, where it has one, ``geometry``."""

    combine = None

    def __init__(self, ens, begin, directory):
        self.ens, self.begin, self.directory = ens, begin, directory
        self.frames = self.pending = 0
        self.kept = []

    def host_part(self, T):
        """The parts of the T pending frames that the host kept (none)."""
        return ()

    def geometry(self, directory):
        pass

    def record(self, call):
        """One more frame: ``call`` queues this shard's; then the drain when
        the device series has grown past MAP_DRAIN_BYTES."""
        self.frames += 1
        self.pending += 1
        if self.ens.n > 0:
            call()
        if self.pending * self.frame_bytes > MAP_DRAIN_BYTES:
            self.drain()

    def drain(self):
        """The frames on the device, combined over the shards, to the files or
        the host list of rank 0; the device series emptied."""
        T, ens = self.pending, self.ens
        if T == 0:
            return
        if ens.n > 0:
            part = self.get(T)
            self.reset()
        else:
            part = tuple(np.zeros((T,) + shape, dtype=dt) for shape, dt in self.layout[:self.ndev])
        self.pending = 0
        host = self.host_part(T)
        if ens.world > 1:
            import torch
            import torch.distributed as dist

            from .dist import _device_for
            dev = _device_for(dist.get_backend())
            shards = []
            for a in part:
                buf = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                if self.combine is None:
                    dist.all_reduce(buf, op=dist.ReduceOp.SUM)  # (int64: exact, order-free)
                    shards.append(buf.cpu().numpy())
                else:
                    out = [torch.empty_like(buf) for _ in range(ens.world)]
                    dist.all_gather(out, buf)
                    shards.append([o.cpu().numpy() for o in out])
            if ens.rank != 0:
                return
            part = shards if self.combine is None else self.combine(zip(*shards))
        part = tuple(part) + host
        if self.directory is None:
            self.kept.append(part)
        else:
            self.append(self.directory, *part)

    def series(self, caller):
        """The ensemble's frames still held (not drained into files): a
        collective; rank 0 gets them, the others None."""
        if self.directory is not None:
            raise ValueError(f"{caller}: {self.begin} drains into a directory (read its files)")
        self.drain()
        if self.ens.rank != 0:
            return None
        if not self.kept:
            return tuple(np.zeros((0,) + shape, dtype=dt) for shape, dt in self.layout)
        return tuple(np.concatenate([p[i] for p in self.kept]) for i in range(len(self.layout)))

    def write(self, caller, directory):
        """What is left on the device and in ``kept`` to the files, then the
        geometry file; returns the frames recorded."""
        if self.directory is not None and os.path.abspath(self.directory) != os.path.abspath(directory):
            raise ValueError(f"{caller}: {self.begin} drained into another directory")
        self.drain()
        if self.ens.rank == 0:
            if self.directory is None:
                for part in self.kept:
                    self.append(directory, *part)
                self.kept = []
            self.geometry(directory)
        return self.frames


class _MapRecorder(_Recorder):
    ndev = 2

    def __init__(self, ens, directory, m, frac_bits):
        super().__init__(ens, "begin_map", directory)
        self.m, self.frac_bits = m, frac_bits
        self.layout = [((4, m, m), np.int64), ((2,), np.int64)]
        self.frame_bytes = 32 * m * m

    def get(self, T):
        return self.ens.ctx.map_series(0, T)

    def reset(self):
        self.ens.ctx.map_series_reset()

    def append(self, directory, planes, stats):
        for fr, s in zip(planes, stats):
            for name, plane in zip(("map_n", "map_omega", "map_k", "map_l"), fr):
                write_field(plane, os.path.join(directory, name))
            write_field(np.array([s[0], s[1], self.m, self.frac_bits], dtype=np.float64),
                        os.path.join(directory, "map_stats"))


class _KmapRecorder(_Recorder):
    ndev = 2

    def __init__(self, ens, directory, K, m, frac_bits):
        super().__init__(ens, "begin_kmap", directory)
        self.K, self.m, self.frac_bits = K, m, frac_bits
        self.layout = [((m, m), np.int64), ((8,), np.int64)]
        self.frame_bytes = 8 * (m * m + 8)

    def get(self, T):
        return self.ens.ctx.kmap_series_get(0, T)

    def reset(self):
        self.ens.ctx.kmap_series_reset()

    @staticmethod
    def append(directory, planes, stats):
        with open(os.path.join(directory, "kmap_n.bin"), "ab") as fn, \
                open(os.path.join(directory, "kmap_stats.bin"), "ab") as fs:
            for fr, s in zip(planes, stats):
                fn.write(np.asarray(fr, dtype=np.int64).tobytes(order="F"))  # (cell (i, j) at i + m*j)
                fs.write(np.asarray(s, dtype=np.int64).tobytes())

    def geometry(self, directory):
        with open(os.path.join(directory, "kmap_geom.bin"), "wb") as fh:
            fh.write(np.array([self.K, self.m, self.frac_bits], dtype=np.float64).tobytes())


class _PlaneRecorder(_Recorder):
    """The class-plane series (cond, trans, refr, absfreq, tangent; at most 4096
    classes an axis and 65536 cells a frame): ``prefix`` names the context's calls and
    the files, ``head`` leads <prefix>_geom.bin before the second axis' edges
    and the omega edges."""
    ndev = 3
    files = ("hist", "sums", "stats")

    def __init__(self, ens, directory, prefix, wedges, edges2, frac_bits, head, combine):
        super().__init__(ens, "begin_" + prefix, directory)
        self.prefix, self.wedges, self.edges2, self.combine = prefix, wedges, edges2, combine
        self.head = [edges2.size - 1, wedges.size - 1, frac_bits] if head is None else head
        nw, n2 = wedges.size - 1, edges2.size - 1
        self.layout = [((n2 + 2, nw + 2), np.int64), (plane_sums_shape(prefix, nw, n2), np.int64),
                       ((PLANE_TAILS[prefix][2],), np.int64)]
        self.frame_bytes = 8 * sum(int(np.prod(shape)) for shape, _ in self.layout)

    def get(self, T):
        return getattr(self.ens.ctx, self.prefix + "_series_get")(0, T)

    def reset(self):
        getattr(self.ens.ctx, self.prefix + "_series_reset")()

    def append(self, directory, *part):
        # (hist: the cell (class of the second axis c, omega class wc) at c*(nw + 2) + wc)
        for name, frames, (_, dt) in zip(self.files, part, self.layout):
            with open(os.path.join(directory, f"{self.prefix}_{name}.bin"), "ab") as fh:
                for fr in frames:
                    fh.write(np.ascontiguousarray(fr, dtype=dt).tobytes())

    def geometry(self, directory):
        with open(os.path.join(directory, self.prefix + "_geom.bin"), "wb") as fh:
            head = np.array(self.head, dtype=np.float64)
            fh.write(np.concatenate([head, self.edges2, self.wedges]).tobytes())


class _TransRecorder(_PlaneRecorder):
    """The transition series keeps [t, t_mark] of every frame on the host."""
    files = _PlaneRecorder.files + ("time",)

    def __init__(self, *a):
        super().__init__(*a)
        self.layout.append(((2,), np.float64))
        self.times, self.t_mark = [], None

    def host_part(self, T):
        times, self.times = np.array(self.times, dtype=np.float64).reshape(T, 2), []
        return (times,)


def _plane_args(omega_edges, edges2, frac_bits, axis, series, frame, n2):
    """begin_cond / _refr / _absfreq / _trans's checks of the two edge arrays,
    frac_bits and the cell cap; ``axis``, ``series``, ``frame`` and ``n2``
    are the series' words in the messages."""
    wedges = np.array(omega_edges, dtype=np.float64).ravel()
    edges2 = np.array(edges2, dtype=np.float64).ravel()
    for name, e in (("omega", wedges), (axis, edges2)):
        if e.size < 2 or not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
            raise ValueError(f"the {name} edges must be at least two finite increasing values")
    frac_bits = int(frac_bits)
    if not 0 <= frac_bits <= 32:
        raise ValueError(f"{series} frac_bits must be 0..32")
    if (edges2.size + 1) * (wedges.size + 1) > 65536:
        raise ValueError(f"{frame} frame holds at most 65536 cells, ({n2} + 2) * (nw + 2)")
    return wedges, edges2, frac_bits


class PacketEnsemble:
    """Device-resident packets advanced through a sequence of background
    snapshots — the packet branch of qgsw_raytrace.m:140-163 /
    qg2layersw_raytrace.m:185-209 with the symplectic integrator instead of
    ode23.

    Per PDE step the caller hands the previous and current spectral PV
    (prev_qk, qk); grid_U runs on the GPU into slots 0/1 and the packets take
    `nsub` leapfrog substeps over [t, t+dt] with the kick of substep s at
    alpha = (s + 1/2)/nsub (interpolate_U's linear blend at the kick time).
    """

    def __init__(self, x, k, L, f, Cg, nx, K_d2, shear=0.0, k_scale=1.0, nlayers=1, device=0,
                 bump=BUMP_QG, ctx: Context | None = None, shard=None, bounds=None, method="leapfrog",
                 iterations=None):
        """``shard`` = (rank, world): x, k are the whole ensemble (the same on
        every rank) and this rank advances its contiguous shard;
        frames are gathered to rank 0 on the device (dist.gather_packets) and
        ode23's error norm is max-reduced over the ranks.  ``bounds``: every
        rank's [lo, hi) (dist.shard_bounds / owner_bounds; default the even
        split).  A rank's shard may be empty (the PDE owner's, with weight 0):
        it then only takes part in the collectives.  ``method``,
        ``iterations``: the packet step (packet_method), set on the context."""
        self.ctx = ctx if ctx is not None else Context(device)
        # the packet step of advance / advance_intervals (packet_method; not advance_ode23's)
        self.method = packet_method(method, iterations)
        self.ctx.set_integrator(*self.method)
        self.L, self.f, self.Cg, self.nx = float(L), float(f), float(Cg), int(nx)
        self.gH = self.Cg ** 2
        self.K_d2, self.shear, self.k_scale = float(K_d2), float(shear), float(k_scale)
        self.ny_period = self.nx * nlayers
        self.bump = bump
        x = np.asarray(x, dtype=np.float64)
        k = np.asarray(k, dtype=np.float64)
        self.n_total = x.shape[0]
        self.rank, self.world = shard if shard is not None else (0, 1)
        self.bounds = None
        if self.world > 1:
            from .dist import shard_range
            self.bounds = list(bounds) if bounds is not None else \
                [shard_range(self.n_total, self.world, r) for r in range(self.world)]
            if len(self.bounds) != self.world or self.bounds[-1][1] != self.n_total:
                raise ValueError("bounds must give one [lo, hi) per rank covering the ensemble")
            lo, hi = self.bounds[self.rank]
            x, k = x[lo:hi], k[lo:hi]
        self.ctx.packets_set(x, k)
        self.n = x.shape[0]
        self._k0 = k  # (this shard's initial wavevectors: begin_recycle's home)
        self._recorders = {}  # the drained count series by name (begin_map ... begin_trans)
        self._rebin = None

    def set_method(self, method="leapfrog", iterations=None):
        """The packet step of advance / advance_intervals from here on (packet_method)."""
        self.method = packet_method(method, iterations)
        self.ctx.set_integrator(*self.method)

    def set_snapshots(self, prev_qk, qk):
        """grid_U(prev_qk) -> slot 0, grid_U(qk) -> slot 1 (layer 1 if 3-D)."""
        for slot, q in enumerate((prev_qk, qk)):
            q = np.asarray(q, dtype=np.complex128)
            if q.ndim == 3:
                q = q[:, :, 0]
            self.ctx.set_field_qk(slot, q, self.nx, self.L, self.K_d2, self.shear, self.k_scale,
                                  self.ny_period)

    def set_grid_snapshots(self, flow1, flow2):
        for slot, fl in enumerate((flow1, flow2)):
            self.ctx.set_field_grid(slot, flow_planes(fl), self.nx, self.L, self.ny_period)

    def advance(self, dt, nsub=1, save_every=0):
        if self.n == 0:
            return
        # re-bin after ~4 PDE intervals of packet motion: every 4 steps at one
        # substep per interval, every 20 at five (tuned on the bench workload)
        if self._rebin != 4 * nsub:
            self._rebin = 4 * nsub
            self.ctx.set_locality(self._rebin, 0)
        h = dt / nsub
        self.ctx.advance(h, nsub, self.f, self.gH, nslots=2, alpha0=0.5 / nsub, dalpha=1.0 / nsub,
                         bump=self.bump, save_every=save_every)

    def advance_intervals(self, dts, nsub=1, save_every=0):
        """len(dts) consecutive PDE intervals in one call, interval i between
        the snapshots in slots i and i+1 (swrt_advance_intervals): the same
        bits as one advance() per interval with the pair moved to slots 0, 1."""
        if self.n == 0:
            return
        if self._rebin != 4 * nsub:
            self._rebin = 4 * nsub
            self.ctx.set_locality(self._rebin, 0)
        self.ctx.advance_intervals([dt / nsub for dt in dts], nsub, self.f, self.gH, alpha0=0.5 / nsub,
                                   dalpha=1.0 / nsub, bump=self.bump, save_every=save_every)

    def advance_ode23(self, dt, rtol=1e-3, atol=1e-6, allreduce_max=None, stats=None, controller=None, hook=None):
        """The reference drivers' own integrator over [0, dt] with
        interpolate_U's alpha = t/dt (ode23(ray_ode, [0, dt], y0));
        ``controller`` and ``hook`` as in ode23_packets."""
        if allreduce_max is None and self.world > 1:
            import torch.distributed as dist

            from .dist import allreduce_max_fn
            allreduce_max = allreduce_max_fn(backend=dist.get_backend())
        # an empty shard contributes 0 to every error max (the max-norm's identity)
        ctx = self.ctx if self.n > 0 else _EmptyShard()
        return ode23_packets(ctx, (0.0, dt), dt, self.f, self.Cg, nslots=2, rtol=rtol, atol=atol,
                             bump=self.bump, allreduce_max=allreduce_max, stats=stats, controller=controller,
                             hook=hook)

    def mark_invariant(self, alpha=0.0):
        """Keep Omega_0 = omega(k) + U(x).k of this shard's packets at the
        current state, U from the snapshot pair at ``alpha``
        (symplectic_full_fourier.m:41)."""
        if self.n > 0:
            self.ctx.raydiag_mark(self.f, self.gH, nslots=2, alpha=alpha, bump=self.bump)

    def record_diagnostics(self, alpha):
        """Append this shard's frame at the current state to the device-side
        series (Context.raydiag_series; queued, no host wait).  The ensemble's
        frames are combine_frames() of the shards' series; an empty shard
        records nothing and stands there as zeros (n = 0)."""
        if self.n > 0:
            self.ctx.raydiag_record(self.f, self.gH, nslots=2, alpha=alpha, bump=self.bump)

    def begin_spectrum(self, edges):
        """Open the energy-vs-omega series of this run over ``edges``
        (load_data.m:39-40): swrt_omega_series_begin with the ensemble's f, Cg."""
        self._spec_edges = np.array(edges, dtype=np.float64).ravel()
        self._spec_frames = 0
        if self.n > 0:
            self.ctx.omega_series_begin(self.f, self.Cg, self._spec_edges)

    def record_spectrum(self):
        """Append this shard's frame at the current state to the device-side
        series (queued, no host wait).  An empty shard records nothing."""
        if getattr(self, "_spec_edges", None) is None:
            raise SwrtError("record_spectrum: call begin_spectrum first")
        self._spec_frames += 1
        if self.n > 0:
            self.ctx.omega_series_record()

    def spectrum_series(self):
        """(counts (T, nbins + 2) int64, stats (T, 4)) of the ensemble.
        Sharded: a collective (every rank calls it); rank 0 gets
        combine_spectra() of the shards' series, the others None."""
        if getattr(self, "_spec_edges", None) is None:
            raise SwrtError("spectrum_series: call begin_spectrum first")
        T, nb = self._spec_frames, self._spec_edges.size - 1
        counts, stats = self.ctx.omega_series(0, T) if self.n > 0 else empty_spectrum(T, nb)
        if self.world == 1:
            return counts, stats
        import torch
        import torch.distributed as dist

        from .dist import _device_for
        dev = _device_for(dist.get_backend())
        parts = []
        for a in (counts, stats):
            buf = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            out = [torch.empty_like(buf) for _ in range(self.world)]
            dist.all_gather(out, buf)
            parts.append([o.cpu().numpy() for o in out])
        if self.rank != 0:
            return None
        return combine_spectra(zip(parts[0], parts[1]))

    def state(self):
        return self.ctx.packets_get()

    def write_spectrum(self, directory):
        """The run's spectrum series as write_field files (read_field reads
        them): omega_hist.bin, one frame of nbins + 2 counts [below, bins,
        above] per recorded frame (fp64, exact: every count <= N < 2^53),
        omega_stats.bin, 4 values per frame, and omega_edges.bin, one frame of
        nbins + 1 values.  Sharded: a collective; rank 0 writes.  Returns the
        frames recorded."""
        series = self.spectrum_series()
        if series is not None:
            counts, stats = series
            for row, st in zip(counts, stats):
                write_field(row, os.path.join(directory, "omega_hist"))
                write_field(st, os.path.join(directory, "omega_stats"))
            write_field(self._spec_edges, os.path.join(directory, "omega_edges"))
        return self._spec_frames

    def _recorder(self, name, caller):
        """The recorder begin_<name> opened, for the public method ``caller``."""
        rec = self._recorders.get(name)
        if rec is None:
            raise SwrtError(f"{caller}: call begin_{name} first")
        return rec

    def _record_blended(self, name, alpha):
        """record_cond / record_refr: slot 0 alone, or slots 0 and 1 at ``alpha``."""
        record = getattr(self.ctx, name + "_series_record")
        blend = dict(nslots=1) if alpha is None else dict(nslots=2, alpha=alpha)
        self._recorder(name, "record_" + name).record(lambda: record(bump=self.bump, **blend))

    def begin_map(self, m, frac_bits=20, directory=None):
        """Open the series of m x m packet density and wave-energy maps of
        this run over the ensemble's periodic square (swrt_map_series_begin
        with its L, f, Cg).  ``directory``: where record_map drains the device
        series when it grows large (default: the drained frames wait in host
        memory for write_maps)."""
        m, frac_bits = int(m), int(frac_bits)
        if not 1 <= m <= 4096:
            raise ValueError("map cells must be 1..4096")
        if not 0 <= frac_bits <= 32:
            raise ValueError("map frac_bits must be 0..32")
        self._recorders["map"] = _MapRecorder(self, directory, m, frac_bits)
        if self.n > 0:
            self.ctx.map_series_begin(self.L, m, self.f, self.Cg, frac_bits)

    def record_map(self):
        """Append this shard's map frame at the current state to the
        device-side series (queued, no host wait).  An empty shard records
        nothing.  When the device series holds more than 256 MB it is drained
        (get, combine, append, reset): a collective when sharded, at the same
        frame on every rank."""
        self._recorder("map", "record_map").record(self.ctx.map_series_record)

    def write_maps(self, directory):
        """The run's map series as write_field files (read_field(name, m, m, 1,
        frames) reads them): map_n.bin, map_omega.bin, map_k.bin, map_l.bin —
        the four planes [count, sum q(omega), sum q(k), sum q(l)] as exact
        fp64 integers (every one below 2^53), one m x m frame each per record,
        first index x — and map_stats.bin, [n, rejected, m, frac_bits] per
        frame.  Sharded: a collective; rank 0 writes.  Returns the frames
        recorded."""
        return self._recorder("map", "write_maps").write("write_maps", directory)

    def begin_kmap(self, K, m, frac_bits=16, directory=None):
        """Open the series of m x m count planes over [-K, K) x [-K, K) of the
        (k, l) plane and the wavevector moments of this run
        (swrt_kmap_series_begin).  ``directory``: where record_kmap drains the
        device series when it grows large (default: the drained frames wait in
        host memory for write_kmaps)."""
        K, m, frac_bits = float(K), int(m), int(frac_bits)
        if not (K > 0 and math.isfinite(K)):
            raise ValueError("k-plane half-width must be positive and finite")
        if not 1 <= m <= 4096:
            raise ValueError("k-plane cells must be 1..4096")
        if not 0 <= frac_bits <= 32:
            raise ValueError("k-plane frac_bits must be 0..32")
        self._recorders["kmap"] = _KmapRecorder(self, directory, K, m, frac_bits)
        if self.n > 0:
            self.ctx.kmap_series_begin(K, m, frac_bits)

    def record_kmap(self):
        """Append this shard's k-plane frame at the current state to the
        device-side series (queued, no host wait).  An empty shard records
        nothing.  When the device series holds more than 256 MB it is drained
        (get, combine, append, reset): a collective when sharded, at the same
        frame on every rank."""
        self._recorder("kmap", "record_kmap").record(self.ctx.kmap_series_record)

    def kmap_series(self):
        """(planes (T, m, m) int64, stats (T, 8) int64) of the ensemble's
        frames still held (not yet drained into files): planes[t, i, j] the
        cell with k index i and l index j.  Sharded: a collective; rank 0 gets
        the sum of the shards' frames, the others None."""
        return self._recorder("kmap", "kmap_series").series("kmap_series")

    def write_kmaps(self, directory):
        """The run's k-plane series as raw native-endian files: kmap_n.bin
        (int64, one m x m plane per frame, cell (i, j) at i + m*j, first index
        k), kmap_stats.bin (8 int64 per frame: n, rejected, outside and the
        five moment sums) and kmap_geom.bin (three doubles [K, m, frac_bits]).
        Sharded: a collective; rank 0 writes.  Returns the frames recorded."""
        return self._recorder("kmap", "write_kmaps").write("write_kmaps", directory)

    def begin_cond(self, omega_edges, which, q_edges, frac_bits=20, directory=None):
        """Open the conditional spectrum series of this run
        (swrt_cond_series_begin with the ensemble's f, Cg): omega classes over
        ``omega_edges`` by the classes of the flow scalar ``which`` ("zeta",
        "sigma" or "D") at the packets over ``q_edges``.  ``directory``: where
        record_cond drains the device series when it grows large (default: the
        drained frames wait in host memory for write_conds)."""
        if which not in COND_WHICH:
            raise ValueError('the conditioning scalar must be "zeta", "sigma" or "D"')
        wedges, qedges, frac_bits = _plane_args(omega_edges, q_edges, frac_bits, "q", "conditional spectrum",
                                                "a conditional spectrum", "nq")
        head = [COND_WHICH[which], qedges.size - 1, wedges.size - 1, frac_bits]
        self._recorders["cond"] = _PlaneRecorder(self, directory, "cond", wedges, qedges, frac_bits, head,
                                                 combine_conds)
        if self.n > 0:
            self.ctx.cond_series_begin(self.f, self.Cg, wedges, COND_WHICH[which], qedges, frac_bits)

    def record_cond(self, alpha=None):
        """Append this shard's conditional spectrum frame at the current state
        to the device-side series (queued, no host wait), in the flow of slot 0
        (``alpha`` None) or of slots 0 and 1 blended at ``alpha``.  An empty
        shard records nothing.  When the device series holds more than 256 MB
        it is drained (get, combine, append, reset): a collective when
        sharded, at the same frame on every rank."""
        self._record_blended("cond", alpha)

    def cond_series(self):
        """(counts (T, nq + 2, nw + 2), sums (T, nq + 2), stats (T, 2)), all
        int64, of the ensemble's frames still held (not yet drained into
        files).  Sharded: a collective; rank 0 gets combine_conds() of the
        shards' frames, the others None."""
        return self._recorder("cond", "cond_series").series("cond_series")

    def write_conds(self, directory):
        """The run's conditional spectrum series as raw native-endian files:
        cond_hist.bin (int64, one (nq + 2) x (nw + 2) plane per frame, cell
        (qc, wc) at qc*(nw + 2) + wc), cond_sums.bin (nq + 2 int64 per frame),
        cond_stats.bin (2 int64 per frame: n, rejected) and cond_geom.bin
        (doubles [which, nq, nw, frac_bits], the nq + 1 q edges, the nw + 1
        omega edges).  Sharded: a collective; rank 0 writes.  Returns the
        frames recorded."""
        return self._recorder("cond", "write_conds").write("write_conds", directory)

    def begin_refr(self, omega_edges, a_edges, frac_bits=20, directory=None):
        """Open the refraction series of this run (swrt_refr_series_begin with
        the ensemble's f, Cg): omega classes over ``omega_edges`` by the
        classes of the alignment c = 2 gamma / sigma over ``a_edges``.
        ``directory``: where record_refr drains the device series when it
        grows large (default: the drained frames wait in host memory for
        write_refrs)."""
        wedges, aedges, frac_bits = _plane_args(omega_edges, a_edges, frac_bits, "alignment", "refraction series",
                                                "a refraction", "na")
        self._recorders["refr"] = _PlaneRecorder(self, directory, "refr", wedges, aedges, frac_bits, None,
                                                 combine_refrs)
        if self.n > 0:
            self.ctx.refr_series_begin(self.f, self.Cg, wedges, aedges, frac_bits)

    def record_refr(self, alpha=None):
        """Append this shard's refraction frame at the current state to the
        device-side series (queued, no host wait), in the flow of slot 0
        (``alpha`` None) or of slots 0 and 1 blended at ``alpha``.  An empty
        shard records nothing.  When the device series holds more than 256 MB
        it is drained (get, combine, append, reset): a collective when
        sharded, at the same frame on every rank."""
        self._record_blended("refr", alpha)

    def refr_series(self):
        """(counts (T, na + 2, nw + 2), sums (T, 3 (nw + 2) + (na + 2)), stats
        (T, 2)), all int64, of the ensemble's frames still held (not yet
        drained into files).  Sharded: a collective; rank 0 gets
        combine_refrs() of the shards' frames, the others None."""
        return self._recorder("refr", "refr_series").series("refr_series")

    def write_refrs(self, directory):
        """The run's refraction series as raw native-endian files:
        refr_hist.bin (int64, one (na + 2) x (nw + 2) plane per frame, cell
        (ac, wc) at ac*(nw + 2) + wc), refr_sums.bin (3 (nw + 2) + (na + 2)
        int64 per frame), refr_stats.bin (2 int64 per frame: n, rejected) and
        refr_geom.bin (doubles [na, nw, frac_bits], the na + 1 alignment
        edges, the nw + 1 omega edges).  Sharded: a collective; rank 0 writes.
        Returns the frames recorded."""
        return self._recorder("refr", "write_refrs").write("write_refrs", directory)

    def begin_absfreq(self, omega_edges, abs_edges, frac_bits=20, directory=None):
        """Open the absolute-frequency series of this run
        (swrt_absfreq_series_begin with the ensemble's f, Cg): omega classes
        over ``omega_edges`` by the classes of Omega = omega + U.k over
        ``abs_edges``.  ``directory``: where record_absfreq drains the device
        series when it grows large (default: the drained frames wait in host
        memory for write_absfreqs)."""
        wedges, oedges, frac_bits = _plane_args(omega_edges, abs_edges, frac_bits, "absolute-frequency",
                                                "absolute-frequency series", "an absolute-frequency", "no")
        self._recorders["absfreq"] = _PlaneRecorder(self, directory, "absfreq", wedges, oedges, frac_bits, None,
                                                    combine_absfreqs)
        if self.n > 0:
            self.ctx.absfreq_series_begin(self.f, self.Cg, wedges, oedges, frac_bits)

    def record_absfreq(self, slot_a=0, slot_b=-1, alpha=0.0, tau=1.0):
        """Append this shard's absolute-frequency frame at the current state
        to the device-side series (queued, no host wait): the flow of
        ``slot_a`` (alpha = 0) and ``slot_b`` (alpha = 1) blended at ``alpha``,
        its rate (slot_b - slot_a) / ``tau``; ``slot_b`` -1: slot_a alone, zero
        rates.  An empty shard records nothing.  When the device series holds
        more than 256 MB it is drained (get, combine, append, reset): a
        collective when sharded, at the same frame on every rank."""
        self._recorder("absfreq", "record_absfreq").record(
            lambda: self.ctx.absfreq_series_record(slot_a, slot_b, alpha, tau, bump=self.bump))

    def absfreq_series(self):
        """(counts (T, no + 2, nw + 2), sums (T, 3 (nw + 2) + 2 (no + 2)),
        stats (T, 2)), all int64, of the ensemble's frames still held (not yet
        drained into files).  Sharded: a collective; rank 0 gets
        combine_absfreqs() of the shards' frames, the others None."""
        return self._recorder("absfreq", "absfreq_series").series("absfreq_series")

    def write_absfreqs(self, directory):
        """The run's absolute-frequency series as raw native-endian files:
        absfreq_hist.bin (int64, one (no + 2) x (nw + 2) plane per frame, cell
        (oc, wc) at oc*(nw + 2) + wc), absfreq_sums.bin (3 (nw + 2) +
        2 (no + 2) int64 per frame), absfreq_stats.bin (2 int64 per frame: n,
        rejected) and absfreq_geom.bin (doubles [no, nw, frac_bits], the
        no + 1 Omega edges, the nw + 1 omega edges).  Sharded: a collective;
        rank 0 writes.  Returns the frames recorded."""
        return self._recorder("absfreq", "write_absfreqs").write("write_absfreqs", directory)

    def begin_trans(self, omega_edges, src_edges, frac_bits=20, by=0, directory=None):
        """Open the transition series of this run (swrt_trans_series_begin
        with the ensemble's f, Cg): omega classes over ``omega_edges`` by the
        classes of each packet's source value over ``src_edges``.  ``by`` (0:
        the source is omega at a mark, 1: a ring index) only goes into
        trans_geom.bin.  ``directory``: where record_trans drains the device
        series when it grows large (default: the drained frames wait in host
        memory for write_trans)."""
        wedges, sedges, frac_bits = _plane_args(omega_edges, src_edges, frac_bits, "source", "transition series",
                                                "a transition", "ns")
        if by not in (0, 1):
            raise ValueError("by must be 0 (omega at the mark) or 1 (ring)")
        head = [sedges.size - 1, wedges.size - 1, frac_bits, int(by)]
        self._recorders["trans"] = _TransRecorder(self, directory, "trans", wedges, sedges, frac_bits, head,
                                                  combine_transitions)
        if self.n > 0:
            self.ctx.trans_series_begin(self.f, self.Cg, wedges, sedges, frac_bits)

    def mark_trans(self, values=None, t=None):
        """Set every packet's source value: its current omega (``values``
        None; queued, no host wait) or ``values``, one per packet of the
        **whole** ensemble in the original order (a shard takes its own).
        ``t``: the time of the mark, kept for trans_time.bin.  Every rank
        calls it at the same frame, so the shards' mark serials agree."""
        rec = self._recorder("trans", "mark_trans")
        if values is not None:
            values = np.asarray(values, dtype=np.float64).ravel()
            if values.size != self.n_total:
                raise ValueError("mark_trans: one source value per packet of the whole ensemble")
            lo, hi = self.bounds[self.rank] if self.bounds is not None else (0, self.n_total)
            values = values[lo:hi]
        if self.n > 0:
            if values is None:
                self.ctx.trans_series_mark()
            else:
                self.ctx.trans_series_mark_values(values)
        rec.t_mark = np.nan if t is None else float(t)

    def record_trans(self, t=None):
        """Append this shard's transition frame at the current state to the
        device-side series (queued, no host wait).  An empty shard records
        nothing.  When the device series holds more than 256 MB it is drained
        (get, combine, append, reset; the mark stays): a collective when
        sharded, at the same frame on every rank."""
        rec = self._recorder("trans", "record_trans")
        if rec.t_mark is None:
            raise SwrtError("record_trans: call mark_trans first")
        rec.times.append((np.nan if t is None else float(t), rec.t_mark))
        rec.record(self.ctx.trans_series_record)

    def trans_series(self):
        """(counts (T, ns + 2, nw + 2), sums (T, ns + 2, 3), stats (T, 3)), all
        int64, and times (T, 2) fp64 [t, t_mark] of the ensemble's frames still
        held (not yet drained into files).  Sharded: a collective; rank 0 gets
        combine_transitions() of the shards' frames, the others None."""
        return self._recorder("trans", "trans_series").series("trans_series")

    def write_trans(self, directory):
        """The run's transition series as raw native-endian files:
        trans_hist.bin (int64, one (ns + 2) x (nw + 2) plane per frame, cell
        (sc, wc) at sc*(nw + 2) + wc), trans_sums.bin (3 (ns + 2) int64 per
        frame: per source class the sums of omega, d and d^2 in quanta),
        trans_stats.bin (3 int64 per frame: n, rejected, mark serial),
        trans_time.bin (2 doubles per frame: t, t_mark) and trans_geom.bin
        (doubles [ns, nw, frac_bits, by], the ns + 1 source edges, the nw + 1
        omega edges).  Sharded: a collective; rank 0 writes.  Returns the
        frames recorded."""
        return self._recorder("trans", "write_trans").write("write_trans", directory)

    def begin_tangent(self, omega_edges, growth_edges, directory=None, t=None):
        """Start carrying the tangent map (swrt_tangent_begin: M = I, the
        caustic counters 0; from here on the leapfrog calls take the per-packet
        route, x and k keep their bits) and open its series with the
        ensemble's f, Cg: the classes of s = |M|_F^2 / 4 over ``growth_edges``
        by the omega classes over ``omega_edges``.  ``t``: the time of this
        first mark, kept for tangent_time.bin.  ``directory``: where
        record_tangent drains the device series when it grows large (default:
        the drained frames wait in host memory for write_tangents)."""
        wedges, gedges, _ = _plane_args(omega_edges, growth_edges, 0, "growth", "tangent series", "a tangent", "ns")
        head = [gedges.size - 1, wedges.size - 1]
        rec = _TransRecorder(self, directory, "tangent", wedges, gedges, 0, head, combine_tangents)
        rec.t_mark = np.nan if t is None else float(t)
        self._recorders["tangent"] = rec
        if self.n > 0:
            self.ctx.tangent_begin()
            self.ctx.tangent_series_begin(self.f, self.Cg, wedges, gedges)

    def mark_tangent(self, t=None):
        """A new window: M = I, the counters 0, the next mark serial (queued, no
        host wait).  Every rank calls it at the same frame, so the shards'
        serials agree."""
        rec = self._recorder("tangent", "mark_tangent")
        if self.n > 0:
            self.ctx.tangent_mark()
        rec.t_mark = np.nan if t is None else float(t)

    def record_tangent(self, t=None):
        """Append this shard's tangent frame at the current state to the
        device-side series (queued, no host wait).  An empty shard records
        nothing.  Drained like the transition series' frames."""
        rec = self._recorder("tangent", "record_tangent")
        rec.times.append((np.nan if t is None else float(t), rec.t_mark))
        rec.record(self.ctx.tangent_series_record)

    def tangent_series(self):
        """(counts (T, ns + 2, nw + 2), sums (T, 3 (nw + 2) + (ns + 2)), stats
        (T, 3)), all int64, and times (T, 2) fp64 [t, t_mark] of the ensemble's
        frames still held.  Sharded: a collective; rank 0 gets
        combine_tangents() of the shards' frames, the others None."""
        return self._recorder("tangent", "tangent_series").series("tangent_series")

    def tangent_state(self):
        """(M (n, 16) row-major, caustics (n,) int32) of this shard's packets in
        their original order (swrt_tangent_get; waits)."""
        self._recorder("tangent", "tangent_state")
        if self.n == 0:
            return np.zeros((0, 16)), np.zeros(0, dtype=np.int32)
        return self.ctx.tangent_get()

    def end_tangent(self):
        """Stop carrying the tangent map (swrt_tangent_end); the series' frames
        already drained or written stay."""
        self._recorder("tangent", "end_tangent")
        if self.n > 0 and self.ctx.tangent_live():
            self.ctx.tangent_end()

    def write_tangents(self, directory):
        """The run's tangent series as raw native-endian files:
        tangent_hist.bin (int64, one (ns + 2) x (nw + 2) plane per frame, cell
        (gc, wc) at gc*(nw + 2) + wc), tangent_sums.bin (3 (nw + 2) + (ns + 2)
        int64 per frame: per omega class the sums of e(s), e(|J|) and the
        caustic counters, then per growth class the caustic counters),
        tangent_stats.bin (3 int64 per frame: n, rejected, mark serial),
        tangent_time.bin (2 doubles per frame: t, t_mark) and tangent_geom.bin
        (doubles [ns, nw], the ns + 1 growth edges, the nw + 1 omega edges).
        Sharded: a collective; rank 0 writes.  Returns the frames recorded."""
        return self._recorder("tangent", "write_tangents").write("write_tangents", directory)

    def begin_recycle(self, omega_cut, seed=0, frac_bits=20, directory=None, every=1):
        """Begin recycling this run's packets (swrt_recycle_begin with the
        ensemble's f, Cg and L): at every recycle() a packet whose omega has
        reached ``omega_cut`` is re-injected with its initial wavevector and a
        fresh uniform position.  A shard passes its first global id as
        index_base, so the ensemble's packets and frames do not depend on the
        sharding.  ``directory``: where write_recycle writes (default: given
        there).  ``every`` only goes into recycle_geom.bin."""
        omega_cut, frac_bits = float(omega_cut), int(frac_bits)
        if not math.isfinite(omega_cut) or not omega_cut > abs(self.f):
            raise ValueError("omega_cut must be finite and above |f|")
        if not 0 <= frac_bits <= 32:
            raise ValueError("recycle frac_bits must be 0..32")
        lo = self.bounds[self.rank][0] if self.bounds is not None else 0
        self._recycle = dict(omega_cut=omega_cut, seed=int(seed), frac_bits=frac_bits, directory=directory,
                             every=int(every), times=[])
        if self.n > 0:
            self.ctx.recycle_begin(self.f, self.Cg, omega_cut, self.L, seed=seed, index_base=lo, frac_bits=frac_bits,
                                   home_k=self._k0)

    def recycle(self, t):
        """One recycle event on this shard's packets at the time ``t``
        (queued, no host wait).  An empty shard only remembers t.  Every rank
        calls it at the same frame, so the shards' serials agree."""
        st = getattr(self, "_recycle", None)
        if st is None:
            raise SwrtError("recycle: call begin_recycle first")
        st["times"].append(float(t))
        if self.n > 0:
            self.ctx.recycle_apply()

    def _gather_shards(self, a, sizes):
        """``a`` of every shard, in rank order (a collective); ``sizes``: the
        shards' first dimensions."""
        import torch
        import torch.distributed as dist

        from .dist import _device_for
        dev = _device_for(dist.get_backend())
        padded = np.zeros((max(sizes),) + a.shape[1:], dtype=a.dtype)
        padded[:a.shape[0]] = a
        buf = torch.from_numpy(padded).to(dev)
        out = [torch.empty_like(buf) for _ in range(self.world)]
        dist.all_gather(out, buf)
        return [o.cpu().numpy()[:s] for o, s in zip(out, sizes)]

    def recycle_series(self):
        """(stats (T, 8) int64, times (T,) fp64) of the ensemble's events.
        Sharded: a collective; rank 0 gets combine_recycles() of the shards'
        frames, the others None."""
        st = getattr(self, "_recycle", None)
        if st is None:
            raise SwrtError("recycle_series: call begin_recycle first")
        T = len(st["times"])
        stats = self.ctx.recycle_get(0, T) if self.n > 0 else np.zeros((T, 8), dtype=np.int64)
        if self.world > 1:
            parts = self._gather_shards(stats, [T] * self.world)
            if self.rank != 0:
                return None
            stats = combine_recycles(parts)
        return stats, np.array(st["times"], dtype=np.float64)

    def recycle_generations(self):
        """How often every packet of the ensemble was re-injected, int32 in
        the original order.  Sharded: a collective; rank 0 gets the whole
        ensemble's, the others None."""
        if getattr(self, "_recycle", None) is None:
            raise SwrtError("recycle_generations: call begin_recycle first")
        gen = self.ctx.recycle_state()[0] if self.n > 0 else np.zeros(0, dtype=np.int32)
        if self.world > 1:
            parts = self._gather_shards(gen, [hi - lo for lo, hi in self.bounds])
            return np.concatenate(parts) if self.rank == 0 else None
        return gen

    def write_recycle(self, directory=None):
        """The run's recycling as raw native-endian files: recycle_stats.bin
        (8 int64 per event: n, absorbed, rejected, sum q(omega_out),
        sum q(omega_home), sum age, max age, serial), recycle_time.bin (one
        double per event), recycle_geom.bin (doubles omega_cut, L, seed,
        frac_bits, f, Cg, every) and recycle_gen.bin (int32 per packet of the
        ensemble in the original order: its re-injections).  Sharded: a
        collective; rank 0 writes.  Returns the events."""
        st = getattr(self, "_recycle", None)
        if st is None:
            raise SwrtError("write_recycle: call begin_recycle first")
        directory = st["directory"] if directory is None else directory
        if directory is None:
            raise ValueError("write_recycle: no directory given here or to begin_recycle")
        series = self.recycle_series()
        gen = self.recycle_generations()
        if self.rank == 0:
            stats, times = series
            for name, a in (("recycle_stats", stats), ("recycle_time", times), ("recycle_gen", gen),
                            ("recycle_geom", np.array([st["omega_cut"], self.L, st["seed"], st["frac_bits"], self.f,
                                                       self.Cg, st["every"]], dtype=np.float64))):
                with open(os.path.join(directory, name + ".bin"), "wb") as fh:
                    fh.write(np.ascontiguousarray(a).tobytes())
        return len(st["times"])

    def begin_tracks(self, ids, directory=None):
        """Track the packets with the **global** ids ``ids`` (distinct, in
        0..N-1 of the whole ensemble; a frame's rows follow their order):
        swrt_track_begin on this shard with the ids inside its bounds, as
        local indices.  A shard that owns none records nothing.
        ``directory``: where record_tracks drains the device series when it
        grows large (default: the drained frames wait in host memory for
        write_tracks)."""
        ids = track_ids_array(ids, self.n_total)
        lo, hi = self.bounds[self.rank] if self.bounds is not None else (0, self.n_total)
        rows = shard_track_rows(ids, lo, hi)
        self._trk = dict(ids=ids, rows=rows, directory=directory, frames=0, pending=0, kept=[], times=[],
                         ids_written=False)
        if rows.size > 0:
            self.ctx.track_begin(ids[rows] - lo)

    def record_tracks(self, t, nslots, alpha=0.0):
        """Append this shard's track frame at the current state, time ``t``,
        to the device-side series (queued, no host wait); the flow from slot 0
        (``nslots=1``), the blend of slots 0 and 1 at ``alpha`` (2), or none
        (0: Omega, zeta, sigma, D are NaN).  When the ensemble's device series
        pass 256 MB they are drained: a collective when sharded, at the same
        frame on every rank."""
        st = getattr(self, "_trk", None)
        if st is None:
            raise SwrtError("record_tracks: call begin_tracks first")
        st["frames"] += 1
        st["pending"] += 1
        st["times"].append(float(t))
        if st["rows"].size > 0:
            self.ctx.track_record(self.f, self.gH, nslots=nslots, alpha=alpha, bump=self.bump)
        if st["pending"] * 64 * st["ids"].size > MAP_DRAIN_BYTES:
            self._drain_tracks()

    def _drain_tracks(self):
        """The frames on the device, every shard's rows back in the caller's
        id order, to the files or the host list of rank 0; the device series
        emptied."""
        st = self._trk
        T, m = st["pending"], st["ids"].size
        if T == 0:
            return
        if st["rows"].size > 0:
            part = self.ctx.track_series(0, T)
            self.ctx.track_reset()
        else:
            part = np.zeros((T, 8, 0))
        times, st["times"] = st["times"], []
        st["pending"] = 0
        if self.world > 1:
            import torch
            import torch.distributed as dist

            from .dist import _device_for
            dev = _device_for(dist.get_backend())
            padded = np.zeros((T, 8, m), dtype=np.int64)  # (as integers: the transport keeps every bit)
            padded[:, :, :part.shape[2]] = part.view(np.int64)
            buf = torch.from_numpy(padded).to(dev)
            out = [torch.empty_like(buf) for _ in range(self.world)]
            dist.all_gather(out, buf)
            if self.rank != 0:
                return
            counts = [shard_track_rows(st["ids"], lo, hi).size for lo, hi in self.bounds]
            parts = [o.cpu().numpy()[:, :, :c].view(np.float64) for o, c in zip(out, counts)]
            series = combine_tracks(parts, st["ids"], self.bounds)
        else:
            series = part
        if st["directory"] is None:
            st["kept"].append((series, times))
        else:
            self._append_tracks(st["directory"], series, times)

    def _append_tracks(self, directory, series, times):
        L = self.L
        for fr, t in zip(series, times):
            write_field(np.mod(fr[0:2].T + L / 2, L) - L / 2, os.path.join(directory, "track_x"))
            write_field(fr[2:4].T, os.path.join(directory, "track_k"))
            write_field(fr[4:8].T, os.path.join(directory, "track_diag"))
            write_field(np.array([[t]]), os.path.join(directory, "track_time"))

    def write_tracks(self, directory):
        """The run's track series as write_field files: track_x.bin (m x 2 per
        frame, x wrapped to [-L/2, L/2) as write_frame wraps packet_x.bin),
        track_k.bin (m x 2), track_diag.bin (m x 4: Omega, zeta, sigma, D),
        track_time.bin (one value per frame) and track_ids.bin (one frame of m
        values, the global ids in row order) — read_field("track_x", m, 2, 1,
        frames) and load_data.m with Npackets = m read them.  Sharded: a
        collective; rank 0 writes.  Returns the frames recorded."""
        st = getattr(self, "_trk", None)
        if st is None:
            raise SwrtError("write_tracks: call begin_tracks first")
        if st["directory"] is not None and os.path.abspath(st["directory"]) != os.path.abspath(directory):
            raise ValueError("write_tracks: begin_tracks drained into another directory")
        self._drain_tracks()
        if self.rank == 0:
            if st["directory"] is None:
                for series, times in st["kept"]:
                    self._append_tracks(directory, series, times)
                st["kept"] = []
            if not st["ids_written"]:
                write_field(st["ids"].astype(np.float64), os.path.join(directory, "track_ids"))
                st["ids_written"] = True
        return st["frames"]

    def write_frame(self, t, directory, packet_files=True):
        """qgsw_raytrace.m:159-162: wrapped x, k and t appended to
        packet_x.bin / packet_k.bin / packet_time.bin.  Sharded: a collective
        (every rank calls it); rank 0 writes the whole ensemble.  Without
        ``packet_files`` only t is written (the time of a spectrum frame) and
        nothing is downloaded."""
        if not packet_files:
            if self.rank == 0:
                write_field(np.array([[t]]), os.path.join(directory, "packet_time"))
            return
        if self.world > 1:
            from .dist import gather_packets
            full = gather_packets(self.ctx, self.n_total, self.world, self.rank, bounds=self.bounds)
            if full is None:
                return
            x, k = full
        else:
            x, k = self.state()
        L = self.L
        write_field(np.mod(x + L / 2, L) - L / 2, os.path.join(directory, "packet_x"))
        write_field(k, os.path.join(directory, "packet_k"))
        write_field(np.array([[t]]), os.path.join(directory, "packet_time"))


def step_packet_xka(P, U, GradU, H, C0, f, dx, dy, dt, nsteps=1, ctx: Context | None = None):
    """Pout = step_packet_xka(P, U, GradU, H, C0, f, dx, dy, dt)
    (ray_trace_sw/step_packet_xka.m:1-91) on the GPU.

    P: dict with x, y, k, l, a (scalars or equal-length arrays = many packets).
    U: dict u, v; GradU: dict u_x, u_y, v_x, v_y; H: field (nx x nx).
    `nsteps` > 1 repeats the step (the raytrace_sw.m:125-130 loop) on device."""
    from .scheme import default_context
    ctx = ctx or default_context()
    if not np.allclose(np.asarray(H).shape, np.asarray(U["u"]).shape) or np.asarray(H).shape[0] != np.asarray(H).shape[1]:
        raise ValueError("fields must be nx x nx")
    ctx.xka_set_fields(U, GradU, H, dx, dy)
    names = ("x", "y", "k", "l", "a")
    scalar = np.ndim(P["x"]) == 0
    st = np.stack([np.atleast_1d(np.asarray(P[n], dtype=np.float64)) for n in names], axis=1)
    out, _ = ctx.xka_step(st, C0, f, dt, nsteps)
    return {n: (float(out[0, i]) if scalar else out[:, i].copy()) for i, n in enumerate(names)}


def raytrace_xka(P0, U, GradU, H, C0, f, dx, dy, dt, nsteps, ctx: Context | None = None):
    """The packet loop of ray_trace_sw/raytrace_sw.m:124-130: P(i, 1) = P0(i),
    P(i, j) = step_packet_xka(P(i, j-1), ...) for j = 2..nsteps.  Returns a dict
    of (np, nsteps) arrays (column j-1 = state after j-1 steps)."""
    from .scheme import default_context
    ctx = ctx or default_context()
    ctx.xka_set_fields(U, GradU, H, dx, dy)
    return _trace_xka(ctx, P0, C0, f, dt, nsteps)


def rsw_background(S, f, Cg, L=2 * np.pi, ctx: Context | None = None):
    """U, GradU, H of ray_trace_sw/raytrace_sw.m:16-52 from an RSW state
    S = [u v eta] (nx x nx x 3): the geostrophic projection and its seven
    k2g run on the GPU, and the result stays there as the xka background
    (the next raytrace_sw / step_packet_xka call on ctx uses it without a
    re-upload).  Returns host copies (U dict, GradU dict, H)."""
    from .scheme import default_context
    ctx = ctx or default_context()
    ctx.xka_set_rsw(S, f, Cg, L)
    return ctx.xka_get_fields()


def raytrace_sw(S, f, Cg, P0, dt, nsteps, L=2 * np.pi, ctx: Context | None = None):
    """ray_trace_sw/raytrace_sw.m end to end on the GPU: the background of
    :16-52 from S = [u v eta], then the packet loop of :124-130 with
    step_packet_xka(P, U, GradU, H, C0 = Cg, f, dx, dx, dt) (:22-23, 130).
    Returns the (np, nsteps) dict of raytrace_xka."""
    from .scheme import default_context
    ctx = ctx or default_context()
    ctx.xka_set_rsw(S, f, Cg, L)
    return _trace_xka(ctx, P0, Cg, f, dt, nsteps)


def _trace_xka(ctx, P0, C0, f, dt, nsteps):
    names = ("x", "y", "k", "l", "a")
    st = np.stack([np.atleast_1d(np.asarray(P0[n], dtype=np.float64)) for n in names], axis=1)
    npk = st.shape[0]
    out = {n: np.zeros((npk, nsteps)) for n in names}
    for i, n in enumerate(names):
        out[n][:, 0] = st[:, i]
    if nsteps > 1:
        _, hist = ctx.xka_step(st, C0, f, dt, nsteps - 1, save_every=1)
        for i, n in enumerate(names):
            out[n][:, 1:] = hist[:, :, i].T
    return out
