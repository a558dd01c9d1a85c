"""The host side of the spectrum series (CPU only): energy_spectrum and
combine_spectra against a numpy restatement of analysis/load_data.m:33-49,63
on a synthetic 40-frame k series.

load_data.m: omega = sqrt(f^2 + Cg^2*dot(k, k, 2)) (:33), edges = linspace(0,
max(omega), bins) (:39), center (:40), w = the omega of a window of frames
(:45), distribution = histcounts(w, edges) (:47), energy = center .*
distribution (:49), mean(omega) per frame (:63).  A series frame is what the
device records: counts [below, bins, above] and [n, sum, min, max]; here the
frames are built with numpy, by the rule the header gives."""
import math

import numpy as np
import pytest

import swraytracing_amd as sw
from swraytracing_amd.integrate import empty_spectrum

F, CG, N, T, BINS = 3.0, 1.0, 500, 40, 30


def _omega_series():
    """(T, N) omega of a synthetic run: a ring |k| = 3 that spreads with time."""
    rng = np.random.default_rng(7)
    th = rng.uniform(0, 2 * np.pi, N)
    k0 = 3.0 * np.stack([np.cos(th), np.sin(th)], axis=1)
    k = k0[None] * (1.0 + 0.02 * np.arange(T)[:, None, None] * rng.standard_normal((1, N, 2)))
    return np.sqrt(F ** 2 + CG ** 2 * np.sum(k * k, axis=2))  # load_data.m:33


def _frames(omega, edges):
    """The series the device records for these omega rows (include/swrt.h)."""
    nb = edges.size - 1
    counts = np.zeros((omega.shape[0], nb + 2), dtype=np.int64)
    stats = np.zeros((omega.shape[0], 4))
    for i, w in enumerate(omega):
        b = np.searchsorted(edges, w, "right") - 1
        b[w == edges[-1]] = nb - 1
        slot = np.where(w < edges[0], 0, np.where(w > edges[-1], nb + 1, b + 1))
        counts[i] = np.bincount(slot, minlength=nb + 2)
        stats[i] = [w.size, w.sum(), w.min(), w.max()] if w.size else [0, 0.0, np.inf, -np.inf]
    return counts, stats


@pytest.fixture(scope="module")
def series():
    omega = _omega_series()
    edges = np.linspace(0, omega.max(), BINS)  # load_data.m:39: the last edge is the largest omega
    return omega, edges, _frames(omega, edges)


@pytest.mark.parametrize("lo,hi", [(0, 11), (5, 26), (29, 40), (0, 40)])
def test_energy_spectrum_is_load_data_window(series, lo, hi):
    omega, edges, (counts, stats) = series
    w = np.sort(omega[lo:hi].ravel())                   # load_data.m:45-46
    distribution = np.histogram(w, edges)[0]            # :47 (histcounts: last bin closed)
    center = (edges[1:] + edges[:-1]) / 2               # :40
    c, e = sw.energy_spectrum(counts, edges, lo, hi)
    np.testing.assert_array_equal(c, center)
    np.testing.assert_array_equal(e, center * distribution)  # :49
    assert distribution.sum() == (hi - lo) * N          # every omega is inside load_data's edges
    assert counts[:, 0].sum() == 0 and counts[:, -1].sum() == 0
    # the largest omega of the run is the last edge itself: the closed last bin holds it
    assert counts[:, -2].sum() >= 1


def test_mean_omega_per_frame(series):
    omega, edges, (counts, stats) = series
    mean = stats[:, 1] / stats[:, 0]                    # load_data.m:63
    np.testing.assert_allclose(mean, omega.mean(axis=1), rtol=4 * N * 2.0 ** -53, atol=0)
    assert stats[:, 3].max() == edges[-1]               # what load_data.m:39 builds its edges from


def test_energy_spectrum_defaults_and_errors(series):
    omega, edges, (counts, stats) = series
    c, e = sw.energy_spectrum(counts, edges)
    np.testing.assert_array_equal(e, c * counts[:, 1:-1].sum(axis=0))
    with pytest.raises(ValueError):
        sw.energy_spectrum(counts[:, 1:], edges)


def test_combining_two_halves_equals_the_whole(series):
    omega, edges, (counts, stats) = series
    # narrower edges: below and above are exercised too
    edges = np.linspace(np.quantile(omega, 0.1), np.quantile(omega, 0.9), 17)
    whole_c, whole_s = _frames(omega, edges)
    assert whole_c[:, 0].sum() > 0 and whole_c[:, -1].sum() > 0
    cut = 201
    parts = [_frames(omega[:, :cut], edges), _frames(omega[:, cut:], edges), empty_spectrum(T, edges.size - 1)]
    got_c, got_s = sw.combine_spectra(parts)
    assert got_c.dtype == np.int64
    np.testing.assert_array_equal(got_c, whole_c)
    np.testing.assert_array_equal(got_s[:, [0, 2, 3]], whole_s[:, [0, 2, 3]])
    # two summation orders of N positive terms differ by at most 2*N*2^-53*sum
    for t in range(T):
        want = math.fsum(omega[t])
        assert abs(got_s[t, 1] - whole_s[t, 1]) <= 2 * N * 2.0 ** -53 * want
        assert abs(got_s[t, 1] - want) <= 2 * N * 2.0 ** -53 * want


def test_combine_spectra_shapes():
    e = empty_spectrum(3, 4)
    assert e[0].shape == (3, 6) and e[1].shape == (3, 4)
    c, s = sw.combine_spectra([e, e])
    assert not c.any() and (s[:, 0] == 0).all() and (s[:, 2] == np.inf).all() and (s[:, 3] == -np.inf).all()
    with pytest.raises(ValueError):
        sw.combine_spectra([])
    with pytest.raises(ValueError):
        sw.combine_spectra([e, empty_spectrum(2, 4)])
