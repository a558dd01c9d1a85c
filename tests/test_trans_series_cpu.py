"""The transition series' host side without a GPU: the numpy restatement
(tests/trans_series_ref.py) against a packet-by-packet loop, trans_moments and
combine_transitions, and the drivers' multi-ring initial packets."""
import math

import numpy as np
import pytest

from swraytracing_amd.integrate import combine_transitions, trans_moments
from swraytracing_amd.qg import _packets, _ring_factors, _ring_index, _rings_line, _trans_args
from tests.cond_series_ref import assert_populated, quantile_edges
from tests.trans_series_ref import (omega_of, ring_bounds, ring_k, ring_of, ring_radius, trans_accepted,
                                    trans_frame_of)

F, CG, FB = 3.0, 1.0, 20


@pytest.fixture(scope="module")
def packets():
    """500 spread packets with planted NaN and over-range values."""
    rng = np.random.default_rng(7)
    ang = 2 * np.pi * rng.random(500)
    k = ring_radius(4.0, F, CG) * np.stack([np.cos(ang), np.sin(ang)], axis=1) * (1 + 0.3 * rng.standard_normal((500, 1)))
    w = omega_of(k, F, CG)
    src = w * (1 + 0.3 * rng.standard_normal(500))
    k[3, 1] = np.nan
    k[5] = [1e9, 0.0]
    src[7] = np.nan
    src[9] = 1e300
    src[11] = 1000.0      # only d^2 leaves the range
    src[13] = -np.inf
    w = omega_of(k, F, CG)
    return src, w


def _slot(v, edges):
    """hist_slot (swrt_diag.hpp) for one value."""
    nb = len(edges) - 1
    if v != v:
        return -1
    if v < edges[0]:
        return 0
    if v > edges[nb]:
        return nb + 1
    if v == edges[nb]:
        return nb
    lo, hi = 0, nb
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if v >= edges[mid]:
            lo = mid
        else:
            hi = mid
    return 1 + lo


def _round_half_even(v):
    fl = math.floor(v)
    r = v - fl
    if r > 0.5 or (r == 0.5 and fl % 2):
        return fl + 1
    return fl


def _loop_frame(src, w, wedges, sedges, fb):
    ns, nw = len(sedges) - 1, len(wedges) - 1
    counts = [[0] * (nw + 2) for _ in range(ns + 2)]
    sums = [[0, 0, 0] for _ in range(ns + 2)]
    rejected = 0
    scale, lim = 2.0 ** fb, 2.0 ** 38
    for s, v in zip(src.tolist(), w.tolist()):
        d = v - s
        d2 = d * d
        if v != v or s != s or d != d or not abs(v * scale) < lim or not abs(d * scale) < lim \
                or not abs(d2 * scale) < lim:
            rejected += 1
            continue
        sc, wc = _slot(s, sedges), _slot(v, wedges)
        counts[sc][wc] += 1
        for j, q in enumerate((v, d, d2)):
            sums[sc][j] += _round_half_even(q * scale)
    return np.array(counts, dtype=np.int64), np.array(sums, dtype=np.int64), \
        np.array([len(src), rejected, 1], dtype=np.int64)


@pytest.mark.parametrize("ns,nw,fb", [(1, 1, 20), (3, 5, 20), (4, 30, 0), (16, 16, 32), (16, 16, 3)])
def test_restatement_against_a_loop(packets, ns, nw, fb):
    src, w = packets
    wedges, sedges = quantile_edges(w, nw), quantile_edges(src, ns)
    # values on the edges themselves: the first edge, an inner edge, the closed last edge
    src, w = src.copy(), w.copy()
    w[20:23] = [wedges[0], wedges[nw // 2], wedges[-1]]
    src[23:26] = [sedges[0], sedges[ns // 2], sedges[-1]]
    if fb == 3:  # exact halves: rint rounds to even (omega = (2 j + 1) / 16 = odd / 2 quanta)
        w[30:40] = 10.0 + (2 * np.arange(10) + 1) / 16.0
    got = trans_frame_of(src, w, wedges, sedges, fb)
    want = _loop_frame(src, w, wedges, sedges, fb)
    # (five planted packets are out whatever the quantum; source 1000 leaves by d^2 from frac_bits 19 on)
    assert want[2][1] >= 5 + (fb >= 19) and got[0].sum() == 500 - want[2][1]
    if fb == 20:
        assert want[2][1] == 6
        assert_populated(got[0], got[2], planted=True)
    for g, x, name in zip(got, want, ("counts", "sums", "stats")):
        np.testing.assert_array_equal(g, x, err_msg=name)
    assert int(trans_accepted(src, w, fb).sum()) == 500 - want[2][1]
    assert (got[1][:, 1] < 0).any() and (got[1][:, 2] >= 0).all()  # signed d sums, non-negative d^2 sums


def test_moments_against_numpy_means(packets):
    src, w = packets
    wedges, sedges = quantile_edges(w, 12), quantile_edges(src, 6)
    counts, sums, _ = trans_frame_of(src, w, wedges, sedges, FB)
    mom = trans_moments(counts, sums, FB)
    ok = trans_accepted(src, w, FB)
    from tests.cond_series_ref import class_of
    sc = class_of(src[ok], sedges)
    quantum = 2.0 ** -FB
    for c in range(8):
        sel = sc == c
        assert mom["n"][c] == sel.sum() > 0
        d = w[ok][sel] - src[ok][sel]
        # each packet's value is rounded to the quantum: half a quantum a packet at most, so of the mean too
        assert abs(mom["omega_mean"][c] - w[ok][sel].mean()) <= 0.5 * quantum + 1e-12
        assert abs(mom["delta_mean"][c] - d.mean()) <= 0.5 * quantum + 1e-12
        var = (d * d).mean() - d.mean() ** 2
        # <d^2> to half a quantum, <d>^2 to |<d>| quanta
        assert abs(mom["delta_var"][c] - var) <= (0.5 + abs(d.mean()) + 1.0) * quantum + 1e-9 * abs(var)
        np.testing.assert_array_equal(mom["spectrum"][c], counts[c] / sel.sum())
        assert abs(mom["spectrum"][c].sum() - 1.0) < 1e-12
    # an empty class: n = 0, the rest NaN; stacked frames keep their leading axes
    counts2, sums2 = np.stack([counts, counts]), np.stack([sums, sums])
    counts2[1, 3] = 0
    sums2[1, 3] = 0
    mom2 = trans_moments(counts2, sums2, FB)
    assert mom2["n"].shape == (2, 8) and mom2["spectrum"].shape == (2, 8, 14)
    assert mom2["n"][1, 3] == 0 and np.isnan(mom2["delta_var"][1, 3]) and np.isnan(mom2["spectrum"][1, 3]).all()
    np.testing.assert_array_equal(mom2["omega_mean"][0], mom["omega_mean"])
    with pytest.raises(ValueError):
        trans_moments(counts, sums[:, :2], FB)
    with pytest.raises(ValueError):
        trans_moments(counts, sums, 33)


def test_combine_is_additive_and_refuses_mixed_serials(packets):
    src, w = packets
    wedges, sedges = quantile_edges(w, 12), quantile_edges(src, 6)
    whole = [a[None] for a in trans_frame_of(src, w, wedges, sedges, FB, serial=3)]
    cuts = [0, 137, 137, 400, 500]  # (one empty shard)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi > lo:
            parts.append([a[None] for a in trans_frame_of(src[lo:hi], w[lo:hi], wedges, sedges, FB, serial=3)])
        else:  # a shard without packets stands as zeros
            parts.append([np.zeros_like(a) for a in whole])
    got = combine_transitions(parts)
    for g, x, name in zip(got, whole, ("counts", "sums", "stats")):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, x, err_msg=name)
    parts[2][2] = parts[2][2].copy()
    parts[2][2][0, 2] = 4
    with pytest.raises(ValueError, match="serial"):
        combine_transitions(parts)
    with pytest.raises(ValueError):
        combine_transitions([])
    with pytest.raises(ValueError):
        combine_transitions([whole, [whole[0], whole[1][:, :, :2], whole[2]]])


def test_a_scalar_factor_is_todays_packets():
    """A scalar near_inertial_factor: the arrays of qgsw_raytrace.m:54-60 as
    the drivers computed them before rings, bit for bit, from the same draws."""
    N, L = 37, 2 * math.pi
    x, k = _packets(N, L, 4.0, F, CG, np.random.default_rng(5))
    rng = np.random.default_rng(5)
    wf = math.sqrt((4.0 ** 2 - 1) * F ** 2 / CG ** 2)
    i = np.arange(1, N + 1, dtype=np.float64)
    k_old = np.stack([wf * np.cos(2 * np.pi * i / N), wf * np.sin(2 * np.pi * i / N)], axis=1)
    x_old = L * rng.random((N, 2)) - L / 2
    assert x.tobytes() == x_old.tobytes() and k.tobytes() == k_old.tobytes()
    assert _ring_factors(4.0) == ([4.0], False) and _ring_factors(4)[0][0] == 4
    # one ring as a sequence: the same formula, hence the same bits
    x1, k1 = _packets(N, L, [4.0], F, CG, np.random.default_rng(5))
    assert x1.tobytes() == x_old.tobytes() and k1.tobytes() == k_old.tobytes()


def test_four_rings_of_ten_packets():
    N, L, factors = 10, 2 * math.pi, [2, 4, 8, 16]
    x, k = _packets(N, L, factors, F, CG, np.random.default_rng(5))
    assert x.tobytes() == (L * np.random.default_rng(5).random((N, 2)) - L / 2).tobytes()  # the same draws
    assert ring_bounds(N, 4) == [(0, 2), (2, 5), (5, 7), (7, 10)]
    assert ring_of(N, 4).tolist() == [0, 0, 1, 1, 1, 2, 2, 3, 3, 3] == _ring_index(N, 4).tolist()
    np.testing.assert_array_equal(k, ring_k(N, factors, F, CG))
    radius = np.hypot(k[:, 0], k[:, 1])
    for fac, (lo, hi) in zip(factors, ring_bounds(N, 4)):
        wf = math.sqrt((fac ** 2 - 1) * F ** 2 / CG ** 2)
        np.testing.assert_allclose(radius[lo:hi], wf, rtol=1e-15)
        np.testing.assert_allclose(omega_of(k[lo:hi], F, CG), fac * F, rtol=1e-14)
        # angles 2 pi j / N_r, j = 1..N_r: the last packet of a ring sits at angle 2 pi
        np.testing.assert_allclose(k[hi - 1], [wf, 0.0], atol=1e-12 * wf)
        ang = np.unwrap(np.arctan2(k[lo:hi, 1], k[lo:hi, 0]))
        if hi - lo > 1:
            np.testing.assert_allclose(np.diff(ang), 2 * np.pi / (hi - lo), rtol=1e-12)
    line = _rings_line([float(v) for v in factors], F, CG)
    assert line.startswith("Rings: ") and line.count("omega0") == 4 and "omega0 = 48" in line
    for bad in ([], [2.0, 1.0], [2.0, np.nan]):
        with pytest.raises(ValueError):
            _ring_factors(bad)


def test_driver_arguments():
    spec = np.linspace(9.0, 15.0, 13)
    assert _trans_args(None, None, None, 20, spec, 1) is None
    by, edges, lag, fb = _trans_args([11.0, 12.0, 13.0], None, 3, 16, spec, 1)
    assert (by, edges.tolist(), lag, fb) == (0, [11.0, 12.0, 13.0], 3, 16)
    by, edges, lag, fb = _trans_args(None, "ring", None, 20, spec, 4)
    assert (by, edges.tolist(), lag, fb) == (1, [-0.5, 0.5, 1.5, 2.5, 3.5], None, 20)
    for args in ((None, None, 2, 20, spec, 1),               # a lag without a series
                 (None, "ring", 2, 20, spec, 2),             # a ring index is never re-marked
                 ([11.0, 12.0], "ring", None, 20, spec, 2),  # the ring sets its own edges
                 ([11.0, 12.0], None, None, 20, None, 1),    # no omega classes
                 ([12.0, 11.0], None, None, 20, spec, 1),
                 ([11.0, 12.0], None, 0, 20, spec, 1),
                 ([11.0, 12.0], None, 1.5, 20, spec, 1),
                 ([11.0, 12.0], None, None, 33, spec, 1),
                 ([11.0, 12.0], "k", None, 20, spec, 1),
                 (np.arange(5000.0), None, None, 20, spec, 1)):
        with pytest.raises(ValueError):
            _trans_args(*args)
