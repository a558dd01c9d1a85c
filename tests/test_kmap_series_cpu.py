"""The wave-vector plane series' contract on the host: the numpy restatement
(tests/kmap_series_ref.py) against a packet-by-packet loop and on its own edge
cases, and combine_kmaps, kmap_moments and the drivers' argument check."""
import math

import numpy as np
import pytest

from swraytracing_amd.integrate import combine_kmaps, kmap_moments
from swraytracing_amd.qg import _kmap_args, _spectrum_args
from tests.kmap_series_ref import kmap_frame

KS = (0.1, 3.3, 5.0, 1000.0)
MS = (1, 2, 7, 128, 129, 300, 4096)


def _rint(v):
    """Round half to even of a finite double, as a Python int."""
    return int(round(v))  # (Python's round(float) is half-even and exact)


def _loop_frame(k, K, m, frac_bits):
    s = float(m) / (2.0 * K)
    scale = 2.0 ** frac_bits
    plane = [[0] * m for _ in range(m)]
    st = [len(k), 0, 0, 0, 0, 0, 0, 0]
    for a, b in k:
        a, b = float(a), float(b)
        vals = (a, b, a * a, b * b, a * b) if math.isfinite(a) and math.isfinite(b) else None
        if vals is None or any(not abs(v * scale) < 2.0 ** 38 for v in vals):
            st[1] += 1
            continue
        for q, v in enumerate(vals):
            st[3 + q] += _rint(v * scale)
        if not (-K <= a < K and -K <= b < K):
            st[2] += 1
            continue
        i = min(math.floor((a + K) * s), m - 1)
        j = min(math.floor((b + K) * s), m - 1)
        plane[i][j] += 1
    return np.array(plane, dtype=np.int64), np.array(st, dtype=np.int64)


def test_ref_equals_a_packet_loop():
    rng = np.random.default_rng(11)
    k = 4.0 * rng.standard_normal((300, 2))
    k[::17] *= 3.0  # (some outside K = 5)
    k[5] = [np.nan, 1.0]
    k[6] = [1.0, -np.inf]
    k[7] = [1e9, 0.0]
    for K, m, fb in ((5.0, 7, 16), (3.3, 128, 20), (5.0, 300, 0), (0.1, 2, 32)):
        plane, stats = kmap_frame(k, K, m, fb)
        lp, ls = _loop_frame(k, K, m, fb)
        np.testing.assert_array_equal(plane, lp)
        np.testing.assert_array_equal(stats, ls)
        assert plane.sum() == stats[0] - stats[1] - stats[2]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("m", MS)
def test_edges(K, m):
    def cell(v):
        plane, stats = kmap_frame([[v, 0.0]], K, m)
        assert stats[1] == 0
        if stats[2]:
            assert plane.sum() == 0
            return None
        (i,), (j,) = np.nonzero(plane)
        assert j == min(math.floor((0.0 + K) * (m / (2.0 * K))), m - 1)
        return int(i)

    assert cell(-K) == 0
    assert cell(K) is None
    assert cell(np.nextafter(K, -np.inf)) == m - 1
    assert cell(np.nextafter(-K, -np.inf)) is None
    assert cell(-0.0) == cell(0.0) is not None
    # the same on the second component
    plane, stats = kmap_frame([[0.0, np.nextafter(K, -np.inf)], [0.0, K], [0.0, -K]], K, m)
    assert stats[2] == 1 and plane[:, m - 1].sum() >= 1 and plane[:, 0].sum() >= 1 and plane.sum() == 2


def test_rejection():
    K, m, fb = 5.0, 16, 16
    for bad in (np.nan, np.inf, -np.inf, 1e9):
        for kk in ([bad, 1.0], [1.0, bad]):
            plane, stats = kmap_frame([kk, [1.0, 2.0]], K, m, fb)
            np.testing.assert_array_equal(stats[:3], [2, 1, 0])
            assert plane.sum() == 1
            np.testing.assert_array_equal(stats[3:], [v * 2 ** fb for v in (1, 2, 1, 4, 2)])
    # 600 * 2^16 < 2^38, 600^2 * 2^16 < 2^38: outside, and in the moments
    plane, stats = kmap_frame([[600.0, 600.0]], K, m, fb)
    np.testing.assert_array_equal(stats[:3], [1, 0, 1])
    assert plane.sum() == 0
    np.testing.assert_array_equal(stats[3:], [600 << fb, 600 << fb, 360000 << fb, 360000 << fb, 360000 << fb])
    # a product over the limit rejects although k and l are under it
    _, stats = kmap_frame([[3000.0, 1.0]], K, m, fb)  # 9e6 * 2^16 > 2^38
    np.testing.assert_array_equal(stats[:3], [1, 1, 0])
    # round half to even: 2.5 -> 2, 3.5 -> 4 at frac_bits 0
    _, stats = kmap_frame([[2.5, 3.5]], K, m, 0)
    np.testing.assert_array_equal(stats[3:5], [2, 4])


def test_additive_over_a_split():
    rng = np.random.default_rng(12)
    k = 3.0 * rng.standard_normal((4097, 2))
    k[100] = [np.nan, 0.0]
    whole = kmap_frame(k, 5.0, 33, 16)
    a, b = kmap_frame(k[:2000], 5.0, 33, 16), kmap_frame(k[2000:], 5.0, 33, 16)
    np.testing.assert_array_equal(whole[0], a[0] + b[0])
    np.testing.assert_array_equal(whole[1], a[1] + b[1])
    planes, stats = combine_kmaps([(a[0][None], a[1][None]), (b[0][None], b[1][None])])
    np.testing.assert_array_equal(planes[0], whole[0])
    np.testing.assert_array_equal(stats[0], whole[1])


def test_combine_kmaps_checks():
    with pytest.raises(ValueError):
        combine_kmaps([])
    p, s = np.zeros((2, 4, 4), dtype=np.int64), np.zeros((2, 8), dtype=np.int64)
    with pytest.raises(ValueError):
        combine_kmaps([(p, s[:1])])
    with pytest.raises(ValueError):
        combine_kmaps([(p[0], s)])
    with pytest.raises(ValueError):
        combine_kmaps([(p, s[:, :2])])
    # a shard without packets stands as zeros; sums stay int64 beyond 2^53
    big = p.copy()
    big[0, 1, 2] = (1 << 60) + 1
    planes, stats = combine_kmaps([(big, s), (p, s)])
    assert planes.dtype == np.int64 and planes[0, 1, 2] == (1 << 60) + 1 and stats.shape == (2, 8)


def test_kmap_moments():
    rng = np.random.default_rng(13)
    fb = 20
    k = rng.standard_normal((500, 2)) * [1.0, 2.0] + [0.5, -1.0]
    k[3] = [np.nan, 0.0]
    _, stats = kmap_frame(k, 5.0, 8, fb)
    good = np.delete(k, 3, axis=0)
    unit = 2.0 ** -fb
    dq = [np.rint(v * 2.0 ** fb) * unit for v in (good[:, 0], good[:, 1], good[:, 0] ** 2, good[:, 1] ** 2,
                                                   good[:, 0] * good[:, 1])]
    mean = np.array([dq[0].mean(), dq[1].mean()])
    cov = np.array([[dq[2].mean() - mean[0] ** 2, dq[4].mean() - mean[0] * mean[1]],
                    [dq[4].mean() - mean[0] * mean[1], dq[3].mean() - mean[1] ** 2]])
    out = kmap_moments(np.stack([stats, np.zeros(8, dtype=np.int64)]), fb)
    assert out["n_used"].tolist() == [499.0, 0.0]
    # (sums of 499 values of magnitude <= 2^5: a few ulp of the mean's scale)
    np.testing.assert_allclose(out["mean"][0], mean, rtol=0, atol=1e-13)
    np.testing.assert_allclose(out["cov"][0], cov, rtol=0, atol=1e-12)
    assert np.isnan(out["mean"][1]).all() and np.isnan(out["cov"][1]).all()
    # and close to the unquantised moments: each value is off by at most 2^-21
    np.testing.assert_allclose(out["mean"][0], good.mean(axis=0), atol=2.0 ** -20)
    np.testing.assert_allclose(out["cov"][0], np.cov(good.T, bias=True), atol=1e-4)
    with pytest.raises(ValueError):
        kmap_moments(np.zeros((2, 7)), fb)
    with pytest.raises(ValueError):
        kmap_moments(stats, 33)


def test_kmap_args():
    assert _kmap_args(None, None, 16) is None
    assert _kmap_args(16, None, 16, ring_radius=2.0) == (8.0, 16, 16)
    assert _kmap_args(np.int64(4096), 3.5, 0) == (3.5, 4096, 0)
    assert _kmap_args(1, 1, 32.0) == (1.0, 1, 32)
    for cells in (True, False, 0, 4097, -1, 2.5, "8", [8]):
        with pytest.raises((ValueError, TypeError)):
            _kmap_args(cells, 5.0, 16)
    for fb in (True, -1, 33, 1.5):
        with pytest.raises(ValueError):
            _kmap_args(8, 5.0, fb)
    for K in (0.0, -1.0, np.inf, np.nan, True):
        with pytest.raises(ValueError):
            _kmap_args(8, K, 16)
    with pytest.raises(ValueError):
        _kmap_args(8, None, 16, ring_radius=0.0)
    # packet_files=False is allowed with kmap_cells alone
    assert _spectrum_args(None, False, 8) is None
    with pytest.raises(ValueError):
        _spectrum_args(None, False)
