"""The refraction series off the device: the numpy restatement
(tests/refr_series_ref.py) against a packet-by-packet Python loop, a known
answer in a pure strain, the marginals, the rejections, and the package's
host-side pieces (combine_refrs, alignment_edges, refr_rates, the drivers'
argument check)."""
import bisect
import math
import warnings

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import swrt_oracle as orc
from swraytracing_amd.qg import _refr_args
from tests.cond_series_ref import assert_populated, central_edges, class_of, omega_of
from tests.refr_series_ref import a_edges_of, gradients, packet_values, refr_frame, refr_frame_of

SHAPES = [(1, 1), (4, 7), (15, 300)]  # (na, nw)
N = 300


@pytest.fixture(scope="module")
def case(qg_case):
    """300 packets over the domain with spread wavevectors; four cannot be
    counted: a NaN k, an infinite k, k = 0 and k = 1e9 (beyond 2^38 quanta at
    20 bits)."""
    q = qg_case
    rng = np.random.default_rng(78)
    x = rng.uniform(-q["L"] / 2, q["L"] / 2, (N, 2))
    th = rng.uniform(0, 2 * np.pi, N)
    k = (np.sqrt(135.0) * (1.0 + 0.3 * rng.standard_normal(N)))[:, None] * np.stack([np.cos(th), np.sin(th)], axis=1)
    k[17, 0] = np.nan
    k[101, 1] = np.inf
    k[200] = [0.0, 0.0]
    k[250] = [1e9, 0.0]
    dx = q["L"] / q["nx"]
    grads = gradients([q["flow"]], 1, 0.0, x, dx, orc.BUMP_QG)
    vals = packet_values(grads, k, q["f"], q["Cg"])
    return dict(q=q, x=x, k=k, dx=dx, grads=grads, vals=vals)


def _slot(v, edges):
    nb = len(edges) - 1
    if v < edges[0]:
        return 0
    if v > edges[nb]:
        return nb + 1
    if v == edges[nb]:
        return nb
    return bisect.bisect_right(edges, v)


def _div(a, b):
    """IEEE division of Python floats (no ZeroDivisionError)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    return math.sqrt(a) if a >= 0 else math.nan  # (NaN compares false: NaN)


def _loop_frame(grads, k, f, Cg, wedges, aedges, fb):
    """The contract one packet at a time, in Python floats and ints."""
    wedges, aedges = [float(e) for e in wedges], [float(e) for e in aedges]
    nw, na = len(wedges) - 1, len(aedges) - 1
    nws = nw + 2
    counts = [[0] * nws for _ in range(na + 2)]
    sums = [0] * (3 * nws + na + 2)
    rejected = 0
    S, lim = 2.0 ** fb, 2.0 ** 38
    for p in range(len(k)):
        ux, uy, vx, vy = (float(g[p]) for g in grads)
        k1, k2 = float(k[p, 0]), float(k[p, 1])
        kk = k1 * k1 + k2 * k2
        w = _sqrt(f * f + (Cg * Cg) * kk)
        kd = -(ux * k1 + vx * k2)
        ld = -(uy * k1 + vy * k2)
        g = k1 * kd + k2 * ld
        wd = _div((Cg * Cg) * g, w)
        gam = _div(g, kk)
        s1, s2 = ux - vy, vx + uy
        sig = _sqrt(s1 * s1 + s2 * s2)
        c = _div(gam + gam, sig)
        sd2 = (wd * wd) * S
        if not abs(w * S) < lim or c != c or not abs(wd * S) < lim or not sd2 < lim or not abs(gam * S) < lim:
            rejected += 1
            continue
        wc, ac = _slot(w, wedges), _slot(c, aedges)
        counts[ac][wc] += 1
        qd = round(wd * S)  # (round half even, as rint)
        sums[wc] += qd
        sums[nws + wc] += round(sd2)
        sums[2 * nws + wc] += round(gam * S)
        sums[3 * nws + ac] += qd
    return np.array(counts, dtype=np.int64), np.array(sums, dtype=np.int64), np.array([len(k), rejected])


def _wedges(c, nw):
    w = c["vals"][0]
    return central_edges(w[w < 1e6], nw)


@pytest.mark.parametrize("na,nw", SHAPES)
def test_restatement_against_a_packet_loop(case, na, nw):
    c, q = case, case["q"]
    wedges, aedges = _wedges(c, nw), a_edges_of(na)
    for fb in (0, 20, 32):
        got = refr_frame([q["flow"]], 1, 0.0, c["x"], c["k"], c["dx"], orc.BUMP_QG, q["f"], q["Cg"], wedges, aedges, fb)
        want = _loop_frame(c["grads"], c["k"], q["f"], q["Cg"], wedges, aedges, fb)
        for g, w_, name in zip(got, want, ("counts", "sums", "stats")):
            np.testing.assert_array_equal(g, w_, err_msg=f"{name} frac_bits {fb}")
        counts, sums, stats = got
        print(f"({na}, {nw}) frac_bits {fb}: a row {counts.sum(axis=1).tolist()} stats {stats.tolist()}")
        assert stats[0] == N and counts.sum() == stats[0] - stats[1]
        # k = 1e9 has omega = 1e9 < 2^38 at frac_bits 0, but gamma is O(1) and omega-dot^2 O(1e18 * s^2) there
        assert stats[1] >= 3
        assert_populated(counts, stats, planted=True)
        # the alignment-class flux sums to the omega-class flux
        nws = nw + 2
        assert sums[:nws].sum() == sums[3 * nws:].sum()


def test_pure_strain_known_answer():
    """u_x = s, v_y = -s, the rest 0, k on a ring: gamma = -s cos 2 theta,
    c = -cos 2 theta, omega-dot = Cg^2 |k|^2 gamma / omega."""
    nx, L, s, f, Cg, K = 16, 2 * np.pi, 0.37, 3.0, 1.3, 5.0
    z = np.zeros((nx, nx))
    flow = dict(u=z, v=z, ux=z + s, uy=z, vx=z, vy=z - s)
    rng = np.random.default_rng(3)
    n = 257
    x = rng.uniform(-L / 2, L / 2, (n, 2))
    th = np.linspace(0.0, 2 * np.pi, n, endpoint=False) + 0.01
    k = K * np.stack([np.cos(th), np.sin(th)], axis=1)
    grads = gradients([flow], 1, 0.0, x, L / nx, orc.BUMP_QG)
    # the interpolant of a constant is the constant up to the weights' rounding
    np.testing.assert_allclose(grads[0], s, rtol=1e-13)
    np.testing.assert_allclose(grads[3], -s, rtol=1e-13)
    assert np.abs(grads[1]).max() == 0 and np.abs(grads[2]).max() == 0
    w, wd, gam, c = packet_values(grads, k, f, Cg)
    c2 = np.cos(2 * th)
    scale = lambda v: np.abs(v).max()  # noqa: E731
    assert np.abs(gam + s * c2).max() <= 1e-12 * s
    assert np.abs(c + c2).max() <= 1e-12
    want_wd = Cg * Cg * K * K * (-s * c2) / np.sqrt(f * f + Cg * Cg * K * K)
    assert np.abs(wd - want_wd).max() <= 1e-12 * scale(want_wd)
    # the arcsine shape: the outer classes of eight hold the most
    counts, sums, stats = refr_frame_of(w, wd, gam, c, [1.0, 100.0], sw.alignment_edges(8), 20)
    row = counts.sum(axis=1)
    assert stats.tolist() == [n, 0] and row[0] + row[-1] <= 2  # (rounding may put c = +-1 a hair outside)
    assert row[1] > row[4] and row[8] > row[5]
    # a symmetric ring: the net flux and the net growth rate vanish to rounding
    assert abs(int(sums[1])) <= n and abs(int(sums[2 * 3 + 1])) <= n


def test_marginals(case):
    c, q = case, case["q"]
    w, wd, gam, cc = c["vals"]
    wedges, aedges = _wedges(c, 300), a_edges_of(15)
    counts, sums, stats = refr_frame_of(w, wd, gam, cc, wedges, aedges, 20)
    ok = (class_of(cc, aedges) >= 0) & (np.abs(w * 2.0 ** 20) < 2.0 ** 38) & (np.abs(wd * 2.0 ** 20) < 2.0 ** 38)
    assert stats[1] == N - ok.sum() == 4
    # the omega-series row [below, histcounts, above] of the accepted packets
    wa = w[ok]
    row = np.concatenate([[np.sum(wa < wedges[0])], np.histogram(wa, wedges)[0], [np.sum(wa > wedges[-1])]])
    np.testing.assert_array_equal(counts.sum(axis=0), row)
    np.testing.assert_array_equal(counts.sum(axis=0), np.bincount(class_of(omega_of(c["k"], q["f"], q["Cg"])[ok], wedges),
                                                                  minlength=302))
    ca = cc[ok]
    arow = np.concatenate([[np.sum(ca < aedges[0])], np.histogram(ca, aedges)[0], [np.sum(ca > aedges[-1])]])
    np.testing.assert_array_equal(counts.sum(axis=1), arow)
    assert_populated(counts, stats, planted=True)


def test_rejections_are_counted_once():
    """NaN k, k = 0, a flow at rest (sigma = 0 and gamma = 0) and a huge k
    each add to rejected alone."""
    nx, L = 16, 2 * np.pi
    z = np.zeros((nx, nx))
    strain = dict(u=z, v=z, ux=z + 0.5, uy=z, vx=z, vy=z - 0.5)
    rest = dict(u=z, v=z, ux=z, uy=z, vx=z, vy=z)
    x = np.zeros((1, 2)) + 0.3
    wedges, aedges = np.array([1.0, 10.0, 100.0]), a_edges_of(4)

    def frame(flow, k, fb=20):
        return refr_frame([flow], 1, 0.0, x, np.array([k], dtype=np.float64), L / nx, orc.BUMP_QG, 3.0, 1.0, wedges,
                          aedges, fb)

    good = frame(strain, [3.0, 4.0])
    assert good[2].tolist() == [1, 0] and good[0].sum() == 1 and np.count_nonzero(good[1]) == 4
    for flow, k, why in ((strain, [np.nan, 1.0], "NaN k"), (strain, [0.0, 0.0], "k = 0"),
                         (rest, [3.0, 4.0], "sigma = 0 with gamma = 0"), (strain, [1e9, 0.0], "omega * S >= 2^38"),
                         (strain, [2e5, 0.0], "omega-dot^2 * S >= 2^38 alone")):
        counts, sums, stats = frame(flow, k)
        assert stats.tolist() == [1, 1], why
        assert counts.sum() == 0 and not sums.any(), why
    # (the last one: omega * S = 2e5 * 2^20 < 2^38, omega-dot = -0.5 * 2e5, its square * 2^20 > 2^38)
    assert 2.1e5 * 2.0 ** 20 < 2.0 ** 38 < (0.5 * 2e5) ** 2 * 2.0 ** 20


def test_combine_refrs(case):
    c = case
    wedges, aedges = _wedges(c, 7), a_edges_of(4)
    whole = refr_frame_of(*c["vals"], wedges, aedges, 20)
    part_of = np.random.default_rng(5).integers(0, 3, N)
    parts = []
    for r in range(3):
        fr = refr_frame_of(*(v[part_of == r] for v in c["vals"]), wedges, aedges, 20)
        parts.append(tuple(a[None] for a in fr))  # one frame each
    got = sw.combine_refrs(parts)
    for g, want in zip(got, whole):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g[0], want)
    assert sw.combine_refrs(parts[:1])[0].shape == (1, 6, 9) and sw.combine_refrs(parts[:1])[1].shape == (1, 33)
    other = tuple(a[None] for a in refr_frame_of(*c["vals"], _wedges(c, 8), aedges, 20))
    with pytest.raises(ValueError):
        sw.combine_refrs([parts[0], other])
    with pytest.raises(ValueError):
        sw.combine_refrs([(parts[1][0], parts[1][1][:, :3], parts[1][2])])
    with pytest.raises(ValueError):
        sw.combine_refrs([])


def test_alignment_edges():
    np.testing.assert_array_equal(sw.alignment_edges(4), [-1.0, -0.5, 0.0, 0.5, 1.0])
    assert sw.alignment_edges(1).tolist() == [-1.0, 1.0]
    for bad in (0, 4097, 2.5, True):
        with pytest.raises(ValueError):
            sw.alignment_edges(bad)


def test_refr_rates_on_a_hand_made_frame():
    # na = 1, nw = 2: alignment classes [below, bin, above], omega classes [below, b0, b1, above]
    counts = np.array([[0, 1, 0, 0], [0, 2, 4, 0], [0, 1, 0, 0]], dtype=np.int64)
    fb = 4
    sums = np.array([0, 4 * 3 * 16, -4 * 16, 0,          # omega-dot: mean 3 in b0 (4 packets), -1 in b1
                     0, 4 * 10 * 16, 4 * 2 * 16 + 8, 0,  # omega-dot^2: mean 10, 2.125
                     0, -4 * 16 // 2, 4 * 16, 0,         # gamma: mean -0.5, 1
                     32, 64, 32], dtype=np.int64)        # omega-dot per alignment class: 2, 4, 2 (in units)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = sw.refr_rates(counts[None], sums[None], fb)
    assert out["n"][0].tolist() == [0, 4, 4, 0]
    assert out["omega_dot_mean"][0, 1:3].tolist() == [3.0, -1.0]
    assert out["omega_dot_sq_mean"][0, 1:3].tolist() == [10.0, 2.125]
    assert out["gamma_mean"][0, 1:3].tolist() == [-0.5, 1.0]
    for name in ("omega_dot_mean", "omega_dot_sq_mean", "gamma_mean"):
        assert np.isnan(out[name][0, [0, 3]]).all()
    assert out["alignment"].shape == (1, 4, 3)
    np.testing.assert_array_equal(out["alignment"][0, 1], [0.25, 0.5, 0.25])
    np.testing.assert_array_equal(out["alignment"][0, 2], [0.0, 1.0, 0.0])
    assert np.isnan(out["alignment"][0, [0, 3]]).all()
    assert out["n_align"][0].tolist() == [1, 6, 1]
    np.testing.assert_array_equal(out["omega_dot_mean_align"][0], [2.0, 4.0 / 6.0, 2.0])
    np.testing.assert_array_equal(out["flux_share"][0], [0.25, 0.5, 0.25])
    # an empty frame: NaN everywhere, no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        empty = sw.refr_rates(np.zeros((3, 4), dtype=np.int64), np.zeros(15, dtype=np.int64), fb)
    assert np.isnan(empty["flux_share"]).all() and np.isnan(empty["omega_dot_mean_align"]).all()
    with pytest.raises(ValueError):
        sw.refr_rates(counts, sums[:14], fb)
    with pytest.raises(ValueError):
        sw.refr_rates(counts, sums, 33)


def test_driver_arguments():
    spec = np.linspace(3.0, 20.0, 11)
    assert _refr_args(None, 20, None) is None and _refr_args(None, 20, spec) is None
    edges, fb = _refr_args([-1.0, 0.0, 1.0], 12, spec)
    assert edges.tolist() == [-1.0, 0.0, 1.0] and fb == 12
    with pytest.raises(ValueError, match="spectrum_edges"):
        _refr_args([-1.0, 1.0], 20, None)
    for bad in ([1.0, 0.0], [0.0, 0.0, 1.0], [0.0], [0.0, np.nan], [0.0, np.inf]):
        with pytest.raises(ValueError, match="refr_edges"):
            _refr_args(bad, 20, spec)
    for bad in (-1, 33, 1.5, True):
        with pytest.raises(ValueError, match="refr_frac_bits"):
            _refr_args([-1.0, 1.0], bad, spec)
    with pytest.raises(ValueError, match="65536"):
        _refr_args(np.arange(4001.0), 20, np.arange(301.0))
    # the drivers refuse before anything runs (no device is touched)
    with pytest.raises(ValueError, match="spectrum_edges"):
        sw.qgsw_raytrace(64, 10, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, refr_edges=[-1.0, 1.0])
    with pytest.raises(ValueError, match="refr_edges"):
        sw.qg2layersw_raytrace(64, 10, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0, refr_edges=[1.0, -1.0], spectrum_edges=spec)
