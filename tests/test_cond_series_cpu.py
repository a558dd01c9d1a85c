"""The conditional spectrum series off the device: the numpy restatement
(tests/cond_series_ref.py) against a packet-by-packet Python loop, the class
rule on the edges, the marginals, and the package's host-side pieces
(combine_conds, cond_spectra, the drivers' argument check)."""
import bisect
import math
import warnings

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import swrt_oracle as orc
from swraytracing_amd.qg import _cond_args
from tests.cond_series_ref import (assert_populated, central_edges, class_of, cond_frame, cond_frame_of, flow_scalars,
                                   omega_of, zeta_edges)

SHAPES = [(1, 1), (4, 7), (15, 300)]  # (nq, nw)
NAMES = ("zeta", "sigma", "D")


@pytest.fixture(scope="module")
def case(qg_case):
    """300 packets over the domain with spread wavevectors; three cannot be
    counted: a NaN k, an infinite k, and k = 1e9 (beyond 2^38 quanta at 20 bits)."""
    q = qg_case
    rng = np.random.default_rng(77)
    x = rng.uniform(-q["L"] / 2, q["L"] / 2, (300, 2))
    th = rng.uniform(0, 2 * np.pi, 300)
    k = (np.sqrt(135.0) * (1.0 + 0.3 * rng.standard_normal(300)))[:, None] * np.stack([np.cos(th), np.sin(th)], axis=1)
    k[17, 0] = np.nan
    k[101, 1] = np.inf
    k[250] = [1e9, 0.0]
    dx = q["L"] / q["nx"]
    scal = dict(zip(NAMES, flow_scalars([q["flow"]], 1, 0.0, x, dx, orc.BUMP_QG)))
    # the loop's gradients, one packet at a time, as Python floats (computed once, read-only)
    grads = [tuple(float(v[0]) for v in orc.interpolate_fields(x[p:p + 1, 0], x[p:p + 1, 1], q["flow"], dx,
                                                               orc.BUMP_QG)[2:]) for p in range(300)]
    return dict(q=q, x=x, k=k, dx=dx, scal=scal, w=omega_of(k, q["f"], q["Cg"]), grads=grads)


def _loop_frame(grads, k, f, Cg, wedges, which, qedges, fb):
    """The contract one packet at a time, in Python floats and ints."""
    wedges, qedges = [float(e) for e in wedges], [float(e) for e in qedges]
    nw, nq = len(wedges) - 1, len(qedges) - 1
    counts = [[0] * (nw + 2) for _ in range(nq + 2)]
    sums = [0] * (nq + 2)
    rejected = 0

    def slot(v, edges):
        nb = len(edges) - 1
        if v < edges[0]:
            return 0
        if v > edges[nb]:
            return nb + 1
        if v == edges[nb]:
            return nb
        return bisect.bisect_right(edges, v)

    for p, (ux, uy, vx, vy) in enumerate(grads):
        if which == 0:
            qv = vx - uy
        elif which == 1:
            s1, s2 = ux - vy, vx + uy
            qv = math.sqrt(s1 * s1 + s2 * s2)
        else:
            qv = vy * vy + vx * uy
        k1, k2 = float(k[p, 0]), float(k[p, 1])
        r2 = f * f + (Cg * Cg) * (k1 * k1 + k2 * k2)
        w = math.sqrt(r2) if r2 == r2 else math.nan
        sw_ = w * 2.0 ** fb
        if math.isnan(w) or math.isnan(qv) or not abs(sw_) < 2.0 ** 38:
            rejected += 1
            continue
        qc = slot(qv, qedges)
        counts[qc][slot(w, wedges)] += 1
        sums[qc] += round(sw_)  # (round half even, as rint)
    return np.array(counts, dtype=np.int64), np.array(sums, dtype=np.int64), np.array([len(grads), rejected])


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("nq,nw", SHAPES)
def test_restatement_against_a_packet_loop(case, nq, nw, which):
    c, q = case, case["q"]
    qv = c["scal"][NAMES[which]]
    qedges = zeta_edges(q["flow"], nq) if which == 0 else central_edges(qv, nq)
    wedges = central_edges(c["w"][c["w"] < 1e6], nw)
    for fb in (0, 20, 32):
        got = cond_frame([q["flow"]], 1, 0.0, c["x"], c["k"], c["dx"], orc.BUMP_QG, q["f"], q["Cg"], wedges, which,
                         qedges, fb)
        want = _loop_frame(c["grads"], c["k"], q["f"], q["Cg"], wedges, which, qedges, fb)
        for g, w_, name in zip(got, want, ("counts", "sums", "stats")):
            np.testing.assert_array_equal(g, w_, err_msg=f"{name} frac_bits {fb}")
        counts, sums, stats = got
        print(f"which {which} ({nq}, {nw}) frac_bits {fb}: q row {counts.sum(axis=1).tolist()} stats {stats.tolist()}")
        assert stats[0] == 300 and counts.sum() == stats[0] - stats[1]
        # k = 1e9 fits 2^38 quanta at frac_bits 0 only; omega < 64 fits them at 32 bits too
        assert stats[1] == {0: 2, 20: 3, 32: 3}[fb]
        assert_populated(counts, stats, planted=True)


def test_the_inputs_of_the_device_tests(qg_case):
    """The class counts of the qg_case packets' vorticity at the initial state
    over zeta_edges: every class is populated by the restatement alone."""
    q = qg_case
    zeta = flow_scalars([q["flow"]], 1, 0.0, q["x"], q["L"] / q["nx"], orc.BUMP_QG)[0]
    rows = {nq: np.bincount(class_of(zeta, zeta_edges(q["flow"], nq)), minlength=nq + 2) for nq in (1, 4, 15)}
    print({nq: r.tolist() for nq, r in rows.items()})
    assert rows[1].tolist() == [7, 243, 6]
    assert rows[4].tolist() == [7, 38, 81, 73, 51, 6]
    assert rows[15].min() >= 5 and rows[15].max() <= 25


def test_values_on_the_edges():
    edges = np.array([-1.5, -0.25, 0.0, 0.75, 2.0])
    nb = edges.size - 1
    assert class_of(edges, edges).tolist() == [1, 2, 3, 4, 4]  # first edge: first bin; interior: right; last: closed
    assert class_of([np.nextafter(-1.5, -2), np.nextafter(2.0, 3), np.nan, -np.inf, np.inf], edges).tolist() == \
        [0, nb + 1, -1, 0, nb + 1]
    # on both axes of a frame: q on every q edge with w inside bin 0, then w on every w edge with q inside bin 0
    wedges = np.array([10.0, 11.0, 12.0, 13.0])
    counts, sums, stats = cond_frame_of(edges, np.full(edges.size, 10.5), wedges, edges, 4)
    assert stats.tolist() == [5, 0]
    assert counts[:, 1].tolist() == [0, 1, 1, 1, 2, 0] and counts.sum() == 5
    assert sums.tolist() == [0, 168, 168, 168, 336, 0]  # 10.5 * 16
    counts, sums, stats = cond_frame_of(np.full(wedges.size, -1.0), wedges, wedges, edges, 0)
    assert counts[1].tolist() == [0, 1, 1, 2, 0] and counts.sum() == 4
    assert sums.tolist() == [0, 10 + 11 + 12 + 13, 0, 0, 0, 0]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_marginals(case, which):
    c, q = case, case["q"]
    qv, w = c["scal"][NAMES[which]], c["w"]
    qedges, wedges = central_edges(qv, 15), central_edges(w[w < 1e6], 300)
    counts, _, stats = cond_frame_of(qv, w, wedges, qedges, 20)
    ok = np.abs(w * 2.0 ** 20) < 2.0 ** 38
    assert stats[1] == 300 - ok.sum() == 3
    # the omega-series row [below, histcounts, above] of the accepted packets
    wa = w[ok]
    row = np.concatenate([[np.sum(wa < wedges[0])], np.histogram(wa, wedges)[0], [np.sum(wa > wedges[-1])]])
    np.testing.assert_array_equal(counts.sum(axis=0), row)
    qa = qv[ok]
    qrow = np.concatenate([[np.sum(qa < qedges[0])], np.histogram(qa, qedges)[0], [np.sum(qa > qedges[-1])]])
    np.testing.assert_array_equal(counts.sum(axis=1), qrow)
    assert_populated(counts, stats, planted=True)


def test_combine_conds(case):
    c, q = case, case["q"]
    qv, w = c["scal"]["zeta"], c["w"]
    qedges, wedges = zeta_edges(q["flow"], 4), central_edges(w[w < 1e6], 7)
    whole = cond_frame_of(qv, w, wedges, qedges, 20)
    part_of = np.random.default_rng(5).integers(0, 3, 300)
    parts = []
    for r in range(3):
        fr = cond_frame_of(qv[part_of == r], w[part_of == r], wedges, qedges, 20)
        parts.append(tuple(a[None] for a in fr))  # one frame each
    got = sw.combine_conds(parts)
    for g, want in zip(got, whole):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g[0], want)
    assert sw.combine_conds(parts[:1])[0].shape == (1, 6, 9)
    other = tuple(a[None] for a in cond_frame_of(qv, w, central_edges(w[w < 1e6], 8), qedges, 20))
    with pytest.raises(ValueError):
        sw.combine_conds([parts[0], other])
    with pytest.raises(ValueError):
        sw.combine_conds([parts[0], (parts[1][0], parts[1][1][:, :3], parts[1][2])])
    with pytest.raises(ValueError):
        sw.combine_conds([])


def test_cond_spectra_on_empty_classes():
    counts = np.array([[0, 0, 0], [1, 2, 1], [0, 0, 0], [0, 5, 0]], dtype=np.int64)
    sums = np.array([0, 4 * 12 * 16, 0, 5 * 10 * 16 + 8], dtype=np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = sw.cond_spectra(counts[None], sums[None], 4)
    assert out["n"][0].tolist() == [0, 4, 0, 5]
    np.testing.assert_array_equal(out["spectrum"][0, 1], [0.25, 0.5, 0.25])
    np.testing.assert_array_equal(out["spectrum"][0, 3], [0.0, 1.0, 0.0])
    assert np.isnan(out["spectrum"][0, [0, 2]]).all() and np.isnan(out["omega_mean"][0, [0, 2]]).all()
    assert out["omega_mean"][0, 1] == 12.0 and out["omega_mean"][0, 3] == 10.1
    with pytest.raises(ValueError):
        sw.cond_spectra(counts, sums[:3], 4)
    with pytest.raises(ValueError):
        sw.cond_spectra(counts, sums, 33)


def test_driver_arguments():
    spec = np.linspace(3.0, 20.0, 11)
    assert _cond_args(None, None, 20, None) is None and _cond_args(None, [0.0, 1.0], 20, spec) is None
    by, edges, fb = _cond_args("sigma", [0.0, 0.5, 1.0], 12, spec)
    assert by == "sigma" and edges.tolist() == [0.0, 0.5, 1.0] and fb == 12
    with pytest.raises(ValueError, match="spectrum_edges"):
        _cond_args("zeta", [-1.0, 1.0], 20, None)
    for name in ("vorticity", "Zeta", 0, True):
        with pytest.raises(ValueError, match="cond_by"):
            _cond_args(name, [-1.0, 1.0], 20, spec)
    for bad in ([1.0, 0.0], [0.0, 0.0, 1.0], [0.0], [0.0, np.nan], [0.0, np.inf], None):
        with pytest.raises(ValueError, match="cond_edges"):
            _cond_args("zeta", bad, 20, spec)
    for bad in (-1, 33, 1.5, True):
        with pytest.raises(ValueError, match="cond_frac_bits"):
            _cond_args("D", [-1.0, 1.0], bad, spec)
    with pytest.raises(ValueError, match="65536"):
        _cond_args("D", np.arange(4001.0), 20, np.arange(301.0))
    # the drivers refuse before anything runs (no device is touched)
    with pytest.raises(ValueError, match="spectrum_edges"):
        sw.qgsw_raytrace(64, 10, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, cond_by="zeta", cond_edges=[-1.0, 1.0])
    with pytest.raises(ValueError, match="cond_by"):
        sw.qg2layersw_raytrace(64, 10, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0, cond_by="vorticity", cond_edges=[-1.0, 1.0],
                               spectrum_edges=spec)
