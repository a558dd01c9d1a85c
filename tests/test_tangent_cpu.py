"""The tangent map's numpy restatement (tests/tangent_ref.py) on its own, no
GPU: its M against central differences of orc.leapfrog, its x and k against
orc.leapfrog's bits, the mark, the frame's layout, and the package's
combine_tangents / tangent_growth on hand-made frames."""
import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import cbind, swrt_oracle as orc
from tests import tangent_ref as tr
from tests.cond_series_ref import omega_of
from tests.test_gpu_refr_series import _flow32

BUMP = 1e-10
N = 1000
STEPS = 20
EPS = 1e-6
EDGE = 1e-4      # cell units: packets whose kick point came this close to a cell edge are left out
FD_TOL = 7.8e-8  # 20 x the measured 3.9e-9 (test_central_differences), below the issue's cap of 1e-5


@pytest.fixture(scope="module")
def case():
    q = _flow32()
    rng = np.random.default_rng(35)
    x0, k0 = orc.initial_packets(N, q["L"], 4.0, q["f"], q["Cg"], rng)
    dx = q["L"] / q["nx"]
    x, k, _, _ = cbind.leapfrog(cbind.planes_of(q["flow"]), None, 0.0, 0.0, q["nx"], q["nx"], dx, BUMP, x0, k0, q["dt"],
                                300, q["f"], q["Cg"] ** 2)
    flows = [q["flow"], {n: 0.8 * np.asarray(v) for n, v in q["flow"].items()}]
    return dict(q=q, x=np.ascontiguousarray(x), k=np.ascontiguousarray(k), dx=dx, flows=flows)


def _oracle(case, two, x, k, steps=STEPS):
    q = case["q"]
    s0 = orc.GridField(case["flows"][0], case["dx"])
    s1 = orc.GridField(case["flows"][1], case["dx"]) if two else None
    xo, ko, _, _ = orc.leapfrog(x, k, q["dt"], steps, q["f"], q["Cg"] ** 2, s0, s1, 0.1 if two else 0.0,
                                0.04 if two else 0.0, BUMP)
    return xo, ko


def _restated(case, two, x, k, steps=STEPS, M=None, caus=None, kick_points=None):
    q = case["q"]
    n = x.shape[0]
    if M is None:
        M, caus = tr.identity(n)
    return tr.tangent_leapfrog(x, k, M, caus, q["dt"], steps, q["f"], q["Cg"] ** 2,
                               case["flows"][:2 if two else 1], case["dx"], 0.1 if two else 0.0,
                               0.04 if two else 0.0, BUMP, kick_points=kick_points)


@pytest.mark.parametrize("two", [False, True], ids=["steady", "two_snapshots"])
def test_central_differences(case, two):
    """max|FD - M| / max|M| over 1000 packets and 20 steps, eps = 1e-6, packets
    whose kick point (of the base ray or a perturbed one) came within 1e-4 cell
    of a cell edge left out.  Measured with the finished restatement: steady
    3.9e-9, two snapshots 3.8e-9 (excluded 0.7 % and 0.9 %); the tolerance is
    20 x the larger, 7.8e-8.  A wrong or missing Jacobian term shows at 1e-3 or more
    (test_a_missing_term_shows)."""
    x, k = case["x"], case["k"]
    pts = []
    _, _, M, _ = _restated(case, two, x, k, kick_points=pts)
    M = M.reshape(N, 4, 4)
    near = np.zeros(N, dtype=bool)

    def note(points):
        for p in points:
            a = p / case["dx"]
            frac = a - np.floor(a)
            near[:] |= (np.minimum(frac, 1 - frac) < EDGE).any(axis=1)

    note(pts)
    FD = np.zeros((N, 4, 4))
    for c in range(4):
        outs = []
        for sgn in (+1.0, -1.0):
            xs, ks = x.copy(), k.copy()
            (xs if c < 2 else ks)[:, c % 2] += sgn * EPS
            pp = []
            _restated(case, two, xs, ks, kick_points=pp)  # (the perturbed rays' kick points)
            note(pp)
            xo, ko = _oracle(case, two, xs, ks)
            outs.append(np.concatenate([xo, ko], axis=1))
        FD[:, :, c] = (outs[0] - outs[1]) / (2 * EPS)
    share = near.mean()
    keep = ~near
    err = np.abs(FD[keep] - M[keep]).max() / np.abs(M[keep]).max()
    print(f"two {two}: excluded {share:.4f}, max|FD - M|/max|M| = {err:.3e}, max|M| = {np.abs(M[keep]).max():.3e}")
    assert share <= 0.05
    assert err <= FD_TOL


def test_a_missing_term_shows(case):
    """Without the interpolant's derivative of the gradient fields (the A, B
    sums of the k rows) the same comparison misses by far more than the tolerance."""
    x, k = case["x"][:200], case["k"][:200]
    _, _, M, _ = _restated(case, False, x, k)
    real = tr.gather_tangent

    def crippled(*a, **kw):
        o, d = real(*a, **kw)
        return o, d[:4] + [np.zeros_like(d[4])] * 4

    tr.gather_tangent = crippled
    try:
        _, _, Mbad, _ = _restated(case, False, x, k)
    finally:
        tr.gather_tangent = real
    assert np.abs(Mbad - M).max() / np.abs(M).max() > 1e-3


@pytest.mark.parametrize("two", [False, True], ids=["steady", "two_snapshots"])
def test_x_and_k_keep_the_oracles_bits(case, two):
    x, k = case["x"], case["k"]
    xr, kr, _, _ = _restated(case, two, x, k)
    xo, ko = _oracle(case, two, x, k)
    assert np.array_equal(xr, xo) and np.array_equal(kr, ko)


def test_split_calls_and_the_mark(case):
    """Steps split over calls give the same bits (a steady flow: no step index
    enters); at a mark M == I, J == 1 and the counters are 0, and the window
    that follows equals a fresh run from there."""
    x, k = case["x"][:257], case["k"][:257]
    whole = _restated(case, False, x, k, 12)
    part = _restated(case, False, x, k, 5)
    both = _restated(case, False, part[0], part[1], 7, part[2], part[3])
    for a, b in zip(whole, both):
        assert np.array_equal(a, b)
    M0, c0 = tr.identity(257)
    assert np.array_equal(M0.reshape(-1, 4, 4), np.broadcast_to(np.eye(4), (257, 4, 4)))
    assert np.array_equal(tr.ray_jacobian(M0), np.ones(257)) and not c0.any() and c0.dtype == np.int32
    fresh = _restated(case, False, part[0], part[1], 7)
    marked = _restated(case, False, part[0], part[1], 7, M0, c0)
    assert np.array_equal(fresh[2], marked[2]) and np.array_equal(fresh[3], marked[3])


def test_tubes_fold_and_the_kick_is_not_symplectic(case):
    """The issue's figures on this flow: ray tubes fold within 20 steps, and
    det M leaves 1 (the Euler kick); the counters count J's sign changes."""
    x, k = case["x"], case["k"]
    _, _, M, caus = _restated(case, False, x, k)
    J = tr.ray_jacobian(M)
    assert (J < 0).any()
    assert np.array_equal(caus % 2 == 1, J < 0)  # (from J = 1: an odd count is a folded tube)
    det = np.linalg.det(M.reshape(N, 4, 4))
    assert 1e-6 < np.abs(det - 1).max() < 1.0


def test_frame_layout_and_stats(case):
    x, k = case["x"], case["k"]
    xr, kr, M, caus = _restated(case, False, x, k)
    M, kr = M.copy(), kr.copy()
    M[3, 7] = np.nan        # s not finite
    M[4, :] = 0.0           # J == 0
    kr[5, 0] = np.nan       # omega not finite
    M[6, 2] = np.inf
    q = case["q"]
    w = omega_of(kr, q["f"], q["Cg"])
    wedges = np.linspace(np.nanmin(w), np.nanmax(w), 13)[1:-1]
    gedges = tr.growth_edges_of(M, 8)
    counts, sums, stats = tr.tangent_frame_of(M, caus, w, wedges, gedges, 3)
    nw, ns = wedges.size - 1, 8
    assert counts.shape == (ns + 2, nw + 2) and sums.shape == (3 * (nw + 2) + ns + 2,) and stats.tolist() == [N, 4, 3]
    assert counts.sum() == N - 4 and (counts >= 0).all()
    ok = np.ones(N, dtype=bool)
    ok[3:7] = False
    assert sums[2 * (nw + 2):3 * (nw + 2)].sum() == caus[ok].sum() == sums[3 * (nw + 2):].sum()
    s, J = tr.growth_of(M)
    assert sums[:nw + 2].sum() == int(np.floor(np.log2(s[ok])).sum())
    assert sums[nw + 2:2 * (nw + 2)].sum() == int(np.floor(np.log2(np.abs(J[ok]))).sum())
    # a packet-by-packet loop gives the same plane
    plane = np.zeros_like(counts)
    for p in np.flatnonzero(ok):
        gc = 0 if s[p] < gedges[0] else ns + 1 if s[p] > gedges[-1] else min(np.searchsorted(gedges, s[p], "right"), ns)
        wc = 0 if w[p] < wedges[0] else nw + 1 if w[p] > wedges[-1] else min(np.searchsorted(wedges, w[p], "right"), nw)
        plane[gc, wc] += 1
    assert np.array_equal(plane, counts)


def _frames(T, ns, nw, n, serial, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 5, size=(T, ns + 2, nw + 2)).astype(np.int64)
    sums = rng.integers(-50, 50, size=(T, 3 * (nw + 2) + ns + 2)).astype(np.int64)
    stats = np.tile(np.array([n, 1, serial], dtype=np.int64), (T, 1))
    return counts, sums, stats


def test_combine_tangents():
    a, b = _frames(3, 2, 4, 10, 2, 1), _frames(3, 2, 4, 7, 2, 2)
    empty = tuple(np.zeros_like(v) for v in a)
    counts, sums, stats = sw.combine_tangents([a, b, empty])
    assert np.array_equal(counts, a[0] + b[0]) and np.array_equal(sums, a[1] + b[1])
    assert stats.tolist() == [[17, 2, 2]] * 3
    other = _frames(3, 2, 4, 7, 3, 2)
    with pytest.raises(ValueError, match="serials differ"):
        sw.combine_tangents([a, other])
    with pytest.raises(ValueError):
        sw.combine_tangents([])
    with pytest.raises(ValueError):
        sw.combine_tangents([a, _frames(3, 3, 4, 7, 2, 2)])


def test_tangent_growth():
    ns, nw = 1, 2
    counts = np.zeros((ns + 2, nw + 2), dtype=np.int64)
    counts[1, 1], counts[2, 1], counts[1, 2] = 3, 1, 2      # omega class 1: 4 packets, class 2: 2
    sums = np.zeros(3 * (nw + 2) + ns + 2, dtype=np.int64)
    sums[1], sums[2] = 8, -2                                 # sum e(s)
    sums[(nw + 2) + 1] = -4                                  # sum e(|J|)
    sums[2 * (nw + 2) + 1] = 6                               # caustics
    sums[3 * (nw + 2) + 1], sums[3 * (nw + 2) + 2] = 5, 1
    stats = np.array([7, 1, 4], dtype=np.int64)
    g = sw.tangent_growth(counts, sums, stats, 2.0)
    assert g["n"].tolist() == [0, 4, 2, 0] and g["accepted"] == 6
    np.testing.assert_array_equal(g["log2_stretch_mean"][1:3], [2.0, -1.0])
    np.testing.assert_allclose(g["lyapunov"][1:3], [np.log(2) / 2 * 2.0 / 2.0, np.log(2) / 2 * -1.0 / 2.0], rtol=1e-15)
    assert g["log2_amplitude_mean"][1] == 1.0 and g["caustics_mean"][1] == 1.5
    assert np.isnan(g["lyapunov"][0]) and np.isnan(g["caustics_mean"][3])
    assert g["n_growth"].tolist() == [0, 5, 1] and g["caustics_mean_growth"][1:].tolist() == [1.0, 1.0]
    with pytest.raises(ValueError):
        sw.tangent_growth(counts, sums[:-1], stats, 2.0)
    with pytest.raises(ValueError):
        sw.tangent_growth(counts, sums, stats, 0.0)


@pytest.mark.parametrize("driver", [sw.qgsw_raytrace, sw.qg2layersw_raytrace])
def test_driver_argument_errors(driver, tmp_path):
    """Every refused combination raises before anything runs (no context, no file)."""
    args = (32, 10, 4.0, 1.0, 0.0, 0.2, 3.0, 1.0)
    spec, edges = [3.0, 4.0], [1.0, 2.0]
    out = tmp_path / "none"
    for kw, msg in ((dict(tangent_edges=edges), "needs spectrum_edges"),
                    (dict(tangent_edges=edges, spectrum_edges=spec, integrator="ode23"), 'integrator="leapfrog"'),
                    (dict(tangent_edges=edges, spectrum_edges=spec, packet_method="midpoint"), "packet_method"),
                    (dict(tangent_edges=edges, spectrum_edges=spec, packet_method="yoshida4"), "packet_method"),
                    (dict(tangent_edges=edges, spectrum_edges=spec, recycle_omega=20.0), "recycled"),
                    (dict(tangent_lag=2), "tangent_lag needs tangent_edges"),
                    (dict(tangent_edges=edges, spectrum_edges=spec, tangent_lag=0), "integer >= 1"),
                    (dict(tangent_edges=edges, spectrum_edges=spec, tangent_lag=1.5), "integer >= 1"),
                    (dict(tangent_edges=[2.0, 1.0], spectrum_edges=spec), "increasing"),
                    (dict(tangent_edges=2.0 ** np.arange(300), spectrum_edges=np.arange(400.0)), "65536")):
        with pytest.raises(ValueError, match=msg):
            driver(*args, out_dir=str(out), **kw)
    with pytest.raises(ValueError, match="needs packets"):
        driver(32, 0, 4.0, 1.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(out), tangent_edges=edges, spectrum_edges=spec)
    assert not out.exists()
