"""The invariant and the flow along the rays, sampled on the device
(swrt_raydiag_*, swraytracing_amd/csrc/swrt_raydiag.hpp).

Reference: symplectic_full_fourier.m:41,54-57 (Omega_0, Omega_abs and
(Omega_abs - Omega_0)./Omega_0) and RaytracingScheme.m:18-31 (vorticity,
strain, Okubo-Weiss).  Expected values are the numpy oracle's interpolation
(orc.interpolate_fields / orc.interpolate_U) at the packets packets_get
returns, followed by the same numpy expressions, so every per-packet value is
compared bit for bit.  A frame's sums are compared with math.fsum within
2*N*2^-53*sum|t_i|: the first-order bound of any summation order, doubled.

All cases: 64^2 grid, L = 2 pi, f = 3, gH = 1, psi = 0.05 (cos(x+y) +
0.7 sin(2x-y)), x uniform in [-pi, pi)^2, |k| = 3."""
import math

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import swrt_oracle as orc
from tests.conftest import periodic_grid

pytestmark = pytest.mark.gpu

NX, L, F, GH = 64, 2 * np.pi, 3.0, 1.0
DX = L / NX
BUMP = orc.BUMP_SW
DT = 0.05
NBIG = 4133  # no multiple of 64 or 256; more than one workgroup


def _psi(which):
    X, Y = periodic_grid(NX, L)
    if which == 0:
        return 0.05 * (np.cos(X + Y) + 0.7 * np.sin(2 * X - Y))
    return 0.04 * (np.sin(X - 2 * Y) + 0.5 * np.cos(3 * X + Y))


def _packets(n, seed=20):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th = rng.uniform(0, 2 * np.pi, n)
    return x, 3.0 * np.stack([np.cos(th), np.sin(th)], axis=1)


@pytest.fixture(scope="module")
def flows():
    """The two snapshots as the device holds them (set_field_psi's planes), in
    the oracle's dict form: computed once, read-only."""
    c = sw.Context(0)
    out = []
    for which in (0, 1):
        c.set_field_psi(0, _psi(which), NX, L)
        p = c.get_field_grid(0, NX)
        out.append({n: p[i].reshape((NX, NX), order="F").copy() for i, n in enumerate(orc.FIELD_ORDER)})
    c.close()
    return out


def _set_fields(c, nslots):
    for s in range(nslots):
        c.set_field_psi(s, _psi(s), NX, L)


def _expected(flows, nslots, alpha, x, k):
    """[Omega zeta sigma D] (N x 4) and omega (N,) in the header's operation order."""
    if nslots == 1:
        u, v, ux, uy, vx, vy = orc.interpolate_fields(x[:, 0], x[:, 1], flows[0], DX, BUMP)
    else:
        U, nab = orc.interpolate_U(flows[0], flows[1], alpha, x, DX, BUMP)
        u, v = U[:, 0], U[:, 1]
        ux, uy, vx, vy = nab["u_x"], nab["u_y"], nab["v_x"], nab["v_y"]
    k1, k2 = k[:, 0], k[:, 1]
    om = np.sqrt(F * F + GH * (k1 * k1 + k2 * k2))
    Om = om + (u * k1 + v * k2)
    zeta = vx - uy
    s1, s2 = ux - vy, vx + uy
    sigma = np.sqrt(s1 * s1 + s2 * s2)
    D = vy * vy + vx * uy  # RaytracingScheme.m:30
    return np.stack([Om, zeta, sigma, D], axis=1), om


def _check_sum(got, terms, what):
    terms = np.asarray(terms, dtype=np.float64)
    want = math.fsum(terms)
    bound = 2 * terms.size * 2.0 ** -53 * math.fsum(np.abs(terms))
    print(f"{what}: got {got!r} fsum {want!r} diff {abs(got - want):.3e} bound {bound:.3e}")
    assert abs(got - want) <= bound, what


def _check_frame(fr, r, om, e4):
    assert fr[0] == r.size
    print(f"max|r| {fr[1]!r} numpy {np.abs(r).max()!r}")
    assert fr[1] == np.abs(r).max()
    _check_sum(fr[2], r, "sum r")
    _check_sum(fr[3], r * r, "sum r^2")
    _check_sum(fr[4], om, "sum omega")
    _check_sum(fr[5], e4[:, 1], "sum zeta")
    _check_sum(fr[6], e4[:, 2], "sum sigma")
    _check_sum(fr[7], e4[:, 3], "sum D")


CASES = [(1, 0.0), (2, 0.3)]


@pytest.mark.parametrize("nslots,alpha", CASES)
@pytest.mark.parametrize("n", [1, 37, NBIG])
def test_per_packet_values_and_frame(fresh_ctx, flows, n, nslots, alpha):
    c = fresh_ctx
    _set_fields(c, nslots)
    c.set_locality(rebin_every=5, tile=16)
    x0, k0 = _packets(n)
    c.packets_set(x0, k0)
    phys = dict(nslots=nslots, alpha=alpha, bump=BUMP)
    # no mark yet: r and its three frame entries are 0
    s4, fr = c.raydiag_sample(F, GH, **phys)
    e4, om = _expected(flows, nslots, alpha, x0, k0)
    np.testing.assert_array_equal(s4[:, [0, 1, 3]], e4[:, [0, 1, 3]])
    np.testing.assert_array_equal(s4[:, 2], e4[:, 2])  # sigma: sqrt correctly rounded
    _check_frame(fr, np.zeros(n), om, e4)
    Om0 = e4[:, 0]
    assert Om0.min() > 3.5  # the division by Omega_0 is safe
    c.raydiag_mark(F, GH, **phys)
    # 40 steps, re-binned every 5: the storage order is no longer the packets' order
    c.advance(DT, 40, F, GH, nslots=nslots, alpha0=alpha, dalpha=0.0, bump=BUMP)
    s4, fr = c.raydiag_sample(F, GH, **phys)
    x, k = c.packets_get()
    if n == NBIG:
        assert np.abs(x).max() > np.pi  # the periodic wrap is exercised
    e4, om = _expected(flows, nslots, alpha, x, k)
    np.testing.assert_array_equal(s4[:, [0, 1, 3]], e4[:, [0, 1, 3]])
    np.testing.assert_array_equal(s4[:, 2], e4[:, 2])
    r = (e4[:, 0] - Om0) / Om0
    if n == NBIG:
        assert 0 < np.abs(r).max() < 1e-2
    _check_frame(fr, r, om, e4)
    # the same state again: the same bits
    s4b, frb = c.raydiag_sample(F, GH, **phys)
    assert s4b.tobytes() == s4.tobytes() and frb.tobytes() == fr.tobytes()
    # the frame alone (no per-packet output) is the same frame
    none, frc = c.raydiag_sample(F, GH, values=False, **phys)
    assert none is None and frc.tobytes() == fr.tobytes()


def test_zero_flow(fresh_ctx):
    c = fresh_ctx
    c.set_field_grid(0, np.zeros((6, NX * NX)), NX, L)
    x0, k0 = _packets(NBIG)
    c.packets_set(x0, k0)
    c.raydiag_mark(F, GH, bump=BUMP)
    s0, _ = c.raydiag_sample(F, GH, bump=BUMP)
    c.advance(DT, 50, F, GH, bump=BUMP)
    s4, fr = c.raydiag_sample(F, GH, bump=BUMP)
    np.testing.assert_array_equal(s4[:, 0], s0[:, 0])  # every Omega is its Omega_0: every r is 0
    assert fr[0] == NBIG
    assert fr[1] == 0.0 and fr[2] == 0.0 and fr[3] == 0.0
    assert fr[5] == 0.0 and fr[6] == 0.0 and fr[7] == 0.0
    assert not s4[:, 1:].any()
    k1, k2 = k0[:, 0], k0[:, 1]
    _check_sum(fr[4], np.sqrt(F * F + GH * (k1 * k1 + k2 * k2)), "sum omega")


def test_series_matches_synchronous_samples(fresh_ctx):
    a, b = fresh_ctx, sw.Context(0)
    try:
        x0, k0 = _packets(NBIG)
        phys = dict(nslots=2, alpha=0.3, bump=BUMP)
        for c in (a, b):
            _set_fields(c, 2)
            c.set_locality(rebin_every=5, tile=16)
            c.packets_set(x0, k0)
            c.raydiag_mark(F, GH, **phys)
        assert a.raydiag_frames() == 0
        sync = []
        for _ in range(4):
            for c in (a, b):
                c.advance(DT, 10, F, GH, nslots=2, alpha0=0.3, dalpha=0.0, bump=BUMP)
            a.raydiag_record(F, GH, **phys)
            sync.append(b.raydiag_sample(F, GH, values=False, **phys)[1])
        assert a.raydiag_frames() == 4
        ser = a.raydiag_series()
        assert ser.shape == (4, 8)
        np.testing.assert_array_equal(ser, np.stack(sync))
        assert (ser[:, 1] > 0).all()
        np.testing.assert_array_equal(a.raydiag_series(1, 2), ser[1:3])
        with pytest.raises(sw.SwrtError):
            a.raydiag_series(2, 3)
        a.raydiag_series_reset()
        assert a.raydiag_frames() == 0 and a.raydiag_series().shape == (0, 8)
        # the mark survives the reset; another N drops it, and the series
        a.raydiag_record(F, GH, **phys)
        assert a.raydiag_series()[0, 1] == ser[-1, 1]
        x1, k1 = _packets(37, seed=21)
        a.packets_set(x1, k1)
        assert a.raydiag_frames() == 0
        fr = a.raydiag_sample(F, GH, values=False, **phys)[1]
        assert fr[0] == 37 and fr[1] == 0.0 and fr[2] == 0.0 and fr[3] == 0.0
    finally:
        b.close()


def test_series_grows_and_resets(fresh_ctx):
    """4,100 frames: past the 4,096 the first record reserves, so the series
    grows once with frames recorded.  Frames 0..4090 are of the packets 10 steps
    after the mark, the rest of the packets at the mark again (the same N keeps
    the mark and the series): each equals raydiag_sample's frame of that state."""
    c = fresh_ctx
    _set_fields(c, 2)
    phys = dict(nslots=2, alpha=0.3, bump=BUMP)
    xa, ka = _packets(37, seed=23)
    c.packets_set(xa, ka)
    c.raydiag_mark(F, GH, **phys)
    c.advance(DT, 10, F, GH, nslots=2, alpha0=0.3, dalpha=0.0, bump=BUMP)
    moved = c.raydiag_sample(F, GH, values=False, **phys)[1]
    for i in range(4100):
        if i == 4091:
            c.packets_set(xa, ka)
            at_mark = c.raydiag_sample(F, GH, values=False, **phys)[1]
        c.raydiag_record(F, GH, **phys)
    assert c.raydiag_frames() == 4100
    assert moved[0] == 37 and moved[1] > 0 and at_mark[0] == 37 and at_mark[1] == 0.0  # the two states differ
    ser = c.raydiag_series()
    assert ser.shape == (4100, 8)
    for i, want in ((0, moved), (4090, moved), (4091, at_mark), (4095, at_mark), (4096, at_mark), (4099, at_mark)):
        assert ser[i].tobytes() == want.tobytes(), f"frame {i}"
    assert (ser[:4091] == ser[0]).all() and (ser[4091:] == ser[4099]).all()
    np.testing.assert_array_equal(c.raydiag_series(4095, 3), ser[4095:4098])
    # a reset keeps the mark (and the buffers): one record, one frame, r measured against the old mark
    c.raydiag_series_reset()
    assert c.raydiag_frames() == 0 and c.raydiag_series().shape == (0, 8)
    c.advance(DT, 10, F, GH, nslots=2, alpha0=0.3, dalpha=0.0, bump=BUMP)
    c.raydiag_record(F, GH, **phys)
    one = c.raydiag_series()
    assert one.shape == (1, 8) and one[0, 1] > 0
    assert one[0].tobytes() == c.raydiag_sample(F, GH, values=False, **phys)[1].tobytes()
    # another N empties the series and drops the mark
    xb, kb = _packets(41, seed=24)
    c.packets_set(xb, kb)
    assert c.raydiag_frames() == 0 and c.raydiag_series().shape == (0, 8)
    fr = c.raydiag_sample(F, GH, values=False, **phys)[1]
    assert fr[0] == 41 and fr[1] == 0.0 and fr[2] == 0.0 and fr[3] == 0.0


def test_advance_unaffected_and_ordered_after_split_launches(fresh_ctx, flows):
    """70,001 packets: above the size from which a tile launch runs as two part
    launches on two streams.  Marks and records between the advance calls leave
    the packets' bits alone, and a frame queued behind a split launch (no host
    wait) is the frame of the state that launch leaves."""
    n = 70_001
    a, b = fresh_ctx, sw.Context(0)
    try:
        x0, k0 = _packets(n, seed=22)
        for c in (a, b):
            _set_fields(c, 1)
            c.set_locality(rebin_every=5, tile=16)
            c.packets_set(x0, k0)
        a.raydiag_mark(F, GH, bump=BUMP)
        for _ in range(4):
            a.advance(DT, 5, F, GH, bump=BUMP)
            a.raydiag_record(F, GH, bump=BUMP)
        a.raydiag_mark(F, GH, bump=BUMP)
        ser = a.raydiag_series()
        xa, ka = a.packets_get()
        b.advance(DT, 20, F, GH, bump=BUMP)
        xb, kb = b.packets_get()
        assert xa.tobytes() == xb.tobytes() and ka.tobytes() == kb.tobytes()
        # the last recorded frame against the oracle at the final state
        e0, _ = _expected(flows, 1, 0.0, x0, k0)
        e4, om = _expected(flows, 1, 0.0, xa, ka)
        _check_frame(ser[-1], (e4[:, 0] - e0[:, 0]) / e0[:, 0], om, e4)
    finally:
        b.close()


def test_ode_symplectic_diagnostics(fresh_ctx, flows):
    sch = sw.SpectralScheme(L, NX, _psi(0), ctx=fresh_ctx)
    x0, k0 = _packets(NBIG)
    X0, K0 = x0.T[None], k0.T[None]  # 1 x 2 x P
    T = 13.5 * DT
    x, k, t = sw.ode_symplectic(X0, K0, DT, T, F, GH, sch)
    xd, kd, td, ser = sw.ode_symplectic(X0, K0, DT, T, F, GH, sch, diagnostics=True)
    assert x.shape[0] == 13 and ser.shape == (13, 8)
    assert xd.tobytes() == x.tobytes() and kd.tobytes() == k.tobytes() and td.tobytes() == t.tobytes()
    assert ser[0, 1] == 0.0 and ser[0, 2] == 0.0 and ser[0, 3] == 0.0
    assert (ser[:, 0] == NBIG).all()
    e0, _ = _expected(flows, 1, 0.0, x0, k0)
    e4, om = _expected(flows, 1, 0.0, np.ascontiguousarray(x[-1].T), np.ascontiguousarray(k[-1].T))
    r = (e4[:, 0] - e0[:, 0]) / e0[:, 0]
    assert ser[-1, 1] == np.abs(r).max() > 0
    _check_frame(ser[-1], r, om, e4)
    # one frame, no step
    x1, k1, t1, s1 = sw.ode_symplectic(X0, K0, DT, 1.5 * DT, F, GH, sch, diagnostics=True)
    assert x1.shape[0] == 1 and s1.shape == (1, 8) and s1[0, 0] == NBIG and s1[0, 1] == 0.0
    with pytest.raises(ValueError):
        sw.ode_symplectic(X0, K0, DT, T, F, GH, sw.DifferenceScheme(lambda x, y, t: 0 * x), diagnostics=True)


def test_errors(fresh_ctx):
    c = fresh_ctx
    x0, k0 = _packets(37)
    calls = [lambda **kw: c.raydiag_mark(F, GH, **kw), lambda **kw: c.raydiag_sample(F, GH, **kw),
             lambda **kw: c.raydiag_record(F, GH, **kw)]
    for call in calls:
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*slot not set"):  # nothing set yet
            call()
    _set_fields(c, 1)
    for call in calls:
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*no packets"):
            call()
    c.packets_set(x0, k0)
    for call in calls:
        for bad in (0, 3):
            with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*nslots"):
                call(nslots=bad)
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*slot not set"):  # slot 1 is not set
            call(nslots=2)
    c.set_field_psi(1, _psi(1)[::2, ::2], NX // 2, L)
    for call in calls:
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*different grids"):
            call(nslots=2)
    assert c.raydiag_frames() == 0
    c.raydiag_record(F, GH)
    for first, count in ((-1, 1), (0, 2), (1, 1), (0, -1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
            c.raydiag_series(first, count)
    assert c._L.swrt_raydiag_series_get(c._h, 0, 1, None) == 1  # NULL where a buffer is required
    assert b"NULL" in c._L.swrt_last_error(c._h)
    # both outputs of a sample may be NULL
    assert c._L.swrt_raydiag_sample(c._h, F, GH, 1, 0.0, BUMP, None, None) == 0
