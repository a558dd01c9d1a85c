"""The spectrum-series commands of the MEX gateway (matlab/swrt_mex.cpp:
omega_series_begin / _record / _record_history / _get / _reset, omega_ideal),
driven through the test mex.h shim as test_mex_gateway.py drives the others:
the arrays MATLAB gets — counts as a double (nbins+2) x frames matrix, stats
4 x frames — are the arrays the Python Context gives for the same calls."""
import numpy as np
import pytest

from oracle import swrt_oracle as orc
from tests.test_mex_gateway import Mex, MexError

F, CG = 3.0, 1.0


@pytest.fixture(scope="module")
def mex():
    return Mex()


def _setup():
    nx, L, n = 64, 2 * np.pi, 1000
    rng = np.random.default_rng(31)
    planes = 0.2 * rng.standard_normal((6, nx * nx))
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th, r = rng.uniform(0, 2 * np.pi, n), 6.0 * rng.random(n)
    k = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    edges = np.linspace(3.5, 6.0, 31)
    t = np.linspace(0, 2 * np.pi, 7)
    ring = 3.0 * np.stack([np.cos(t), np.sin(t)], axis=1)
    omega0 = float(np.sqrt(F ** 2 + CG ** 2 * 9.0))
    return nx, L, planes, x, k, edges, ring, omega0, omega0 + np.linspace(-0.3, 0.3, 7)


@pytest.mark.gpu
def test_gateway_series_and_ideal_equal_the_context(mex, fresh_ctx):
    nx, L, planes, x, k, edges, ring, omega0, iedges = _setup()
    dt, steps = 0.05, 6
    # the Context
    c = fresh_ctx
    c.set_field_grid(0, planes, nx, L)
    c.packets_set(x, k)
    c.omega_series_begin(F, CG, edges)
    c.omega_series_record()
    c.advance(dt, steps, F, CG ** 2, bump=orc.BUMP_QG, save_every=1)
    c.omega_series_record()
    c.omega_series_record_history(1, 4)
    counts, stats = c.omega_series()
    ideal = c.omega_ideal(0, ring, omega0, iedges)
    assert counts.shape == (6, 32) and counts[0].sum() == 1000 and len({r.tobytes() for r in counts}) > 1
    # the gateway
    h = mex("create", 0.0)
    try:
        with pytest.raises(MexError, match="swrt_omega_series_record.*begin"):
            mex("omega_series_record", h, nlhs=0)
        fields = [planes[i].reshape((nx, nx), order="F") for i in range(6)]
        mex("set_field_grid", h, 0.0, *fields, L, float(nx), nlhs=0)
        mex("packets_set", h, x, k, nlhs=0)
        mex("omega_series_begin", h, F, CG, edges.reshape(1, -1), nlhs=0)
        mex("omega_series_record", h, nlhs=0)
        mex("advance", h, dt, float(steps), F, CG ** 2, 1.0, 0.0, 0.0, orc.BUMP_QG, nlhs=0)
        mex("omega_series_record", h, nlhs=0)
        mc, ms = mex("omega_series_get", h, nlhs=2)
        assert mc.shape == (32, 2) and ms.shape == (4, 2) and mc.dtype == np.float64
        np.testing.assert_array_equal(mc.T, counts[:2])
        np.testing.assert_array_equal(ms.T, stats[:2])
        # the gateway's advance saves no history: record_history refuses the range
        with pytest.raises(MexError, match="swrt_omega_series_record_history.*history"):
            mex("omega_series_record_history", h, 1.0, 4.0, nlhs=0)
        # frames from ode23_ntrp's history instead: the same rows as a record_history on the Context
        mex("omega_series_reset", h, nlhs=0)
        assert mex("omega_series_get", h).shape == (32, 0)
        mex("packets_set", h, x, k, nlhs=0)
        mex("history_reset", h, nlhs=0)
        mex("ode23_set_dense", h, 1.0, nlhs=0)
        mex("ode23_f1", h, 0.0, 0.0, F, CG, 1.0, 1e-3, orc.BUMP_QG)
        mex("ode23_attempt", h, 0.0, 0.02, 0.02, 0.0, F, CG, 1.0, 1e-3, orc.BUMP_QG)
        mex("ode23_ntrp", h, 0.0, 0.02, np.array([[0.005, 0.01, 0.02]]), nlhs=0)
        mex("ode23_accept", h, nlhs=0)
        mex("ode23_set_dense", h, 0.0, nlhs=0)
        hx, hk = mex("history", h, nlhs=2)
        assert hk.shape == (1000, 2, 3)
        mex("omega_series_record_history", h, 0.0, 3.0, nlhs=0)
        mc, ms = mex("omega_series_get", h, nlhs=2)
        assert mc.shape == (32, 3)
        for i in range(3):
            c.packets_set(hx[:, :, i], hk[:, :, i])
            c.omega_series_reset()
            c.omega_series_record()
            ci, si = c.omega_series()
            np.testing.assert_array_equal(mc[:, i], ci[0])
            np.testing.assert_array_equal(ms[:, i], si[0])
        mi = mex("omega_ideal", h, 0.0, ring, omega0, iedges.reshape(1, -1))
        assert mi.shape == (8, 1)
        np.testing.assert_array_equal(mi[:, 0], ideal)
        with pytest.raises(MexError, match="ring must be m x 2"):
            mex("omega_ideal", h, 0.0, ring.T, omega0, iedges.reshape(1, -1))
        with pytest.raises(MexError, match="swrt_omega_series_begin.*nbins"):
            mex("omega_series_begin", h, F, CG, np.array([[3.0]]), nlhs=0)
    finally:
        mex("destroy", h, nlhs=0)
