"""The map-series commands of the MEX gateway (matlab/swrt_mex.cpp:
map_series_begin / _record / _record_history / _get / _reset), driven through
the test mex.h shim as test_mex_omega_series.py drives the spectrum's: the
arrays MATLAB gets — planes as a double m x m x 4 x frames array, stats
2 x frames — are the arrays the Python Context gives for the same calls, and
those are the restatement's (tests/map_series_ref.py)."""
import numpy as np
import pytest

from oracle import swrt_oracle as orc
from tests.map_series_ref import map_frame
from tests.test_mex_gateway import Mex, MexError

F, CG = 3.0, 1.0


@pytest.fixture(scope="module")
def mex():
    return Mex()


@pytest.mark.gpu
def test_gateway_maps_equal_the_context(mex, fresh_ctx):
    nx, L, n, m = 64, 2 * np.pi, 1000, 16
    rng = np.random.default_rng(31)
    planes = 0.2 * rng.standard_normal((6, nx * nx))
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th, r = rng.uniform(0, 2 * np.pi, n), 6.0 * rng.random(n)
    k = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    dt, steps = 0.05, 6
    # the Context
    c = fresh_ctx
    c.set_field_grid(0, planes, nx, L)
    c.packets_set(x, k)
    c.map_series_begin(L, m, F, CG)
    c.map_series_record()
    c.advance(dt, steps, F, CG ** 2, bump=orc.BUMP_QG)
    c.map_series_record()
    cp, cs = c.map_series()
    want, _ = map_frame(x, k, L, m, F, CG)
    np.testing.assert_array_equal(cp[0], want)
    assert not np.array_equal(cp[0], cp[1])
    # the gateway
    h = mex("create", 0.0)
    try:
        with pytest.raises(MexError, match="swrt_map_series_record.*begin"):
            mex("map_series_record", h, nlhs=0)
        fields = [planes[i].reshape((nx, nx), order="F") for i in range(6)]
        mex("set_field_grid", h, 0.0, *fields, L, float(nx), nlhs=0)
        mex("packets_set", h, x, k, nlhs=0)
        mex("map_series_begin", h, L, float(m), F, CG, nlhs=0)  # frac_bits: the default 20
        mex("map_series_record", h, nlhs=0)
        mex("advance", h, dt, float(steps), F, CG ** 2, 1.0, 0.0, 0.0, orc.BUMP_QG, nlhs=0)
        mex("map_series_record", h, nlhs=0)
        mp, ms = mex("map_series_get", h, nlhs=2)
        assert mp.shape == (m, m, 4, 2) and ms.shape == (2, 2) and mp.dtype == np.float64
        np.testing.assert_array_equal(mp.transpose(3, 2, 0, 1), cp)  # (MATLAB's first index is x as well)
        np.testing.assert_array_equal(ms.T, cs)
        # the gateway's advance saves no history: record_history refuses the range
        with pytest.raises(MexError, match="swrt_map_series_record_history.*history"):
            mex("map_series_record_history", h, 1.0, 4.0, nlhs=0)
        mex("map_series_reset", h, nlhs=0)
        assert mex("map_series_get", h).shape == (m, m, 4, 0)
        # frames from ode23_ntrp's history: the same planes as a record on the Context set to each frame
        mex("packets_set", h, x, k, nlhs=0)
        mex("history_reset", h, nlhs=0)
        mex("ode23_set_dense", h, 1.0, nlhs=0)
        mex("ode23_f1", h, 0.0, 0.0, F, CG, 1.0, 1e-3, orc.BUMP_QG)
        mex("ode23_attempt", h, 0.0, 0.02, 0.02, 0.0, F, CG, 1.0, 1e-3, orc.BUMP_QG)
        mex("ode23_ntrp", h, 0.0, 0.02, np.array([[0.005, 0.01, 0.02]]), nlhs=0)
        mex("ode23_accept", h, nlhs=0)
        mex("ode23_set_dense", h, 0.0, nlhs=0)
        hx, hk = mex("history", h, nlhs=2)
        assert hk.shape == (n, 2, 3)
        mex("map_series_begin", h, L, float(m), F, CG, 12.0, nlhs=0)
        mex("map_series_record_history", h, 0.0, 3.0, nlhs=0)
        mp, ms = mex("map_series_get", h, nlhs=2)
        assert mp.shape == (m, m, 4, 3)
        c.map_series_begin(L, m, F, CG, 12)
        for i in range(3):
            c.packets_set(hx[:, :, i], hk[:, :, i])
            c.map_series_reset()
            c.map_series_record()
            pi, si = c.map_series()
            np.testing.assert_array_equal(mp[:, :, :, i].transpose(2, 0, 1), pi[0])
            np.testing.assert_array_equal(ms[:, i], si[0])
        with pytest.raises(MexError, match="swrt_map_series_begin.*m must be"):
            mex("map_series_begin", h, L, 0.0, F, CG, nlhs=0)
    finally:
        mex("destroy", h, nlhs=0)
