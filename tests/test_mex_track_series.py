"""The track-series commands of the MEX gateway (matlab/swrt_mex.cpp:
track_begin / _record / _record_history / _get / _reset), driven through the
test mex.h shim as test_mex_map_series.py drives the maps': the array MATLAB
gets — m x 8 x frames, row j the packet ids(j) — is the Python Context's
series for the same calls, transposed, bit for bit."""
import numpy as np
import pytest

from oracle import swrt_oracle as orc
from tests.test_mex_gateway import Mex, MexError

F, CG = 3.0, 1.0


@pytest.fixture(scope="module")
def mex():
    return Mex()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
def test_gateway_tracks_equal_the_context(mex, fresh_ctx):
    nx, L, n = 64, 2 * np.pi, 1000
    ids = [999, 0, 517, 64, 63]
    rng = np.random.default_rng(31)
    planes = 0.2 * rng.standard_normal((6, nx * nx))
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th = rng.uniform(0, 2 * np.pi, n)
    k = 3.0 * np.stack([np.cos(th), np.sin(th)], axis=1)
    dt, steps = 0.05, 6
    # the Context
    c = fresh_ctx
    c.set_field_grid(0, planes, nx, L)
    c.packets_set(x, k)
    c.track_begin(ids)
    c.track_record(F, CG ** 2, nslots=0)
    c.track_record(F, CG ** 2, nslots=1, bump=orc.BUMP_QG)
    c.advance(dt, steps, F, CG ** 2, bump=orc.BUMP_QG)
    c.track_record(F, CG ** 2, nslots=1, bump=orc.BUMP_QG)
    cs = c.track_series()
    assert cs.shape == (3, 8, 5) and not np.array_equal(cs[1], cs[2])
    # the gateway
    h = mex("create", 0.0)
    try:
        with pytest.raises(MexError, match="swrt_track_record.*call swrt_track_begin first"):
            mex("track_record", h, F, CG ** 2, 0.0, 0.0, orc.BUMP_QG, nlhs=0)
        fields = [planes[i].reshape((nx, nx), order="F") for i in range(6)]
        mex("set_field_grid", h, 0.0, *fields, L, float(nx), nlhs=0)
        mex("packets_set", h, x, k, nlhs=0)
        mex("track_begin", h, np.array([[float(i) for i in ids]]), nlhs=0)  # 0-based, as doubles
        mex("track_record", h, F, CG ** 2, 0.0, 0.0, orc.BUMP_QG, nlhs=0)
        mex("track_record", h, F, CG ** 2, 1.0, 0.0, orc.BUMP_QG, nlhs=0)
        mex("advance", h, dt, float(steps), F, CG ** 2, 1.0, 0.0, 0.0, orc.BUMP_QG, nlhs=0)
        mex("track_record", h, F, CG ** 2, 1.0, 0.0, orc.BUMP_QG, nlhs=0)
        mt = mex("track_get", h)
        assert mt.shape == (5, 8, 3) and mt.dtype == np.float64
        np.testing.assert_array_equal(_bits(mt.transpose(2, 1, 0)), _bits(cs))
        with pytest.raises(MexError, match="swrt_track_begin.*given twice"):
            mex("track_begin", h, np.array([[3.0, 7.0, 3.0]]), nlhs=0)
        with pytest.raises(MexError, match="whole numbers"):
            mex("track_begin", h, np.array([[1.5]]), nlhs=0)
        # the gateway's advance saves no history: record_history refuses the range
        with pytest.raises(MexError, match="swrt_track_record_history.*history"):
            mex("track_record_history", h, 1.0, 4.0, F, CG ** 2, 1.0, np.zeros((0, 0)), orc.BUMP_QG, nlhs=0)
        mex("track_reset", h, nlhs=0)
        assert mex("track_get", h).shape == (5, 8, 0)
        # frames from ode23_ntrp's history: the same rows as a record on the Context set to each frame
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
        mex("track_record_history", h, 0.0, 3.0, F, CG ** 2, 1.0, np.zeros((0, 0)), orc.BUMP_QG, nlhs=0)
        mt = mex("track_get", h)
        assert mt.shape == (5, 8, 3)
        c.track_reset()
        for i in range(3):
            c.packets_set(hx[:, :, i], hk[:, :, i])  # (the same N: the ids stay)
            c.track_record(F, CG ** 2, nslots=1, bump=orc.BUMP_QG)
        np.testing.assert_array_equal(_bits(mt.transpose(2, 1, 0)), _bits(c.track_series()))
        assert not np.array_equal(mt[:, :, 0], mt[:, :, 2])
    finally:
        mex("destroy", h, nlhs=0)
