"""The wave-vector plane commands of the MEX gateway (matlab/swrt_mex.cpp:
kmap_series_begin / _record / _record_history / _frames / _get / _reset),
driven through the test mex.h shim as test_mex_map_series.py drives the map
series': the int64 arrays MATLAB gets — planes m x m x frames, stats
8 x frames — hold the integers the Python Context gives for the same calls,
and those are the restatement's (tests/kmap_series_ref.py).  The shim's
arrays are untyped 8-byte words (tests/mex_shim/mex_int64.h gives the gateway's
test build mxINT64_CLASS and mxGetInt64s over them): the test views the words
it gets back as int64."""
import numpy as np
import pytest

from oracle import swrt_oracle as orc
from tests.kmap_series_ref import kmap_frame
from tests.test_mex_gateway import Mex, MexError

F, CG = 3.0, 1.0


@pytest.fixture(scope="module")
def mex():
    return Mex()


def _i64(a):
    return a.view(np.int64)  # (the same 8-byte words, any layout)


@pytest.mark.gpu
def test_gateway_kmaps_equal_the_context(mex, fresh_ctx):
    nx, L, n, m, K = 64, 2 * np.pi, 257, 7, 8.0
    rng = np.random.default_rng(31)
    planes = 0.2 * rng.standard_normal((6, nx * nx))
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th, r = rng.uniform(0, 2 * np.pi, n), 9.0 * rng.random(n)
    k = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    dt, steps = 0.05, 6
    # the Context
    c = fresh_ctx
    c.set_field_grid(0, planes, nx, L)
    c.packets_set(x, k)
    c.kmap_series_begin(K, m)
    c.kmap_series_record()
    c.advance(dt, steps, F, CG ** 2, bump=orc.BUMP_QG)
    c.kmap_series_record()
    cp, cs = c.kmap_series_get()
    want_p, want_s = kmap_frame(k, K, m)
    np.testing.assert_array_equal(cp[0], want_p)
    np.testing.assert_array_equal(cs[0], want_s)
    assert want_s[2] > 0 and not np.array_equal(cs[0], cs[1])
    # the gateway
    h = mex("create", 0.0)
    try:
        with pytest.raises(MexError, match="swrt_kmap_series_record.*begin"):
            mex("kmap_series_record", h, nlhs=0)
        fields = [planes[i].reshape((nx, nx), order="F") for i in range(6)]
        mex("set_field_grid", h, 0.0, *fields, L, float(nx), nlhs=0)
        mex("packets_set", h, x, k, nlhs=0)
        mex("kmap_series_begin", h, K, float(m), nlhs=0)  # frac_bits: the default 16
        assert mex("kmap_series_frames", h) == 0
        mex("kmap_series_record", h, nlhs=0)
        mex("advance", h, dt, float(steps), F, CG ** 2, 1.0, 0.0, 0.0, orc.BUMP_QG, nlhs=0)
        mex("kmap_series_record", h, nlhs=0)
        assert mex("kmap_series_frames", h) == 2
        mp, ms = mex("kmap_series_get", h, nlhs=2)
        assert mp.shape == (m, m, 2) and ms.shape == (8, 2)
        mp, ms = _i64(mp), _i64(ms)
        np.testing.assert_array_equal(mp.transpose(2, 0, 1), cp)  # (MATLAB's first index is k as well)
        np.testing.assert_array_equal(ms.T, cs)
        # the gateway's advance saves no history: record_history refuses the range
        with pytest.raises(MexError, match="swrt_kmap_series_record_history.*history"):
            mex("kmap_series_record_history", h, 1.0, 4.0, nlhs=0)
        mex("kmap_series_reset", h, nlhs=0)
        assert mex("kmap_series_frames", h) == 0
        assert mex("kmap_series_get", h).shape == (m, m, 0)
        # frames from ode23_ntrp's history: the same integers as a record on the Context set to each frame
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
        mex("kmap_series_begin", h, K, float(m), 12.0, nlhs=0)
        mex("kmap_series_record_history", h, 0.0, 3.0, nlhs=0)
        mp, ms = mex("kmap_series_get", h, nlhs=2)
        assert mp.shape == (m, m, 3)
        mp, ms = _i64(mp), _i64(ms)
        c.kmap_series_begin(K, m, 12)
        for i in range(3):
            c.packets_set(hx[:, :, i], hk[:, :, i])
            c.kmap_series_reset()
            c.kmap_series_record()
            pi, si = c.kmap_series_get()
            np.testing.assert_array_equal(mp[:, :, i], pi[0])
            np.testing.assert_array_equal(ms[:, i], si[0])
            np.testing.assert_array_equal(pi[0], kmap_frame(hk[:, :, i], K, m, 12)[0])
        with pytest.raises(MexError, match="swrt_kmap_series_begin.*m must be"):
            mex("kmap_series_begin", h, K, 0.0, nlhs=0)
    finally:
        mex("destroy", h, nlhs=0)
