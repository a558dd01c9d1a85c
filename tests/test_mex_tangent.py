"""The tangent map commands of the MEX gateway (matlab/swrt_mex.cpp:
tangent_begin / _mark / _get / _end and tangent_series_begin / _record /
_frames / _get / _reset), driven through the test mex.h shim as
test_mex_absfreq_series.py drives the absolute-frequency series': M (16 x n
doubles), the counters and the int64 frames MATLAB gets hold what the Python
Context gives for the same calls, and a refused call becomes a MATLAB error."""
import numpy as np
import pytest

from oracle import cbind, swrt_oracle as orc
from tests.cond_series_ref import central_edges, omega_of
from tests.test_mex_gateway import Mex, MexError

BUMP = orc.BUMP_QG


@pytest.fixture(scope="module")
def mex():
    return Mex()


def _i64(a):
    return a.view(np.int64)  # (the same 8-byte words, any layout)


@pytest.mark.gpu
def test_gateway_tangents_equal_the_context(mex, fresh_ctx, qg_case):
    q = qg_case
    nx, L, F, CG = q["nx"], q["L"], q["f"], q["Cg"]
    n, ns, nw = 257, 4, 7
    rng = np.random.default_rng(43)
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th, r = rng.uniform(0, 2 * np.pi, n), 6.0 + 9.0 * rng.random(n)
    k = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    planes = cbind.planes_of(q["flow"])
    wedges = central_edges(omega_of(k, F, CG), nw)
    gedges = 2.0 ** np.arange(ns + 1)
    dt, steps = q["dt"], 12
    # the Context
    c = fresh_ctx
    c.set_field_grid(0, planes, nx, L)
    c.packets_set(x, k)
    c.tangent_begin()
    c.tangent_series_begin(F, CG, wedges, gedges)
    c.tangent_series_record()
    c.advance(dt, steps, F, CG ** 2, bump=BUMP)
    c.tangent_series_record()
    cM, ccaus = c.tangent_get()
    c.tangent_mark()
    c.tangent_series_record()
    cc, cu, cs = c.tangent_series_get()
    assert cs[:, 2].tolist() == [1, 1, 2] and not np.array_equal(cc[0], cc[1])
    # the gateway
    h = mex("create", 0.0)
    try:
        with pytest.raises(MexError, match="swrt_tangent_series_record.*begin"):
            mex("tangent_series_record", h, nlhs=0)
        with pytest.raises(MexError, match="swrt_tangent_get.*swrt_tangent_begin"):
            mex("tangent_get", h, nlhs=2)
        fields = [np.asarray(planes[i]).reshape((nx, nx), order="F") for i in range(6)]
        mex("set_field_grid", h, 0.0, *fields, L, float(nx), nlhs=0)
        mex("packets_set", h, x, k, nlhs=0)
        mex("tangent_begin", h, nlhs=0)
        mex("tangent_series_begin", h, F, CG, wedges[None, :], gedges[None, :], nlhs=0)
        assert mex("tangent_series_frames", h) == 0
        mex("tangent_series_record", h, nlhs=0)
        mex("advance", h, dt, float(steps), F, CG ** 2, 1.0, 0.0, 0.0, BUMP, nlhs=0)
        mex("tangent_series_record", h, nlhs=0)
        mM, mcaus = mex("tangent_get", h, nlhs=2)
        assert mM.shape == (16, n) and mcaus.shape == (n, 1)
        assert np.array_equal(np.asarray(mM).T, cM) and np.array_equal(_i64(mcaus).ravel(), ccaus)
        mex("tangent_mark", h, nlhs=0)
        mex("tangent_series_record", h, nlhs=0)
        assert mex("tangent_series_frames", h) == 3
        mc, mu, ms = mex("tangent_series_get", h, nlhs=3)
        nsum = 3 * (nw + 2) + ns + 2
        assert mc.shape == (nw + 2, ns + 2, 3) and mu.shape == (nsum, 3) and ms.shape == (3, 3)
        np.testing.assert_array_equal(_i64(mc).transpose(2, 1, 0), cc)  # (MATLAB's first index is the omega class)
        np.testing.assert_array_equal(_i64(mu).T, cu)
        np.testing.assert_array_equal(_i64(ms).T, cs)
        mex("tangent_series_reset", h, nlhs=0)
        assert mex("tangent_series_frames", h) == 0
        assert mex("tangent_series_get", h).shape == (nw + 2, ns + 2, 0)
        # refused calls and bad arguments become MATLAB errors
        with pytest.raises(MexError, match="swrt_recycle_apply.*tangent set is live"):
            mex("recycle_apply", h, nlhs=0)
        with pytest.raises(MexError, match="swrt_tangent_series_begin.*increase"):
            mex("tangent_series_begin", h, F, CG, wedges[None, ::-1].copy(), gedges[None, :], nlhs=0)
        with pytest.raises(MexError):
            mex("tangent_series_begin", h, F, CG, nlhs=0)  # too few arguments
        mex("tangent_end", h, nlhs=0)
        with pytest.raises(MexError, match="swrt_tangent_mark.*swrt_tangent_begin"):
            mex("tangent_mark", h, nlhs=0)
    finally:
        mex("destroy", h, nlhs=0)
