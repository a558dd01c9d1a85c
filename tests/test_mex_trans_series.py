"""The transition series commands of the MEX gateway (matlab/swrt_mex.cpp:
trans_series_begin / _mark / _mark_values / _record / _record_history /
_frames / _get / _reset), driven through the test mex.h shim as
test_mex_cond_series.py drives the conditional series': the int64 arrays
MATLAB gets — counts (nw + 2) x (ns + 2) x frames, sums 3 x (ns + 2) x frames,
stats 3 x frames — hold the integers the Python Context gives for the same
calls, and a bad argument becomes a MATLAB error.  The shim's arrays are
untyped 8-byte words (tests/mex_shim/mex_int64.h): the test views the words it
gets back as int64."""
import numpy as np
import pytest

from oracle import cbind, swrt_oracle as orc
from tests.cond_series_ref import quantile_edges
from tests.test_mex_gateway import Mex, MexError
from tests.trans_series_ref import omega_of, trans_frame_of

BUMP = orc.BUMP_QG


@pytest.fixture(scope="module")
def mex():
    return Mex()


def _i64(a):
    return a.view(np.int64)  # (the same 8-byte words, any layout)


@pytest.mark.gpu
def test_gateway_transitions_equal_the_context(mex, fresh_ctx, qg_case):
    q = qg_case
    nx, L, F, CG = q["nx"], q["L"], q["f"], q["Cg"]
    n, ns, nw, fb = 257, 4, 7, 12
    rng = np.random.default_rng(44)
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th, r = rng.uniform(0, 2 * np.pi, n), 6.0 + 9.0 * rng.random(n)
    k = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    k[7] = [1e9, 0.0]  # beyond 2^38 quanta: rejected (finite, so its position stays finite through the advance)
    planes = cbind.planes_of(q["flow"])
    w = omega_of(k, F, CG)
    src = w * (1.0 + 0.3 * rng.standard_normal(n))
    src[9] = np.nan
    wedges, sedges = quantile_edges(w[w < 1e6], nw), quantile_edges(src, ns)
    dt, steps = q["dt"], 6
    # the Context: a frame against given values, a mark, an advance, a frame against the mark
    c = fresh_ctx
    c.set_field_grid(0, planes, nx, L)
    c.packets_set(x, k)
    c.trans_series_begin(F, CG, wedges, sedges, fb)
    c.trans_series_mark_values(src)
    c.trans_series_record()
    c.trans_series_mark()
    c.advance(dt, steps, F, CG ** 2, bump=BUMP)
    c.trans_series_record()
    cc, cu, cs = c.trans_series_get()
    want = trans_frame_of(src, w, wedges, sedges, fb)
    for got, v in zip((cc[0], cu[0], cs[0]), want):
        np.testing.assert_array_equal(got, v)
    assert want[2].tolist() == [n, 2, 1] and np.count_nonzero(want[0].sum(axis=1)) == ns + 2
    assert cs[1].tolist() == [n, 1, 2] and not np.array_equal(cc[0], cc[1])
    # the gateway
    h = mex("create", 0.0)
    try:
        with pytest.raises(MexError, match="swrt_trans_series_record.*begin"):
            mex("trans_series_record", h, nlhs=0)
        fields = [np.asarray(planes[i]).reshape((nx, nx), order="F") for i in range(6)]
        mex("set_field_grid", h, 0.0, *fields, L, float(nx), nlhs=0)
        mex("packets_set", h, x, k, nlhs=0)
        mex("trans_series_begin", h, F, CG, wedges[None, :], sedges[None, :], float(fb), nlhs=0)
        assert mex("trans_series_frames", h) == 0
        with pytest.raises(MexError, match="swrt_trans_series_record.*mark"):
            mex("trans_series_record", h, nlhs=0)
        mex("trans_series_mark_values", h, src[:, None], nlhs=0)
        mex("trans_series_record", h, nlhs=0)
        mex("trans_series_mark", h, nlhs=0)
        mex("advance", h, dt, float(steps), F, CG ** 2, 1.0, 0.0, 0.0, BUMP, nlhs=0)
        mex("trans_series_record", h, nlhs=0)
        assert mex("trans_series_frames", h) == 2
        mc, mu, ms = mex("trans_series_get", h, nlhs=3)
        assert mc.shape == (nw + 2, ns + 2, 2) and mu.shape == (3, ns + 2, 2) and ms.shape == (3, 2)
        mc, mu, ms = _i64(mc), _i64(mu), _i64(ms)
        np.testing.assert_array_equal(mc.transpose(2, 1, 0), cc)  # (MATLAB's first index is the omega class)
        np.testing.assert_array_equal(mu.transpose(2, 1, 0), cu)
        np.testing.assert_array_equal(ms.T, cs)
        # the gateway's advance saves no history: record_history refuses the range
        with pytest.raises(MexError, match="swrt_trans_series_record_history.*history"):
            mex("trans_series_record_history", h, 1.0, 4.0, nlhs=0)
        mex("trans_series_reset", h, nlhs=0)
        assert mex("trans_series_frames", h) == 0
        assert mex("trans_series_get", h).shape == (nw + 2, ns + 2, 0)
        mex("trans_series_record", h, nlhs=0)  # the mark stays
        assert mex("trans_series_frames", h) == 1
        # bad arguments become MATLAB errors
        with pytest.raises(MexError, match="swrt_trans_series_mark_values.*packet count"):
            mex("trans_series_mark_values", h, src[:100, None], nlhs=0)
        with pytest.raises(MexError, match="swrt_trans_series_begin.*increase"):
            mex("trans_series_begin", h, F, CG, wedges[None, ::-1].copy(), sedges[None, :], nlhs=0)
        with pytest.raises(MexError, match="swrt_trans_series_begin.*nbins"):
            mex("trans_series_begin", h, F, CG, wedges[None, :], sedges[None, :1], nlhs=0)
        with pytest.raises(MexError):
            mex("trans_series_begin", h, F, CG, nlhs=0)  # too few arguments
    finally:
        mex("destroy", h, nlhs=0)
