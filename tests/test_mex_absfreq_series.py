"""The absolute-frequency series commands of the MEX gateway
(matlab/swrt_mex.cpp: absfreq_series_begin / _record / _record_history /
_frames / _get / _reset), driven through the test mex.h shim as
test_mex_refr_series.py drives the refraction series': the int64 arrays MATLAB
gets — counts (nw + 2) x (no + 2) x frames, sums (3 (nw + 2) + 2 (no + 2)) x
frames, stats 2 x frames — hold the integers the Python Context gives for the
same calls, and a bad argument becomes a MATLAB error.  The shim's arrays are
untyped 8-byte words (tests/mex_shim/mex_int64.h): the test views the words it
gets back as int64."""
import numpy as np
import pytest

from oracle import cbind, swrt_oracle as orc
from tests.absfreq_series_ref import absfreq_frame
from tests.cond_series_ref import central_edges, omega_of
from tests.test_mex_gateway import Mex, MexError

BUMP = orc.BUMP_QG
TAU = 0.37


@pytest.fixture(scope="module")
def mex():
    return Mex()


def _i64(a):
    return a.view(np.int64)  # (the same 8-byte words, any layout)


@pytest.mark.gpu
def test_gateway_absfreqs_equal_the_context(mex, fresh_ctx, qg_case):
    q = qg_case
    nx, L, F, CG = q["nx"], q["L"], q["f"], q["Cg"]
    n, no, nw, fb = 257, 4, 7, 12
    rng = np.random.default_rng(42)
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th, r = rng.uniform(0, 2 * np.pi, n), 6.0 + 9.0 * rng.random(n)
    k = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    k[7] = [1e9, 0.0]  # beyond 2^38 quanta: rejected (finite, so its position stays finite through the advance)
    planes = cbind.planes_of(q["flow"])
    w = omega_of(k, F, CG)
    wedges = central_edges(w[w < 1e6], nw)
    oedges = central_edges(w[w < 1e6] + 0.5, no)
    dt, steps = q["dt"], 6
    # the Context
    c = fresh_ctx
    c.set_field_grid(0, planes, nx, L)
    c.set_field_grid(1, 0.8 * np.asarray(planes), nx, L)
    c.packets_set(x, k)
    c.absfreq_series_begin(F, CG, wedges, oedges, fb)
    c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
    c.advance(dt, steps, F, CG ** 2, bump=BUMP)
    c.absfreq_series_record(1, 0, 0.3, -TAU, BUMP)
    c.absfreq_series_record(1, -1, 0.0, 0.0, BUMP)
    cc, cu, cs = c.absfreq_series_get()
    A = np.array(c.eval(x[:, 0], x[:, 1], nslots=1, bump=BUMP)[:2])
    c.swap_slots(0, 1)
    B = np.array(c.eval(x[:, 0], x[:, 1], nslots=1, bump=BUMP)[:2])
    c.swap_slots(0, 1)
    want = absfreq_frame(A, B, 0.3, TAU, k, F, CG, wedges, oedges, fb)
    for got, w_ in zip((cc[0], cu[0], cs[0]), want):
        np.testing.assert_array_equal(got, w_)
    assert want[2].tolist() == [n, 1] and np.count_nonzero(want[0].sum(axis=1)) == no + 2
    assert not np.array_equal(cu[0], cu[1]) and cu[0][:nw + 2].any() and not cu[2][:nw + 2].any()
    # the gateway
    h = mex("create", 0.0)
    try:
        with pytest.raises(MexError, match="swrt_absfreq_series_record.*begin"):
            mex("absfreq_series_record", h, 0.0, 1.0, 0.3, TAU, BUMP, nlhs=0)
        fields = [np.asarray(planes[i]).reshape((nx, nx), order="F") for i in range(6)]
        mex("set_field_grid", h, 0.0, *fields, L, float(nx), nlhs=0)
        mex("set_field_grid", h, 1.0, *[0.8 * f for f in fields], L, float(nx), nlhs=0)
        mex("packets_set", h, x, k, nlhs=0)
        mex("absfreq_series_begin", h, F, CG, wedges[None, :], oedges[None, :], float(fb), nlhs=0)
        assert mex("absfreq_series_frames", h) == 0
        mex("absfreq_series_record", h, 0.0, 1.0, 0.3, TAU, BUMP, nlhs=0)
        mex("advance", h, dt, float(steps), F, CG ** 2, 1.0, 0.0, 0.0, BUMP, nlhs=0)
        mex("absfreq_series_record", h, 1.0, 0.0, 0.3, -TAU, BUMP, nlhs=0)
        mex("absfreq_series_record", h, 1.0, -1.0, 0.0, 0.0, BUMP, nlhs=0)
        assert mex("absfreq_series_frames", h) == 3
        mc, mu, ms = mex("absfreq_series_get", h, nlhs=3)
        nsum = 3 * (nw + 2) + 2 * (no + 2)
        assert mc.shape == (nw + 2, no + 2, 3) and mu.shape == (nsum, 3) and ms.shape == (2, 3)
        mc, mu, ms = _i64(mc), _i64(mu), _i64(ms)
        np.testing.assert_array_equal(mc.transpose(2, 1, 0), cc)  # (MATLAB's first index is the omega class)
        np.testing.assert_array_equal(mu.T, cu)
        np.testing.assert_array_equal(ms.T, cs)
        # the gateway's advance saves no history: record_history refuses the range
        with pytest.raises(MexError, match="swrt_absfreq_series_record_history.*history"):
            mex("absfreq_series_record_history", h, 1.0, 4.0, 0.0, -1.0, np.zeros((0, 0)), TAU, BUMP, nlhs=0)
        with pytest.raises(MexError, match="alphas must hold one value per frame"):
            mex("absfreq_series_record_history", h, 0.0, 3.0, 0.0, 1.0, np.array([[0.1, 0.2]]), TAU, BUMP, nlhs=0)
        mex("absfreq_series_reset", h, nlhs=0)
        assert mex("absfreq_series_frames", h) == 0
        assert mex("absfreq_series_get", h).shape == (nw + 2, no + 2, 0)
        # the default frac_bits is 20
        mex("absfreq_series_begin", h, F, CG, wedges[None, :], oedges[None, :], nlhs=0)
        mex("absfreq_series_record", h, 0.0, 1.0, 0.3, TAU, BUMP, nlhs=0)
        c.absfreq_series_begin(F, CG, wedges, oedges)
        c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
        np.testing.assert_array_equal(_i64(mex("absfreq_series_get", h, nlhs=2)[1]).T, c.absfreq_series_get()[1])
        # bad arguments become MATLAB errors
        with pytest.raises(MexError, match="swrt_absfreq_series_record.*differ"):
            mex("absfreq_series_record", h, 1.0, 1.0, 0.3, TAU, BUMP, nlhs=0)
        with pytest.raises(MexError, match="swrt_absfreq_series_record.*tau"):
            mex("absfreq_series_record", h, 0.0, 1.0, 0.3, 0.0, BUMP, nlhs=0)
        with pytest.raises(MexError, match="swrt_absfreq_series_begin.*increase"):
            mex("absfreq_series_begin", h, F, CG, wedges[None, ::-1].copy(), oedges[None, :], nlhs=0)
        with pytest.raises(MexError, match="swrt_absfreq_series_begin.*nbins"):
            mex("absfreq_series_begin", h, F, CG, wedges[None, :], oedges[None, :1], nlhs=0)
        with pytest.raises(MexError):
            mex("absfreq_series_begin", h, F, CG, nlhs=0)  # too few arguments
    finally:
        mex("destroy", h, nlhs=0)
