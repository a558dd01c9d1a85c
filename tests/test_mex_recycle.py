"""The recycle commands of the MEX gateway (matlab/swrt_mex.cpp: recycle_begin
/ _apply / _frames / _get / _state / _reset / _end), driven through the test
mex.h shim as test_mex_trans_series.py drives the transition series': the
int64 arrays MATLAB gets — the frames 8 x events, gen and born n x 1 — hold
the integers the Python Context gives for the same calls, the packets are the
same bits, and a bad argument becomes a MATLAB error.  The shim's arrays are
untyped 8-byte words (tests/mex_shim/mex_int64.h): the test views the words it
gets back as int64."""
import numpy as np
import pytest

from oracle import cbind, swrt_oracle as orc
from tests.recycle_ref import omega_of, recycle_event
from tests.test_mex_gateway import Mex, MexError

BUMP = orc.BUMP_QG


@pytest.fixture(scope="module")
def mex():
    return Mex()


def _i64(a):
    return a.view(np.int64)  # (the same 8-byte words, any layout)


@pytest.mark.gpu
def test_gateway_recycling_equals_the_context(mex, fresh_ctx, qg_case):
    q = qg_case
    nx, L, F, CG = q["nx"], q["L"], q["f"], q["Cg"]
    n, fb, seed, base = 257, 12, 77, 300
    rng = np.random.default_rng(45)
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th, r = rng.uniform(0, 2 * np.pi, n), 6.0 + 9.0 * rng.random(n)
    k = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    k[7] = [1e9, 0.0]  # beyond 2^38 quanta: rejected (finite, so its position stays finite through the advance)
    home = 0.4 * k
    home[7] = [1.0, 1.0]
    cut = float(np.percentile(omega_of(k, F, CG), 60))
    planes = cbind.planes_of(q["flow"])
    dt, steps = q["dt"], 6
    # the Context: an event on the given packets, an advance, another event
    c = fresh_ctx
    c.set_field_grid(0, planes, nx, L)
    c.packets_set(x, k)
    c.recycle_begin(F, CG, cut, L, seed=seed, index_base=base, frac_bits=fb, home_k=home)
    c.recycle_apply()
    zeros = np.zeros(n, dtype=np.int32)
    want = recycle_event(x, k, home, zeros, zeros, 1, F, CG, cut, L, seed, base, fb)
    assert 50 < want[4][1] < 200 and want[4][2] == 1
    np.testing.assert_array_equal(c.recycle_get()[0], want[4])
    c.advance(dt, steps, F, CG ** 2, bump=BUMP)
    c.recycle_apply()
    cs = c.recycle_get()
    cgen, cborn = c.recycle_state()
    cx, ck = c.packets_get()
    assert cs.shape == (2, 8) and cs[1, 7] == 2 and cgen.sum() == cs[:, 1].sum()
    # the gateway
    h = mex("create", 0.0)
    try:
        with pytest.raises(MexError, match="swrt_recycle_apply.*begin"):
            mex("recycle_apply", h, nlhs=0)
        with pytest.raises(MexError, match="swrt_recycle_get.*begin"):
            mex("recycle_get", h)
        fields = [np.asarray(planes[i]).reshape((nx, nx), order="F") for i in range(6)]
        mex("set_field_grid", h, 0.0, *fields, L, float(nx), nlhs=0)
        mex("packets_set", h, x, k, nlhs=0)
        mex("recycle_begin", h, F, CG, cut, L, float(seed), float(base), float(fb), home, nlhs=0)
        assert mex("recycle_frames", h) == 0 and mex("recycle_get", h).shape == (8, 0)
        mex("recycle_apply", h, nlhs=0)
        mex("advance", h, dt, float(steps), F, CG ** 2, 1.0, 0.0, 0.0, BUMP, nlhs=0)
        mex("recycle_apply", h, nlhs=0)
        assert mex("recycle_frames", h) == 2
        ms = mex("recycle_get", h)
        assert ms.shape == (8, 2)
        np.testing.assert_array_equal(_i64(ms).T, cs)
        mgen, mborn = mex("recycle_state", h, nlhs=2)
        assert mgen.shape == (n, 1) and mborn.shape == (n, 1)
        np.testing.assert_array_equal(_i64(mgen)[:, 0], cgen)
        np.testing.assert_array_equal(_i64(mborn)[:, 0], cborn)
        mx, mk = mex("packets_get", h, nlhs=2)
        np.testing.assert_array_equal(np.asarray(mx).view(np.uint64), np.ascontiguousarray(cx).view(np.uint64))
        np.testing.assert_array_equal(np.asarray(mk).view(np.uint64), np.ascontiguousarray(ck).view(np.uint64))
        mex("recycle_reset", h, nlhs=0)
        assert mex("recycle_frames", h) == 0
        mgen, mborn = mex("recycle_state", h, nlhs=2)
        assert not _i64(mgen).any() and not _i64(mborn).any()
        # home left out: the packets' k now (k[7] = 1e9 would be rejected, so such a home is refused)
        with pytest.raises(MexError, match="swrt_recycle_begin.*home"):
            mex("recycle_begin", h, F, CG, 1e6, L, nlhs=0)
        mex("packets_set", h, x, home, nlhs=0)
        with pytest.raises(MexError, match="swrt_recycle_apply.*begin"):  # (a refused begin leaves nothing begun)
            mex("recycle_apply", h, nlhs=0)
        mex("recycle_begin", h, F, CG, 1e6, L, nlhs=0)
        mex("recycle_apply", h, nlhs=0)
        assert _i64(mex("recycle_get", h))[:, 0].tolist() == [n, 0, 0, 0, 0, 0, 0, 1]
        mex("packets_set", h, x, k, nlhs=0)
        # bad arguments become MATLAB errors
        with pytest.raises(MexError, match="swrt_recycle_begin.*above"):
            mex("recycle_begin", h, F, CG, 0.5 * F, L, nlhs=0)
        with pytest.raises(MexError, match="swrt_recycle_begin.*home"):
            mex("recycle_begin", h, F, CG, cut, L, nlhs=0)  # (the packets' own k reaches the cut)
        with pytest.raises(MexError, match="home_k"):
            mex("recycle_begin", h, F, CG, cut, L, 0.0, 0.0, 20.0, home[:100], nlhs=0)
        with pytest.raises(MexError):
            mex("recycle_begin", h, F, CG, nlhs=0)  # too few arguments
        mex("recycle_end", h, nlhs=0)
        with pytest.raises(MexError, match="swrt_recycle_apply.*begin"):
            mex("recycle_apply", h, nlhs=0)
    finally:
        mex("destroy", h, nlhs=0)
