"""The integrator commands of the MEX gateway (matlab/swrt_mex.cpp:
set_integrator / get_integrator / integrator_weights), driven through the test
mex.h shim as test_mex_recycle.py drives the recycle commands: the gateway's
set_integrator followed by its leapfrog gives the Context's bits, the weights
are the library's doubles, and a bad value becomes a MATLAB error."""
import numpy as np
import pytest

from oracle import cbind, swrt_oracle as orc
from tests.test_mex_gateway import Mex, MexError

BUMP = orc.BUMP_QG


@pytest.fixture(scope="module")
def mex():
    return Mex()


def test_gateway_weights_need_no_context(mex):
    import swraytracing_amd as sw
    for comp in (0, 1, 2):
        w, off = mex("integrator_weights", float(comp), nlhs=2)
        ww, oo = sw.integrator_weights(comp)
        assert np.asarray(w).size == ww.size  # (1 x S; the harness hands a 1 x 1 back as a scalar)
        assert np.array_equal(np.asarray(w).ravel(), ww) and np.array_equal(np.asarray(off).ravel(), oo)
    with pytest.raises(MexError, match="composition"):
        mex("integrator_weights", 3.0)


@pytest.mark.gpu
def test_gateway_integrator_equals_the_context(mex, fresh_ctx, qg_case):
    q = qg_case
    nx, L, F, CG = q["nx"], q["L"], q["f"], q["Cg"]
    planes = cbind.planes_of(q["flow"])
    x, k = np.asfortranarray(q["x"]), np.asfortranarray(q["k"])
    dt, steps = 4 * q["dt"], 6
    c = fresh_ctx
    c.set_field_grid(0, planes, nx, L)
    want = {}
    for integ in ((1, 2, 0), (1, 4, 1), (0, 1, 0)):
        c.set_integrator(*integ)
        want[integ] = c.leapfrog(x, k, dt, steps, F, CG ** 2, nslots=1, bump=BUMP, save_every=2)
    assert not np.array_equal(want[1, 2, 0][1], want[0, 1, 0][1])
    h = mex("create", 0.0)
    try:
        fields = [np.asarray(planes[i]).reshape((nx, nx), order="F") for i in range(6)]
        mex("set_field_grid", h, 0.0, *fields, L, float(nx), nlhs=0)
        assert np.asarray(mex("get_integrator", h)).ravel().tolist() == [0, 1, 0]
        for integ in ((1, 2, 0), (1, 4, 1), (0, 1, 0)):
            mex("set_integrator", h, *[float(v) for v in integ], nlhs=0)
            assert np.asarray(mex("get_integrator", h)).ravel().tolist() == list(integ)
            mx, mk, mhx, mhk = mex("leapfrog", h, x, k, dt, float(steps), F, CG ** 2, 1.0, 0.0, 0.0, BUMP, 2.0, nlhs=4)
            cx, ck, chx, chk = want[integ]
            for got, ref in ((mx, cx), (mk, ck)):
                np.testing.assert_array_equal(np.asarray(got).view(np.uint64), np.ascontiguousarray(ref).view(np.uint64))
            # frames: N x 2 x F in MATLAB, F x 2 x N from the Context
            for got, ref in ((mhx, chx), (mhk, chk)):
                np.testing.assert_array_equal(np.transpose(np.asarray(got), (2, 1, 0)), ref)
        # bad values become MATLAB errors and leave the setting
        mex("set_integrator", h, 1.0, 3.0, 2.0, nlhs=0)
        for bad in ((2.0, 1.0, 0.0), (1.0, 0.0, 0.0), (1.0, 5.0, 0.0), (1.0, 2.0, 3.0)):
            with pytest.raises(MexError, match="swrt_set_integrator"):
                mex("set_integrator", h, *bad, nlhs=0)
        with pytest.raises(MexError):
            mex("set_integrator", h, 1.0, nlhs=0)  # too few arguments
        assert np.asarray(mex("get_integrator", h)).ravel().tolist() == [1, 3, 2]
    finally:
        mex("destroy", h, nlhs=0)
