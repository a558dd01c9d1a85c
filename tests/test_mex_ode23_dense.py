"""matlab/ode23_packets_gpu.m with a vector tspan over the MEX gateway
(commands ode23_set_dense, ode23_ntrp, history, history_reset), driven through
the test mex.h shim as test_mex_gateway.py drives the two-point one: the .m
loop is restated here line by line (MATLAB eps(t) = np.spacing)."""
import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import swrt_oracle as orc
from tests import ode23_dense_ref as R
from tests.test_mex_gateway import Mex


@pytest.fixture(scope="module")
def mex():
    return Mex()


def _ode23_packets_gpu_m(mex, hctx, tspan, tmax, f, Cg, nslots, rtol=1e-3, atol=1e-6):
    rtol, bump = max(rtol, 100 * np.finfo(float).eps), 1e-10
    thr, pw = atol / rtol, 1.0 / 3.0
    nt = len(tspan)
    dense = nt > 2
    t0, tfinal = tspan[0], tspan[-1]
    tdir = np.sign(tfinal - t0)
    htspan = abs(tspan[1] - tspan[0])
    hmax = 0.1 * abs(tfinal - t0)
    if dense:
        mex("history_reset", hctx, nlhs=0)
        mex("ode23_set_dense", hctx, 1.0, nlhs=0)
    nxt = 1  # (0-based: the .m's next = 2)
    t = t0
    rh = mex("ode23_f1", hctx, t, tmax, f, Cg, nslots, thr, bump) / (0.8 * rtol ** pw)
    absh = min(hmax, htspan)
    if absh * rh > 1:
        absh = 1 / rh
    absh = max(absh, 16 * np.spacing(t))
    acc = [t]
    done = False
    while not done:
        hmin = 16 * np.spacing(t)
        absh = min(hmax, max(hmin, absh))
        h = tdir * absh
        if 1.1 * absh >= abs(tfinal - t):
            h = tfinal - t
            absh = abs(h)
            done = True
        nofailed = True
        while True:
            tnew = t + h
            if done:
                tnew = tfinal
            err = absh * mex("ode23_attempt", hctx, t, h, tnew, tmax, f, Cg, nslots, thr, bump)
            h = tnew - t
            if err > rtol:
                assert absh > hmin
                if nofailed:
                    nofailed = False
                    absh = max(hmin, absh * max(0.5, 0.8 * (rtol / err) ** pw))
                else:
                    absh = max(hmin, 0.5 * absh)
                h = tdir * absh
                done = False
            else:
                break
        if dense:
            first = nxt
            while nxt < nt and tdir * (tnew - tspan[nxt]) >= 0:
                nxt += 1
            if nxt > first:
                mex("ode23_ntrp", hctx, t, tnew, np.asarray(tspan[first:nxt]).reshape(1, -1), nlhs=0)
        mex("ode23_accept", hctx, nlhs=0)
        t = tnew
        acc.append(t)
        if done:
            break
        if nofailed:
            temp = 1.25 * (err / rtol) ** pw
            absh = absh / temp if temp > 0.2 else 5.0 * absh
    if dense:
        mex("ode23_set_dense", hctx, 0.0, nlhs=0)
        hx, hk = mex("history", hctx, nlhs=2)
        return np.array(acc), hx, hk
    return np.array(acc), None, None


@pytest.mark.gpu
def test_ode23_packets_gpu_m_vector_tspan_matches_library(mex, ctx):
    """N x 2 x frames from the gateway's history command equal the frames of
    swrt_ode23_run_at (integrate.ode23_packets, library controller), and the
    accepted times are the same."""
    c = R.low_mode_case(257)
    nx, Lx, f, Cg = c["nx"], c["L"], c["f"], c["Cg"]
    T = 1.0
    tspan = np.linspace(0.0, T, 201)  # the first gap binds; many outputs per step (more than one ntrp launch)
    h = mex("create", 0.0)
    for slot, fl in ((0.0, c["flow1"]), (1.0, c["flow2"])):
        mex("set_field_grid", h, slot, *[np.asarray(fl[n]) for n in orc.FIELD_ORDER], Lx, float(nx), nlhs=0)
    mex("packets_set", h, c["x"], c["k"], nlhs=0)
    tm, hxm, hkm = _ode23_packets_gpu_m(mex, h, list(tspan), T, f, Cg, 2.0)
    xm, km = mex("packets_get", h, nlhs=2)
    with pytest.raises(Exception, match="dense"):  # no dense attempt in the buffers any more
        mex("ode23_ntrp", h, 0.0, 0.1, np.array([[0.05]]), nlhs=0)
    mex("destroy", h, nlhs=0)
    planes = lambda fl: np.ascontiguousarray(np.stack([np.asarray(fl[n]).ravel(order="F") for n in orc.FIELD_ORDER]))
    ctx.set_field_grid(0, planes(c["flow1"]), nx, Lx, nx)
    ctx.set_field_grid(1, planes(c["flow2"]), nx, Lx, nx)
    ctx.packets_set(c["x"], c["k"])
    tp = sw.ode23_packets(ctx, tspan, T, f, Cg, 2, bump=1e-10)
    hx, hk = ctx.history()
    xp, kp = ctx.packets_get()
    assert tm[1] - tm[0] == tspan[1] and np.diff(tm).max() > 8 * tspan[1]
    np.testing.assert_array_equal(tm, tp)
    assert hxm.shape == (257, 2, 200)
    np.testing.assert_array_equal(np.transpose(hxm, (2, 1, 0)), hx)
    np.testing.assert_array_equal(np.transpose(hkm, (2, 1, 0)), hk)
    np.testing.assert_array_equal(xm, xp)
    np.testing.assert_array_equal(km, kp)
