"""The flow spectrum commands of the MEX gateway (matlab/swrt_mex.cpp:
flow_spectrum_begin / _record_qg / _record_qk / _frames / _shells / _get /
_reset), driven through the test mex.h shim as test_mex_kmap_series.py drives
the k-plane series': the arrays MATLAB gets — spectra nshell x 3 x frames,
stats 4 x frames — hold the doubles the Python Context gives for the same
calls, and those are the restatement's (tests/flow_spectrum_ref.py)."""
import numpy as np
import pytest

from tests.flow_spectrum_ref import flow_frame
from tests.test_mex_gateway import Mex, MexError


@pytest.fixture(scope="module")
def mex():
    return Mex()


@pytest.mark.gpu
def test_gateway_flow_spectra_equal_the_context(mex, fresh_ctx):
    import swraytracing_amd as sw
    nx, L, f, Cg = 32, 20.0, 3.0, 1.0
    rng = np.random.default_rng(9)
    c = fresh_ctx
    fk = c.g2k(rng.standard_normal((nx, nx)) * 0.05)
    qk0 = np.stack([fk, -fk], axis=2)
    other = c.g2k(rng.standard_normal((nx, nx)))
    # the Context
    m = sw.QGModel.two_layer(qk0, nx, f, Cg, L=L, ctx=c)
    p = m.params
    U0 = m.max_speed()
    dt = 0.25 * (L / nx) / U0
    m.begin_flow_spectrum(1)
    m.record_flow_spectrum()
    m.step(dt, 4)
    m.record_flow_spectrum()
    c.flow_spectrum_record_qk(other, 7.5)
    cs, ct = c.flow_spectrum_get()
    want_sp, want_st = flow_frame(other, m.kscale, p.K_d2, 7.5)
    np.testing.assert_array_equal(cs[2], want_sp)
    np.testing.assert_array_equal(ct[2], want_st)
    assert not np.array_equal(cs[0], cs[1])
    # the gateway
    h = mex("create", 0.0)
    try:
        with pytest.raises(MexError, match="swrt_flow_spectrum_record_qg.*begin"):
            mex("flow_spectrum_record_qg", h, nlhs=0)
        params = {"nlayers": 2.0, "filter": float(p.filter), "L": p.L, "K_d2": p.K_d2, "beta": p.beta,
                  "r_drag": p.r_drag, "force_strength": p.force_strength, "f": p.f, "Cg": p.Cg, "shear": p.shear,
                  "nu": p.nu, "hyper_order": p.hyper_order, "r": p.r}
        mex("qg_init", h, params, qk0, nlhs=0)
        assert mex("qg_max_speed", h) == U0
        mex("flow_spectrum_begin", h, float(nx), m.kscale, p.K_d2, nlhs=0)
        assert mex("flow_spectrum_frames", h) == 0 and mex("flow_spectrum_shells", h) == cs.shape[2]
        mex("flow_spectrum_record_qg", h, 1.0, nlhs=0)
        mex("qg_step", h, dt, 4.0, nlhs=0)
        mex("flow_spectrum_record_qg", h, 1.0, nlhs=0)
        mex("flow_spectrum_record_qk", h, other, 7.5, nlhs=0)
        assert mex("flow_spectrum_frames", h) == 3
        ms, mt = mex("flow_spectrum_get", h, nlhs=2)
        assert ms.shape == (cs.shape[2], 3, 3) and mt.shape == (4, 3)
        np.testing.assert_array_equal(ms.transpose(2, 1, 0), cs)
        np.testing.assert_array_equal(mt.T, ct)
        with pytest.raises(MexError, match="swrt_flow_spectrum_record_qg.*layer"):
            mex("flow_spectrum_record_qg", h, 2.0, nlhs=0)
        with pytest.raises(MexError, match="qk must be"):
            mex("flow_spectrum_record_qk", h, other[:, :-1], 0.0, nlhs=0)
        mex("flow_spectrum_reset", h, nlhs=0)
        assert mex("flow_spectrum_frames", h) == 0
        assert mex("flow_spectrum_get", h).shape == (cs.shape[2], 3, 0)
        mex("flow_spectrum_record_qg", h, nlhs=0)  # layer 0 by default
        ms = mex("flow_spectrum_get", h)
        assert ms.shape == (cs.shape[2], 3)  # (one frame: a trailing dimension of 1 is dropped, as MATLAB does)
        m.begin_flow_spectrum(0)
        m.record_flow_spectrum()
        np.testing.assert_array_equal(ms.T, c.flow_spectrum_get()[0][0])
        with pytest.raises(MexError, match="swrt_flow_spectrum_begin.*nx must"):
            mex("flow_spectrum_begin", h, 48.0, 1.0, 0.0, nlhs=0)
    finally:
        mex("destroy", h, nlhs=0)
