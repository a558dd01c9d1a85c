"""ode23 with output at requested times, on the CPU: the tests' reference
(tests/ode23_dense_ref.py: oracle.ode23's loop, the tspan-vector rules, the
pinned ntrp23) against oracle.ode23 itself, against a tight DOP853 solve and
against the closed form at U = 0.  The GPU tests (test_gpu_ode23_dense.py)
compare bits with this reference."""
import numpy as np
import pytest

from oracle import swrt_oracle as orc
from tests import ode23_dense_ref as R

T = 1.2


@pytest.fixture(scope="module")
def case():
    c = R.low_mode_case(64)
    h = c["L"] / c["nx"]
    c["y0"] = R.y_of(c["x"], c["k"])
    c["rhs"] = {"steady": R.steady_rhs(c["flow1"], c["f"], c["Cg"], h, orc.BUMP_SW),
                "pair": orc.raytracing_rhs(c["flow1"], c["flow2"], c["f"], c["Cg"], T, h)}
    return c


@pytest.fixture(scope="module")
def runs(case):
    """The reference runs the tests share: (field, points) -> (ts, yout, stats)."""
    out = {}
    for field in ("steady", "pair"):
        for nt in (2, 9, 41, 401):
            st = {}
            ts, yo, _ = R.ode23_dense(case["rhs"][field], np.linspace(0.0, T, nt), case["y0"], stats=st)
            out[field, nt] = (ts, yo, st)
    return out


@pytest.mark.parametrize("field", ["steady", "pair"])
def test_two_point_tspan_is_oracle_ode23(case, runs, field):
    so = {}
    to, yo = orc.ode23(case["rhs"][field], [0.0, T], case["y0"], stats=so)
    ts, yout, st = runs[field, 2]
    np.testing.assert_array_equal(ts, to)
    np.testing.assert_array_equal(yout[-1], yo)
    assert (st["steps"], st["failed"]) == (so["steps"], so["failed"])
    assert st["failed"] > 0  # the reject path ran


@pytest.mark.parametrize("field", ["steady", "pair"])
def test_output_times_leave_the_steps_alone(case, runs, field):
    """41 output times whose first gap (0.03) exceeds the initial step (~0.023):
    the accepted times are those of the two-point run; so are 9."""
    ts2 = runs[field, 2][0]
    assert ts2[1] - ts2[0] < T / 40
    for nt in (9, 41):
        ts, yout, _ = runs[field, nt]
        np.testing.assert_array_equal(ts, ts2)
        assert yout.shape == (nt, case["y0"].size)
        np.testing.assert_array_equal(yout[0], case["y0"])
        np.testing.assert_array_equal(yout[-1], runs[field, 2][1][-1])  # the last point is ynew itself


@pytest.mark.parametrize("field", ["steady", "pair"])
def test_fine_output_grid_binds_the_first_step_only(case, runs, field):
    """401 output times: the first gap (0.003) is below the heuristic's initial
    step, so it is the first step (htspan of odearguments); hmax stays 0.1*T."""
    ts2 = runs[field, 2][0]
    ts, yout, _ = runs[field, 401]
    gap = np.linspace(0.0, T, 401)[1]
    assert ts[1] - ts[0] <= gap
    assert ts[1] - ts[0] != ts2[1] - ts2[0]
    assert np.diff(ts).max() > 10 * gap  # later steps hold many outputs
    assert np.diff(ts).max() <= 0.1 * T * (1 + 1e-15)
    assert yout.shape[0] == 401


@pytest.fixture(scope="module")
def dop(case):
    """y at 401 times from a DOP853 solve far tighter than ode23's RelTol."""
    from scipy.integrate import solve_ivp
    out = {}
    for field in ("steady", "pair"):
        s = solve_ivp(case["rhs"][field], (0.0, T), case["y0"], method="DOP853", rtol=1e-11, atol=1e-13,
                      t_eval=np.linspace(0.0, T, 401))
        assert s.success
        out[field] = s.y.T
    return out


# worst |yout - DOP853| / (rtol * max|y|) measured on these inputs (max|y| = 27.9 / 25.9):
#   steady: 9 outputs 0.120, 41 outputs 0.122, 401 outputs 0.108;  pair: 0.235 / 0.235 / 0.184
# i.e. a 4-9x margin, and no worse with many outputs per step than with few
# (the interpolant is as accurate as the step ends); RelTol 1e-6: 0.095.
# BI[0][1] = -1 instead of -4/3 gives 16.6 (4.6e-1 absolute), see
# test_wrong_bi_entry_is_caught.
@pytest.mark.parametrize("field", ["steady", "pair"])
@pytest.mark.parametrize("nt", [9, 41, 401])
def test_outputs_agree_with_tight_solve(case, runs, dop, field, nt):
    rtol = 1e-3
    _, yout, _ = runs[field, nt]
    ref = dop[field][:: 400 // (nt - 1)]
    err = np.abs(yout - ref).max()
    bound = rtol * np.abs(ref).max()
    print(f"{field} nt={nt}: max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound


def test_tight_tolerance_outputs(case, dop):
    """SW_zero's RelTol 1e-6 / AbsTol 1e-7 over half the span, 41 outputs."""
    tspan = np.linspace(0.0, T, 401)[0:201:5]
    _, yout, _ = R.ode23_dense(case["rhs"]["steady"], tspan, case["y0"], rtol=1e-6, atol=1e-7)
    ref = dop["steady"][0:201:5]
    err = np.abs(yout - ref).max()
    bound = 1e-6 * np.abs(ref).max()
    print(f"rtol 1e-6: max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert tspan.size == 41 and err <= bound


def test_wrong_bi_entry_is_caught(case, runs, dop):
    bad = [list(r) for r in R.BI]
    bad[0][1] = -1.0
    _, yout, _ = R.ode23_dense(case["rhs"]["steady"], np.linspace(0.0, T, 41), case["y0"], bi=bad)
    ref = dop["steady"][::10]
    err = np.abs(yout - ref).max()
    print(f"wrong BI: max err {err:.3e}")
    assert err > 5 * 1e-3 * np.abs(ref).max()


def test_zero_flow_outputs_are_the_straight_rays():
    """U = 0 (SW_zero_background_raytracing): x(t) = x0 + t*Cg*k/omega, k constant."""
    nx, L, f, Cg = 32, 2 * np.pi, 3.0, 1.0
    z = {n: np.zeros((nx, nx)) for n in orc.FIELD_ORDER}
    x, k = orc.initial_packets(64, L, 4.0, f, Cg, np.random.default_rng(5))
    tspan = np.linspace(0.0, 3.0, 31)
    _, yout, _ = R.ode23_dense(R.steady_rhs(z, f, Cg, L / nx, orc.BUMP_SW), tspan, R.y_of(x, k), rtol=1e-6, atol=1e-7)
    w = np.sqrt(f * f + Cg * Cg * (k[:, 0] ** 2 + k[:, 1] ** 2))
    n = x.shape[0]
    for i, t in enumerate(tspan):
        np.testing.assert_allclose(yout[i, :n], x[:, 0] + t * Cg * k[:, 0] / w, rtol=0, atol=1e-12)
        np.testing.assert_allclose(yout[i, n:2 * n], x[:, 1] + t * Cg * k[:, 1] / w, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(yout[i, 2 * n:], np.concatenate([k[:, 0], k[:, 1]]))


def test_decreasing_tspan_mirrors_the_steps(case):
    """A decreasing tspan integrates backwards with the same rules (tdir = -1)."""
    tspan = np.linspace(T / 4, 0.0, 6)
    ts, yout, _ = R.ode23_dense(case["rhs"]["pair"], tspan, case["y0"])
    assert np.all(np.diff(ts) < 0) and ts[0] == T / 4 and ts[-1] == 0.0
    assert yout.shape[0] == 6
