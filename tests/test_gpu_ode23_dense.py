"""GPU ode23 with output at requested times (swrt_ode23_set_dense / _ntrp /
_run_at, swrt_raydiag_record_history, integrate.ode23_packets with a vector
tspan, integrate.ode23_trajectory) against the tests' CPU reference
(tests/ode23_dense_ref.py).  The stages are the oracle's operation sequence,
the interpolant's order is pinned, so accepted times, frames and the final
state are compared bit for bit."""
import ctypes
import math

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import swrt_oracle as orc
from swraytracing_amd import _lib as L
from tests import ode23_dense_ref as R
from tests.conftest import periodic_grid
from tests.test_gpu_parity import _planes

pytestmark = pytest.mark.gpu

T = 1.4      # the fastest packets cross ~20 cells: more than one 16-cell tile
N_BIG = 3001  # not a multiple of 64; ~190 packets per tile of the 4 x 4 binning
N_SMALL = 257
ERR_ARG, ERR_STATE = 1, 3  # include/swrt.h


@pytest.fixture(scope="module")
def big():
    return _case(N_BIG)


@pytest.fixture(scope="module")
def small():
    return _case(N_SMALL)


def _case(n):
    c = R.low_mode_case(n)
    c["h"] = c["L"] / c["nx"]
    c["y0"] = R.y_of(c["x"], c["k"])
    c["pair"] = orc.raytracing_rhs(c["flow1"], c["flow2"], c["f"], c["Cg"], T, c["h"])
    c["steady"] = R.steady_rhs(c["flow1"], c["f"], c["Cg"], c["h"], orc.BUMP_SW)
    c["refs"] = {}
    return c


def _ref(c, field, tspan, rtol=1e-3, atol=1e-6):
    """The CPU reference of one run, computed once per module and never changed."""
    key = (field, tuple(tspan), rtol, atol)
    if key not in c["refs"]:
        st, steps = {}, []
        ts, yout, _ = R.ode23_dense(c[field], tspan, c["y0"], rtol, atol, stats=st, steps_out=steps)
        for a in (ts, yout):
            a.setflags(write=False)
        c["refs"][key] = (ts, yout, st, steps)
    return c["refs"][key]


def _set_pair(ctx, c):
    ctx.set_field_grid(0, _planes(c["flow1"]), c["nx"], c["L"])
    ctx.set_field_grid(1, _planes(c["flow2"]), c["nx"], c["L"])


def _rows(hx, hk):
    """history frames (count x 2 x n each) as rows [x; y; k; l] of the 4N-vector"""
    return np.concatenate([hx[:, 0], hx[:, 1], hk[:, 0], hk[:, 1]], axis=1)


def _run(ctx, c, tspan, controller="library", nslots=2, tmax=T, rtol=1e-3, atol=1e-6, bump=orc.BUMP_QG):
    ctx.packets_set(c["x"], c["k"])
    st = {}
    ts = sw.ode23_packets(ctx, tspan, tmax, c["f"], c["Cg"], nslots=nslots, rtol=rtol, atol=atol, bump=bump,
                          stats=st, controller=controller)
    frames = _rows(*ctx.history())
    xg, kg = ctx.packets_get()
    return ts, frames, R.y_of(xg, kg), st


@pytest.mark.parametrize("nt", [9, 401])
def test_base_case_tile_path(ctx, big, nt):
    """N = 3001 on the binned tile path, two snapshots, RelTol 1e-3: 9 outputs
    (most steps hold none) and 401 (many per step, the first gap binds)."""
    c = big
    tspan = np.linspace(0.0, T, nt)
    ts_r, yout, st_r, _ = _ref(c, "pair", tspan)
    n = N_BIG
    travel = np.hypot(yout[-1, :n] - yout[0, :n], yout[-1, n:2 * n] - yout[0, n:2 * n]).max() / c["h"]
    assert st_r["failed"] >= 1 and travel > 16
    if nt == 401:
        assert ts_r[1] - ts_r[0] == tspan[1]  # the first gap is the first step
    _set_pair(ctx, c)
    ctx.set_locality(4, 0)
    ts, frames, yend, st = _run(ctx, c, tspan)
    np.testing.assert_array_equal(ts, ts_r)
    assert (st["steps"], st["failed"], st["attempts"]) == (st_r["steps"], st_r["failed"], st_r["attempts"])
    assert frames.shape == (nt - 1, 4 * n)
    np.testing.assert_array_equal(frames, yout[1:])
    np.testing.assert_array_equal(yend, frames[-1])  # the packets are left at the last frame
    if nt == 9:
        # the first gap does not bind: the steps and the end state of swrt_ode23_run on [t0 tfinal]
        ctx.packets_set(c["x"], c["k"])
        ts2, st2 = ctx.ode23_run(0.0, T, T, c["f"], c["Cg"], 2, 1e-3, 1e-6, orc.BUMP_QG)
        np.testing.assert_array_equal(ts2, ts)
        np.testing.assert_array_equal(R.y_of(*ctx.packets_get()), yend)


def test_sw_zero_settings_steady_field(ctx, small):
    """SW_zero_background_raytracing.m:69-72: a steady field (one slot, no time
    blend), RelTol 1e-6 / AbsTol 1e-7, 41 output times."""
    c = small
    tspan = np.linspace(0.0, 0.5, 41)
    ts_r, yout, st_r, _ = _ref(c, "steady", tspan, 1e-6, 1e-7)
    ctx.set_field_grid(0, _planes(c["flow1"]), c["nx"], c["L"])
    ts, frames, yend, st = _run(ctx, c, tspan, nslots=1, tmax=0.0, rtol=1e-6, atol=1e-7, bump=orc.BUMP_SW)
    np.testing.assert_array_equal(ts, ts_r)
    assert st["steps"] == st_r["steps"] > 40
    np.testing.assert_array_equal(frames, yout[1:])
    np.testing.assert_array_equal(yend, yout[-1])


def test_per_packet_path_equals_tile_path(ctx, small):
    """N = 257 with binning off (one lane per packet, three stage launches per
    attempt) gives the tile path's frames, and the reference's."""
    c = small
    tspan = np.linspace(0.0, T, 9)
    ts_r, yout, _, _ = _ref(c, "pair", tspan)
    _set_pair(ctx, c)
    out = []
    try:
        for rebin in (0, 4):
            ctx.set_locality(rebin, 0)
            out.append(_run(ctx, c, tspan))
    finally:
        ctx.set_locality(4, 0)
    for ts, frames, yend, _ in out:
        np.testing.assert_array_equal(ts, ts_r)
        np.testing.assert_array_equal(frames, yout[1:])
        np.testing.assert_array_equal(yend, yout[-1])


def test_rebinning_cadence_changes_nothing(ctx, big):
    """swrt_ode23_run_at re-bins by re-queuing stage 1 at the current time:
    every step, every 5 steps or never inside the run, the same bits."""
    c = big
    tspan = np.linspace(0.0, T, 9)
    ts_r, yout, st_r, _ = _ref(c, "pair", tspan)
    _set_pair(ctx, c)
    ctx.set_locality(4, 0)
    try:
        for every in (1, 5, 0):
            ctx.debug_set(L.DEBUG_ODE23_DENSE_REBIN, every)
            before = ctx.debug_get(L.DEBUG_ODE23_DENSE_REBINS)
            ts, frames, yend, _ = _run(ctx, c, tspan)
            made = ctx.debug_get(L.DEBUG_ODE23_DENSE_REBINS) - before
            assert made == ((st_r["steps"] - 1) // every if every else 0)
            np.testing.assert_array_equal(ts, ts_r)
            np.testing.assert_array_equal(frames, yout[1:])
            np.testing.assert_array_equal(yend, yout[-1])
    finally:
        ctx.debug_set(L.DEBUG_ODE23_DENSE_REBIN, 8)


def test_exact_hit_is_ynew(ctx, small):
    """An accepted interior time put into tspan (after its second entry, so the
    first gap stays): that frame is ynew's bits, not the interpolant's, and
    the steps and every other frame are unchanged."""
    c = small
    tspan = np.linspace(0.0, T, 9)
    ts_r, yout, _, steps = _ref(c, "pair", tspan)
    inside = [(t, y) for t, y in steps if tspan[1] < t < tspan[2]]
    assert inside
    t_hit, ynew = inside[len(inside) // 2]
    tspan2 = np.concatenate([tspan[:2], [t_hit], tspan[2:]])
    _set_pair(ctx, c)
    ts1, frames1, _, _ = _run(ctx, c, tspan)
    ts2, frames2, _, _ = _run(ctx, c, tspan2)
    np.testing.assert_array_equal(ts1, ts_r)
    np.testing.assert_array_equal(ts2, ts_r)
    np.testing.assert_array_equal(frames2[1], ynew)
    np.testing.assert_array_equal(np.delete(frames2, 1, axis=0), frames1)
    # the interpolant evaluated there (s = 1) is close to ynew but not it
    _, yref2, _, _ = _ref(c, "pair", tspan2)
    np.testing.assert_array_equal(frames2, yref2[1:])


def test_decreasing_tspan(ctx, small):
    c = small
    tspan = np.linspace(T, 0.0, 9)
    ts_r, yout, st_r, _ = _ref(c, "pair", tspan)
    _set_pair(ctx, c)
    ts, frames, yend, st = _run(ctx, c, tspan)
    assert np.all(np.diff(ts) < 0)
    np.testing.assert_array_equal(ts, ts_r)
    np.testing.assert_array_equal(frames, yout[1:])
    np.testing.assert_array_equal(yend, yout[-1])


def test_controller_paths_give_equal_frames(ctx, big):
    """controller="python" (ode23_set_dense, ode23_attempt, ode23_ntrp,
    ode23_accept from the Python loop) and the library's swrt_ode23_run_at."""
    c = big
    tspan = np.linspace(0.0, T, 401)
    ts_r, yout, _, _ = _ref(c, "pair", tspan)
    _set_pair(ctx, c)
    ctx.set_locality(4, 0)
    ts_p, frames_p, yend_p, st_p = _run(ctx, c, tspan, controller="python")
    ts_l, frames_l, yend_l, st_l = _run(ctx, c, tspan, controller="library")
    np.testing.assert_array_equal(ts_p, ts_l)
    np.testing.assert_array_equal(frames_p, frames_l)
    np.testing.assert_array_equal(yend_p, yend_l)
    np.testing.assert_array_equal(frames_p, yout[1:])
    assert (st_p["steps"], st_p["failed"], st_p["attempts"]) == (st_l["steps"], st_l["failed"], st_l["attempts"])


def test_frames_append_to_history_and_reset(ctx, small):
    c = small
    _set_pair(ctx, c)
    ctx.packets_set(c["x"], c["k"])
    ctx.advance(1e-3, 3, c["f"], c["Cg"] ** 2, nslots=2, alpha0=0.0, dalpha=0.0, bump=orc.BUMP_QG, save_every=1)
    hx0, hk0 = ctx.history()
    assert hx0.shape[0] == 3
    tspan = np.linspace(0.0, 0.2, 6)
    sw.ode23_packets(ctx, tspan, T, c["f"], c["Cg"])
    hx, hk = ctx.history()
    assert hx.shape[0] == 3 + 5
    np.testing.assert_array_equal(hx[:3], hx0)
    np.testing.assert_array_equal(hk[:3], hk0)
    xg, kg = ctx.packets_get()
    np.testing.assert_array_equal(hx[-1].T, xg)
    np.testing.assert_array_equal(hk[-1].T, kg)
    ctx.history_reset()
    assert ctx.history()[0].shape[0] == 0


def test_errors_are_reported(ctx, small):
    c = small
    _set_pair(ctx, c)
    ctx.packets_set(c["x"], c["k"])
    lib, h = ctx._L, ctx._h
    ts = np.empty(16)
    nts = ctypes.c_int64()
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def run_at(tspan, nt, ts_buf=ts, nts_ref=ctypes.byref(nts)):
        return lib.swrt_ode23_run_at(h, None if tspan is None else p(tspan), nt, T, c["f"], c["Cg"], 2, 1e-3, 1e-6,
                                     orc.BUMP_QG, None if ts_buf is None else p(ts_buf), 16, nts_ref, None)

    def message():
        return lib.swrt_last_error(h).decode()

    one = np.array([0.0, 1.0])
    assert run_at(one, 1) == ERR_ARG and "two" in message()
    assert run_at(np.array([0.0, 0.5, 0.4, 1.0]), 4) == ERR_ARG and "strictly" in message()
    assert run_at(np.array([0.0, 0.5, 0.5]), 3) == ERR_ARG and "strictly" in message()
    assert run_at(None, 3) == ERR_ARG and "NULL" in message()
    assert run_at(one, 2, ts_buf=None) == ERR_ARG and message()
    assert run_at(one, 2, nts_ref=None) == ERR_ARG and message()
    # ntrp: nothing attempted; attempted but not dense; dense but already accepted
    tout = np.array([0.005])
    frames0 = ctx.history()[0].shape[0]
    thr = 1e-6 / 1e-3
    with pytest.raises(sw.SwrtError, match="dense"):
        ctx.ode23_ntrp(0.0, 0.01, tout)
    ctx.ode23_f1(0.0, T, c["f"], c["Cg"], 2, thr, orc.BUMP_QG)
    ctx.ode23_attempt(0.0, 0.01, 0.01, T, c["f"], c["Cg"], 2, thr, orc.BUMP_QG)
    assert lib.swrt_ode23_ntrp(h, 0.0, 0.01, p(tout), 1) == ERR_STATE and "dense" in message()
    ctx.ode23_set_dense(1)
    try:
        ctx.ode23_attempt(0.0, 0.01, 0.01, T, c["f"], c["Cg"], 2, thr, orc.BUMP_QG)
        assert lib.swrt_ode23_ntrp(h, 0.0, 0.01, None, 1) == ERR_ARG and "NULL" in message()
        assert lib.swrt_ode23_ntrp(h, 0.0, 0.01, p(np.array([0.02])), 1) == ERR_ARG and "outside" in message()
        ctx.ode23_ntrp(0.0, 0.01, tout)  # the valid call, after the refused ones
        assert ctx.history()[0].shape[0] == frames0 + 1
        ctx.ode23_attempt(0.0, 0.01, 0.01, T, c["f"], c["Cg"], 2, thr, orc.BUMP_QG)
        ctx.ode23_accept()
        with pytest.raises(sw.SwrtError, match="dense"):
            ctx.ode23_ntrp(0.0, 0.01, tout)
    finally:
        ctx.ode23_set_dense(0)
    assert lib.swrt_ode23_set_dense(h, 2) == ERR_ARG
    # record_history: a frame range the history does not hold; two snapshots without alphas
    assert lib.swrt_raydiag_record_history(h, 0, 10_000, c["f"], 1.0, 1, None, orc.BUMP_QG) == ERR_ARG
    assert "range" in message()
    assert lib.swrt_raydiag_record_history(h, 0, 1, c["f"], 1.0, 2, None, orc.BUMP_QG) == ERR_ARG
    assert "NULL" in message()


def test_raydiag_record_history_equals_sample(ctx, small):
    """One series frame per history frame, each the bits of raydiag_sample on
    packets set to that frame (the mark survives packets_set of the same N)."""
    c = small
    f, gH = c["f"], c["Cg"] ** 2
    tspan = np.linspace(0.0, T, 9)
    alphas = tspan / T
    _set_pair(ctx, c)
    ctx.packets_set(c["x"], c["k"])
    ctx.raydiag_series_reset()
    ctx.raydiag_mark(f, gH, nslots=2, alpha=0.0, bump=orc.BUMP_QG)
    sw.ode23_packets(ctx, tspan, T, f, c["Cg"])
    hx, hk = ctx.history()
    ctx.raydiag_record_history(0, 8, f, gH, nslots=2, alphas=alphas[1:], bump=orc.BUMP_QG)
    series = ctx.raydiag_series()
    assert series.shape == (8, 8)
    assert series[:, 1].max() > 0  # the field is unsteady: Omega drifts from its mark
    for i in (0, 3, 7):
        ctx.packets_set(np.asfortranarray(hx[i].T), np.asfortranarray(hk[i].T))
        _, fr = ctx.raydiag_sample(f, gH, nslots=2, alpha=alphas[1 + i], bump=orc.BUMP_QG, values=False)
        np.testing.assert_array_equal(series[i], fr)


def test_ode23_trajectory_with_diagnostics(ctx):
    """The single-mode case of test_oracle_kats (a steady psi = A cos(x + y),
    8 packets on a ring of |k| = 3) through ode23_trajectory at SW_zero's
    RelTol 1e-6 / AbsTol 1e-7: shapes, row 0, and solver_error.  The
    reference's figure band for this case is |dOmega/Omega_0| ~ 1e-5
    (test_single_mode_absolute_frequency_conservation asserts 5e-5); the CPU
    reference (ode23_dense_ref) measures max|r| = 2.44e-8 over these 101 output
    times (2.11e-5 at the default RelTol 1e-3)."""
    nx, A = 64, 0.05
    X, Y = periodic_grid(nx)
    psi = A * np.cos(X + Y)
    f, Cg = 3.0, 1.0
    rng = np.random.default_rng(123)
    P = 8
    x0 = np.zeros((1, 2, P))
    k0 = np.zeros((1, 2, P))
    for i in range(P):
        k0[0, :, i] = 3 * np.array([math.cos(2 * math.pi * (i + 1) / P), math.sin(2 * math.pi * (i + 1) / P)])
        x0[0, :, i] = 2 * np.pi * rng.random(2) - np.pi
    sch = sw.SpectralScheme(2 * np.pi, nx, psi, ctx=ctx)
    t_hist = 0.05 * np.arange(101)
    xs, ks, diag = sw.ode23_trajectory(x0, k0, t_hist, f, Cg, sch, rtol=1e-6, atol=1e-7, diagnostics=True)
    assert xs.shape == ks.shape == (101, 2, P) and diag.shape == (101, 8)
    np.testing.assert_array_equal(xs[0], x0[0])
    np.testing.assert_array_equal(ks[0], k0[0])
    assert np.all(diag[:, 0] == P) and diag[0, 1] == 0.0
    print(f"ode23_trajectory single mode: max|r| = {diag[:, 1].max():.3e}")
    assert 0 < diag[:, 1].max() < 5e-5
    # without diagnostics: the same trajectory
    xs2, ks2 = sw.ode23_trajectory(x0, k0, t_hist, f, Cg, sch, rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(xs2, xs)
    np.testing.assert_array_equal(ks2, ks)


def test_ode23_trajectory_snapshot_pair(ctx, small):
    """ode23_trajectory over a SnapshotPairScheme (alpha = t / tmax): the rows
    are the reference's outputs, the series the frames' raydiag samples."""
    c = small
    tspan = np.linspace(0.0, T, 9)
    _, yout, _, _ = _ref(c, "pair", tspan)
    n = N_SMALL
    sch = sw.SnapshotPairScheme(c["flow1"], c["flow2"], c["L"], tmax=T, ctx=ctx)
    xs, ks, diag = sw.ode23_trajectory(c["x"].T[None], c["k"].T[None], tspan, c["f"], c["Cg"], sch, diagnostics=True)
    assert xs.shape == ks.shape == (9, 2, n) and diag.shape == (9, 8)
    rows = np.concatenate([xs[:, 0], xs[:, 1], ks[:, 0], ks[:, 1]], axis=1)
    np.testing.assert_array_equal(rows, yout)
    assert diag[0, 1] == 0.0 and np.all(diag[:, 0] == n)
    ctx.packets_set(np.asfortranarray(xs[5].T), np.asfortranarray(ks[5].T))
    _, fr = ctx.raydiag_sample(c["f"], c["Cg"] ** 2, nslots=2, alpha=tspan[5] / T, bump=sch.bump, values=False)
    np.testing.assert_array_equal(diag[5], fr)
    with pytest.raises(ValueError, match="three"):
        sw.ode23_trajectory(c["x"].T[None], c["k"].T[None], tspan[:2], c["f"], c["Cg"], sch)
