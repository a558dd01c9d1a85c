"""Lifetime of a context's GPU resources: the grow, replace and destroy paths
of the packet, ode23 and slot buffers and of every subsystem's state, checked
by results (bit-equal to the C oracle / the oracle's ode23), never by memory
counters.  Small shapes throughout: 64^2 fields, at most 4096 packets, 20
steps."""
import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import cbind, swrt_oracle as orc
from tests.test_gpu_parity import _planes, _rsw_background

pytestmark = pytest.mark.gpu

F, GH, BUMP, STEPS = 3.0, 1.0, 1e-13, 20


def _flow(nx, L, rng):
    q = orc.initial_q(nx, L, 0.2, 3.0, 5 if nx >= 64 else 3, 8 if nx >= 64 else 6, rng)
    kx_, ky_, K2 = orc.wavenumber_grids(nx)
    return orc.grid_U(orc.g2k(q), 3.0, K2, kx_, ky_)


@pytest.fixture(scope="module")
def case(oracle_lib):
    """smoke()'s setup with 4096 packets, and the oracle's leapfrog of the
    first 512 and of all of them (computed once, shared, never modified)."""
    nx, L = 64, 2 * np.pi
    rng = np.random.default_rng(146)
    flow = _flow(nx, L, rng)
    planes = _planes(flow)
    x, k = orc.initial_packets(4096, L, 4.0, 3.0, 1.0, rng)
    dt = 0.05 * (L / nx) / 0.2
    ref = {}
    for n in (512, 4096):
        xo, ko, _, _ = cbind.leapfrog(planes, None, 0.0, 0.0, nx, nx, L / nx, BUMP, x[:n], k[:n], dt, STEPS, F, GH)
        ref[n] = (xo, ko)
    for v in (planes, x, k, *[a for r in ref.values() for a in r]):
        v.setflags(write=False)
    return dict(nx=nx, L=L, flow=flow, planes=planes, x=x, k=k, dt=dt, ref=ref,
                planes32=_planes(_flow(32, L, np.random.default_rng(7))))


def _leap(ctx, c, n):
    ctx.packets_set(c["x"][:n], c["k"][:n])
    ctx.advance(c["dt"], STEPS, F, GH, 1, bump=BUMP)
    return ctx.packets_get()


def _assert_leap(ctx, c, n, what):
    xg, kg = _leap(ctx, c, n)
    np.testing.assert_array_equal(xg, c["ref"][n][0], err_msg=what)
    np.testing.assert_array_equal(kg, c["ref"][n][1], err_msg=what)


def test_packet_buffers_grow_and_shrink(fresh_ctx, case):
    """packets_set with 512, 4096, then 512 packets on one context: the
    buffers are replaced by larger ones once and kept after; every leapfrog
    (per-packet kernel and LDS-tiled kernel) equals the oracle bit for bit."""
    ctx = fresh_ctx
    ctx.set_field_grid(0, case["planes"], case["nx"], case["L"])
    for n in (512, 4096, 512):
        for kernel in (1, 2):
            ctx.set_kernel(kernel)
            _assert_leap(ctx, case, n, f"{n} packets, kernel {kernel}")


def test_ode23_buffers_follow_the_packet_capacity(fresh_ctx, case):
    """ode23_run at 512 packets, then packets_set(4096) and ode23_run again
    (the stage buffers are smaller than the packet capacity and are replaced):
    times, counts and final state equal the oracle's ode23 both times."""
    ctx = fresh_ctx
    nx, L, Cg = case["nx"], case["L"], 1.0
    flow1 = case["flow"]
    flow2 = {n: np.asarray(v) * 1.3 for n, v in flow1.items()}
    ctx.set_field_grid(0, _planes(flow1), nx, L)
    ctx.set_field_grid(1, _planes(flow2), nx, L)
    tmax = STEPS * case["dt"]
    rhs = orc.raytracing_rhs(flow1, flow2, F, Cg, tmax, L / nx)
    for n in (512, 4096):
        x, k = case["x"][:n], case["k"][:n]
        ctx.packets_set(x, k)
        st = {}
        ts = sw.ode23_packets(ctx, (0.0, tmax), tmax, F, Cg, stats=st, controller="library")
        xg, kg = ctx.packets_get()
        so = {}
        to, yo = orc.ode23(rhs, [0.0, tmax], np.concatenate([x[:, 0], x[:, 1], k[:, 0], k[:, 1]]), stats=so)
        np.testing.assert_array_equal(ts, to)
        assert st["steps"] == so["steps"] and st["failed"] == so["failed"] and so["steps"] > 3
        np.testing.assert_array_equal(np.concatenate([xg[:, 0], xg[:, 1], kg[:, 0], kg[:, 1]]), yo)


def test_slot_replacement_keeps_planes_and_results(fresh_ctx, case):
    """set_field_grid on slot 0 at nx 64, 32, 64: the slot's node array is
    replaced each time and get_field_grid returns the planes bit for bit; a
    leapfrog on the last 64^2 field equals the oracle."""
    ctx = fresh_ctx
    for nx, planes in ((64, case["planes"]), (32, case["planes32"]), (64, case["planes"])):
        ctx.set_field_grid(0, planes, nx, case["L"])
        np.testing.assert_array_equal(ctx.get_field_grid(0, nx), planes)
    _assert_leap(ctx, case, 512, "after slot replacement")


def _touch_everything(ctx, case):
    """Packets, xka, spectral and QG state on one context; the results."""
    nx, L = case["nx"], case["L"]
    ctx.set_field_grid(0, case["planes"], nx, L)
    out = {"leap": _leap(ctx, case, 512)}
    U, G, H = _rsw_background(nx)
    rng = np.random.default_rng(21)
    n = 256
    st = np.stack([rng.uniform(0, L, n), rng.uniform(0, L, n), rng.normal(size=n), rng.normal(size=n), np.ones(n)],
                  axis=1)
    ctx.xka_set_fields(U, G, H, L / nx, L / nx)
    out["xka"] = ctx.xka_step(st, 1.0, 4.0, 0.1 * L / nx, 8, 0)[0]
    m = 3
    amp = 0.5 * rng.random((2 * m + 1, 2 * m + 1)) / (2 * m + 1) ** 2
    C, kx0, ky0, s = orc.modes_from_amp_phase(amp, 2 * np.pi * rng.random(amp.shape), m)
    pts = rng.uniform(-np.pi, np.pi, (100, 2))
    ctx.spectral_set_modes(C, kx0, ky0, s)
    out["spec"] = ctx.spectral_eval(pts[:, 0], pts[:, 1], 64)
    out["spec_ref"] = orc.spectral_direct(C, kx0, ky0, s, pts[:, 0], pts[:, 1])
    model = sw.QGModel.one_layer(orc.g2k(orc.initial_q(nx, L, 0.2, 3.0, 5, 8, np.random.default_rng(146))), nx, F,
                                 1.0, r_drag=0.0, ctx=ctx)
    model.step(case["dt"])
    ctx.qg_snapshot(1)
    out["qg_steps"] = ctx.qg_get()[2]
    out["snap"] = ctx.get_field_grid(1, nx)
    return out


def test_destroy_with_work_queued_then_reuse(case):
    """close() right after advance, with the launches still queued and
    nothing read back; a new context then runs the same case to the oracle's
    bits.  Three rounds of create, use, close follow, each touching packets,
    xka, spectral and QG state, so every state struct's handles are filled
    and released: same results every round, no exception."""
    c0 = sw.Context(0)
    c0.set_field_grid(0, case["planes"], case["nx"], case["L"])
    c0.packets_set(case["x"], case["k"])
    c0.advance(case["dt"], STEPS, F, GH, 1, bump=BUMP)
    c0.close()
    c1 = sw.Context(0)
    try:
        c1.set_field_grid(0, case["planes"], case["nx"], case["L"])
        _assert_leap(c1, case, 4096, "new context after a close with work queued")
    finally:
        c1.close()
    rounds = []
    for _ in range(3):
        c = sw.Context(0)
        try:
            rounds.append(_touch_everything(c, case))
        finally:
            c.close()
    for r in rounds:
        np.testing.assert_array_equal(r["leap"][0], case["ref"][512][0])
        np.testing.assert_array_equal(r["leap"][1], case["ref"][512][1])
        assert r["qg_steps"] == 1 and np.isfinite(r["snap"]).all() and np.isfinite(r["xka"]).all()
        for q in range(6):  # the spectral evaluator's own tolerance (test_gpu_spectral.py)
            assert np.abs(r["spec"][q] - r["spec_ref"][q]).max() <= 1e-12 * np.abs(r["spec_ref"][q]).max()
        for key in ("xka", "spec", "snap"):
            np.testing.assert_array_equal(r[key], rounds[0][key])
