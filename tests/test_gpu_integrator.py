"""The staged packet step (swrt_set_integrator) on the device: implicit-
midpoint kick, Yoshida and Suzuki compositions, in the per-packet and the
LDS-tiled kernel.

The main property: a composite step is, bit for bit, its stages as single-step
advance calls of size w_j*dt at blend a_j under the same kick — with the Euler
kick that ties the new stage loop (negative stage included) to the kernel that
existed before.  The midpoint formula itself is fixed by the numpy restatement
(tests/integrator_ref.py).  Weights and offsets always come from
swrt_integrator_weights."""
import numpy as np
import pytest

from oracle import swrt_oracle as orc
from tests import integrator_ref as ref

pytestmark = pytest.mark.gpu

F, GH, BUMP, L = ref.F, ref.GH, ref.BUMP, 2 * np.pi
N = 257
STEPS = 6
A0, DA = 0.5 / STEPS, 1.0 / STEPS  # the drivers' midpoint convention over one interval

# (kick, iterations, composition)
SCHEMES = [(0, 1, 1), (1, 1, 0), (1, 4, 0), (1, 1, 1), (1, 4, 1), (1, 1, 2), (1, 4, 2)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    if bad.size:
        g, w = got.reshape(-1), want.reshape(-1)
        lines = [f"  [{i}] got {g[i].hex()} want {w[i].hex()}" for i in bad[:5]]
        raise AssertionError(f"{what}: {bad.size} of {g.size} values differ\n" + "\n".join(lines))


def _psi(nx, phase):
    xs = np.arange(nx) * (L / nx)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    return (0.1 * np.sin(X + 2 * Y + 0.3 + phase) + 0.03 * np.sin(3 * X - Y + 1.1 + phase)
            + 0.012 * np.sin(2 * X + 5 * Y + 2.0 + 2 * phase))


def _planes6(nx, phase):
    """Six planes whose v_y is NOT -u_x (a weak divergent part): the six-sum window."""
    xs = np.arange(nx) * (L / nx)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    f = {n: np.zeros_like(X) for n in orc.FIELD_ORDER}
    for a, b, amp, ph in [(1, 2, 0.05, 0.3), (3, -1, 0.03, 1.1), (2, 5, 0.012, 2.0)]:
        s, c = np.sin(a * X + b * Y + ph + phase), np.cos(a * X + b * Y + ph + phase)
        f["u"] += -amp * b * c
        f["v"] += amp * a * c
        f["ux"] += amp * a * b * s
        f["uy"] += amp * b * b * s
        f["vx"] += -amp * a * a * s
        f["vy"] += -amp * a * b * s
    f["u"] += 0.01 * np.sin(X + 0.2 + phase)
    f["ux"] += 0.01 * np.cos(X + 0.2 + phase)
    return np.ascontiguousarray(np.stack([f[n].ravel(order="F") for n in orc.FIELD_ORDER]))


def _set_fields(ctx, nx, kind, nslots=2):
    for s in range(nslots):
        if kind == "psi":
            ctx.set_field_psi(s, _psi(nx, 0.4 * s), nx, L)
        else:
            ctx.set_field_grid(s, _planes6(nx, 0.4 * s), nx, L)
    assert ctx.field_div_free(0) == (kind == "psi")


def _packets(n, seed=7):
    rng = np.random.default_rng(seed)
    x, k = orc.initial_packets(n, L, 4.0, F, np.sqrt(GH), rng)
    return np.asfortranarray(x), np.asfortranarray(k)


@pytest.fixture(scope="module")
def mod_ctx():
    import swraytracing_amd as sw
    c = sw.Context(0)
    yield c
    c.close()


@pytest.fixture()
def ictx(mod_ctx):
    """The module's context with the settings these tests touch at their defaults."""
    yield mod_ctx
    mod_ctx.set_gather_mode(0)
    mod_ctx.set_integrator(0, 1, 0)
    mod_ctx.set_kernel(0)
    mod_ctx.set_locality(4, 0)


def _fused(ctx, scheme, x, k, dt, steps, nslots, save_every=2, a0=A0, da=DA):
    kick, it, comp = scheme
    ctx.set_integrator(kick, it, comp)
    ctx.packets_set(x, k)
    ctx.advance(dt, steps, F, GH, nslots=nslots, alpha0=a0, dalpha=da, bump=BUMP, save_every=save_every)
    xg, kg = ctx.packets_get()
    hx, hk = ctx.history() if save_every else (None, None)
    return xg, kg, hx, hk


def _sequential(ctx, scheme, x, k, dt, steps, nslots, save_every=2, a0=A0, da=DA):
    """The same steps as single-stage, single-step advance calls."""
    import swraytracing_amd as sw
    kick, it, comp = scheme
    w, off = sw.integrator_weights(comp)
    ctx.set_integrator(kick, it, 0)
    ctx.packets_set(x, k)
    hx, hk = [], []
    for s in range(steps):
        a_s = a0 + float(s) * da
        for wj, oj in zip(w, off):
            ctx.advance(float(wj) * dt, 1, F, GH, nslots=nslots, alpha0=a_s + float(oj) * da, dalpha=0.0, bump=BUMP)
        if save_every and (s + 1) % save_every == 0:
            xs, ks = ctx.packets_get()
            hx.append(xs.T.copy())
            hk.append(ks.T.copy())
    xg, kg = ctx.packets_get()
    return xg, kg, (np.array(hx) if save_every else None), (np.array(hk) if save_every else None)


def _check_fused_is_sequential(ctx, scheme, x, k, dt, steps, nslots, save_every=2):
    fx, fk, fhx, fhk = _fused(ctx, scheme, x, k, dt, steps, nslots, save_every)
    sx, sk, shx, shk = _sequential(ctx, scheme, x, k, dt, steps, nslots, save_every)
    assert np.isfinite(fx).all() and np.isfinite(fk).all()
    assert not np.array_equal(fk, k)  # (the packets moved)
    _assert_same(fx, sx, "x, fused against sequential stages")
    _assert_same(fk, sk, "k, fused against sequential stages")
    if save_every:
        assert fhx.shape == (steps // save_every, 2, x.shape[0])
        _assert_same(fhx, shx, "history x, fused against sequential stages")
        _assert_same(fhk, shk, "history k, fused against sequential stages")


@pytest.mark.parametrize("nx", [32, 64])
@pytest.mark.parametrize("kind", ["psi", "grid6"])
@pytest.mark.parametrize("nslots", [1, 2])
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("scheme", SCHEMES, ids=lambda s: "k%d_it%d_c%d" % s)
def test_fused_is_sequential(ictx, scheme, variant, nslots, kind, nx):
    ctx = ictx
    _set_fields(ctx, nx, kind, nslots)
    ctx.set_kernel(variant)
    x, k = _packets(N)
    dt = 0.05 * (L / nx) / 0.2 * 4
    _check_fused_is_sequential(ctx, scheme, x, k, dt, STEPS, nslots)


def test_fused_is_sequential_two_part_streams(ictx):
    """65,536 + 257 packets at nx = 64: the tile launches run as two part launches."""
    ctx, nx = ictx, 64
    _set_fields(ctx, nx, "psi")
    x, k = _packets(65_536 + 257, seed=8)
    _check_fused_is_sequential(ctx, (1, 2, 1), x, k, 0.05 * (L / nx) / 0.2 * 4, STEPS, 2)


def test_packets_leave_the_window(ictx, qg_case):
    """40 long steps without a re-binning: packets leave the staged window, so
    the global gathers (u, v alone and the full one) run; the tile kernel, the
    per-packet kernel and the sequential stages agree bit for bit."""
    ctx, nx = ictx, 64
    _set_fields(ctx, nx, "psi")
    x, k = _packets(4096 + 257, seed=9)
    dt = 8 * qg_case["dt"]
    scheme = (1, 2, 1)
    ctx.set_locality(1000, 16)
    ctx.set_kernel(2)
    fx, fk, _, _ = _fused(ctx, scheme, x, k, dt, 40, 2, save_every=0, a0=0.5 / 40, da=1.0 / 40)
    dx = L / nx
    assert (np.abs(fx - x).max(axis=1) > 19 * dx).sum() > 50  # beyond a tile and its margin
    ctx.set_kernel(1)
    px, pk, _, _ = _fused(ctx, scheme, x, k, dt, 40, 2, save_every=0, a0=0.5 / 40, da=1.0 / 40)
    _assert_same(fx, px, "x, tile kernel against per-packet kernel")
    _assert_same(fk, pk, "k, tile kernel against per-packet kernel")
    ctx.set_locality(4, 0)  # (re-binning mid-way)
    ctx.set_kernel(2)
    sx, sk, _, _ = _sequential(ctx, scheme, x, k, dt, 40, 2, save_every=0, a0=0.5 / 40, da=1.0 / 40)
    _assert_same(fx, sx, "x, fused against sequential stages")
    _assert_same(fk, sk, "k, fused against sequential stages")


@pytest.mark.parametrize("nslots", [1, 2])
@pytest.mark.parametrize("scheme", [(1, 2, 0), (1, 4, 1)], ids=lambda s: "k%d_it%d_c%d" % s)
@pytest.mark.parametrize("variant", [1, 2])
def test_equals_restatement(ictx, variant, scheme, nslots):
    """The midpoint formula: the device against the numpy restatement over the
    oracle's interpolation of the device's own planes."""
    import swraytracing_amd as sw
    ctx, nx = ictx, 32
    _set_fields(ctx, nx, "psi", nslots)
    ctx.set_kernel(variant)
    snaps = []
    for s in range(nslots):
        pl = ctx.get_field_grid(s)
        snaps.append(orc.GridField({n: pl[i].reshape((nx, nx), order="F") for i, n in enumerate(orc.FIELD_ORDER)},
                                   L / nx))
    flow = ref.grid_flow(snaps[0], snaps[1] if nslots == 2 else None, BUMP)
    x, k = _packets(N)
    dt = 0.05 * (L / nx) / 0.2 * 4
    kick, it, comp = scheme
    w, off = sw.integrator_weights(comp)
    rx, rk, rhx, rhk = ref.integrate(x, k, dt, 5, F, GH, flow, w, off, kick, it, A0, DA, save_every=1)
    gx, gk, ghx, ghk = _fused(ctx, scheme, x, k, dt, 5, nslots, save_every=1)
    _assert_same(gx, rx, "x against the restatement")
    _assert_same(gk, rk, "k against the restatement")
    _assert_same(ghx, np.array([a.T for a in rhx]), "history x against the restatement")
    _assert_same(ghk, np.array([a.T for a in rhk]), "history k against the restatement")


def test_advance_intervals_is_three_advances(ictx):
    ctx, nx, nsub = ictx, 32, 2
    x, k = _packets(N)
    dts = [0.11, 0.13, 0.09]
    ctx.set_kernel(2)
    ctx.set_locality(4 * nsub, 0)
    ctx.set_integrator(1, 4, 1)
    for s in range(4):
        ctx.set_field_psi(s, _psi(nx, 0.4 * s), nx, L)
    ctx.packets_set(x, k)
    ctx.advance_intervals(dts, nsub, F, GH, alpha0=0.5 / nsub, dalpha=1.0 / nsub, bump=BUMP, save_every=1)
    ix, ik = ctx.packets_get()
    ihx, ihk = ctx.history()
    ctx.packets_set(x, k)
    for i, h in enumerate(dts):
        ctx.set_field_psi(0, _psi(nx, 0.4 * i), nx, L)
        ctx.set_field_psi(1, _psi(nx, 0.4 * (i + 1)), nx, L)
        ctx.advance(h, nsub, F, GH, nslots=2, alpha0=0.5 / nsub, dalpha=1.0 / nsub, bump=BUMP, save_every=1)
    ax, ak = ctx.packets_get()
    ahx, ahk = ctx.history()
    _assert_same(ix, ax, "x")
    _assert_same(ik, ak, "k")
    assert ihx.shape == (3 * nsub, 2, N)
    _assert_same(ihx, ahx, "history x")
    _assert_same(ihk, ahk, "history k")


@pytest.mark.parametrize("variant", [1, 2])
def test_default_is_todays_step(ictx, variant):
    """Back at (0, 1, 0) after a non-default run: the oracle's leapfrog bits."""
    ctx, nx = ictx, 32
    _set_fields(ctx, nx, "psi")
    ctx.set_kernel(variant)
    x, k = _packets(N)
    dt = 0.05 * (L / nx) / 0.2 * 4
    _fused(ctx, (1, 2, 2), x, k, dt, STEPS, 2)
    ctx.set_integrator(0, 1, 0)
    assert ctx.get_integrator() == (0, 1, 0)
    gx, gk, _, _ = _fused(ctx, (0, 1, 0), x, k, dt, STEPS, 2)
    snaps = []
    for s in range(2):
        pl = ctx.get_field_grid(s)
        snaps.append(orc.GridField({n: pl[i].reshape((nx, nx), order="F") for i, n in enumerate(orc.FIELD_ORDER)},
                                   L / nx))
    ox, ok, _, _ = orc.leapfrog(x, k, dt, STEPS, F, GH, snaps[0], snaps[1], A0, DA, BUMP)
    _assert_same(gx, ox, "x against oracle.leapfrog")
    _assert_same(gk, ok, "k against oracle.leapfrog")


def test_fma_gather_is_rejected(ictx):
    import swraytracing_amd as sw
    ctx, nx = ictx, 32
    _set_fields(ctx, nx, "psi")
    x, k = _packets(N)
    ctx.packets_set(x, k)
    ctx.set_integrator("midpoint", 2, None)
    ctx.set_gather_mode(1)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*FMA gather"):
        ctx.advance(0.1, 2, F, GH, nslots=2, alpha0=A0, dalpha=DA, bump=BUMP)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*FMA gather"):
        ctx.advance_intervals([0.1], 2, F, GH, alpha0=A0, dalpha=DA, bump=BUMP)
    gx, gk = ctx.packets_get()
    _assert_same(gx, x, "x untouched")
    _assert_same(gk, k, "k untouched")
    ctx.set_integrator(0, 1, 0)
    ctx.advance(0.1, 2, F, GH, nslots=2, alpha0=A0, dalpha=DA, bump=BUMP)  # the FMA gather keeps today's step


@pytest.mark.parametrize("args", [(2, 1, 0), (-1, 1, 0), (1, 0, 0), (1, 5, 1), (1, 2, 3), (0, 1, -1)])
def test_bad_settings_are_rejected(ictx, args):
    import swraytracing_amd as sw
    ictx.set_integrator(1, 3, 2)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
        ictx.set_integrator(*args)
    assert ictx.get_integrator() == (1, 3, 2)
    ictx.set_integrator(0, 9, 1)  # iterations are ignored for the Euler kick
    assert ictx.get_integrator() == (0, 1, 1)


@pytest.fixture(scope="module")
def device_orders(mod_ctx):
    """max|r| of the device's own Omega series on the steady case, per method and dt,
    with the trajectories of the diagnostics run."""
    import swraytracing_amd as sw
    c = ref.steady_case()
    sch = sw.SpectralScheme(c["L"], c["nx"], c["psi"], bump=BUMP, ctx=mod_ctx)
    x0, k0 = c["x0"].T[None], c["k0"].T[None]
    out = {}
    for m in ("leapfrog", "midpoint", "yoshida4", "suzuki4"):
        for dt, n in ((0.2, 10), (0.1, 20), (0.05, 40)):
            x, k, t, d = sw.ode_symplectic(x0, k0, dt, (n + 1) * dt * (1 + 1e-12), F, GH, sch, diagnostics=True, method=m)
            assert x.shape[0] == n + 1 and d.shape == (n + 1, 8)
            out[m, dt] = (d[:, 1].max(), x, k)
    mod_ctx.set_integrator(0, 1, 0)
    return c, sch, out


def test_device_omega_series_shows_the_orders(device_orders):
    _, _, out = device_orders
    e = {key: v[0] for key, v in out.items()}
    for m in ("leapfrog", "midpoint", "yoshida4", "suzuki4"):
        print(m, [e[m, dt] for dt in (0.2, 0.1, 0.05)])
    assert 1.7 <= e["leapfrog", 0.2] / e["leapfrog", 0.1] <= 2.4
    assert e["midpoint", 0.2] / e["midpoint", 0.1] >= 3.5
    assert e["yoshida4", 0.2] / e["yoshida4", 0.1] >= 10
    assert e["midpoint", 0.05] < e["leapfrog", 0.05] / 20


@pytest.mark.parametrize("method", ["leapfrog", "midpoint", "yoshida4", "suzuki4"])
def test_diagnostics_run_has_the_plain_runs_bits(device_orders, mod_ctx, method):
    import swraytracing_amd as sw
    c, sch, out = device_orders
    before = mod_ctx.get_integrator()
    x, k, t = sw.ode_symplectic(c["x0"].T[None], c["k0"].T[None], 0.1, 21 * 0.1 * (1 + 1e-12), F, GH, sch, method=method)
    assert mod_ctx.get_integrator() == before  # the setting is restored
    _assert_same(x, out[method, 0.1][1], "x")
    _assert_same(k, out[method, 0.1][2], "k")
