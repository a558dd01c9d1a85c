"""The tile kernel's code around the step loop against the C oracle.

swrt_tile.hpp: the kernel comes in a plain form and one with history frames
and several intervals (the host picks), the window is staged by whole rows
with one conditional periodic wrap (the remainder for grids smaller than the
window), a launch that does not sort takes a tile's packets in one pass
instead of batches, and a round's addresses are scalar bases plus the lane's
rank.  None of it may change a bit or a slot: every case is compared bit for
bit with the oracle (or with the same run on one packet stream), in the
original packet order, so the carried permutation is checked with it.
"""
import numpy as np
import pytest

from oracle import cbind, swrt_oracle as orc

pytestmark = pytest.mark.gpu

F, GH = 3.0, 1.0
L = 2 * np.pi
# blend weight alpha = A0 + step * DA, dyadic: a call that starts at step s
# passes alpha0 = A0 + s * DA without a rounding
A0, DA = 0.125, 0.015625
BUMP = orc.BUMP_QG


def _field(nx, phase):
    """Six planes of a smooth divergence-free flow (v_y = -u_x bit for bit),
    periodic with L in both directions, |U| about 0.2."""
    xs = np.arange(nx) * (L / nx)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    k0 = 2 * np.pi / L
    z = np.zeros_like(X)
    f = {n: z.copy() for n in ("u", "v", "ux", "uy", "vx")}
    for kx, ky, amp, ph in [(1, 2, 0.05, 0.3), (3, -1, 0.03, 1.1), (2, 5, 0.012, 2.0)]:
        a, b = kx * k0, ky * k0
        s, c = np.sin(a * X + b * Y + ph + phase), np.cos(a * X + b * Y + ph + phase)
        amp = amp / k0
        f["u"] += -amp * b * c
        f["v"] += amp * a * c
        f["ux"] += amp * a * b * s
        f["uy"] += amp * b * b * s
        f["vx"] += -amp * a * a * s
    f["vy"] = -f["ux"]
    return cbind.planes_of(f)


def _wavevectors(n, rng):
    th = 2 * np.pi * rng.random(n)
    return 4.0 * np.stack([np.cos(th), np.sin(th)], axis=1)


def _box(n, lo, span, rng):
    """n positions uniform in [lo, lo + span)^2 (lo: one value or a pair)."""
    return np.asarray(lo, dtype=np.float64) + rng.random((n, 2)) * span


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _assert_same(got, want, what):
    g, w = _bits(got).reshape(-1), _bits(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} values differ, first at flat index {bad[:6]}"


@pytest.fixture()
def own_ctx():
    import swraytracing_amd as sw
    c = sw.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fields64():
    return [_field(64, ph) for ph in (0.0, 0.4, 0.9)]


def _steps(ctx, first, count, dt, per_call=1):
    """`count` steps from global step `first` in calls of `per_call`."""
    for s in range(first, first + count, per_call):
        ctx.advance(dt, per_call, F, GH, nslots=2, alpha0=A0 + s * DA, dalpha=DA, bump=BUMP)


@pytest.mark.parametrize("sparse", [1, 2], ids=["dense512", "sparse256"])
def test_overflow_tile_single_pass(own_ctx, oracle_lib, fields64, sparse):
    """One tile with 2,100 packets and one with exactly 1,024 (the dense
    shape's batch; the sparse shape's is 512), 12 one-step launches with
    re-binning every 4: each cycle is a sort launch, in batches, and three
    launches without a sort, in one pass.  The packets sit in their tiles'
    inner 8 x 8 cells and move at most a quarter cell per step, so the two
    counts hold at every re-binning.  Every packet equals the oracle."""
    nx, ctx = 64, own_ctx
    dx = L / nx
    rng = np.random.default_rng(31)
    x = np.concatenate([_box(2100, (20 * dx, 36 * dx), 8 * dx, rng),   # tile (1, 2)
                        _box(1024, (36 * dx, 20 * dx), 8 * dx, rng),   # tile (2, 1)
                        _box(500, (52 * dx, 0.0), (8 * dx, L), rng)])  # row 3: the other tiles
    x = x[rng.permutation(len(x))]
    k = _wavevectors(len(x), rng)
    p0, p1 = fields64[0], fields64[1]
    ctx.set_field_grid(0, p0, nx, L, 2 * nx)
    ctx.set_field_grid(1, p1, nx, L, 2 * nx)
    dt = 0.05 * dx / 0.2
    ctx.set_locality(4, 0)
    ctx.set_sparse_tiles(sparse)
    ctx.packets_set(x, k)
    _steps(ctx, 0, 12, dt)
    xg, kg = ctx.packets_get()
    xo, ko, _, _ = oracle_lib.leapfrog(p0, p1, A0, DA, nx, 2 * nx, dx, BUMP, x, k, dt, 12, F, GH)
    # the layout the case is about: nobody left the inner cells' tiles
    tiles = (np.floor(xo[:, 0] / dx).astype(int) // 16) * 4 + np.floor(xo[:, 1] / dx).astype(int) // 16
    assert np.count_nonzero(tiles == 1 * 4 + 2) == 2100 and np.count_nonzero(tiles == 2 * 4 + 1) == 1024
    _assert_same(xg, xo, "x against the oracle")
    _assert_same(kg, ko, "k against the oracle")


@pytest.mark.parametrize("nx,yfac,kernel", [(64, 2, 0), (48, 1, 0), (16, 1, 2)], ids=["nx64", "nx48", "nx16_one_tile"])
def test_window_wraps_at_the_periodic_seam(own_ctx, oracle_lib, nx, yfac, kernel):
    """Packets only in the corner tiles (0, 0) and (ntx-1, ntx-1), within two
    cells of the periodic seam (a step moves them up to a quarter cell, so
    some cross it): their stencils read the wrapped part of the window.  64^2
    and 48^2 (three tiles a side, y period nx) take one conditional wrap;
    16^2 is one tile whose 27-node window is wider than the grid: the
    remainder.  8 one-step launches, re-binning every 4."""
    ctx = own_ctx
    dx = L / nx
    rng = np.random.default_rng(32)
    x = np.concatenate([_box(600, 0.0, 2 * dx, rng), _box(600, L - 2 * dx, 2 * dx, rng)])
    x[:4] = [[0.0, 0.0], [-0.0, dx], [L - dx, L - 0.25 * dx], [0.5 * dx, -0.0]]
    x = x[rng.permutation(len(x))]
    k = _wavevectors(len(x), rng)
    p0, p1 = _field(nx, 0.0), _field(nx, 0.4)
    ctx.set_field_grid(0, p0, nx, L, yfac * nx)
    ctx.set_field_grid(1, p1, nx, L, yfac * nx)
    dt = 0.05 * dx / 0.2
    ctx.set_kernel(kernel)
    ctx.set_locality(4, 0)
    ctx.set_sparse_tiles(1)
    ctx.packets_set(x, k)
    _steps(ctx, 0, 8, dt)
    xg, kg = ctx.packets_get()
    xo, ko, _, _ = oracle_lib.leapfrog(p0, p1, A0, DA, nx, yfac * nx, dx, BUMP, x, k, dt, 8, F, GH)
    _assert_same(xg, xo, "x against the oracle")
    _assert_same(kg, ko, "k against the oracle")


@pytest.fixture(scope="module")
def dispatch_case(oracle_lib, fields64):
    """Packets, step sizes and the oracle's results of the three calls of
    test_dispatch_*: 8 steps of one interval (frames every 2 steps), and two
    intervals of 4 steps over three snapshots (alpha restarts per interval)."""
    nx = 64
    dx = L / nx
    rng = np.random.default_rng(33)
    x = _box(6000, 0.0, L, rng)
    k = _wavevectors(len(x), rng)
    dt = 0.05 * dx / 0.2
    hs = [dt, 0.9 * dt]
    p = fields64
    lf = oracle_lib.leapfrog
    one = lf(p[0], p[1], A0, DA, nx, 2 * nx, dx, BUMP, x, k, dt, 8, F, GH, save_every=2)
    xa, ka, hxa, hka = lf(p[0], p[1], A0, DA, nx, 2 * nx, dx, BUMP, x, k, hs[0], 4, F, GH, save_every=2)
    xb, kb, hxb, hkb = lf(p[1], p[2], A0, DA, nx, 2 * nx, dx, BUMP, xa, ka, hs[1], 4, F, GH, save_every=2)
    two = (xb, kb, np.concatenate([hxa, hxb]), np.concatenate([hka, hkb]))
    return dict(nx=nx, x=x, k=k, dt=dt, hs=hs, one=one, two=two)


def _dispatch_ctx(ctx, c, fields):
    for slot, p in enumerate(fields):
        ctx.set_field_grid(slot, p, c["nx"], L, 2 * c["nx"])
    ctx.set_locality(20, 0)   # the whole call in one launch
    ctx.set_sparse_tiles(1)   # the 512-thread shape, the flagship's
    ctx.packets_set(c["x"], c["k"])
    ctx.history_reset()


def test_dispatch_plain_call(own_ctx, oracle_lib, fields64, dispatch_case):
    """No history, one interval: the plain form of the kernel."""
    c, ctx = dispatch_case, own_ctx
    _dispatch_ctx(ctx, c, fields64)
    ctx.advance(c["dt"], 8, F, GH, nslots=2, alpha0=A0, dalpha=DA, bump=BUMP)
    xg, kg = ctx.packets_get()
    _assert_same(xg, c["one"][0], "x against the oracle")
    _assert_same(kg, c["one"][1], "k against the oracle")


def test_dispatch_history_call(own_ctx, oracle_lib, fields64, dispatch_case):
    """History frames every 2 steps: the other form; frames and final state."""
    c, ctx = dispatch_case, own_ctx
    _dispatch_ctx(ctx, c, fields64)
    ctx.advance(c["dt"], 8, F, GH, nslots=2, alpha0=A0, dalpha=DA, bump=BUMP, save_every=2)
    xg, kg = ctx.packets_get()
    hx, hk = ctx.history()
    assert hx.shape == c["one"][2].shape
    for got, want, what in zip((xg, kg, hx, hk), c["one"], ("x", "k", "history x", "history k")):
        _assert_same(got, want, what + " against the oracle")


def test_dispatch_two_intervals_with_history(own_ctx, oracle_lib, fields64, dispatch_case):
    """Two intervals of 4 steps in one launch, frames every 2 steps."""
    c, ctx = dispatch_case, own_ctx
    _dispatch_ctx(ctx, c, fields64)
    ctx.advance_intervals(c["hs"], 4, F, GH, alpha0=A0, dalpha=DA, bump=BUMP, save_every=2)
    xg, kg = ctx.packets_get()
    hx, hk = ctx.history()
    assert hx.shape == c["two"][2].shape
    for got, want, what in zip((xg, kg, hx, hk), c["two"], ("x", "k", "history x", "history k")):
        _assert_same(got, want, what + " against the oracle")


def test_two_part_streams_equal_one(own_ctx, oracle_lib, fields64):
    """65,536 packets on 64^2 (the split's threshold, 16 tiles): 8 steps in
    calls of 2 across one re-binning on two part streams are bit-equal to the
    same run on one stream; a subset equals the oracle."""
    nx, ctx = 64, own_ctx
    dx = L / nx
    rng = np.random.default_rng(34)
    n = 65_536
    x = _box(n, 0.0, L, rng)
    k = _wavevectors(n, rng)
    p0, p1 = fields64[0], fields64[1]
    ctx.set_field_grid(0, p0, nx, L, 2 * nx)
    ctx.set_field_grid(1, p1, nx, L, 2 * nx)
    dt = 0.05 * dx / 0.2
    ctx.set_locality(4, 0)
    out = []
    for streams in (2, 1):
        ctx.set_packet_streams(streams)
        ctx.packets_set(x, k)
        _steps(ctx, 0, 8, dt, per_call=2)
        out.append(ctx.packets_get())
    _assert_same(out[0][0], out[1][0], "x on two streams against one")
    _assert_same(out[0][1], out[1][1], "k on two streams against one")
    idx = np.sort(rng.choice(n, 1000, replace=False))
    xo, ko, _, _ = oracle_lib.leapfrog(p0, p1, A0, DA, nx, 2 * nx, dx, BUMP, x[idx], k[idx], dt, 8, F, GH)
    _assert_same(out[0][0][idx], xo, "x against the oracle")
    _assert_same(out[0][1][idx], ko, "k against the oracle")
