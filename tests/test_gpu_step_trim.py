"""The trimmed step loop and the re-binning kernels against the C oracle.

Step loop (swrt_kernels.hpp / swrt_tile.hpp): the Lagrange weights carry
kScale in a Markstein step's constants, cell_frac takes its power-of-two and
single-wrap short paths, and the tile kernel tests the window by ring
position.  Re-binning (swrt_bin.hpp): the scan runs on wave shuffles and the
scatter ranks runs of equal keys.  None of it may change a bit: every case
here is compared bit for bit with the oracle (interpolate.m:21-49 and
ode_symplectic.m:10-28 in C), with a re-binning and a sort launch inside the
run, on periods that take the short paths and on periods that do not.
"""
import numpy as np
import pytest

from oracle import cbind, swrt_oracle as orc

pytestmark = pytest.mark.gpu

F, GH = 3.0, 1.0
# blend weight alpha = A0 + step * DA; dyadic, so that a call's alpha0 = A0 +
# (its first step) * DA plus the step within the call is the oracle's A0 +
# step * DA without a rounding
A0, DA = 0.125, 0.015625
NSUB = 5             # steps per advance call (one fused launch each)


def _field(nx, L, phase):
    """Six planes of a smooth divergence-free flow (v_y = -u_x bit for bit),
    periodic with L in both directions, |U| about 0.2."""
    xs = np.arange(nx) * (L / nx)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    k0 = 2 * np.pi / L
    modes = [(1, 2, 0.05, 0.3), (3, -1, 0.03, 1.1), (2, 5, 0.012, 2.0)]
    z = np.zeros_like(X)
    f = {n: z.copy() for n in ("u", "v", "ux", "uy", "vx")}
    for kx, ky, amp, ph in modes:
        a, b = kx * k0, ky * k0
        s, c = np.sin(a * X + b * Y + ph + phase), np.cos(a * X + b * Y + ph + phase)
        amp = amp / k0
        f["u"] += -amp * b * c     # -psi_y, psi = amp * sin
        f["v"] += amp * a * c      # psi_x
        f["ux"] += amp * a * b * s
        f["uy"] += amp * b * b * s
        f["vx"] += -amp * a * a * s
    f["vy"] = -f["ux"]
    return cbind.planes_of(f)


def _packets(n, nx, L, seed, lo=(0.0, 0.0), span=None):
    """Random packets in [lo, lo + span)^2 (default the whole domain); the
    first 12 sit exactly on cell edges, on the period and at x = +-0."""
    rng = np.random.default_rng(seed)
    x, k = orc.initial_packets(n, L, 4.0, F, np.sqrt(GH), rng)
    dx = L / nx
    if span is not None:
        x = np.asarray(lo)[None, :] + rng.random((n, 2)) * span
    edge = np.array([[0.0, 0.0], [-0.0, 3 * dx], [5 * dx, -0.0], [-0.0, -0.0], [7 * dx, 7 * dx], [16 * dx, 2.5 * dx],
                     [2.5 * dx, 16 * dx], [L, 0.5 * dx], [0.5 * dx, L], [(nx - 1) * dx, (nx - 1) * dx],
                     [-3 * dx, 2 * L], [31 * dx, -17 * dx]])
    if span is None:
        x[:len(edge)] = edge
    return np.asfortranarray(x), np.asfortranarray(k)


def _advance(ctx, steps, dt, nslots, bump):
    for c in range(steps // NSUB):
        ctx.advance(dt, NSUB, F, GH, nslots=nslots, alpha0=A0 + c * NSUB * DA, dalpha=DA, bump=bump)


def _oracle(p0, p1, nx, yper, L, bump, x, k, dt, steps):
    xo, ko, _, _ = cbind.leapfrog(p0, p1, A0, DA, nx, yper, L / nx, bump, x, k, dt, steps, F, GH)
    return xo, ko


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _assert_same(got, want, what, rows=None):
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    if bad.size:
        r = bad[:6]
        ids = r if rows is None else np.asarray(rows)[r]
        lines = [f"row {i}: got {got[j, 0].hex()} {got[j, 1].hex()} want {want[j, 0].hex()} {want[j, 1].hex()}"
                 for i, j in zip(ids, r)]
        raise AssertionError(f"{what}: {bad.size} of {len(got)} rows differ\n" + "\n".join(lines))


CONFIGS = {
    # nx, y period / nx, snapshots, packets, kernel variant
    "pow2_blend_tile": (64, 2, 2, 65_536, 0),   # 16 tiles, two-stream tile launches, both short paths of x
    "nx48_single_tile": (48, 1, 1, 4_096, 0),   # 9 tiles, div_rn and one wrap in both directions
    "pow2_per_packet": (64, 2, 2, 8_192, 1),    # cell_frac / lagrange_w outside the tile kernel
}


@pytest.fixture()
def own_ctx():
    import swraytracing_amd as sw
    c = sw.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("bump", [orc.BUMP_QG, 0.0], ids=["bump_qg", "bump0"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_leapfrog_25_steps_with_rebinning_bitexact(own_ctx, oracle_lib, name, bump):
    """25 steps in calls of 5 with re-binning every 20 (one re-binning and one
    sort launch inside the run): a subset holding the cell-edge and +-0
    packets is bit-identical to the oracle."""
    nx, yfac, nslots, n, variant = CONFIGS[name]
    ctx, L = own_ctx, 2 * np.pi
    p0 = _field(nx, L, 0.0)
    p1 = _field(nx, L, 0.4) if nslots == 2 else None
    ctx.set_field_grid(0, p0, nx, L, yfac * nx)
    if nslots == 2:
        ctx.set_field_grid(1, p1, nx, L, yfac * nx)
    x, k = _packets(n, nx, L, 5)
    dt = 0.05 * (L / nx) / 0.2
    ctx.set_kernel(variant)
    ctx.set_locality(20, 0)
    ctx.packets_set(x, k)
    _advance(ctx, 25, dt, nslots, bump)
    xg, kg = ctx.packets_get()
    idx = np.unique(np.concatenate([np.arange(16), np.random.default_rng(1).choice(n, 2000, replace=False)]))
    xo, ko = _oracle(p0, p1, nx, yfac * nx, L, bump, x[idx], k[idx], dt, 25)
    _assert_same(xg[idx], xo, "x against the oracle", idx)
    _assert_same(kg[idx], ko, "k against the oracle", idx)


@pytest.fixture(scope="module")
def rebin_case():
    nx, L = 64, 2 * np.pi
    return dict(nx=nx, L=L, p0=_field(nx, L, 0.0), p1=_field(nx, L, 0.4), dt=0.05 * (L / nx) / 0.2, n=65_536)


def _placed(c, layout):
    nx, L, n = c["nx"], c["L"], c["n"]
    dx = L / nx
    if layout == "spread":
        return _packets(n, nx, L, 9)
    if layout == "one_tile":       # one key run spanning whole waves
        return _packets(n, nx, L, 10, lo=(16 * dx, 32 * dx), span=16 * dx)
    x, k = _packets(n, nx, L, 11, lo=(0.0, 0.0), span=16 * dx)  # keys alternate between two tiles: runs of 1
    x[1::2] += np.array([32 * dx, 16 * dx])[None, :]
    return x, k


@pytest.mark.parametrize("layout", ["spread", "one_tile", "two_tiles_alternating"])
def test_rebinning_keeps_every_packet_once(own_ctx, oracle_lib, rebin_case, layout):
    """65,536 packets on 64^2, 40 steps with re-binning every 20: every row of
    packets_get equals the per-packet kernel's run without any binning (so
    each original index is held exactly once, with its own state), and a
    subset equals the oracle."""
    c, ctx = rebin_case, own_ctx
    nx, L, n, dt = c["nx"], c["L"], c["n"], c["dt"]
    ctx.set_field_grid(0, c["p0"], nx, L, 2 * nx)
    ctx.set_field_grid(1, c["p1"], nx, L, 2 * nx)
    x, k = _placed(c, layout)
    ctx.set_locality(20, 0)
    ctx.packets_set(x, k)
    _advance(ctx, 40, dt, 2, orc.BUMP_QG)
    xg, kg = ctx.packets_get()
    ctx.set_kernel(1)
    ctx.set_locality(0, 0)  # no binning: the packets never leave their order
    ctx.packets_set(x, k)
    _advance(ctx, 40, dt, 2, orc.BUMP_QG)
    xu, ku = ctx.packets_get()
    _assert_same(xg, xu, "x against the unbinned per-packet run")
    _assert_same(kg, ku, "k against the unbinned per-packet run")
    assert np.unique(np.ascontiguousarray(kg).view(np.uint64), axis=0).shape[0] == n  # the states are distinct
    idx = np.sort(np.random.default_rng(2).choice(n, 1500, replace=False))
    xo, ko = _oracle(c["p0"], c["p1"], nx, 2 * nx, L, orc.BUMP_QG, x[idx], k[idx], dt, 40)
    _assert_same(xg[idx], xo, "x against the oracle", idx)
    _assert_same(kg[idx], ko, "k against the oracle", idx)


def test_corrupted_count_still_raises(own_ctx, rebin_case):
    """The scan's guard with the shuffle scan: a corrupted tile count leaves an
    empty binning and the next synchronisation reports it; packets_set clears
    the state."""
    import swraytracing_amd as sw
    import swraytracing_amd._lib as lib
    c, ctx = rebin_case, own_ctx
    nx, L, dt = c["nx"], c["L"], c["dt"]
    ctx.set_field_grid(0, c["p0"], nx, L, 2 * nx)
    ctx.set_field_grid(1, c["p1"], nx, L, 2 * nx)
    x, k = _placed(c, "spread")
    ctx.set_locality(20, 0)
    ctx.packets_set(x, k)
    _advance(ctx, 10, dt, 2, orc.BUMP_QG)
    ctx.debug_set(lib.DEBUG_CORRUPT_COUNT, 1000)
    with pytest.raises(sw.SwrtError, match="binning"):
        _advance(ctx, 30, dt, 2, orc.BUMP_QG)  # the re-binning at step 20 meets it
        ctx.synchronize()
    ctx.packets_set(x, k)
    _advance(ctx, 5, dt, 2, orc.BUMP_QG)
    xg, kg = ctx.packets_get()
    assert np.isfinite(xg).all() and np.isfinite(kg).all()
