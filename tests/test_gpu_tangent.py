"""The tangent map on the device (swrt_tangent_*;
swraytracing_amd/csrc/swrt_tangent.hpp).

Expected values are tests/tangent_ref.py, the numpy restatement of the header's
operation order on the oracle's interpolation.  Every comparison is exact: a
float comparison is equality of the bits with the NaN positions equal, the
frames are integers.

The packets are 4099 (64^2, conftest's qg_case flow) and 1000 (32^2, built the
same way) on the initial ring spread by 300 leapfrog steps of the C oracle;
bump 1e-10; the second snapshot is 0.8 x the first, alpha0 = 0.1, dalpha =
0.04.  The restatement runs once per grid, as calls of 1, 4 and 32 steps (37 in
all, checkpoints after 1, 5 and 37), and is shared read-only.  Growth edges
are 2.0 ** (equally spaced exponents) over the restatement's range of
e(s): whole exponents (2.0 ** arange, as the issue words it) where the range
has a binade per class, (1, 1) and (8, 12).  For (126, 126) and (200, 300) the
test departs from the issue's wording: s spans some 10 binades after 37 steps,
so 2.0 ** arange would leave all but ten classes empty and assert_populated,
which the issue also asks for, could not hold; the exponents there are
fractional (2.0 ** linspace over the same range), the shapes and every other
check as the issue sets them."""
import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import cbind, swrt_oracle as orc
from swraytracing_amd._lib import DEBUG_TANGENT_GLOBAL
from tests import tangent_ref as tr
from tests.cond_series_ref import assert_populated, central_edges, omega_of
from tests.test_gpu_refr_series import _flow32

pytestmark = pytest.mark.gpu

BUMP = 1e-10
A0, DA = 0.1, 0.04
CALLS = (1, 4, 32)                      # 37 steps; checkpoints after 1, 5, 37
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
SHAPES = [(1, 1), (8, 12), (126, 126), (200, 300)]  # (ns, nw)


def _spread(q, n, seed):
    rng = np.random.default_rng(seed)
    x0, k0 = orc.initial_packets(n, q["L"], 4.0, q["f"], q["Cg"], rng)
    planes = cbind.planes_of(q["flow"])
    dx = q["L"] / q["nx"]
    x, k, _, _ = cbind.leapfrog(planes, None, 0.0, 0.0, q["nx"], q["nx"], dx, BUMP, x0, k0, q["dt"], 300, q["f"],
                                q["Cg"] ** 2)
    return np.ascontiguousarray(x), np.ascontiguousarray(k), np.asarray(planes), dx


def _reference(q, x, k, dx, nslots, M=None, caus=None, calls=CALLS):
    """The restatement's states after each call of ``calls``: [(x, k, M, caustics), ...]."""
    flows = [q["flow"], {n: 0.8 * np.asarray(v) for n, v in q["flow"].items()}][:nslots]
    if M is None:
        M, caus = tr.identity(x.shape[0])
    out = []
    for steps in calls:
        x, k, M, caus = tr.tangent_leapfrog(x, k, M, caus, q["dt"], steps, q["f"], q["Cg"] ** 2, flows, dx,
                                            A0 if nslots == 2 else 0.0, DA if nslots == 2 else 0.0, BUMP)
        out.append((x, k, M, caus))
    for st in out:
        for a in st:
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def cases(qg_case):
    """64^2 with two snapshots and 4099 packets, 32^2 steady with 1000."""
    out = {}
    for nx, q, n, nslots, seed in ((64, qg_case, 4099, 2, 33), (32, _flow32(), 1000, 1, 34)):
        x, k, planes, dx = _spread(q, n, seed)
        out[nx] = dict(q=q, x=x, k=k, planes=planes, dx=dx, nslots=nslots, ref=_reference(q, x, k, dx, nslots))
    return out


@pytest.fixture(scope="module")
def plain_ctx():
    """A second context that never has a tangent set: the default (tile) route."""
    c = sw.Context(0)
    yield c
    c.close()


@pytest.fixture()
def tctx(ctx):
    """The session context, left without a tangent set, on its default settings."""
    yield ctx
    if ctx.tangent_live():
        ctx.tangent_end()
    ctx.set_integrator("euler", 1, None)
    ctx.set_gather_mode(0)
    ctx.set_locality(4, 0)
    ctx.debug_set(DEBUG_TANGENT_GLOBAL, 0)
    ctx.history_reset()


def _fields(c, cs, slots=2):
    q = cs["q"]
    for s in range(slots):
        c.set_field_grid(s, (0.8 ** s) * cs["planes"], q["nx"], q["L"])


def _same(got, want, what=""):
    """Equal bits, NaN positions equal."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype == np.float64:
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), f"{what}: NaN positions"
        bad = got.view(np.uint64)[~gn] != want.view(np.uint64)[~wn]
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ in their bits"
    else:
        np.testing.assert_array_equal(got, want, err_msg=what)


def _advance(c, cs, steps, nslots=None, save_every=0):
    q = cs["q"]
    nslots = nslots or cs["nslots"]
    c.advance(q["dt"], steps, q["f"], q["Cg"] ** 2, nslots, A0 if nslots == 2 else 0.0, DA if nslots == 2 else 0.0,
              BUMP, save_every)


def _check_state(c, want, what):
    x, k = c.packets_get()
    M, caus = c.tangent_get()
    _same(x, want[0], what + " x"), _same(k, want[1], what + " k")
    _same(M, want[2], what + " M"), _same(caus, want[3], what + " caustics")


@pytest.mark.parametrize("hist", [0, 5], ids=["nohist", "hist"])
@pytest.mark.parametrize("nslots", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_packet_bits_are_unchanged(tctx, plain_ctx, cases, n, nslots, hist):
    """x, k (and the history frames) after a tangent-live advance and
    advance_intervals (3 intervals, nsub 5) equal a context without a tangent
    set on its default tile route."""
    cs = cases[64]
    q = cs["q"]
    x, k = cs["x"][:n], cs["k"][:n]
    got = []
    for c, live in ((tctx, True), (plain_ctx, False)):
        _fields(c, cs, 4)
        c.packets_set(x, k)
        c.history_reset()
        if live:
            c.tangent_begin()
        _advance(c, cs, 10, nslots, hist)
        c.advance_intervals([q["dt"], 0.9 * q["dt"], 1.1 * q["dt"]], 5, q["f"], q["Cg"] ** 2, A0, DA, BUMP, hist)
        got.append(c.packets_get() + (c.history() if hist else ()))
    assert len(got[0]) == (4 if hist else 2)
    for a, b, name in zip(got[0], got[1], ("x", "k", "hist x", "hist k")):
        _same(a, b, f"n {n} nslots {nslots} {name}")
    if hist:
        assert got[0][2].shape[0] == 2 + 3
    M, caus = tctx.tangent_get()
    assert np.isfinite(M).all() and M.shape == (n, 16) and caus.dtype == np.int32
    assert not np.array_equal(M, tr.identity(n)[0])


@pytest.mark.parametrize("rebin", [5, 0, 4], ids=["rebin5", "locality_off", "default"])
@pytest.mark.parametrize("nx", [64, 32])
def test_maps_equal_the_restatement(tctx, cases, nx, rebin):
    """M and the counters after 1, 5 and 37 steps in calls of 1, 4 and 32: with
    rebin_every = 5 a re-binning falls between (and inside) the launches."""
    cs = cases[nx]
    c = tctx
    _fields(c, cs)
    c.set_locality(rebin, 0)
    c.packets_set(cs["x"], cs["k"])
    c.tangent_begin()
    assert c.tangent_live() and c.tangent_serial() == 1
    M, caus = c.tangent_get()
    _same(M, tr.identity(cs["x"].shape[0])[0], "begin"), assert_zero(caus)
    done = 0
    for steps, want in zip(CALLS, cs["ref"]):
        _advance(c, cs, steps)
        done += steps
        _check_state(c, want, f"{nx}^2 rebin {rebin} after {done} steps")
    J = tr.ray_jacobian(cs["ref"][-1][2])
    assert (J < 0).any() and cs["ref"][-1][3].max() >= 1  # (the restatement's tubes fold: the counters are exercised)


def assert_zero(a):
    assert not np.asarray(a).any()


def test_one_call_equals_split_calls(tctx, cases):
    """Steady flow (no step index enters): 37 steps in one call give the bits of 1 + 4 + 32."""
    cs = cases[32]
    c = tctx
    _fields(c, cs)
    c.packets_set(cs["x"], cs["k"])
    c.tangent_begin()
    _advance(c, cs, 37)
    _check_state(c, cs["ref"][-1], "37 steps at once")


def test_mark_restarts_the_window_and_get_disturbs_nothing(tctx, cases):
    cs = cases[32]
    c, q = tctx, cases[32]["q"]
    _fields(c, cs)
    c.packets_set(cs["x"], cs["k"])
    c.tangent_begin()
    _advance(c, cs, 5)
    c.tangent_get()  # (a get between launches)
    c.tangent_mark()
    assert c.tangent_serial() == 2
    M, caus = c.tangent_get()
    _same(M, tr.identity(1000)[0], "mark"), assert_zero(caus)
    _advance(c, cs, 4)
    x5, k5 = cs["ref"][1][0], cs["ref"][1][1]
    want = _reference(q, x5, k5, cs["dx"], 1, calls=(4,))[0]
    _check_state(c, want, "the window after a mark")
    # the same N marks, another N drops
    c.packets_set(cs["x"], cs["k"])
    assert c.tangent_live() and c.tangent_serial() == 3
    _same(c.tangent_get()[0], tr.identity(1000)[0], "packets_set, same N")
    c.packets_set(cs["x"][:10], cs["k"][:10])
    assert not c.tangent_live() and c.tangent_serial() == 0
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*swrt_tangent_begin"):
        c.tangent_get()


def _planted(cs, n):
    x, k = cs["x"][:n].copy(), cs["k"][:n].copy()
    k[3, 1] = np.nan
    k[4] = [0.0, 0.0]
    k[5] = [1e9, 0.0]
    return x, k


def test_planted_packets(tctx, cases):
    """NaN k, k = 0 and k = 1e9: the run completes, every packet (the planted
    ones too) has the restatement's bits, and the frame rejects or classes
    them as the restatement says."""
    cs = cases[64]
    c, q = tctx, cases[64]["q"]
    n = 257
    x, k = _planted(cs, n)
    _fields(c, cs)
    c.packets_set(x, k)
    c.tangent_begin()
    _advance(c, cs, 5)
    want = _reference(q, x, k, cs["dx"], 2, calls=(5,))[0]
    _check_state(c, want, "planted")
    assert np.isnan(want[2][3]).any() and np.isfinite(want[2][4]).all() and np.isfinite(want[2][5]).all()
    w = omega_of(want[1], q["f"], q["Cg"])
    wedges, gedges = central_edges(w, 12), tr.growth_edges_of(want[2], 8)
    c.tangent_series_begin(q["f"], q["Cg"], wedges, gedges)
    c.tangent_series_record()
    got = c.tangent_series_get()
    frame = tr.tangent_frame_of(want[2], want[3], w, wedges, gedges, 1)
    assert frame[2].tolist() == [n, 1, 1]
    for g, f_, name in zip(got, frame, ("counts", "sums", "stats")):
        _same(g[0], f_, "planted frame " + name)


@pytest.mark.parametrize("path", [0, 1], ids=["by_shape", "global"])
@pytest.mark.parametrize("ns,nw", SHAPES)
def test_series_frames(tctx, cases, ns, nw, path):
    """Frames after 5 and 37 steps (and one after a mark) against the
    restatement's; (200, 300) takes the global kernel by its shape, the debug
    switch sends every shape there.  The growth-axis marginal plus the
    rejected count is the omega series' row."""
    cs = cases[64]
    c, q = tctx, cases[64]["q"]
    ref5, ref37 = cs["ref"][1], cs["ref"][2]
    w37 = omega_of(ref37[1], q["f"], q["Cg"])
    wedges, gedges = central_edges(w37, nw), tr.growth_edges_of(ref37[2], ns)
    want37 = tr.tangent_frame_of(ref37[2], ref37[3], w37, wedges, gedges, 1)
    assert want37[2].tolist() == [4099, 0, 1]
    assert_populated(want37[0])
    _fields(c, cs)
    c.debug_set(DEBUG_TANGENT_GLOBAL, path)
    c.packets_set(cs["x"], cs["k"])
    c.tangent_begin()
    c.tangent_series_begin(q["f"], q["Cg"], wedges, gedges)
    c.omega_series_begin(q["f"], q["Cg"], wedges)
    assert c.tangent_series_bins() == (nw, ns) and c.tangent_series_frames() == 0
    _advance(c, cs, 1), _advance(c, cs, 4)
    c.tangent_series_record()
    _advance(c, cs, 32)
    c.tangent_series_record()
    c.omega_series_record()
    c.tangent_mark()
    c.tangent_series_record()
    got = c.tangent_series_get()
    assert c.tangent_series_frames() == 3 and got[0].shape == (3, ns + 2, nw + 2)
    assert got[1].shape == (3, 3 * (nw + 2) + ns + 2) and got[2].shape == (3, 3)
    want5 = tr.tangent_frame_of(ref5[2], ref5[3], omega_of(ref5[1], q["f"], q["Cg"]), wedges, gedges, 1)
    M0, c0 = tr.identity(4099)
    want0 = tr.tangent_frame_of(M0, c0, w37, wedges, gedges, 2)
    for t, want in enumerate((want5, want37, want0)):
        for g, f_, name in zip(got, want, ("counts", "sums", "stats")):
            assert g.dtype == np.int64
            _same(g[t], f_, f"({ns}, {nw}) path {path} frame {t} {name}")
    row = c.omega_series()[0][-1]
    np.testing.assert_array_equal(got[0][1].sum(axis=0), row)
    assert got[0][1].sum() + got[2][1, 1] == row.sum() == 4099
    c.tangent_series_reset()
    assert c.tangent_series_frames() == 0


def test_refusals(tctx, cases):
    cs = cases[32]
    c, q = tctx, cases[32]["q"]
    f, gH, dt = q["f"], q["Cg"] ** 2, q["dt"]
    _fields(c, cs)
    c.packets_set(cs["x"][:65], cs["k"][:65])
    state = "SWRT_ERR_STATE.*"
    empty = sw.Context(0)
    with pytest.raises(sw.SwrtError, match=state + "swrt_tangent_series_begin"):
        empty.tangent_series_record()
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*no packets"):
        empty.tangent_begin()
    empty.close()
    for call in (c.tangent_mark, c.tangent_get):
        with pytest.raises(sw.SwrtError, match=state + "swrt_tangent_begin"):
            call()
    wedges = np.linspace(3.0, 15.0, 5)
    c.tangent_series_begin(f, q["Cg"], wedges, 2.0 ** np.arange(4))
    with pytest.raises(sw.SwrtError, match=state + "swrt_tangent_begin"):
        c.tangent_series_record()
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*edges must increase"):
        c.tangent_series_begin(f, q["Cg"], wedges, [1.0, 4.0, 2.0])
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*edges must be finite"):
        c.tangent_series_begin(f, q["Cg"], [1.0, np.nan], [1.0, 2.0])
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*at most 65536"):
        c.tangent_series_begin(f, q["Cg"], np.arange(400.0), 2.0 ** np.arange(300))

    c.tangent_begin()
    x, k = cs["x"][:65].copy(), cs["k"][:65].copy()
    for name, call in (
            ("swrt_ode23_f1", lambda: c.ode23_f1(0.0, 1.0, f, q["Cg"], 1, 1e-3, BUMP)),
            ("swrt_ode23_attempt", lambda: c.ode23_attempt(0.0, dt, dt, 1.0, f, q["Cg"], 1, 1e-3, BUMP)),
            ("swrt_ode23_accept", c.ode23_accept),
            ("swrt_ode23_ntrp", lambda: c.ode23_ntrp(0.0, dt, [0.5 * dt])),
            ("swrt_ode23_run_at", lambda: c.ode23_run_at([0.0, dt, 2 * dt], 1.0, f, q["Cg"], 1, 1e-3, 1e-6, BUMP)),
            ("swrt_ode23_run_sharded", lambda: c.ode23_run(0.0, dt, 1.0, f, q["Cg"], 1, 1e-3, 1e-6, BUMP)),
            ("swrt_xka_step", lambda: c.xka_step(np.zeros((65, 5)), 1.0, f, dt, 1)),
            ("swrt_spectral_leapfrog", lambda: c.spectral_leapfrog(x, k, dt, 1, f, gH)),
            ("swrt_recycle_apply", c.recycle_apply)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE: " + name + ": a tangent set is live"):
            call()
    c.set_integrator("midpoint", 2, None)
    for call in (lambda: c.advance(dt, 1, f, gH, 1, 0.0, 0.0, BUMP),
                 lambda: c.advance_intervals([dt], 1, f, gH, 0.0, 1.0, BUMP),
                 lambda: c.leapfrog(x, k, dt, 1, f, gH, 1, 0.0, 0.0, BUMP)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*tangent set is live.*leapfrog step only"):
            call()
    c.set_integrator("euler", 1, None)
    c.set_gather_mode(1)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*tangent set is live.*mul-then-add"):
        c.advance(dt, 1, f, gH, 1, 0.0, 0.0, BUMP)
    c.set_gather_mode(0)
    # nothing above moved a packet or touched M
    xg, kg = c.packets_get()
    _same(xg, cs["x"][:65], "x after the refusals"), _same(kg, cs["k"][:65], "k after the refusals")
    _same(c.tangent_get()[0], tr.identity(65)[0], "M after the refusals")


def test_leapfrog_call_carries_the_maps(tctx, cases):
    """swrt_leapfrog (set, advance, get) with a live set of the same N: a mark, then the per-packet route."""
    cs = cases[32]
    c, q = tctx, cases[32]["q"]
    _fields(c, cs)
    c.packets_set(cs["x"], cs["k"])
    c.tangent_begin()
    xg, kg, _, _ = c.leapfrog(cs["x"], cs["k"], q["dt"], 1, q["f"], q["Cg"] ** 2, 1, 0.0, 0.0, BUMP)
    want = cs["ref"][0]
    _same(xg, want[0], "x"), _same(kg, want[1], "k")
    assert c.tangent_serial() == 2
    M, caus = c.tangent_get()
    _same(M, want[2], "M"), _same(caus, want[3], "caustics")


def test_after_end_everything_is_as_before(tctx, plain_ctx, cases):
    """After tangent_end an advance has the plain context's bits again and is
    timed the same way (the same number of timed launches)."""
    cs = cases[64]
    q = cs["q"]
    out = []
    for c, live in ((tctx, True), (plain_ctx, False)):
        _fields(c, cs)
        c.packets_set(cs["x"], cs["k"])
        if live:
            c.tangent_begin()
            _advance(c, cs, 3)
            c.tangent_end()
            assert not c.tangent_live()
            c.packets_set(cs["x"], cs["k"])
        c.set_timing(1)
        c.kernel_time(True)
        _advance(c, cs, 12)
        ms, launches = c.kernel_time(True)
        assert ms > 0 and launches > 0
        out.append(c.packets_get() + (launches,))
    _same(out[0][0], out[1][0], "x"), _same(out[0][1], out[1][1], "k")
    assert out[0][2] == out[1][2]
    _same(out[0][0], _plain_reference(cs, 12)[0], "x against the oracle")


def _plain_reference(cs, steps):
    q = cs["q"]
    s0 = orc.GridField(q["flow"], cs["dx"])
    s1 = orc.GridField({n: 0.8 * np.asarray(v) for n, v in q["flow"].items()}, cs["dx"])
    x, k, _, _ = orc.leapfrog(cs["x"], cs["k"], q["dt"], steps, q["f"], q["Cg"] ** 2, s0, s1, A0, DA, BUMP)
    return x, k


# ---- the drivers ----
TANGENT_FILES = ("tangent_hist.bin", "tangent_sums.bin", "tangent_stats.bin", "tangent_time.bin", "tangent_geom.bin")
SPEC_EDGES = np.linspace(9.0, 15.0, 13)  # the ring starts at omega = 12
G_EDGES = 2.0 ** np.arange(5)


def _files(d):
    import os
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


def _watch_frames(monkeypatch, ctx, seen):
    """Before every packet frame that records a tangent frame: the device's M,
    counters, k and mark serial (the record comes before the re-mark)."""
    import swraytracing_amd.qg as qgmod
    saved = qgmod._save_frame

    def save(ens, t, *args, **kw):
        if len(args) > 10 and args[10] is not None:
            seen.append(ctx.tangent_get() + (np.array(ctx.packets_get()[1]), ctx.tangent_serial(), t))
        return saved(ens, t, *args, **kw)

    monkeypatch.setattr(qgmod, "_save_frame", save)


@pytest.mark.parametrize("driver,args,kw", [
    ("qgsw_raytrace", (32, 257, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0), dict(max_steps=25, nsub=2, r_drag=0.0)),
    ("qg2layersw_raytrace", (32, 257, 4.0, 120.0, 0.0, 0.2, 3.0, 1.0), dict(max_steps=100, nsub=2, seed=5))],
    ids=["one_layer", "two_layer"])
def test_driver(ctx, tmp_path, monkeypatch, driver, args, kw):
    """tangent_edges with tangent_lag = 2: the five files equal the
    restatement's frames of the device's states at the packet frames; every
    other file and fact equals a run without the keywords (the packets keep
    their bits through the whole drive)."""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    kw = dict(kw, ctx=ctx, spectrum_edges=SPEC_EDGES)
    seen = []
    _watch_frames(monkeypatch, ctx, seen)
    facts = getattr(sw, driver)(*args, out_dir=a, tangent_edges=G_EDGES, tangent_lag=2, **kw)
    assert not ctx.tangent_live()
    fa = _files(a)
    ns, nw, n = G_EDGES.size - 1, SPEC_EDGES.size - 1, 257
    frames = facts["packet_frames"] - 1
    assert facts["tangent_frames"] == frames == len(seen) >= 4 and set(TANGENT_FILES) <= set(fa)
    nsum = 3 * (nw + 2) + ns + 2
    counts = np.frombuffer(fa["tangent_hist.bin"], dtype=np.int64).reshape(frames, ns + 2, nw + 2)
    sums = np.frombuffer(fa["tangent_sums.bin"], dtype=np.int64).reshape(frames, nsum)
    stats = np.frombuffer(fa["tangent_stats.bin"], dtype=np.int64).reshape(frames, 3)
    times = np.frombuffer(fa["tangent_time.bin"], dtype=np.float64).reshape(frames, 2)
    geom = np.frombuffer(fa["tangent_geom.bin"], dtype=np.float64)
    assert geom.tolist() == [ns, nw] + G_EDGES.tolist() + SPEC_EDGES.tolist()
    ptime = sw.read_field(str(tmp_path / "a" / "packet_time"), 1, 1, 1, is_real=True).ravel()
    t_mark = ptime[0]
    for i, (M, caus, k, serial, t) in enumerate(seen):
        assert serial == 1 + i // 2 and not np.array_equal(M, tr.identity(n)[0])
        want = tr.tangent_frame_of(M, caus, omega_of(k, 3.0, 1.0), SPEC_EDGES, G_EDGES, serial)
        for g, w_, name in zip((counts[i], sums[i], stats[i]), want, ("counts", "sums", "stats")):
            _same(g, w_, f"{driver} frame {i} {name}")
        assert times[i].tolist() == [t, t_mark] and t == ptime[i + 1]
        if (i + 1) % 2 == 0:  # re-marked after every second frame
            t_mark = t
    assert (stats[:, 0] == n).all() and (stats[:, 1] == 0).all() and counts[:, 2:].any()
    g = sw.tangent_growth(counts, sums, stats, times[:, 0] - times[:, 1])
    assert np.nanmax(g["lyapunov"]) > 0
    plain = getattr(sw, driver)(*args, out_dir=b, **kw)
    assert plain["tangent_frames"] == 0
    assert {n_: v for n_, v in fa.items() if n_ not in TANGENT_FILES} == _files(b)
    assert {k_: v for k_, v in facts.items() if k_ != "tangent_frames"} == \
        {k_: v for k_, v in plain.items() if k_ != "tangent_frames"}


def test_ode_symplectic_returns_the_maps(tctx, qg_case):
    """ode_symplectic(..., tangent=True): x, k and t of the plain call, and the
    M and counters the context's own calls give on the scheme's fields."""
    c = qg_case
    psi = orc.k2g(-c["qk"] / (c["K_d2"] + c["K2"]))
    gs = sw.SpectralScheme(c["L"], c["nx"], psi, ctx=tctx)
    P = 65
    x0, k0 = c["x"][:P].T[None].copy(), c["k"][:P].T[None].copy()
    T = c["dt"] * 12.5
    x, k, t, M, caus = sw.ode_symplectic(x0, k0, c["dt"], T, c["f"], 1.0, gs, tangent=True)
    assert not tctx.tangent_live()
    xp, kp, tp = sw.ode_symplectic(x0, k0, c["dt"], T, c["f"], 1.0, gs)
    _same(x, xp, "x"), _same(k, kp, "k"), _same(t, tp, "t")
    assert M.shape == (P, 4, 4) and caus.shape == (P,) and caus.dtype == np.int32
    tctx.packets_set(c["x"][:P], c["k"][:P])
    tctx.tangent_begin()
    tctx.advance(c["dt"], 11, c["f"], 1.0, nslots=1, bump=gs.bump)
    Mc, cc = tctx.tangent_get()
    _same(M.reshape(P, 16), Mc, "M"), _same(caus, cc, "caustics")
    with pytest.raises(ValueError, match="tangent needs"):
        sw.ode_symplectic(x0, k0, c["dt"], T, c["f"], 1.0, gs, tangent=True, method="midpoint")
    with pytest.raises(ValueError, match="tangent needs"):
        sw.ode_symplectic(x0, k0, c["dt"], T, c["f"], 1.0, gs, tangent=True, diagnostics=True)


def test_a_failing_driver_run_leaves_no_live_set(ctx, tmp_path, monkeypatch):
    """An exception in mid-run: the caller's context is back on its own route."""
    import swraytracing_amd.qg as qgmod
    saved, calls = qgmod._save_frame, []

    def save(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            assert ctx.tangent_live()
            raise RuntimeError("stop here")
        return saved(*a, **kw)

    monkeypatch.setattr(qgmod, "_save_frame", save)
    with pytest.raises(RuntimeError, match="stop here"):
        sw.qgsw_raytrace(32, 65, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path), ctx=ctx, max_steps=25, nsub=2,
                         r_drag=0.0, spectrum_edges=SPEC_EDGES, tangent_edges=G_EDGES)
    assert not ctx.tangent_live()
