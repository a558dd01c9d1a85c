"""The flow spectrum series on the device (swrt_flow_spectrum_*) against the
numpy restatement (tests/flow_spectrum_ref.py): the frame is defined to the
bit (include/swrt.h), so every comparison is assert_array_equal on the spectra
and the stats.  Then the drivers' flow_spectrum keyword: frames at the packet
frames' times, totals against the oracle on the pv.bin frames, and nothing
else changed."""
import ctypes
import math
import os

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import swrt_oracle as orc
from swraytracing_amd.qg import initial_q
from tests.flow_spectrum_ref import flow_frame, nshells

pytestmark = pytest.mark.gpu

F, CG = 3.0, 1.0
K_D2 = F / CG


def _half_plane(nx, seed, scale=1.0):
    kmax = nx // 2 - 1
    rng = np.random.default_rng(seed)
    return scale * (rng.standard_normal((2 * kmax + 1, kmax + 1)) + 1j * rng.standard_normal((2 * kmax + 1, kmax + 1)))


def _check(spectra, stats, qk, k_scale, K_d2, t, what=""):
    want_sp, want_st = flow_frame(qk, k_scale, K_d2, t)
    np.testing.assert_array_equal(spectra, want_sp, err_msg=what)
    np.testing.assert_array_equal(stats, want_st, err_msg=what)
    return want_sp, want_st


def _one_layer(ctx, nx=16, seed=146):
    rng = np.random.default_rng(seed)
    q = initial_q(nx, 2 * math.pi, 0.2, K_D2, 2, 5, rng)
    m = sw.QGModel.one_layer(ctx.g2k(q), nx, F, CG, r_drag=0.0, ctx=ctx)
    dt = 0.05 * m.dx / m.max_speed()
    return m, dt


def _two_layer(ctx, nx=64, L=20.0, seed=5):
    rng = np.random.default_rng(seed)
    q1 = initial_q(nx, L, 0.2, K_D2, 3, 8, rng, ndgrid=True)
    qk = np.stack([ctx.g2k(q1), ctx.g2k(-q1)], axis=2)
    m = sw.QGModel.two_layer(qk, nx, F, CG, L=L, ctx=ctx)
    dt = 0.25 * m.dx / m.max_speed()
    return m, dt


def test_one_layer_nx16(fresh_ctx):
    """k_scale exactly 1; the initial state, then after several steps."""
    c = fresh_ctx
    m, dt = _one_layer(c)
    assert m.kscale == 1.0
    m.begin_flow_spectrum()
    assert c.flow_spectrum_shells() == 11 and c.flow_spectrum_frames() == 0
    m.record_flow_spectrum()
    qk0, t0, _ = c.qg_get()
    m.step(dt, 7)
    m.record_flow_spectrum()
    qk1, t1, steps = c.qg_get()
    assert steps == 7 and t0 == 0.0 and t1 > 0.0
    sp, st = c.flow_spectrum_get()
    assert sp.shape == (2, 3, 11) and st.shape == (2, 4)
    _check(sp[0], st[0], qk0[:, :, 0], 1.0, K_D2, t0, "initial")
    _check(sp[1], st[1], qk1[:, :, 0], 1.0, K_D2, t1, "after 7 steps")
    assert not np.array_equal(sp[0], sp[1])
    f = sw.flow_spectrum_fields(sp, st, Cg=CG)
    assert 0.01 < f["U_rms"][0] < 0.2 and np.array_equal(f["Fr"], f["U_rms"] / CG)  # max|U| = 0.2 at the start


def test_two_layers_nx64_and_a_pending_speculative_step(fresh_ctx):
    """Both layers at L = 20, after several steps; with a speculative step
    pending the frame is the committed qk's, at the committed time."""
    c = fresh_ctx
    m, dt = _two_layer(c)
    ks = 2.0 * math.pi / 20.0
    assert m.kscale == ks
    m.step(dt, 3)
    for layer in (0, 1):
        m.begin_flow_spectrum(layer)
        assert c.flow_spectrum_shells() == 45
        m.record_flow_spectrum()
        m.step_speculative(dt)  # (dt is the propagators': the step before set them)
        m.record_flow_spectrum()
        qk, t, steps = c.qg_get()  # the committed state
        m.resolve(True)
        m.max_speed_result()  # (the accepted step's CFL read-back: popped as a driver would)
        m.record_flow_spectrum()
        qk2, t2, steps2 = c.qg_get()
        assert steps2 == steps + 1 and t2 == t + dt
        sp, st = c.flow_spectrum_get()
        want = _check(sp[0], st[0], qk[:, :, layer], ks, K_D2, t, f"layer {layer}")
        np.testing.assert_array_equal(sp[1], want[0], err_msg="speculative step pending")
        np.testing.assert_array_equal(st[1], want[1], err_msg="speculative step pending")
        _check(sp[2], st[2], qk2[:, :, layer], ks, K_D2, t2, f"layer {layer}, the accepted step")
        assert not np.array_equal(sp[2], sp[0])
    with pytest.raises(ValueError, match="layer"):
        m.begin_flow_spectrum(2)


def test_record_qk_gives_record_qg_bytes(fresh_ctx):
    """The host half plane (kx fastest) and the device's (ky fastest) through
    one kernel with strides: the same bytes; the ky = 0, kx < 0 entries are
    never read, whatever they hold."""
    c = fresh_ctx
    m, dt = _two_layer(c)
    m.step(dt, 2)
    m.begin_flow_spectrum(0)
    m.record_flow_spectrum()
    qk, t, _ = c.qg_get()
    plane = np.ascontiguousarray(qk[:, :, 0])
    c.flow_spectrum_record_qk(plane, t)
    kmax = 31
    for poison in (1e300, np.nan):
        bad = plane.copy()
        bad[:kmax, 0] = poison * (1 + 1j)
        c.flow_spectrum_record_qk(bad, t)
    sp, st = c.flow_spectrum_get()
    assert sp.shape[0] == 4
    for i in (1, 2, 3):
        assert sp[i].tobytes() == sp[0].tobytes() and st[i].tobytes() == st[0].tobytes(), i
    assert np.all(np.isfinite(sp)) and st[0, 1] > 0


@pytest.mark.parametrize("K_d2", [3.0, 0.0])
def test_corner_modes_mean_mode_and_zero_den(fresh_ctx, K_d2):
    """Energy in |kx| = ky = kmax only: the last shell alone, beyond kmax.
    The mean mode only: shell 0 with weight 1/2; K_d2 = 0 makes den = 0 there
    and psi 0."""
    c = fresh_ctx
    nx, kmax = 16, 7
    c.flow_spectrum_begin(nx, 1.0, K_d2)
    corner = np.zeros((2 * kmax + 1, kmax + 1), dtype=complex)
    corner[0, kmax] = 1.5 - 0.5j
    corner[2 * kmax, kmax] = -0.25 + 2.0j
    mean = np.zeros_like(corner)
    mean[kmax, 0] = 3.0 + 1.0j
    c.flow_spectrum_record_qk(corner, 0.5)
    c.flow_spectrum_record_qk(mean, 1.5)
    c.flow_spectrum_record_qk(_half_plane(nx, 3), 2.5)
    sp, st = c.flow_spectrum_get()
    _check(sp[0], st[0], corner, 1.0, K_d2, 0.5, "corners")
    _check(sp[1], st[1], mean, 1.0, K_d2, 1.5, "mean mode")
    _check(sp[2], st[2], _half_plane(nx, 3), 1.0, K_d2, 2.5, "random")
    assert np.all(sp[0][:, :10] == 0.0) and np.all(sp[0][:, 10] > 0.0)  # shell 10 > kmax = 7 is kept
    assert np.all(sp[1][:, 1:] == 0.0) and sp[1][2, 0] == 0.5 * 10.0
    if K_d2 == 0.0:
        assert sp[1][0, 0] == 0.0 and sp[1][1, 0] == 0.0 and np.all(np.isfinite(sp))


@pytest.mark.parametrize("nx,k_scale", [(8, 1.0), (256, 0.7), (512, 1.0), (1024, 2.0 * math.pi / 20.0)])
def test_grid_sizes_across_the_workgroup(fresh_ctx, nx, k_scale):
    """A lane takes the slot pair (i, i + nx/2): up to nx = 512 one pair per
    lane of the 256, from nx = 1024 on the lanes loop.  Both sides, and the
    smallest grid."""
    c = fresh_ctx
    qk = _half_plane(nx, nx, 0.1)
    c.flow_spectrum_begin(nx, k_scale, 1.75)
    assert c.flow_spectrum_shells() == nshells(nx)
    c.flow_spectrum_record_qk(qk, 4.0)
    sp, st = c.flow_spectrum_get()
    _check(sp[0], st[0], qk, k_scale, 1.75, 4.0, f"nx = {nx}")


def test_series_grows_and_keeps_earlier_frames(fresh_ctx):
    """nx = 16: 264 B a frame, the first reservation holds 4096; the 4097th record grows it."""
    c = fresh_ctx
    m, dt = _one_layer(c)
    m.begin_flow_spectrum()
    a, b = _half_plane(16, 1), _half_plane(16, 2)
    c.flow_spectrum_record_qk(a, 1.0)
    for _ in range(4095):
        m.record_flow_spectrum()
    assert c.flow_spectrum_frames() == 4096
    c.flow_spectrum_record_qk(b, 2.0)
    assert c.flow_spectrum_frames() == 4097
    sp, st = c.flow_spectrum_get()
    qk, t, _ = c.qg_get()
    _check(sp[0], st[0], a, 1.0, K_D2, 1.0, "frame 0, before the growth")
    want = _check(sp[1], st[1], qk[:, :, 0], 1.0, K_D2, t, "frame 1")
    assert np.all(sp[1:4096] == want[0]) and np.all(st[1:4096] == want[1])
    _check(sp[4096], st[4096], b, 1.0, K_D2, 2.0, "the growing record")


def test_get_and_reset(fresh_ctx):
    c = fresh_ctx
    a, b = _half_plane(16, 7), _half_plane(16, 8)
    c.flow_spectrum_begin(16, 0.5, 2.0)
    c.flow_spectrum_record_qk(a, 0.25)
    c.flow_spectrum_record_qk(b, 0.75)
    sp, st = c.flow_spectrum_get()
    wa, wb = _check(sp[0], st[0], a, 0.5, 2.0, 0.25), _check(sp[1], st[1], b, 0.5, 2.0, 0.75)
    P = ctypes.POINTER(ctypes.c_double)
    only_sp, only_st = np.zeros((2, 3, 11)), np.zeros((2, 4))
    assert c._L.swrt_flow_spectrum_get(c._h, 0, 2, only_sp.ctypes.data_as(P), None) == 0
    assert c._L.swrt_flow_spectrum_get(c._h, 0, 2, None, only_st.ctypes.data_as(P)) == 0
    np.testing.assert_array_equal(only_sp, np.stack([wa[0], wb[0]]))
    np.testing.assert_array_equal(only_st, np.stack([wa[1], wb[1]]))
    assert c.flow_spectrum_get(spectra=False)[0] is None and c.flow_spectrum_get(stats=False)[1] is None
    s1, t1 = c.flow_spectrum_get(1, 1)
    assert np.array_equal(s1[0], sp[1]) and np.array_equal(t1[0], st[1])
    c.flow_spectrum_reset()
    assert c.flow_spectrum_frames() == 0 and c.flow_spectrum_shells() == 11
    assert c.flow_spectrum_get()[0].shape == (0, 3, 11)
    c.flow_spectrum_record_qk(b, 0.75)  # nx, k_scale and K_d2 stay
    sp, st = c.flow_spectrum_get()
    _check(sp[0], st[0], b, 0.5, 2.0, 0.75, "frame 0 after the reset")
    c.flow_spectrum_begin(64, 1.0, 0.0)  # another begin empties the series and takes the new geometry
    assert c.flow_spectrum_frames() == 0 and c.flow_spectrum_shells() == 45


def test_errors(fresh_ctx):
    c = fresh_ctx
    plane = _half_plane(16, 4)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):
        c.flow_spectrum_record_qg(0)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):
        c.flow_spectrum_record_qk(plane, 0.0)
    assert c.flow_spectrum_frames() == 0 and c.flow_spectrum_shells() == 0
    for bad, name in ((dict(nx=48), "nx must"), (dict(nx=4), "nx must"), (dict(nx=8192), "nx must"),
                      (dict(nx=0), "nx must"), (dict(k_scale=0.0), "k_scale must"), (dict(k_scale=-1.0), "k_scale must"),
                      (dict(k_scale=np.inf), "k_scale must"), (dict(k_scale=np.nan), "k_scale must"),
                      (dict(K_d2=-1e-300), "K_d2 must"), (dict(K_d2=np.inf), "K_d2 must"), (dict(K_d2=np.nan), "K_d2 must")):
        kw = dict(nx=16, k_scale=1.0, K_d2=3.0)
        kw.update(bad)
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*" + name):
            c.flow_spectrum_begin(**kw)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):  # a refused begin opens nothing
        c.flow_spectrum_record_qk(plane, 0.0)
    c.flow_spectrum_begin(32, 1.0, 3.0)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*swrt_qg_init"):
        c.flow_spectrum_record_qg(0)
    m, _ = _one_layer(c)  # a 16^2 state beside a 32^2 series
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*nx"):
        c.flow_spectrum_record_qg(0)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*nx"):
        c.flow_spectrum_record_qk(plane, 0.0)
    with pytest.raises(ValueError, match="half plane"):
        c.flow_spectrum_record_qk(np.zeros((15, 9), dtype=complex))
    m.begin_flow_spectrum()
    for layer in (1, -1):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*layer"):
            c.flow_spectrum_record_qg(layer)
    assert c._L.swrt_flow_spectrum_record_qk(c._h, None, 16, 0.0) == 1
    c.flow_spectrum_record_qg(0)
    for first, count in ((-1, 1), (0, 2), (1, 1), (0, -1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*range"):
            c.flow_spectrum_get(first, count)
    assert c._L.swrt_flow_spectrum_get(c._h, 0, 1, None, None) == 1 and b"NULL" in c._L.swrt_last_error(c._h)
    c.flow_spectrum_record_qg(0)  # the open series is still usable
    assert c.flow_spectrum_frames() == 2


# ---- the drivers ------------------------------------------------------------

FLOW_FILES = ("flow_spec.bin", "flow_stats.bin", "flow_geom.bin")


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


def _check_flow_files(d, facts, nx, L, one_layer):
    """flow_frames == packet_frames; column 0 of flow_stats.bin is
    packet_time.bin byte for byte; where a pv.bin frame has the same time the
    totals agree with the oracle on that frame within 1e-10 relative (the pv
    frame went through k2g: its round trip errs by about nx^2 eps = 4e-13 at
    nx = 64).  Returns how many pv frames matched."""
    files = _files(d)
    assert set(FLOW_FILES) <= set(files)
    frames = facts["packet_frames"]
    assert facts["flow_frames"] == frames > 1
    ns = nshells(nx)
    ks = 1.0 if one_layer else 2.0 * math.pi / L
    assert np.frombuffer(files["flow_geom.bin"]).tolist() == [nx, ns, ks, K_D2, 0.0]
    stats = np.frombuffer(files["flow_stats.bin"]).reshape(frames, 4)
    spectra = np.frombuffer(files["flow_spec.bin"]).reshape(frames, 3, ns)
    assert stats[:, 0].tobytes() == files["packet_time.bin"]
    for p in range(3):  # the totals are the shells' sequential sums
        for i in range(frames):
            s = np.float64(0.0)
            for v in spectra[i, p]:
                s = s + v
            assert s == stats[i, 1 + p]
    pv_t = np.frombuffer(files["pv_time.bin"])
    nl = 1 if one_layer else 2
    pv = np.frombuffer(files["pv.bin"]).reshape(len(pv_t), nl, nx, nx)
    kx_, ky_, K2 = orc.wavenumber_grids(nx, L, scale=not one_layer)
    matched = 0
    for t, frame in zip(pv_t, pv):
        for i in np.flatnonzero(stats[:, 0] == t):
            q = frame[0].T  # (column-major frames; layer 0)
            U = orc.grid_U(orc.g2k(q), K_D2, K2, kx_, ky_)
            want = [0.5 * np.mean(U["u"] ** 2 + U["v"] ** 2), 0.5 * np.mean((U["vx"] - U["uy"]) ** 2),
                    0.5 * np.mean(q ** 2)]
            for got, w in zip(stats[i, 1:], want):
                assert abs(got - w) <= 1e-10 * abs(w), (t, got, w)
            matched += 1
    return matched


def test_one_layer_driver(ctx, tmp_path):
    """A tiny positive packet delay puts packet_step_start at 1: packet frames
    at steps 5, 10, .., 50 and pv frames at t = 0 and step 50 share two times."""
    a, b, c2 = (str(tmp_path / n) for n in "abc")
    args = (64, 200, 4.0, 20.0, 1e-9, 0.2, 3.0, 1.0)
    kw = dict(ctx=ctx, max_steps=50, nsub=2, r_drag=0.0)
    facts = sw.qgsw_raytrace(*args, out_dir=a, flow_spectrum=True, **kw)
    assert facts["packet_step_start"] == 1 and facts["packet_frames"] == 11
    assert _check_flow_files(a, facts, 64, 2 * math.pi, True) == 2
    # with the keyword off: the same files and bytes run after run, none of the three, and the run
    # with it on wrote the same bytes beside them
    plain = sw.qgsw_raytrace(*args, out_dir=b, **kw)
    again = sw.qgsw_raytrace(*args, out_dir=c2, flow_spectrum=False, **kw)
    fa, fb, fc = _files(a), _files(b), _files(c2)
    assert plain["flow_frames"] == 0 and again["flow_frames"] == 0
    assert fb == fc and not set(FLOW_FILES) & set(fb)
    assert {n: v for n, v in fa.items() if n not in FLOW_FILES} == fb
    assert plain == again and {k: v for k, v in facts.items() if k != "flow_frames"} == \
        {k: v for k, v in plain.items() if k != "flow_frames"}  # the return value: the new key alone
    with pytest.raises(ValueError, match="flow_spectrum"):
        sw.qgsw_raytrace(64, 0, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=b, flow_spectrum=True, **kw)


@pytest.mark.parametrize("delay,start,matches", [(1e-9, 1, 1), (0.0, 0, 0)])
def test_two_layer_driver(ctx, tmp_path, delay, start, matches):
    """The loop returns from a step with the next one queued speculatively:
    the frame must carry the committed time.  delay = 0 labels the first packet
    frame -dt (packet_step_start = 0): flow_stats.bin takes the same label."""
    facts = sw.qg2layersw_raytrace(32, 200, 4.0, 40.0, delay, 0.2, 3.0, 1.0, out_dir=str(tmp_path), nsub=2,
                                   max_steps=30, seed=5, ctx=ctx, flow_spectrum=True)
    assert facts["packet_step_start"] == start and facts["packet_frames"] == 2
    assert _check_flow_files(str(tmp_path), facts, 32, 20.0, False) == matches
    t = np.fromfile(tmp_path / "flow_stats.bin").reshape(-1, 4)[:, 0]
    assert t[1] == sum_in_order(facts["dts"][:25 - (1 - start)])


def sum_in_order(dts):
    t = 0.0
    for d in dts:
        t = t + d
    return t
