"""The track series on the device (swrt_track_*; swraytracing_amd/csrc/
swrt_track.hpp) and the drivers' track files.

A frame's columns [x, y, k, l] are compared with packets_get()[ids] and
[Omega, zeta, sigma, D] with raydiag_sample(values=True)[ids] on the same
state, bit for bit (the uint64 view), and with tests/track_series_ref.py, the
numpy restatement on the oracle's interpolation, also bit for bit: the
standard tests/test_gpu_raydiag.py holds its per-packet samples to.  There is
no tolerance anywhere in this file.

Unless a case says otherwise: 64^2 grid, L = 2 pi, f = 3, gH = 1, the two
snapshots of tests/test_gpu_raydiag.py, x uniform in [-pi, pi)^2, |k| = 3."""
import ctypes
import os

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import swrt_oracle as orc
from swraytracing_amd import _lib as lib
from tests.conftest import periodic_grid
from tests.track_series_ref import QUIET_NAN, track_frame

pytestmark = pytest.mark.gpu

NX, L, F, GH = 64, 2 * np.pi, 3.0, 1.0
DX = L / NX
BUMP = orc.BUMP_SW
DT = 0.05
NSPLIT = 70_000  # above the two-packet-stream threshold (65536)


def _psi(which):
    X, Y = periodic_grid(NX, L)
    if which == 0:
        return 0.05 * (np.cos(X + Y) + 0.7 * np.sin(2 * X - Y))
    return 0.04 * (np.sin(X - 2 * Y) + 0.5 * np.cos(3 * X + Y))


def _packets(n, seed=20):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th = rng.uniform(0, 2 * np.pi, n)
    return x, 3.0 * np.stack([np.cos(th), np.sin(th)], axis=1)


@pytest.fixture(scope="module")
def flows():
    """The two snapshots as the device holds them, in the oracle's dict form: computed once, read-only."""
    c = sw.Context(0)
    out = []
    for which in (0, 1):
        c.set_field_psi(0, _psi(which), NX, L)
        p = c.get_field_grid(0, NX)
        out.append({n: p[i].reshape((NX, NX), order="F").copy() for i, n in enumerate(orc.FIELD_ORDER)})
    c.close()
    return out


def _set_fields(c, nslots):
    for s in range(nslots):
        c.set_field_psi(s, _psi(s), NX, L)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _download(c, ids, nslots, alpha=0.0, bump=BUMP, f=F, gH=GH):
    """The frame (8, m) the route without the track series gives: a whole-ensemble download, then indexing."""
    x, k = c.packets_get()
    out = np.empty((8, len(ids)))
    out[0:2] = x[ids].T
    out[2:4] = k[ids].T
    if nslots == 0:
        out[4:8].view(np.uint64)[...] = QUIET_NAN
    else:
        s4, _ = c.raydiag_sample(f, gH, nslots=nslots, alpha=alpha, bump=bump, values=True)
        out[4:8] = s4[ids].T
    return out, x, k


def _same(got, want, what=""):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _record_and_check(c, flows, ids, nslots, alpha, what):
    """One more frame; it equals the download and the restatement on the same state."""
    c.track_record(F, GH, nslots=nslots, alpha=alpha, bump=BUMP)
    want, x, k = _download(c, ids, nslots, alpha)
    got = c.track_series(c.track_frames() - 1, 1)[0]
    assert got.shape == (8, len(ids))
    _same(got, want, f"{what}: against the download")
    ref = track_frame(x, k, ids, flows[:nslots], alpha, F, GH, DX, BUMP)
    _same(got, ref.T, f"{what}: against the restatement")
    return got


# ---- 1, 2: the storage order and the other paths ------------------------------

IDS5 = [999, 0, 517, 64, 63]


@pytest.mark.parametrize("rebin,nslots,alpha", [(2, 1, 0.0), (0, 1, 0.0), (2, 2, 0.37), (0, 2, 0.37)])
def test_frames_follow_the_ids_whatever_the_storage_order(fresh_ctx, flows, rebin, nslots, alpha):
    c = fresh_ctx
    n = 1000  # no multiple of 64
    _set_fields(c, nslots)
    c.set_locality(rebin, 0)  # 2: the tile kernel re-bins; 0: the per-packet kernel, identity order
    x0, k0 = _packets(n)
    c.packets_set(x0, k0)
    c.track_begin(IDS5)
    assert c.track_ids().tolist() == IDS5 and c.track_frames() == 0
    a = _record_and_check(c, flows, IDS5, nslots, alpha, "frame 0")
    _same(a[0:4], np.concatenate([x0[IDS5].T, k0[IDS5].T]))
    c.advance(DT, 6, F, GH, nslots=nslots, alpha0=alpha, dalpha=0.0, bump=BUMP)
    b = _record_and_check(c, flows, IDS5, nslots, alpha, "frame 1")
    assert c.track_frames() == 2
    assert not np.array_equal(a[0:4], b[0:4]) and (a[4:8] != b[4:8]).any()  # the packets moved
    # without a flow: the same four stored columns, then the quiet NaN
    c.track_record(F, GH, nslots=0)
    nf = c.track_series(2, 1)[0]
    _same(nf[0:4], b[0:4])
    assert (_bits(nf[4:8]) == QUIET_NAN).all()
    _same(c.track_series(), np.stack([a, b, nf]))


def test_no_flow_needs_no_slot(fresh_ctx):
    c = fresh_ctx
    x0, k0 = _packets(37)
    c.packets_set(x0, k0)  # no field set at all: the drivers' first frame
    c.track_begin([36, 5])
    c.track_record(F, GH, nslots=0)
    fr = c.track_series()[0]
    _same(fr[0:4], np.concatenate([x0[[36, 5]].T, k0[[36, 5]].T]))
    assert (_bits(fr[4:8]) == QUIET_NAN).all()
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*slot"):
        c.track_record(F, GH, nslots=1)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*nslots"):
        c.track_record(F, GH, nslots=3)


# ---- 3: extremes ---------------------------------------------------------------

@pytest.mark.parametrize("n,ids", [(1000, [999]), (300, list(range(299, -1, -1)))], ids=["m=1", "m=n"])
def test_extremes(fresh_ctx, flows, n, ids):
    c = fresh_ctx
    _set_fields(c, 1)
    c.set_locality(2, 0)
    x0, k0 = _packets(n, seed=21)
    c.packets_set(x0, k0)
    c.track_begin(ids)
    c.advance(DT, 4, F, GH, bump=BUMP)
    _record_and_check(c, flows, ids, 1, 0.0, f"m={len(ids)}")


# ---- 4, 9: two packet streams, the parked set, the hazard checker ------------

def _split_setup(c, streams):
    _set_fields(c, 1)
    c.set_packet_streams(streams)
    c.set_locality(2, 0)
    x0, k0 = _packets(NSPLIT, seed=22)
    c.packets_set(x0, k0)
    rng = np.random.default_rng(23)
    ids = np.concatenate([[NSPLIT - 1, 0], rng.choice(np.arange(1, NSPLIT - 1), 255, replace=False)])
    c.track_begin(ids)
    return ids


@pytest.fixture(scope="module")
def split_twin():
    """Case 4's twin: one packet stream, synchronised and downloaded after each call.  Computed once."""
    c = sw.Context(0)
    try:
        ids = _split_setup(c, 1)
        frames = []
        for _ in range(3):
            c.advance(DT, 2, F, GH, bump=BUMP)
            c.synchronize()
            frames.append(_download(c, ids, 1)[0])
        assert not np.array_equal(frames[0], frames[2])
        return ids, np.stack(frames)
    finally:
        c.close()


def _split_run(c):
    ids = _split_setup(c, 2)
    for _ in range(3):  # no synchronize in between: the records are ordered on the device
        c.advance(DT, 2, F, GH, bump=BUMP)
        c.track_record(F, GH, nslots=1, bump=BUMP)
    return ids, c.track_series()


def test_record_behind_two_packet_streams_and_the_parked_set(fresh_ctx, split_twin):
    ids, got = _split_run(fresh_ctx)
    assert np.array_equal(ids, split_twin[0]) and got.shape == (3, 8, 257)
    _same(got, split_twin[1])


def test_record_under_the_hazard_checker(fresh_ctx, split_twin):
    c = fresh_ctx
    c.debug_set(lib.DEBUG_HAZARD_CHECK, 1)
    _, got = _split_run(c)  # a hazard would be SWRT_ERR_STATE from the call that met it
    assert c.debug_get(lib.DEBUG_HAZARD_CHECKS) > 0
    c.debug_set(lib.DEBUG_HAZARD_CHECK, 0)
    _same(got, split_twin[1])


# ---- 5: history ---------------------------------------------------------------

def test_record_history_equals_records_on_packets_set_to_each_frame(fresh_ctx):
    a, b = fresh_ctx, sw.Context(0)
    try:
        n, ids = 1000, [999, 0, 517, 64, 63, 2]
        x0, k0 = _packets(n, seed=24)
        for c in (a, b):
            _set_fields(c, 2)
            c.set_locality(2, 0)
            c.packets_set(x0, k0)
            c.track_begin(ids)
        a.advance(DT, 5, F, GH, nslots=2, alpha0=0.1, dalpha=0.2, bump=BUMP, save_every=1)
        alphas = np.array([0.2, 0.4, 0.6, 0.8, 1.0])
        a.track_record_history(0, 5, F, GH, nslots=2, alphas=alphas, bump=BUMP)
        assert a.track_frames() == 5
        hx, hk = a.history()
        for i in range(5):
            b.packets_set(np.ascontiguousarray(hx[i].T), np.ascontiguousarray(hk[i].T))  # (the same N: the ids stay)
            b.track_record(F, GH, nslots=2, alpha=alphas[i], bump=BUMP)
        got, want = a.track_series(), b.track_series()
        _same(got, want)
        assert len({fr.tobytes() for fr in got}) == 5
        # a subrange with one snapshot (alphas may be None), appended behind them
        a.track_record_history(1, 2, F, GH, nslots=1, bump=BUMP)
        b.track_reset()
        for i in (1, 2):
            b.packets_set(np.ascontiguousarray(hx[i].T), np.ascontiguousarray(hk[i].T))
            b.track_record(F, GH, nslots=1, bump=BUMP)
        _same(a.track_series(5, 2), b.track_series())
        for first, count in ((0, 6), (5, 1), (-1, 2), (2, -1)):
            with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*history"):
                a.track_record_history(first, count, F, GH, nslots=1, bump=BUMP)
        rc = a._L.swrt_track_record_history(a._h, 0, 2, F, GH, 2, None, BUMP)
        assert rc == 1 and b"alphas" in a._L.swrt_last_error(a._h)
        assert a.track_frames() == 7
    finally:
        b.close()


# ---- 6: after ode23 -----------------------------------------------------------

def test_record_right_after_an_ode23_interval(fresh_ctx, flows):
    c = fresh_ctx
    ids = [499, 0, 250, 13]
    _set_fields(c, 2)
    x0, k0 = _packets(500, seed=25)
    c.packets_set(x0, k0)
    c.track_begin(ids)
    ts = sw.ode23_packets(c, (0.0, 0.3), 0.3, F, 1.0, nslots=2, bump=BUMP)
    assert len(ts) > 2
    c.track_record(F, GH, nslots=2, alpha=1.0, bump=BUMP)  # at once: nothing in between
    want, x, k = _download(c, ids, 2, 1.0)
    got = c.track_series()[0]
    _same(got, want)
    _same(got, track_frame(x, k, ids, flows, 1.0, F, GH, DX, BUMP).T)
    assert not np.array_equal(x[ids], x0[ids])


# ---- 7: growth ----------------------------------------------------------------

def test_series_grows_past_the_first_reservation_and_resets(fresh_ctx):
    c = fresh_ctx
    ids = [299, 0, 150]
    _set_fields(c, 1)
    x0, k0 = _packets(300, seed=26)
    c.packets_set(x0, k0)
    c.track_begin(ids)
    total = 4100  # the first reservation holds 4096 frames
    states = []
    for i in range(total):
        if i % 1000 == 0:
            if i:
                c.advance(DT, 1, F, GH, bump=BUMP)
            states.append(_download(c, ids, 1)[0])
        c.track_record(F, GH, nslots=1, bump=BUMP)
    assert c.track_frames() == total and len(states) == 5
    got = c.track_series()
    assert got.shape == (total, 8, 3)
    for i in range(total):
        if not np.array_equal(_bits(got[i]), _bits(states[i // 1000])):
            raise AssertionError(f"frame {i} differs from the download taken at that point")
    assert len({s.tobytes() for s in states}) == 5
    _same(c.track_series(4094, 4), got[4094:4098])
    c.track_reset()
    assert c.track_frames() == 0 and c.track_series().shape == (0, 8, 3)
    assert c.track_ids().tolist() == ids
    c.track_record(F, GH, nslots=1, bump=BUMP)
    _same(c.track_series()[0], states[4])


# ---- 8: errors ----------------------------------------------------------------

def test_errors(fresh_ctx):
    c = fresh_ctx
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*swrt_track_begin"):
        c.track_record(F, GH, nslots=0)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*swrt_track_begin"):
        c.track_record_history(0, 0, F, GH, nslots=0)
    assert c.track_frames() == 0 and c._L.swrt_track_count(c._h) == 0 and c.track_ids().size == 0
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*no packets"):
        c.track_begin([0])
    n = 100
    x0, k0 = _packets(n)
    c.packets_set(x0, k0)
    for bad, msg in (([], "m must be"), (list(range(n)) + [0], "m must be"), ([3, 7, 3], "3 given twice"),
                     ([0, n], f"{n} out of range"), ([5, -1], "-1 out of range")):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*" + msg):
            c.track_begin(bad)
    assert c._L.swrt_track_begin(c._h, None, 3) == 1 and b"NULL" in c._L.swrt_last_error(c._h)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*swrt_track_begin"):  # a refused begin opens nothing
        c.track_record(F, GH, nslots=0)
    with pytest.raises(ValueError):
        c.track_begin([1.5, 2.0])
    c.track_begin([7, 3])
    assert c._L.swrt_track_count(c._h) == 2
    c.track_record(F, GH, nslots=0)
    for first, count in ((-1, 1), (0, 2), (1, 1), (0, -1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
            c.track_series(first, count)
    assert c._L.swrt_track_get(c._h, 0, 1, None) == 1 and b"NULL" in c._L.swrt_last_error(c._h)
    # the same N keeps the series and the ids; another N closes it
    c.packets_set(x0 + 0.5, k0)
    c.track_record(F, GH, nslots=0)
    got = c.track_series()
    assert got.shape == (2, 8, 2)
    _same(got[1, 0:2], (x0 + 0.5)[[7, 3]].T)
    c.track_begin([9])  # a new begin empties the series
    assert c.track_frames() == 0 and c.track_ids().tolist() == [9]
    c.track_record(F, GH, nslots=0)
    x1, k1 = _packets(37, seed=3)
    c.packets_set(x1, k1)
    assert c._L.swrt_track_count(c._h) == 0 and c.track_frames() == 0
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*swrt_track_begin"):
        c.track_record(F, GH, nslots=0)
    ids_out = (ctypes.c_int64 * 2)()
    assert c._L.swrt_track_ids(c._h, ids_out) == 3  # SWRT_ERR_STATE: none open


# ---- 10: the drivers ----------------------------------------------------------

TRACK_FILES = ("track_x.bin", "track_k.bin", "track_diag.bin", "track_time.bin", "track_ids.bin")


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


def _series(d, name, rows, cols):
    a = np.fromfile(os.path.join(d, name + ".bin"))
    return a.reshape(-1, cols, rows)  # (frames, cols, rows): a frame is rows x cols, column-major


def _check_track_files(d, plain, ids, n, every_fifth):
    """The track files of the run in ``d`` against its own packet files, and every other file against ``plain``."""
    m = len(ids)
    fd, fp = _files(d), _files(plain)
    assert set(fd) == set(fp) | set(TRACK_FILES) and not set(TRACK_FILES) & set(fp)
    for name in fp:
        assert fd[name] == fp[name], name  # tracking changes no other output
    px, pk = _series(d, "packet_x", n, 2), _series(d, "packet_k", n, 2)
    pt = np.fromfile(os.path.join(d, "packet_time.bin"))
    tx, tk, td = _series(d, "track_x", m, 2), _series(d, "track_k", m, 2), _series(d, "track_diag", m, 4)
    tt = np.fromfile(os.path.join(d, "track_time.bin"))
    assert np.fromfile(os.path.join(d, "track_ids.bin")).tolist() == [float(i) for i in ids]
    assert tx.shape[0] == tk.shape[0] == td.shape[0] == tt.size and pt.size >= 2
    if every_fifth:
        # (the first packet frame stands one step before the first PDE step, qgsw_raytrace.m:104-106, so the
        # second one may come one track frame early; from then on the cadences are commensurate)
        at = [int(np.nonzero(tt == t)[0][0]) for t in pt]
        gaps = np.diff(at)
        assert at[0] == 0 and gaps[0] in (every_fifth - 1, every_fifth) and (gaps[1:] == every_fifth).all()
        assert tt.size > pt.size
    else:
        assert tt.tobytes() == pt.tobytes()
        at = list(range(pt.size))
    assert tx[at].tobytes() == np.ascontiguousarray(px[:, :, ids]).tobytes()
    assert tk[at].tobytes() == np.ascontiguousarray(pk[:, :, ids]).tobytes()
    assert (_bits(td[0]) == QUIET_NAN).all() and np.isfinite(td[1:]).all()
    # read_field reads them as load_data.m would with Npackets = m (is_real: m = 3 on 2 columns is the
    # shape read_field.m:37-41 takes for a spectral field)
    assert np.array_equal(sw.read_field(os.path.join(d, "track_x"), m, 2, 1, is_real=True)[:, :, -1], tx[-1].T)
    return tx, tk, td, tt


def _check_last_omega(ctx, td_last, tk_last, ids, f, gH, bump):
    """The run's last track frame was recorded at the packets' final state with slot 0 the snapshot there."""
    x, k = ctx.packets_get()
    xs, ks = x[ids], k[ids]
    _same(tk_last.T, ks)
    I = ctx.eval(xs[:, 0], xs[:, 1], nslots=1, bump=bump)
    om = np.sqrt(f * f + gH * (ks[:, 0] * ks[:, 0] + ks[:, 1] * ks[:, 1]))
    _same(td_last[0], om + (I[0] * ks[:, 0] + I[1] * ks[:, 1]), "Omega of the last frame")
    assert np.abs(td_last[1]).max() > 0  # zeta: the flow is not at rest


def test_driver_track_files(ctx, tmp_path):
    args, kw = (64, 500, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0), dict(nsub=2, max_steps=12, r_drag=0.0, ctx=ctx)
    ids = [499, 0, 250]
    p, a, b = (str(tmp_path / n) for n in "pab")
    plain = sw.qgsw_raytrace(*args, out_dir=p, **kw)
    assert plain["track_frames"] == 0 and plain["packet_frames"] == 3
    fa = sw.qgsw_raytrace(*args, out_dir=a, track_ids=ids, **kw)
    assert fa["track_frames"] == 3
    assert {k: v for k, v in fa.items() if k != "track_frames"} == {k: v for k, v in plain.items() if k != "track_frames"}
    _check_track_files(a, p, ids, 500, 0)
    # earlier track files are removed by a fresh run; every step a frame
    for name in TRACK_FILES:
        (tmp_path / "b").mkdir(exist_ok=True)
        (tmp_path / "b" / name).write_bytes(b"\0" * 8)
    fb = sw.qgsw_raytrace(*args, out_dir=b, track_ids=ids, track_every=1, **kw)
    assert fb["track_frames"] == 13
    tx, tk, td, tt = _check_track_files(b, p, ids, 500, 5)
    _check_last_omega(ctx, td[-1], tk[-1], ids, 3.0, 1.0, orc.BUMP_QG)
    # an integer K spreads the ids; several intervals per call give the same track files
    c, d = str(tmp_path / "c"), str(tmp_path / "d")
    sw.qgsw_raytrace(*args, out_dir=c, track_ids=4, track_every=2, **kw)
    sw.qgsw_raytrace(*args, out_dir=d, track_ids=[0, 125, 250, 375], track_every=2, packet_intervals=3, **kw)
    assert _files(c) == _files(d) and len(_files(c)["track_time.bin"]) == 8 * 7


def test_two_layer_driver_track_files(ctx, tmp_path):
    args, kw = (64, 500, 4.0, 10.0, 0.0, 0.2, 3.0, 1.0), dict(nsub=2, max_steps=29, seed=5, ctx=ctx)
    ids = [499, 0, 250]
    p, a, b = (str(tmp_path / n) for n in "pab")
    plain = sw.qg2layersw_raytrace(*args, out_dir=p, **kw)
    assert plain["packet_frames"] == 2 and plain["track_frames"] == 0
    fa = sw.qg2layersw_raytrace(*args, out_dir=a, track_ids=ids, **kw)
    assert fa["track_frames"] == 2 and fa["dts"] == plain["dts"]
    _check_track_files(a, p, ids, 500, 0)
    fb = sw.qg2layersw_raytrace(*args, out_dir=b, track_ids=ids, track_every=5, **kw)
    assert fb["track_frames"] == 7
    tx, tk, td, tt = _check_track_files(b, p, ids, 500, 5)
    _check_last_omega(ctx, td[-1], tk[-1], ids, 3.0, 1.0, orc.BUMP_QG)


def test_trace_stored_track_files(ctx, qg_case, tmp_path):
    """Seven stored PV frames at times of tests/golden/pv_time_ref.bin's first run."""
    q = qg_case
    nx, f, Cg = q["nx"], q["f"], q["Cg"]
    tref = np.fromfile(os.path.join(os.path.dirname(__file__), "golden", "pv_time_ref.bin"))
    run = tref[:int(np.nonzero(np.diff(tref) < 0)[0][0]) + 1]  # the first run: up to the first restart
    times = [float(t) for t in np.unique(run)[:7]]  # (a time may stand twice in the file)
    assert len(times) == 7 and times[0] == 0.0
    pv = tmp_path / "pv"
    X = np.arange(nx) * (q["L"] / nx)
    for s in range(7):
        sw.write_field(q["q"] * (1.0 + 0.1 * s) + 0.05 * s * np.cos(X[:, None] + 2 * X[None, :]), str(pv))
    rng = np.random.default_rng(14)
    x0, k0 = orc.initial_packets(500, q["L"], 4.0, f, Cg, rng)
    ids = [499, 0, 250]
    kw = dict(times=times, nsub=2, intervals_per_call=3, ctx=ctx)
    p, a, b = (str(tmp_path / n) for n in "pab")
    xp, kp, _ = sw.trace_stored(str(pv), nx, x0, k0, f, Cg, out_dir=p, **kw)
    xa, ka, _ = sw.trace_stored(str(pv), nx, x0, k0, f, Cg, out_dir=a, track_ids=ids, **kw)
    _check_track_files(a, p, ids, 500, 0)  # packet frames after intervals 0, 3, 6
    xb, kb, _ = sw.trace_stored(str(pv), nx, x0, k0, f, Cg, out_dir=b, track_ids=ids, track_every=1, **kw)
    tx, tk, td, tt = _check_track_files(b, p, ids, 500, 3)
    assert tt.tolist() == times
    for got in ((xa, ka), (xb, kb)):
        assert got[0].tobytes() == xp.tobytes() and got[1].tobytes() == kp.tobytes()
    _check_last_omega(ctx, td[-1], tk[-1], ids, f, Cg ** 2, orc.BUMP_QG)
    with pytest.raises(ValueError, match="out_dir"):
        sw.trace_stored(str(pv), nx, x0, k0, f, Cg, track_ids=ids, **kw)


def test_record_tracks_drains_a_large_series(fresh_ctx, tmp_path, monkeypatch):
    """The drain (get, append, reset) at a lowered threshold: the same files as one write at the end."""
    import swraytracing_amd.integrate as integ
    x, k = _packets(1000, seed=10)
    ids = [999, 3, 500, 4]
    _set_fields(fresh_ctx, 1)

    def run(d, threshold):
        monkeypatch.setattr(integ, "MAP_DRAIN_BYTES", threshold)
        os.makedirs(d)
        ens = sw.PacketEnsemble(x, k, L, F, 1.0, NX, F / 1.0, ctx=fresh_ctx, bump=BUMP)
        ens.begin_tracks(ids, directory=d if threshold < 1 << 20 else None)
        for i in range(7):
            fresh_ctx.packets_set(x + 0.05 * i, k)
            ens.record_tracks(0.25 * i, 1 if i else 0)
        assert ens.write_tracks(d) == 7
        return _files(d)

    whole = run(str(tmp_path / "whole"), 256 << 20)
    drained = run(str(tmp_path / "drained"), 3 * 64 * 4 - 1)  # drains at every third frame
    assert set(whole) == set(TRACK_FILES) and whole == drained
    assert len(whole["track_x.bin"]) == 7 * 4 * 2 * 8 and len(whole["track_ids.bin"]) == 4 * 8
    tx = _series(str(tmp_path / "whole"), "track_x", 4, 2)
    want = np.mod((x + 0.05 * 6)[ids] + L / 2, L) - L / 2
    _same(tx[6].T, want)
