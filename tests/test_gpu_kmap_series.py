"""The wave-vector plane series on the device (swrt_kmap_series_*;
swraytracing_amd/csrc/swrt_kmap.hpp) and the drivers' k-plane files.

Expected values are tests/kmap_series_ref.py, the numpy restatement of the
contract in include/swrt.h, on the packets swrt_packets_get returns.  Every
comparison is exact integer equality: integer sums are order-free, so there is
no tolerance.  Each m runs through the kernel its size selects and, with
SWRT_DEBUG_KMAP_GLOBAL, through the global kernel with and without its wave
merge: m <= 128 thereby meets the LDS kernel and the global one."""
import ctypes
import os

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import cbind, swrt_oracle as orc
from swraytracing_amd._lib import DEBUG_KMAP_GLOBAL
from tests.kmap_series_ref import edge_wavevectors, kmap_frame

pytestmark = pytest.mark.gpu

K, FB = 5.0, 16
PATHS = (0, 1, 2, 3)  # by m; global as shipped; global merged; global unmerged


@pytest.fixture()
def kctx(ctx):
    """The session context with the path key back at 0 afterwards."""
    yield ctx
    ctx.debug_set(DEBUG_KMAP_GLOBAL, 0)


def _wavevectors(n, seed=3, sigma=2.0):
    """Gaussian wavevectors (a few beyond K = 5) and unrelated positions."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-3.0, 3.0, (n, 2)), sigma * rng.standard_normal((n, 2))


def _check(plane, stats, k, m, Kp=K, fb=FB, what=""):
    want_p, want_s = kmap_frame(k, Kp, m, fb)
    print(f"{what}: stats {stats.tolist()} occupied cells {np.count_nonzero(want_p)} largest count {want_p.max()}")
    assert plane.shape == (m, m) and plane.dtype == np.int64 and stats.dtype == np.int64
    np.testing.assert_array_equal(stats, want_s)
    np.testing.assert_array_equal(plane, want_p)
    return want_p, want_s


def _record_on_every_path(c, k, m, Kp=K, fb=FB, what=""):
    """One frame per path of the current packets; all equal the restatement."""
    c.kmap_series_begin(Kp, m, fb)
    for path in PATHS:
        c.debug_set(DEBUG_KMAP_GLOBAL, path)
        assert c.debug_get(DEBUG_KMAP_GLOBAL) == path
        c.kmap_series_record()
    c.debug_set(DEBUG_KMAP_GLOBAL, 0)
    planes, stats = c.kmap_series_get()
    assert planes.shape == (len(PATHS), m, m) and stats.shape == (len(PATHS), 8)
    want = _check(planes[0], stats[0], k, m, Kp, fb, what)
    for i in range(1, len(PATHS)):
        assert np.array_equal(planes[i], planes[0]) and np.array_equal(stats[i], stats[0]), f"path {PATHS[i]}"
    return want


@pytest.mark.parametrize("m", [1, 2, 7, 128, 300])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097])
def test_both_paths_match_the_restatement(kctx, n, m):
    x, k = _wavevectors(n)
    kctx.packets_set(x, k)
    _, kg = kctx.packets_get()
    want_p, want_s = _record_on_every_path(kctx, kg, m, what=f"n={n} m={m}")
    assert want_s[0] == n and want_p.sum() == n - want_s[1] - want_s[2]
    if n >= 1000:
        assert want_s[2] > 0 and want_s[3] != 0 and want_s[7] != 0  # some outside; signed sums
        assert m < 7 or np.count_nonzero(want_p) > m


def test_one_shared_cell(kctx):
    n = 4096
    x, _ = _wavevectors(n)
    k = np.tile([[1.2345, -2.5]], (n, 1))
    kctx.packets_set(x, k)
    for m in (7, 128, 300):
        want_p, want_s = _record_on_every_path(kctx, k, m, what=f"one cell m={m}")
        assert np.count_nonzero(want_p) == 1 and want_p.max() == n
        assert want_s[3] == n * int(np.rint(1.2345 * 2 ** FB))


def test_exact_ring(kctx):
    n = 4097
    x, _ = _wavevectors(n)
    th = 2 * np.pi * np.arange(1, n + 1) / n
    k = np.stack([3.0 * np.cos(th), 3.0 * np.sin(th)], axis=1)
    kctx.packets_set(x, k)
    for m in (64, 128, 512):
        want_p, want_s = _record_on_every_path(kctx, k, m, what=f"ring m={m}")
        assert want_s[1] == want_s[2] == 0 and want_p.sum() == n
        assert np.count_nonzero(want_p) < 4 * m  # the ring's cells only


def test_rejected_and_edge_packets(kctx):
    e = edge_wavevectors(K)
    k = np.array([[a, b] for a in e for b in e] + [[600.0, 600.0], [3000.0, 1.0], [2.5, 3.5]])
    x = np.zeros_like(k)
    kctx.packets_set(x, k)
    _, kg = kctx.packets_get()
    for m in (1, 7, 128, 129, 300):
        _, want_s = _record_on_every_path(kctx, kg, m, what=f"edges m={m}")
        assert want_s[1] > 0 and want_s[2] > 0
    _record_on_every_path(kctx, kg, 7, fb=0, what="edges frac_bits 0")
    _record_on_every_path(kctx, kg, 7, fb=32, what="edges frac_bits 32")
    for Kp in (0.1, 3.3, 1000.0):
        e = edge_wavevectors(Kp)
        k = np.array([[a, b] for a in e for b in e])
        kctx.packets_set(np.zeros_like(k), k)
        for m in (2, 128, 300):
            _record_on_every_path(kctx, k, m, Kp=Kp, what=f"edges K={Kp} m={m}")
    # nothing but rejected packets: an empty plane
    kctx.packets_set(np.zeros((3, 2)), np.array([[np.nan, 0.0], [0.0, np.inf], [1e9, 0.0]]))
    kctx.kmap_series_begin(K, 7, FB)
    kctx.kmap_series_record()
    planes, stats = kctx.kmap_series_get()
    assert not planes.any() and stats[0].tolist() == [3, 3, 0, 0, 0, 0, 0, 0]


KB = 40.0  # the blend cases' half-width: their ring has |k| = sqrt(135) (1 + 0.3 g), a few beyond it


def _blend_case(c, q, rebin_every, n=4097, seed=11):
    """Two 64^2 snapshots to blend and n packets on a thickened ring over the domain."""
    rng = np.random.default_rng(seed)
    x0, k0 = orc.initial_packets(n, q["L"], 4.0, q["f"], q["Cg"], rng)
    k0 = k0 * (1.0 + 0.3 * rng.standard_normal((n, 1)))
    planes = cbind.planes_of(q["flow"])
    c.set_field_grid(0, planes, q["nx"], q["L"])
    c.set_field_grid(1, 0.8 * np.asarray(planes), q["nx"], q["L"])
    c.set_locality(rebin_every, 0)
    c.packets_set(x0, k0)
    return x0, k0


def test_after_an_advance_and_a_rebinning(qg_case):
    q = qg_case
    frames = {}
    for rebin in (4, 0):
        c = sw.Context(0)
        try:
            _blend_case(c, q, rebin)
            c.kmap_series_begin(KB, 128, FB)
            c.advance(q["dt"], 10, q["f"], q["Cg"] ** 2, nslots=2, alpha0=0.05, dalpha=0.1, bump=orc.BUMP_QG)
            c.kmap_series_record()
            _, k1 = c.packets_get()
            c.advance(q["dt"], 3, q["f"], q["Cg"] ** 2, nslots=2, alpha0=0.0, dalpha=0.1,
                      bump=orc.BUMP_QG)  # (binning on: re-bins at step 12)
            c.debug_set(DEBUG_KMAP_GLOBAL, 1)
            c.kmap_series_record()
            _, k2 = c.packets_get()
            planes, stats = c.kmap_series_get()
            _check(planes[0], stats[0], k1, 128, KB, what=f"rebin_every={rebin}, 10 steps")
            _check(planes[1], stats[1], k2, 128, KB, what=f"rebin_every={rebin}, 13 steps")
            assert not np.array_equal(planes[0], planes[1])
            frames[rebin] = (planes, stats)
        finally:
            c.close()
    assert np.array_equal(frames[4][0], frames[0][0]) and np.array_equal(frames[4][1], frames[0][1])


def _check_history(c, m):
    frames = c._L.swrt_history_frames(c._h)
    hx, hk = c.history()
    c.kmap_series_begin(KB, m, FB)
    c.kmap_series_record_history(0, frames)
    assert c.kmap_series_frames() == frames
    planes, stats = c.kmap_series_get()
    for i in range(frames):
        _check(planes[i], stats[i], np.ascontiguousarray(hk[i].T), m, KB, what=f"history frame {i}")
    assert len({p.tobytes() for p in planes}) > 1  # the frames differ
    c.kmap_series_record_history(1, 3)  # a subrange, appended behind them
    p2, s2 = c.kmap_series_get(frames, 3)
    assert np.array_equal(p2, planes[1:4]) and np.array_equal(s2, stats[1:4])
    for bad_first, bad_count in ((0, frames + 1), (-1, 2), (frames, 1), (2, -1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*history"):
            c.kmap_series_record_history(bad_first, bad_count)
    # the bits of a record on packets set to each frame
    for i in range(frames):
        c.packets_set(np.ascontiguousarray(hx[i].T), np.ascontiguousarray(hk[i].T))
        c.kmap_series_reset()
        c.kmap_series_record()
        p1, s1 = c.kmap_series_get()
        assert np.array_equal(p1[0], planes[i]) and np.array_equal(s1[0], stats[i]), i
    return frames


@pytest.mark.parametrize("m", [64, 200])
def test_record_history_after_advance(fresh_ctx, qg_case, m):
    q = qg_case
    _blend_case(fresh_ctx, q, 4, n=1000)
    fresh_ctx.history_reset()
    fresh_ctx.advance(q["dt"], 12, q["f"], q["Cg"] ** 2, bump=orc.BUMP_QG, save_every=2)
    assert _check_history(fresh_ctx, m) == 6


def test_record_history_after_ode23_run_at(fresh_ctx, qg_case):
    q = qg_case
    _blend_case(fresh_ctx, q, 4, n=1000)
    fresh_ctx.history_reset()
    fresh_ctx.ode23_run_at(np.linspace(0.0, 40 * q["dt"], 7), 0.0, q["f"], q["Cg"], 1, 1e-3, 1e-6, orc.BUMP_QG)
    assert _check_history(fresh_ctx, 64) == 6


def test_series_grows(fresh_ctx):
    """m = 1024: 8 MiB a frame, the first reservation holds 8; the ninth record grows it."""
    c = fresh_ctx
    m = 1024
    sets = [_wavevectors(100 + i, seed=20 + i) for i in range(9)]
    c.kmap_series_begin(K, m, FB)
    for x, k in sets:
        c.packets_set(x, k)  # (another N keeps the frames: each is self-contained)
        c.kmap_series_record()
    assert c.kmap_series_frames() == 9
    planes, stats = c.kmap_series_get()
    for i, (_, k) in enumerate(sets):
        _check(planes[i], stats[i], k, m, what=f"frame {i}")


def test_get_reset_and_another_n(fresh_ctx):
    c = fresh_ctx
    m = 9
    xa, ka = _wavevectors(37, seed=8)
    xb, kb = _wavevectors(41, seed=9)
    c.packets_set(xa, ka)
    c.kmap_series_begin(3.3, m, 12)
    c.kmap_series_record()
    c.packets_set(xb, kb)
    assert c.kmap_series_frames() == 1 and c.kmap_series_cells() == m
    c.kmap_series_record()
    planes, stats = c.kmap_series_get()
    want_a = _check(planes[0], stats[0], ka, m, 3.3, 12, "frame of the first set")
    want_b = _check(planes[1], stats[1], kb, m, 3.3, 12, "frame of the second set")
    i64 = ctypes.POINTER(ctypes.c_int64)
    only_p = np.zeros((2, m, m), dtype=np.int64)
    only_s = np.zeros((2, 8), dtype=np.int64)
    assert c._L.swrt_kmap_series_get(c._h, 0, 2, only_p.ctypes.data_as(i64), None) == 0
    assert c._L.swrt_kmap_series_get(c._h, 0, 2, None, only_s.ctypes.data_as(i64)) == 0
    np.testing.assert_array_equal(only_p.transpose(0, 2, 1), np.stack([want_a[0], want_b[0]]))
    np.testing.assert_array_equal(only_s, np.stack([want_a[1], want_b[1]]))
    p1, s1 = c.kmap_series_get(1, 1)
    assert np.array_equal(p1[0], planes[1]) and np.array_equal(s1[0], stats[1])
    c.kmap_series_reset()
    assert c.kmap_series_frames() == 0 and c.kmap_series_cells() == m
    assert c.kmap_series_get()[0].shape == (0, m, m)
    c.kmap_series_record()  # K, m and frac_bits stay
    planes, stats = c.kmap_series_get()
    _check(planes[0], stats[0], kb, m, 3.3, 12, "frame 0 after the reset")


def test_errors(fresh_ctx):
    c = fresh_ctx
    x, k = _wavevectors(37)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):
        c.kmap_series_record()
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):
        c.kmap_series_record_history(0, 0)
    assert c.kmap_series_frames() == 0 and c.kmap_series_cells() == 0
    for bad, name in ((dict(m=0), "m must"), (dict(m=4097), "m must"), (dict(m=-3), "m must"), (dict(K=0.0), "K must"),
                      (dict(K=-1.0), "K must"), (dict(K=np.inf), "K must"), (dict(K=np.nan), "K must"),
                      (dict(frac_bits=-1), "frac_bits must"), (dict(frac_bits=33), "frac_bits must")):
        kw = dict(K=K, m=8, frac_bits=FB)
        kw.update(bad)
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*" + name):
            c.kmap_series_begin(**kw)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):  # a refused begin opens nothing
        c.kmap_series_record()
    c.kmap_series_begin(K, 8, FB)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*no packets"):
        c.kmap_series_record()
    c.packets_set(x, k)
    c.kmap_series_record()
    for first, count in ((-1, 1), (0, 2), (1, 1), (0, -1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*range"):
            c.kmap_series_get(first, count)
    assert c._L.swrt_kmap_series_get(c._h, 0, 1, None, None) == 1 and b"NULL" in c._L.swrt_last_error(c._h)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*history"):
        c.kmap_series_record_history(0, 1)  # no history frames
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
        c.debug_set(DEBUG_KMAP_GLOBAL, 4)
    c.kmap_series_record()  # the open series is still usable
    assert c.kmap_series_frames() == 2


# ---- the ensemble and the drivers ---------------------------------------------

KMAP_FILES = ("kmap_n.bin", "kmap_stats.bin", "kmap_geom.bin")


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


def _check_driver_files(d, facts, n, m, ring, fb=16):
    frames = facts["packet_frames"]
    assert facts["kmap_frames"] == frames > 1
    kf = sw.read_field(os.path.join(d, "packet_k"), n, 2, 1).reshape(n, 2, frames)
    got = np.fromfile(os.path.join(d, "kmap_n.bin"), dtype=np.int64).reshape(frames, m, m).transpose(0, 2, 1)
    stats = np.fromfile(os.path.join(d, "kmap_stats.bin"), dtype=np.int64).reshape(frames, 8)
    geom = np.fromfile(os.path.join(d, "kmap_geom.bin"), dtype=np.float64)
    assert geom.tolist() == [4.0 * ring, m, fb]
    assert sw.read_field(os.path.join(d, "packet_time")).shape == (1, frames)
    for i in range(frames):
        _check(got[i], stats[i], kf[:, :, i], m, 4.0 * ring, fb, what=f"driver frame {i}")
    assert not np.array_equal(got[0], got[-1])  # the wavevectors moved
    assert (stats[:, 0] == n).all() and (stats[:, 1] == 0).all()  # nobody rejected: the run stayed finite
    mom = sw.kmap_moments(stats, fb)
    np.testing.assert_allclose(mom["mean"][0], 0.0, atol=1e-3)  # the initial ring: centred, radius `ring`
    np.testing.assert_allclose(np.trace(mom["cov"][0]), ring ** 2, rtol=1e-3)


def test_driver_kmaps_equal_the_restatement_on_its_packet_frames(ctx, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    args = (32, 200, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0)
    ring = np.sqrt((4.0 ** 2 - 1) * 3.0 ** 2 / 1.0 ** 2)
    kw = dict(ctx=ctx, max_steps=12, nsub=2, r_drag=0.0)
    facts = sw.qgsw_raytrace(*args, out_dir=a, kmap_cells=16, **kw)
    assert set(KMAP_FILES) <= set(_files(a))
    _check_driver_files(a, facts, 200, 16, ring)
    # packet_files=False with kmap_cells alone: the k-plane files, no packet frames
    facts_b = sw.qgsw_raytrace(*args, out_dir=b, kmap_cells=16, packet_files=False, **kw)
    fa, fb = _files(a), _files(b)
    assert facts_b["kmap_frames"] == facts["kmap_frames"]
    assert "packet_x.bin" not in fb and "packet_k.bin" not in fb and fb["packet_time.bin"] == fa["packet_time.bin"]
    for name in KMAP_FILES:
        assert fa[name] == fb[name], name
    with pytest.raises(ValueError, match="packet_files=False"):
        sw.qgsw_raytrace(*args, out_dir=b, packet_files=False, **kw)
    # a plain run writes none of them and reports no frames
    plain = sw.qgsw_raytrace(*args, out_dir=b, **kw)
    assert plain["kmap_frames"] == 0 and not set(KMAP_FILES) & set(_files(b))
    # an explicit half-width and frac_bits
    facts = sw.qgsw_raytrace(*args, out_dir=b, kmap_cells=7, kmap_kmax=ring, kmap_frac_bits=8, **kw)
    geom = np.fromfile(os.path.join(b, "kmap_geom.bin"))
    assert geom.tolist() == [ring, 7, 8]
    kf = sw.read_field(os.path.join(b, "packet_k"), 200, 2, 1).reshape(200, 2, -1)
    got = np.fromfile(os.path.join(b, "kmap_n.bin"), dtype=np.int64).reshape(-1, 7, 7).transpose(0, 2, 1)
    stats = np.fromfile(os.path.join(b, "kmap_stats.bin"), dtype=np.int64).reshape(-1, 8)
    for i in range(facts["packet_frames"]):
        _check(got[i], stats[i], kf[:, :, i], 7, ring, 8, what=f"K = ring, frame {i}")
    assert stats[:, 2].max() > 0  # the ring sits on the plane's edge: some packets are outside


def test_two_layer_driver_kmaps(ctx, tmp_path):
    facts = sw.qg2layersw_raytrace(32, 200, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path), nsub=2,
                                   max_steps=30, seed=5, ctx=ctx, kmap_cells=16)
    _check_driver_files(str(tmp_path), facts, 200, 16, np.sqrt(15.0 * 9.0))


def test_record_kmap_drains_a_large_series(fresh_ctx, tmp_path, monkeypatch):
    """The drain (get, combine, append, reset) at a lowered threshold: the same files as one write at the end."""
    import swraytracing_amd.integrate as integ
    x, k = _wavevectors(1000, seed=10)
    m = 16

    def run(d, threshold):
        monkeypatch.setattr(integ, "MAP_DRAIN_BYTES", threshold)
        os.makedirs(d)
        ens = sw.PacketEnsemble(x, k, 2 * np.pi, 3.0, 1.0, 64, 3.0, ctx=fresh_ctx)
        ens.begin_kmap(K, m, FB, directory=d if threshold < 1 << 20 else None)
        for i in range(7):
            fresh_ctx.packets_set(x, k * (1.0 + 0.05 * i))
            ens.record_kmap()
        if threshold >= 1 << 20:
            planes, stats = ens.kmap_series()
            assert planes.shape == (7, m, m)
            np.testing.assert_array_equal(planes[6], kmap_frame(k * (1.0 + 0.05 * 6), K, m, FB)[0])
            assert stats[:, 0].tolist() == [1000] * 7
        assert ens.write_kmaps(d) == 7
        return _files(d)

    whole = run(str(tmp_path / "whole"), 256 << 20)
    drained = run(str(tmp_path / "drained"), 3 * 8 * (m * m + 8) - 1)  # drains at every third frame
    assert set(whole) == set(KMAP_FILES) and whole == drained
    assert len(whole["kmap_n.bin"]) == 7 * m * m * 8 and len(whole["kmap_stats.bin"]) == 7 * 8 * 8
