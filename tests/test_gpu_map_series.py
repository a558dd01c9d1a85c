"""The packet density and wave-energy maps on the device (swrt_map_series_*;
swraytracing_amd/csrc/swrt_map.hpp) and the drivers' map files.

Expected values are tests/map_series_ref.py, the numpy restatement of the
contract in include/swrt.h, on the same packets.  Every comparison is exact
integer equality: integer sums are order-free, so there is no tolerance.
Unless a case says otherwise f = 3, Cg = 1, frac_bits = 20."""
import os

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import cbind, swrt_oracle as orc
from swraytracing_amd._lib import DEBUG_HAZARD_CHECK, DEBUG_MAP_STRAYS, DEBUG_MAP_TILED_FRAMES
from tests.map_series_ref import edge_positions, map_frame

pytestmark = pytest.mark.gpu

F, CG, L = 3.0, 1.0, 2 * np.pi
NTILE = 70001  # above the two-packet-stream threshold (65536)


def _packets(n, seed=3, span=40.0, kmax=6.0):
    """Positions uniform in [-span, span]^2 with the edge positions in front, |k| < kmax."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-span, span, (n, 2))
    e = edge_positions(L)[:n]
    x[:e.size, 0] = e
    x[:e.size, 1] = e[::-1]
    th = rng.uniform(0, 2 * np.pi, n)
    r = kmax * rng.random(n)
    return x, np.stack([r * np.cos(th), r * np.sin(th)], axis=1)


def _check(planes, stats, x, k, m, Lm=L, fb=20, what=""):
    want_p, want_s = map_frame(x, k, Lm, m, F, CG, fb)
    print(f"{what}: n {stats[0]} rejected {stats[1]} occupied cells {np.count_nonzero(want_p[0])} "
          f"largest count {want_p[0].max()}")
    assert planes.shape == (4, m, m) and planes.dtype == np.int64 and stats.dtype == np.int64
    np.testing.assert_array_equal(stats, want_s)
    np.testing.assert_array_equal(planes, want_p)
    return want_p, want_s


@pytest.mark.parametrize("m", [1, 5, 64, 100])
@pytest.mark.parametrize("n", [1, 37, 1000, 70001])
def test_general_path_matches_the_restatement(ctx, n, m):
    x, k = _packets(n)
    ctx.packets_set(x, k)  # no field set, nothing binned: the general path
    tiled = ctx.debug_get(DEBUG_MAP_TILED_FRAMES)
    ctx.map_series_begin(L, m, F, CG)
    ctx.map_series_record()
    planes, stats = ctx.map_series()
    assert planes.shape == (1, 4, m, m) and stats.shape == (1, 2)
    want_p, _ = _check(planes[0], stats[0], x, k, m, what=f"n={n} m={m}")
    assert want_p[0].sum() == n
    if n >= 1000 and m >= 5:
        assert np.count_nonzero(want_p[0]) > m and (want_p[2] < 0).any() and (want_p[3] > 0).any()
    # the same state again: the same bits, appended
    ctx.map_series_record()
    p2, s2 = ctx.map_series()
    assert ctx.map_series_frames() == 2
    assert np.array_equal(p2[1], planes[0]) and np.array_equal(p2[0], planes[0]) and np.array_equal(s2[1], stats[0])
    assert ctx.debug_get(DEBUG_MAP_TILED_FRAMES) == tiled


@pytest.mark.parametrize("fb", [0, 20, 32])
def test_frac_bits(ctx, fb):
    x, k = _packets(1000, seed=4)
    k[:4] = [[0.5, 1.5], [2.5, -0.5], [2.0 ** -21, 3 * 2.0 ** -21], [-1.5, 3.5]]  # halves: round to even
    ctx.packets_set(x, k)
    ctx.map_series_begin(L, 7, F, CG, fb)
    ctx.map_series_record()
    planes, stats = ctx.map_series()
    _check(planes[0], stats[0], x, k, 7, fb=fb, what=f"frac_bits={fb}")


def test_rejected_packets(ctx):
    n = 1000
    x, k = _packets(n, seed=5)
    x[11, 0] = np.nan
    x[12, 1] = np.inf
    x[13] = [-np.inf, np.nan]
    k[14, 0] = np.nan
    k[15, 1] = -np.inf
    k[16, 0] = 2.0 ** 18            # k * 2^20 == 2^38
    k[17, 1] = -3.0e5               # above it
    k[18, 0] = np.nextafter(2.0 ** 18, 0)  # k in range, omega not
    k[19, 0] = 2.0 ** 17            # in range: kept
    ctx.packets_set(x, k)
    ctx.map_series_begin(L, 9, F, CG)
    ctx.map_series_record()
    planes, stats = ctx.map_series()
    want_p, want_s = _check(planes[0], stats[0], x, k, 9, what="rejected")
    assert want_s.tolist() == [n, 8] and planes[0, 0].sum() == n - 8
    # nothing but rejected packets: empty planes
    ctx.packets_set(x[11:14], k[11:14])
    ctx.map_series_record()
    planes, stats = ctx.map_series(1, 1)
    assert not planes.any() and stats[0].tolist() == [3, 3]


def _flow_planes(q):
    return cbind.planes_of(q["flow"])


def _tile_case(c, q, rebin_every, n=NTILE, seed=11):
    """A 64^2 field (4 x 4 tiles of the LDS tile kernel) and n packets over the domain."""
    rng = np.random.default_rng(seed)
    x0, k0 = orc.initial_packets(n, q["L"], 4.0, q["f"], q["Cg"], rng)
    k0 = k0 * (1.0 + 0.3 * rng.standard_normal((n, 1)))
    c.set_field_grid(0, _flow_planes(q), q["nx"], q["L"])
    c.set_locality(rebin_every, 0)
    c.packets_set(x0, k0)
    return x0, k0


def test_tile_path_matches_the_restatement(fresh_ctx, qg_case):
    c, q = fresh_ctx, qg_case
    _tile_case(c, q, 5)
    c.advance(q["dt"], 7, q["f"], q["Cg"] ** 2, bump=orc.BUMP_QG)
    x, k = c.packets_get()
    tiled = c.debug_get(DEBUG_MAP_TILED_FRAMES)
    assert tiled == 0
    first = None
    for m in (64, 32, 16, 8, 4):  # c = 1, 2, 4, 8, 16 field cells per map cell
        c.map_series_begin(q["L"], m, F, CG)
        c.map_series_record()
        tiled += 1
        assert c.debug_get(DEBUG_MAP_TILED_FRAMES) == tiled, m
        planes, stats = c.map_series()
        want_p, _ = _check(planes[0], stats[0], x, k, m, q["L"], what=f"tile path m={m}")
        assert np.count_nonzero(want_p[0]) == m * m  # every cell holds packets
        first = planes[0] if first is None else first
    # a coarse map is the block sum of a fine one (c x c cells): the integers say so exactly
    c.map_series_begin(q["L"], 16, F, CG)
    c.map_series_record()
    coarse = c.map_series()[0][0]
    np.testing.assert_array_equal(first.reshape(4, 16, 4, 16, 4).sum(axis=(2, 4)), coarse)
    tiled += 1
    # a cell that is not c x c field cells with c | 16, or another domain: the general path, the same contract
    for m, Lm in ((48, q["L"]), (100, q["L"]), (2, q["L"]), (32, 2 * q["L"]), (64, 0.5 * q["L"])):
        c.map_series_begin(Lm, m, F, CG)
        c.map_series_record()
        assert c.debug_get(DEBUG_MAP_TILED_FRAMES) == tiled, (m, Lm)
        planes, stats = c.map_series()
        _check(planes[0], stats[0], x, k, m, Lm, what=f"general path on binned packets m={m} L={Lm:.3f}")
    # the two paths on the same packets: binning switched off, the same bits
    c.set_locality(0, 0)
    c.map_series_begin(q["L"], 64, F, CG)
    c.map_series_record()
    assert c.debug_get(DEBUG_MAP_TILED_FRAMES) == tiled
    assert np.array_equal(c.map_series()[0][0], first)
    assert c.debug_get(DEBUG_MAP_STRAYS) == 0  # five steps of ~0.2 cells since the re-binning: nobody left a window


def test_tile_path_rejects_like_the_general_path(fresh_ctx, qg_case):
    """Moments out of range on binned packets: |k| up to ~200, frac_bits 32 keeps |v| < 64."""
    c, q = fresh_ctx, qg_case
    n = NTILE
    rng = np.random.default_rng(12)
    x0, k0 = orc.initial_packets(n, q["L"], 4.0, q["f"], q["Cg"], rng)
    k0 = k0 * (4.0 * np.abs(rng.standard_normal((n, 1))))
    c.set_field_grid(0, _flow_planes(q), q["nx"], q["L"])
    c.set_locality(5, 0)
    c.packets_set(x0, k0)
    c.advance(q["dt"], 1, q["f"], q["Cg"] ** 2, bump=orc.BUMP_QG)  # bins the packets
    x, k = c.packets_get()
    c.map_series_begin(q["L"], 32, F, CG, 32)  # frac_bits 32: |k| >= 64 is out of range
    c.map_series_record()
    assert c.debug_get(DEBUG_MAP_TILED_FRAMES) == 1
    planes, stats = c.map_series()
    _, want_s = _check(planes[0], stats[0], x, k, 32, q["L"], fb=32, what="tile path, frac_bits 32")
    assert n // 20 < want_s[1] < n // 2
    c.map_series_begin(q["L"], 32, 2.0 ** 19, CG, 20)  # omega >= f = 2^19: every packet rejected
    c.map_series_record()
    planes, stats = c.map_series()
    assert c.debug_get(DEBUG_MAP_TILED_FRAMES) == 2
    assert not planes.any() and stats[0].tolist() == [n, n]


def test_strays_add_through_global_memory(fresh_ctx, qg_case):
    c, q = fresh_ctx, qg_case
    x0, _ = _tile_case(c, q, 1000)
    c.advance(q["dt"], 60, q["f"], q["Cg"] ** 2, bump=orc.BUMP_QG)  # one binning, then 60 steps of drift
    x, k = c.packets_get()
    drift = np.abs(x - x0).max() / (q["L"] / q["nx"])
    print(f"largest drift {drift:.1f} cells")
    assert drift > 6  # past the window's ring of 3 cells at m = 64
    strays = 0
    for m in (64, 16, 4):
        c.map_series_begin(q["L"], m, F, CG)
        c.map_series_record()
        planes, stats = c.map_series()
        _check(planes[0], stats[0], x, k, m, q["L"], what=f"strays m={m}")
        now = c.debug_get(DEBUG_MAP_STRAYS)
        print(f"m={m}: strays {now - strays} of {NTILE}")
        if m == 64:
            assert 0 < now - strays < NTILE
        strays = now
    assert c.debug_get(DEBUG_MAP_TILED_FRAMES) == 3


def test_record_after_split_advance_under_the_hazard_checker(fresh_ctx, qg_case):
    """Two packet streams: advance leaves part launches on the second stream;
    record reads the packet buffers and must be ordered behind them."""
    c, q = fresh_ctx, qg_case
    c.debug_set(DEBUG_HAZARD_CHECK, 1)
    _tile_case(c, q, 5)
    c.map_series_begin(q["L"], 32, F, CG)
    states = []
    for _ in range(3):
        c.advance(q["dt"], 3, q["f"], q["Cg"] ** 2, bump=orc.BUMP_QG)
        c.map_series_record()
    c.map_series_reset()
    for _ in range(3):
        c.advance(q["dt"], 3, q["f"], q["Cg"] ** 2, bump=orc.BUMP_QG)
        c.map_series_record()
        states.append(c.packets_get())
    planes, stats = c.map_series()
    for i, (x, k) in enumerate(states):
        _check(planes[i], stats[i], x, k, 32, q["L"], what=f"hazard-checked frame {i}")
    assert c.debug_get(DEBUG_MAP_TILED_FRAMES) == 6


def test_record_history_equals_per_frame_records(fresh_ctx, qg_case):
    c, q = fresh_ctx, qg_case
    _tile_case(c, q, 4, n=1000)
    c.history_reset()
    c.advance(q["dt"], 12, q["f"], q["Cg"] ** 2, bump=orc.BUMP_QG, save_every=1)
    frames = c._L.swrt_history_frames(c._h)
    assert frames == 12
    hx, hk = c.history()
    m = 16
    c.map_series_begin(q["L"], m, F, CG)
    c.map_series_record_history(0, frames)
    assert c.map_series_frames() == frames
    planes, stats = c.map_series()
    for i in range(frames):
        _check(planes[i], stats[i], np.ascontiguousarray(hx[i].T), np.ascontiguousarray(hk[i].T), m, q["L"],
               what=f"history frame {i}")
    assert len({p.tobytes() for p in planes}) > 1  # the frames differ
    c.map_series_record_history(3, 4)  # a subrange, appended behind them
    p2, s2 = c.map_series(frames, 4)
    assert np.array_equal(p2, planes[3:7]) and np.array_equal(s2, stats[3:7])
    for bad_first, bad_count in ((0, frames + 1), (-1, 2), (frames, 1), (2, -1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*history"):
            c.map_series_record_history(bad_first, bad_count)
    # the bits of a record on packets set to that frame
    c.packets_set(np.ascontiguousarray(hx[frames - 2].T), np.ascontiguousarray(hk[frames - 2].T))
    c.map_series_reset()
    c.map_series_record()
    p1, s1 = c.map_series()
    assert np.array_equal(p1[0], planes[frames - 2]) and np.array_equal(s1[0], stats[frames - 2])


def test_series_grows_and_resets(fresh_ctx):
    c = fresh_ctx
    m = 100  # 320 kB a frame: the first reservation holds 209 frames
    xa, ka = _packets(37, seed=8)
    xb, kb = _packets(41, seed=9)  # another N keeps the series: a frame is self-contained
    c.packets_set(xa, ka)
    c.map_series_begin(L, m, F, CG)
    for i in range(215):
        if i == 205:
            c.packets_set(xb, kb)
        c.map_series_record()
    assert c.map_series_frames() == 215
    planes, stats = c.map_series()
    for i, (x, k) in ((0, (xa, ka)), (204, (xa, ka)), (205, (xb, kb)), (209, (xb, kb)), (214, (xb, kb))):
        _check(planes[i], stats[i], x, k, m, what=f"frame {i}")
    assert (planes[:205] == planes[0]).all() and (planes[205:] == planes[214]).all()
    p2, s2 = c.map_series(208, 3)
    assert np.array_equal(p2, planes[208:211]) and np.array_equal(s2, stats[208:211])
    c.map_series_reset()
    assert c.map_series_frames() == 0 and c.map_series()[0].shape == (0, 4, m, m)
    c.packets_set(xa, ka)
    c.map_series_record()  # L, m, f, Cg and frac_bits stay
    planes, stats = c.map_series()
    _check(planes[0], stats[0], xa, ka, m, what="frame 0 after the reset")


def test_errors(fresh_ctx):
    c = fresh_ctx
    x, k = _packets(37)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):
        c.map_series_record()
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):
        c.map_series_record_history(0, 0)
    assert c.map_series_frames() == 0 and c._L.swrt_map_series_cells(c._h) == 0
    for bad in (dict(m=0), dict(m=4097), dict(m=-3), dict(L=0.0), dict(L=-1.0), dict(L=np.inf), dict(L=np.nan),
                dict(frac_bits=-1), dict(frac_bits=33)):
        kw = dict(L=L, m=8, f=F, Cg=CG, frac_bits=20)
        kw.update(bad)
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
            c.map_series_begin(**kw)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):  # a refused begin opens nothing
        c.map_series_record()
    c.map_series_begin(L, 8, F, CG)
    assert c._L.swrt_map_series_cells(c._h) == 8
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*no packets"):
        c.map_series_record()
    c.packets_set(x, k)
    c.map_series_record()
    for first, count in ((-1, 1), (0, 2), (1, 1), (0, -1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
            c.map_series(first, count)
    assert c._L.swrt_map_series_get(c._h, 0, 1, None, None) == 1 and b"NULL" in c._L.swrt_last_error(c._h)
    import ctypes
    out = np.zeros(4 * 64, dtype=np.int64)  # the stats may be NULL
    assert c._L.swrt_map_series_get(c._h, 0, 1, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None) == 0
    want, _ = map_frame(x, k, L, 8, F, CG)
    np.testing.assert_array_equal(out.reshape(4, 8, 8).transpose(0, 2, 1), want)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*history"):
        c.map_series_record_history(0, 1)  # no history frames
    # more than 2^24 packets: refused by begin and by record
    big = (1 << 24) + 1
    c.packets_set(np.zeros((big, 2)), np.zeros((big, 2)))
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*2\\^24"):
        c.map_series_record()
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*2\\^24"):
        c.map_series_begin(L, 8, F, CG)
    c.packets_set(x, k)
    c.map_series_record()  # the open series is still usable
    assert c.map_series_frames() == 2


def test_largest_map(fresh_ctx):
    """m = 4096: one frame is 512 MB, the first reservation a single frame."""
    c = fresh_ctx
    x, k = _packets(37)
    c.packets_set(x, k)
    c.map_series_begin(L, 4096, F, CG)
    c.map_series_record()
    assert c.map_series_frames() == 1
    planes, stats = c.map_series()
    assert planes[0, 0].sum() == 37 and stats[0].tolist() == [37, 0]
    want, _ = map_frame(x, k, L, 4096, F, CG)
    assert np.array_equal(planes[0], want)


# ---- the ensemble and the drivers ---------------------------------------------

MAP_FILES = ("map_n.bin", "map_omega.bin", "map_k.bin", "map_l.bin", "map_stats.bin")
QG1 = (64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0)
QG1_KW = dict(nsub=2, max_steps=24, r_drag=0.0)


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


def _check_driver_files(d, facts, n, m, Ld, fb=20):
    frames = facts["packet_frames"]
    assert facts["map_frames"] == frames > 1
    xf = sw.read_field(os.path.join(d, "packet_x"), n, 2, 1).reshape(n, 2, frames)
    kf = sw.read_field(os.path.join(d, "packet_k"), n, 2, 1).reshape(n, 2, frames)
    got = [sw.read_field(os.path.join(d, name), m, m, 1).reshape(m, m, frames)
           for name in ("map_n", "map_omega", "map_k", "map_l")]
    stats = sw.read_field(os.path.join(d, "map_stats"), 4, 1, 1).reshape(4, frames)
    assert sw.read_field(os.path.join(d, "packet_time")).shape == (1, frames)
    for i in range(frames):
        # (packet_x.bin holds positions wrapped to [-L/2, L/2): the restatement's own mod maps them back)
        want_p, want_s = map_frame(xf[:, :, i], kf[:, :, i], Ld, m, 3.0, 1.0, fb)
        for p in range(4):
            np.testing.assert_array_equal(got[p][:, :, i], want_p[p].astype(np.float64), err_msg=f"frame {i} plane {p}")
        assert stats[:, i].tolist() == [n, 0, m, fb] and want_s.tolist() == [n, 0]
    assert not np.array_equal(got[0][:, :, 0], got[0][:, :, -1])  # the packets moved
    return got


def test_driver_maps_equal_the_restatement_on_its_packet_frames(ctx, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    facts = sw.qgsw_raytrace(*QG1, out_dir=a, ctx=ctx, map_cells=32, **QG1_KW)
    assert set(MAP_FILES) <= set(_files(a))
    _check_driver_files(a, facts, 4001, 32, 2 * np.pi)
    # nothing else changes: the other files are those of a run without maps
    plain = sw.qgsw_raytrace(*QG1, out_dir=b, ctx=ctx, **QG1_KW)
    fa, fb = _files(a), _files(b)
    assert plain["map_frames"] == 0 and not set(MAP_FILES) & set(fb)
    assert {k: v for k, v in plain.items() if k != "map_frames"} == {k: v for k, v in facts.items() if k != "map_frames"}
    assert set(fa) == set(fb) | set(MAP_FILES)
    for name in fb:
        assert fa[name] == fb[name], name
    # fresh=True removes earlier map files; another frac_bits scales the sums
    for name in MAP_FILES:
        (tmp_path / "b" / name).write_bytes(b"\0" * 8)
    facts = sw.qgsw_raytrace(*QG1, out_dir=b, ctx=ctx, map_cells=32, map_frac_bits=8, **QG1_KW)
    _check_driver_files(b, facts, 4001, 32, 2 * np.pi, fb=8)


def test_two_layer_driver_maps(ctx, tmp_path):
    facts = sw.qg2layersw_raytrace(64, 5001, 4.0, 10.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path), nsub=2,
                                   max_steps=30, seed=5, ctx=ctx, map_cells=32)
    _check_driver_files(str(tmp_path), facts, 5001, 32, 20.0)


def test_record_map_drains_a_large_series(fresh_ctx, tmp_path, monkeypatch):
    """The drain (get, combine, append, reset) at a lowered threshold: the same files as one write at the end."""
    import swraytracing_amd.integrate as integ
    x, k = _packets(1000, seed=10, span=np.pi)
    m = 16

    def run(d, threshold):
        monkeypatch.setattr(integ, "MAP_DRAIN_BYTES", threshold)
        os.makedirs(d)
        ens = sw.PacketEnsemble(x, k, L, F, CG, 64, F / CG, ctx=fresh_ctx)
        ens.begin_map(m, directory=d if threshold < 1 << 20 else None)
        for i in range(7):
            fresh_ctx.packets_set(x + 0.05 * i, k)
            ens.record_map()
        assert ens.write_maps(d) == 7
        return _files(d)

    whole = run(str(tmp_path / "whole"), 256 << 20)
    drained = run(str(tmp_path / "drained"), 3 * 32 * m * m - 1)  # drains at every third frame
    assert set(whole) == set(MAP_FILES) and whole == drained
    assert len(whole["map_n.bin"]) == 7 * m * m * 8 and len(whole["map_stats.bin"]) == 7 * 4 * 8
    got = sw.read_field(str(tmp_path / "whole" / "map_n"), m, m, 1).reshape(m, m, 7)
    np.testing.assert_array_equal(got[:, :, 6], map_frame(x + 0.05 * 6, k, L, m, F, CG)[0][0])
