"""The energy-vs-omega series on the device (swrt_omega_series_*,
swrt_omega_ideal; swraytracing_amd/csrc/swrt_diag.hpp) and the drivers'
spectrum files.

Reference: analysis/load_data.m:33-52,63 and ideal_omega_distribution.m:3-11.
Expected values are numpy on the same k: omega in the header's operation
order, the bin by np.searchsorted(edges, w, "right") - 1 with the closed last
bin (not np.histogram's uniform fast path).  Counts, n, min and max must be
equal exactly; sum omega is compared with math.fsum within 2*N*2^-53*sum, the
first-order bound between any two summation orders of N positive terms.
Unless a case says otherwise f = 3, Cg = 1."""
import math
import os

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import cbind, swrt_oracle as orc

pytestmark = pytest.mark.gpu

F, CG = 3.0, 1.0
NPASS = 262144 + 257  # past one pass of a 1024 x 256 grid


def _omega(k, f=F, Cg=CG):
    k1, k2 = k[:, 0], k[:, 1]
    return np.sqrt(f * f + Cg * Cg * (k1 * k1 + k2 * k2))  # load_data.m:33


def _row(w, edges):
    """[below, bins, above] of the omega values w; NaN counted nowhere."""
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    w = w[~np.isnan(w)]
    b = np.searchsorted(edges, w, "right") - 1
    b[w == edges[-1]] = nb - 1
    slot = np.where(w < edges[0], 0, np.where(w > edges[-1], nb + 1, b + 1))
    return np.bincount(slot, minlength=nb + 2).astype(np.int64)


def _check(counts, stats, k, edges, f=F, Cg=CG, what=""):
    w = _omega(k, f, Cg)
    want = _row(w, edges)
    print(f"{what}: n {stats[0]!r} sum {stats[1]!r} min {stats[2]!r} max {stats[3]!r} "
          f"below {counts[0]} above {counts[-1]} nonzero bins {np.count_nonzero(counts[1:-1])}")
    np.testing.assert_array_equal(counts, want)
    assert stats[0] == w.size
    if np.isnan(w).any():
        assert np.isnan(stats[1])
    else:
        s = math.fsum(w)
        print(f"{what}: sum diff {abs(stats[1] - s):.3e} bound {2 * w.size * 2.0 ** -53 * s:.3e}")
        assert abs(stats[1] - s) <= 2 * w.size * 2.0 ** -53 * s
    assert stats[2] == np.nanmin(w) and stats[3] == np.nanmax(w)
    return want


def _packets(n, seed=3, kmax=6.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-np.pi, np.pi, (n, 2))
    th = rng.uniform(0, 2 * np.pi, n)
    r = kmax * rng.random(n)
    return x, np.stack([r * np.cos(th), r * np.sin(th)], axis=1)


def _one(c, x, k, edges, f=F, Cg=CG):
    """begin, packets, one record -> (counts row, stats row)"""
    c.packets_set(x, k)
    c.omega_series_begin(f, Cg, edges)
    c.omega_series_record()
    counts, stats = c.omega_series()
    assert counts.shape == (1, len(edges) + 1) and stats.shape == (1, 4) and counts.dtype == np.int64
    return counts[0], stats[0]


@pytest.mark.parametrize("nbins", [1, 300, 4096])
@pytest.mark.parametrize("n", [1, 37, 1000, NPASS])
def test_frame_matches_numpy(ctx, n, nbins):
    # omega of |k| < 6 lies in [3, 6.71): edges inside that range leave packets below and above
    edges = np.linspace(3.5, 6.0, nbins + 1)
    x, k = _packets(n)
    counts, stats = _one(ctx, x, k, edges)
    want = _check(counts, stats, k, edges, what=f"n={n} nbins={nbins}")
    if n >= 1000:
        assert want[0] > 0 and want[-1] > 0 and np.count_nonzero(want[1:-1]) >= min(nbins, 2)
    # the same state again: the same bits, appended
    ctx.omega_series_record()
    c2, s2 = ctx.omega_series()
    assert ctx.omega_series_frames() == 2
    assert c2[1].tobytes() == counts.tobytes() and s2[1].tobytes() == stats.tobytes()
    assert c2[0].tobytes() == counts.tobytes()


def test_every_packet_in_one_bin(ctx):
    """The drivers' initial ring (qgsw_raytrace.m:56-60): |k| the same for all."""
    rng = np.random.default_rng(146)
    x, k = orc.initial_packets(NPASS, 2 * np.pi, 4.0, F, CG, rng)
    edges = np.linspace(0.02, 15.02, 301)
    want = _row(_omega(k), edges)
    assert np.count_nonzero(want) == 1 and want[1:-1].max() == NPASS
    counts, stats = _one(ctx, x, k, edges)
    _check(counts, stats, k, edges, what="ring")
    # ... and in two neighbouring bins (an edge through the ring's rounding spread, or beside it)
    w = _omega(k)
    edges2 = np.array([0.0, np.median(w), 15.0])
    counts, stats = _one(ctx, x, k, edges2)
    _check(counts, stats, k, edges2, what="ring, two bins")


@pytest.mark.parametrize("edges,slot", [([1.0, 2.0, 3.0, 4.0, 5.0], 3),   # an edge at f: bin 2
                                        ([0.0, 1.0, 2.0, 3.0], 3),        # the last edge at f: the closed last bin
                                        ([3.0, 4.0], 1)])                 # the first edge at f
@pytest.mark.parametrize("n", [37, 1000])
def test_omega_exactly_on_an_edge(ctx, n, edges, slot):
    x, _ = _packets(n)
    k = np.zeros((n, 2))
    assert (_omega(k) == F).all()
    counts, stats = _one(ctx, x, k, edges)
    _check(counts, stats, k, edges, what=f"k=0 edges={edges}")
    assert counts[slot] == n and counts.sum() == n
    assert stats[2] == F and stats[3] == F


def test_below_above_and_nan(ctx):
    n = 1000
    x, k = _packets(n, seed=5)
    k[17] = np.nan
    k[640, 1] = np.nan
    edges = np.linspace(4.0, 5.0, 11)
    counts, stats = _one(ctx, x, k, edges)
    _check(counts, stats, k, edges, what="nan")
    assert counts[0] > 0 and counts[-1] > 0
    assert stats[0] - counts.sum() == 2
    assert np.isnan(stats[1]) and np.isfinite(stats[2]) and np.isfinite(stats[3])
    # nothing but NaN: min and max are +inf and -inf
    counts, stats = _one(ctx, x[:3], np.full((3, 2), np.nan), edges)
    assert counts.sum() == 0 and stats[0] == 3 and stats[2] == np.inf and stats[3] == -np.inf


def test_errors(fresh_ctx):
    c = fresh_ctx
    x, k = _packets(37)
    good = np.linspace(0.0, 15.0, 11)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):
        c.omega_series_record()
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):
        c.omega_series_record_history(0, 0)
    assert c.omega_series_frames() == 0 and c._L.swrt_omega_series_bins(c._h) == 0
    for bad in (np.linspace(0.0, 15.0, 4098), [0.0, 1.0, 1.0, 2.0], [0.0, 2.0, 1.0], [3.0], [0.0, np.nan, 2.0],
                [0.0, 1.0, np.inf]):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
            c.omega_series_begin(F, CG, bad)
    assert c._L.swrt_omega_series_begin(c._h, F, CG, None, 4) == 1 and b"NULL" in c._L.swrt_last_error(c._h)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):  # a refused begin opens nothing
        c.omega_series_record()
    c.omega_series_begin(F, CG, np.linspace(0.0, 15.0, 4097))  # 4096 bins: allowed
    assert c._L.swrt_omega_series_bins(c._h) == 4096
    c.omega_series_begin(F, CG, good)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*no packets"):
        c.omega_series_record()
    c.packets_set(x, k)
    c.omega_series_record()
    for first, count in ((-1, 1), (0, 2), (1, 1), (0, -1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
            c.omega_series(first, count)
    assert c._L.swrt_omega_series_get(c._h, 0, 1, None, None) == 1 and b"NULL" in c._L.swrt_last_error(c._h)
    # the stats may be NULL
    row = np.zeros(12, dtype=np.int64)
    import ctypes
    assert c._L.swrt_omega_series_get(c._h, 0, 1, row.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None) == 0
    np.testing.assert_array_equal(row, _row(_omega(k), good))
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*history"):
        c.omega_series_record_history(0, 1)  # no history frames


def _qg_planes(qg_case):
    return cbind.planes_of(qg_case["flow"])


def test_frame_depends_on_the_packets_alone(fresh_ctx, qg_case):
    """A re-binning between two records, and another context holding the same
    packets in another storage order: the same bits, sum omega included."""
    q = qg_case
    a, b = fresh_ctx, sw.Context(0)
    try:
        rng = np.random.default_rng(11)
        x0, k0 = orc.initial_packets(5000, q["L"], 4.0, q["f"], q["Cg"], rng)
        k0 = k0 * (1.0 + 0.3 * rng.standard_normal((5000, 1)))  # a spread of omega: the sum's order matters
        edges = np.linspace(0.0, 30.0, 301)
        for c in (a, b):
            c.set_field_grid(0, _qg_planes(q), q["nx"], q["L"])
            c.set_locality(4, 0)
        a.packets_set(x0, k0)
        a.omega_series_begin(q["f"], q["Cg"], edges)
        a.omega_series_record()
        a.advance(q["dt"], 40, q["f"], q["Cg"] ** 2, bump=orc.BUMP_QG)  # re-binned every 4 steps
        a.omega_series_record()
        x, k = a.packets_get()
        assert np.abs(x - x0).max() > 2 * q["L"] / q["nx"]  # the packets moved across cells
        ca, sa = a.omega_series()
        _check(ca[0], sa[0], k0, edges, q["f"], q["Cg"], "first")
        _check(ca[1], sa[1], k, edges, q["f"], q["Cg"], "after 40 steps")
        assert not np.array_equal(ca[0], ca[1])
        # the same packets in their original order, never binned
        b.packets_set(x, k)
        b.omega_series_begin(q["f"], q["Cg"], edges)
        b.omega_series_record()
        cb, sb = b.omega_series()
        assert cb[0].tobytes() == ca[1].tobytes() and sb[0].tobytes() == sa[1].tobytes()
        # and in a shuffled order the counts, min and max stay (the sum may not)
        p = rng.permutation(5000)
        b.packets_set(x[p], k[p])
        b.omega_series_record()
        cb, sb = b.omega_series()
        np.testing.assert_array_equal(cb[1], ca[1])
        np.testing.assert_array_equal(sb[1, [0, 2, 3]], sa[1, [0, 2, 3]])
    finally:
        b.close()


def test_series_grows_and_resets(fresh_ctx):
    c = fresh_ctx
    edges = np.linspace(3.0, 7.0, 5)
    xa, ka = _packets(37, seed=8)
    xb, kb = _packets(41, seed=9)  # another N keeps the series: a frame is self-contained
    c.packets_set(xa, ka)
    c.omega_series_begin(F, CG, edges)
    for i in range(4100):
        if i == 4091:
            c.packets_set(xb, kb)
        c.omega_series_record()
    assert c.omega_series_frames() == 4100
    counts, stats = c.omega_series()
    assert counts.shape == (4100, 6)
    for i, k in ((0, ka), (4090, ka), (4091, kb), (4095, kb), (4096, kb), (4099, kb)):
        _check(counts[i], stats[i], k, edges, what=f"frame {i}")
    assert (counts[:4091] == counts[0]).all() and (counts[4091:] == counts[4099]).all()
    assert (stats[:4091] == stats[0]).all() and (stats[4091:] == stats[4099]).all()
    c2, s2 = c.omega_series(4095, 3)
    np.testing.assert_array_equal(c2, counts[4095:4098])
    np.testing.assert_array_equal(s2, stats[4095:4098])
    c.omega_series_reset()
    assert c.omega_series_frames() == 0 and c.omega_series()[0].shape == (0, 6)
    c.packets_set(xa, ka)
    c.omega_series_record()  # f, Cg and the edges stay
    counts, stats = c.omega_series()
    assert counts.shape == (1, 6)
    _check(counts[0], stats[0], ka, edges, what="frame 0 after the reset")


def _check_history(c, f, Cg, edges, sub):
    frames = c._L.swrt_history_frames(c._h)
    hx, hk = c.history()
    c.omega_series_begin(f, Cg, edges)
    c.omega_series_record_history(0, frames)
    assert c.omega_series_frames() == frames
    counts, stats = c.omega_series()
    for i in range(frames):
        _check(counts[i], stats[i], np.ascontiguousarray(hk[i].T), edges, f, Cg, f"history frame {i}")
    assert len({r.tobytes() for r in counts}) > 1  # the frames differ
    first, count = sub
    c.omega_series_record_history(first, count)  # a subrange, appended behind them
    assert c.omega_series_frames() == frames + count
    c2, s2 = c.omega_series(frames, count)
    assert c2.tobytes() == counts[first:first + count].tobytes()
    assert s2.tobytes() == stats[first:first + count].tobytes()
    for bad_first, bad_count in ((0, frames + 1), (-1, 2), (frames, 1), (2, -1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*history"):
            c.omega_series_record_history(bad_first, bad_count)
    assert c.omega_series_frames() == frames + count
    # the bits of a record on packets set to that frame
    c.packets_set(np.ascontiguousarray(hx[frames - 2].T), np.ascontiguousarray(hk[frames - 2].T))
    c.omega_series_reset()
    c.omega_series_record()
    c1, s1 = c.omega_series()
    assert c1[0].tobytes() == counts[frames - 2].tobytes() and s1[0].tobytes() == stats[frames - 2].tobytes()
    return frames


def _history_case(c, q, n=1000):
    rng = np.random.default_rng(12)
    x0, k0 = orc.initial_packets(n, q["L"], 4.0, q["f"], q["Cg"], rng)
    k0 = k0 * (1.0 + 0.3 * rng.standard_normal((n, 1)))
    c.set_field_grid(0, _qg_planes(q), q["nx"], q["L"])
    c.set_locality(4, 0)
    c.packets_set(x0, k0)
    c.history_reset()


def test_record_history_after_advance(fresh_ctx, qg_case):
    q = qg_case
    _history_case(fresh_ctx, q)
    fresh_ctx.advance(q["dt"], 12, q["f"], q["Cg"] ** 2, bump=orc.BUMP_QG, save_every=1)
    assert _check_history(fresh_ctx, q["f"], q["Cg"], np.linspace(0.0, 30.0, 301), (3, 4)) == 12


def test_record_history_after_ode23_run_at(fresh_ctx, qg_case):
    q = qg_case
    _history_case(fresh_ctx, q)
    fresh_ctx.ode23_run_at(np.linspace(0.0, 40 * q["dt"], 7), 0.0, q["f"], q["Cg"], 1, 1e-3, 1e-6, orc.BUMP_QG)
    assert _check_history(fresh_ctx, q["f"], q["Cg"], np.linspace(0.0, 30.0, 301), (1, 4)) == 6


@pytest.mark.parametrize("ny_period", [0, 32])
def test_omega_ideal(fresh_ctx, ny_period):
    """ideal_omega_distribution.m:3-11 on a 16^2 grid; with a 2*nx y-period the
    slot still holds layer 1 alone (nx x nx nodes), and only those are counted."""
    c = fresh_ctx
    nx, m, k_0 = 16, 7, 3.0
    rng = np.random.default_rng(13)
    planes = 0.2 * rng.standard_normal((6, nx * nx))
    planes[0, 77] = planes[1, 77] = 0.0  # one node at rest: Omega == omega0 exactly
    c.set_field_grid(0, planes, nx, 2 * np.pi, ny_period)
    t = np.linspace(0, 2 * np.pi, m)                      # :3
    ring = k_0 * np.stack([np.cos(t), np.sin(t)], axis=1)  # :5
    omega0 = math.sqrt(F ** 2 + CG ** 2 * k_0 ** 2)       # :9
    edges = omega0 + np.array([-0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3])
    assert edges[3] == omega0
    u, v = planes[0], planes[1]
    Om = omega0 + (u[:, None] * ring[None, :, 0] + v[:, None] * ring[None, :, 1])  # :6,10
    want = _row(Om.ravel(), edges)
    assert want.sum() == nx * nx * m and want[0] > 0 and want[-1] > 0 and (Om == omega0).sum() >= m
    got = c.omega_ideal(0, ring, omega0, edges)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, want)
    # 300 bins over every sample; one ring vector
    edges = np.linspace(Om.min(), Om.max(), 301)
    np.testing.assert_array_equal(c.omega_ideal(0, ring, omega0, edges), _row(Om.ravel(), edges))
    np.testing.assert_array_equal(c.omega_ideal(0, ring[2:3], omega0, edges), _row(Om[:, 2], edges))
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*slot"):
        c.omega_ideal(1, ring, omega0, edges)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
        c.omega_ideal(0, ring[:0], omega0, edges)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*increase"):
        c.omega_ideal(0, ring, omega0, edges[::-1])


# ---- the drivers ------------------------------------------------------------

EDGES = np.linspace(0, 15, 301)
QG1 = (64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0)
QG1_KW = dict(nsub=2, max_steps=24, r_drag=0.0)
SPEC_FILES = ("omega_hist.bin", "omega_stats.bin", "omega_edges.bin")
PACKET_FILES = ("packet_x.bin", "packet_k.bin", "packet_time.bin")


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


@pytest.fixture(scope="module")
def qg1_run(ctx, tmp_path_factory):
    """The 1-layer driver with spectrum_edges, run once: (facts, files)."""
    d = str(tmp_path_factory.mktemp("qg1_spectrum"))
    facts = sw.qgsw_raytrace(*QG1, out_dir=d, ctx=ctx, spectrum_edges=EDGES, **QG1_KW)
    return facts, _files(d), d


def _check_driver_files(d, facts, n, f, Cg, spread=True):
    frames = facts["packet_frames"]
    assert facts["spectrum_frames"] == frames > 1
    nb = EDGES.size - 1
    kf = sw.read_field(os.path.join(d, "packet_k"), n, 2, 1).reshape(n, 2, frames)
    hist = sw.read_field(os.path.join(d, "omega_hist"), nb + 2, 1, 1).reshape(nb + 2, frames)
    stats = sw.read_field(os.path.join(d, "omega_stats"), 4, 1, 1).reshape(4, frames)
    np.testing.assert_array_equal(sw.read_field(os.path.join(d, "omega_edges"), nb + 1, 1, 1).ravel(), EDGES)
    assert sw.read_field(os.path.join(d, "packet_time")).shape == (1, frames)
    # the expected side first: the run is long enough for the ring to have spread
    last = _row(_omega(kf[:, :, -1], f, Cg), EDGES)
    print("non-zero bins of the last frame:", np.count_nonzero(last[1:-1]))
    if spread:
        assert np.count_nonzero(last[1:-1]) >= 3
    for i in range(frames):
        _check(hist[:, i].astype(np.int64), stats[:, i], kf[:, :, i], EDGES, f, Cg, f"driver frame {i}")
        assert hist[:, i].sum() == n
    return hist, stats


def test_driver_spectrum_equals_numpy_on_its_packet_frames(qg1_run):
    facts, files, d = qg1_run
    assert set(SPEC_FILES) <= set(files)
    _check_driver_files(d, facts, 4001, 3.0, 1.0)


def test_driver_packet_files_unchanged_by_the_spectrum(ctx, qg1_run, tmp_path):
    facts, files, _ = qg1_run
    plain = sw.qgsw_raytrace(*QG1, out_dir=str(tmp_path), ctx=ctx, **QG1_KW)
    got = _files(str(tmp_path))
    assert plain["spectrum_frames"] == 0 and not set(SPEC_FILES) & set(got)
    assert {k: v for k, v in plain.items() if k != "spectrum_frames"} == \
        {k: v for k, v in facts.items() if k != "spectrum_frames"}
    for name in PACKET_FILES + ("pv.bin", "pv_time.bin"):
        assert len(got[name]) > 0 and got[name] == files[name], name


def test_driver_without_packet_files(ctx, qg1_run, tmp_path):
    facts, files, _ = qg1_run
    out = sw.qgsw_raytrace(*QG1, out_dir=str(tmp_path), ctx=ctx, spectrum_edges=EDGES, packet_files=False, **QG1_KW)
    got = _files(str(tmp_path))
    assert "packet_x.bin" not in got and "packet_k.bin" not in got
    assert out["spectrum_frames"] == facts["spectrum_frames"] == out["packet_frames"]
    for name in SPEC_FILES + ("packet_time.bin",):
        assert got[name] == files[name], name


def test_driver_packet_intervals_4_same_spectrum(ctx, qg1_run, tmp_path):
    facts, files, _ = qg1_run
    sw.qgsw_raytrace(*QG1, out_dir=str(tmp_path), ctx=ctx, spectrum_edges=EDGES, packet_intervals=4, **QG1_KW)
    got = _files(str(tmp_path))
    for name in SPEC_FILES + PACKET_FILES:
        assert got[name] == files[name], name


def test_driver_fresh_removes_earlier_spectrum_files(ctx, qg1_run, tmp_path):
    facts, files, _ = qg1_run
    for name in SPEC_FILES:
        (tmp_path / name).write_bytes(b"\0" * 8)
    sw.qgsw_raytrace(*QG1, out_dir=str(tmp_path), ctx=ctx, spectrum_edges=EDGES, packet_files=False, **QG1_KW)
    got = _files(str(tmp_path))
    for name in SPEC_FILES:
        assert got[name] == files[name], name


def test_two_layer_driver_spectrum(ctx, tmp_path):
    facts = sw.qg2layersw_raytrace(64, 5001, 4.0, 10.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path), nsub=2,
                                   max_steps=30, seed=5, ctx=ctx, spectrum_edges=EDGES)
    _check_driver_files(str(tmp_path), facts, 5001, 3.0, 1.0, spread=False)  # (two frames, 25 steps apart)


def test_packet_files_false_needs_spectrum_edges(ctx, tmp_path):
    with pytest.raises(ValueError, match="spectrum_edges"):
        sw.qgsw_raytrace(*QG1, out_dir=str(tmp_path / "a"), ctx=ctx, packet_files=False, **QG1_KW)
    with pytest.raises(ValueError, match="spectrum_edges"):
        sw.qg2layersw_raytrace(64, 5001, 4.0, 10.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path / "b"), ctx=ctx,
                               packet_files=False, max_steps=30)
    assert not (tmp_path / "a").exists() and not (tmp_path / "b").exists()  # refused before anything ran


def test_trace_stored_spectrum(ctx, qg_case, tmp_path):
    """trace_stored through three stored PV frames: the spectrum files equal
    numpy on its packet_k.bin frames, the packet files and the returned state
    are the bits of a run without spectrum_edges, and packet_files=False
    writes the same spectrum files."""
    q = qg_case
    nx, f, Cg = q["nx"], q["f"], q["Cg"]
    pv = tmp_path / "pv"
    X = np.arange(nx) * (q["L"] / nx)
    for s in range(3):
        sw.write_field(q["q"] * (1.0 + 0.2 * s) + 0.05 * s * np.cos(X[:, None] + 2 * X[None, :]), str(pv))
    times = [0.0, 0.6, 1.3]
    rng = np.random.default_rng(14)
    x0, k0 = orc.initial_packets(3001, q["L"], 4.0, f, Cg, rng)
    kw = dict(times=times, nsub=8, intervals_per_call=1, ctx=ctx)
    a, b, c = (str(tmp_path / n) for n in "abc")
    xs, ks, t_end = sw.trace_stored(str(pv), nx, x0, k0, f, Cg, out_dir=a, spectrum_edges=EDGES, **kw)
    xp, kp, _ = sw.trace_stored(str(pv), nx, x0, k0, f, Cg, out_dir=b, **kw)
    xn, kn, _ = sw.trace_stored(str(pv), nx, x0, k0, f, Cg, out_dir=c, spectrum_edges=EDGES, packet_files=False, **kw)
    assert t_end == times[-1]
    for got in ((xp, kp), (xn, kn)):
        assert got[0].tobytes() == xs.tobytes() and got[1].tobytes() == ks.tobytes()
    fa, fb, fc = _files(a), _files(b), _files(c)
    assert set(fb) == set(PACKET_FILES) and set(fa) == set(PACKET_FILES + SPEC_FILES)
    assert set(fc) == set(SPEC_FILES + ("packet_time.bin",))
    for name in PACKET_FILES:
        assert fa[name] == fb[name], name
    for name in SPEC_FILES + ("packet_time.bin",):
        assert fa[name] == fc[name], name
    _check_driver_files(a, dict(packet_frames=3, spectrum_frames=3), 3001, f, Cg, spread=False)
    with pytest.raises(ValueError, match="out_dir"):
        sw.trace_stored(str(pv), nx, x0, k0, f, Cg, spectrum_edges=EDGES, **kw)
    with pytest.raises(ValueError, match="spectrum_edges"):
        sw.trace_stored(str(pv), nx, x0, k0, f, Cg, out_dir=c, packet_files=False, **kw)
