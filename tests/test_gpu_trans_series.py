"""The transition series on the device (swrt_trans_series_*;
swraytracing_amd/csrc/swrt_trans.hpp) and the drivers' trans_*.bin files.

Expected values are tests/trans_series_ref.py, the numpy restatement of the
contract in include/swrt.h.  Every comparison is exact integer equality:
integer sums are order-free, so there is no tolerance.

The packets are 1000 on the qg_case ring with |k| scaled by 1 + 0.3 N(0, 1),
their source values omega * (1 + 0.3 N(0, 1)); a case with N packets takes the
first N.  Both edge sets are linspace between the 10th and 90th percentile of
the restatement's values, so a tenth of the packets fills below and above on
either axis by construction.  Where a test says so it asserts on the
restatement's frame (never the device's) that below, above and half of the
interior classes of both axes are populated."""
import ctypes
import os

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import cbind, swrt_oracle as orc
from swraytracing_amd._lib import DEBUG_TRANS_GLOBAL
from tests.cond_series_ref import assert_populated, class_of, quantile_edges
from tests.trans_series_ref import omega_of, ring_k, ring_of, trans_frame_of

pytestmark = pytest.mark.gpu

FB = 20
BUMP = orc.BUMP_QG
SHAPES = [(1, 1), (3, 5), (4, 300), (64, 64)]  # (ns, nw)
PLANTED = 5


@pytest.fixture(scope="module")
def state(qg_case):
    """1000 spread packets and their source values (computed once, read-only)."""
    q = qg_case
    rng = np.random.default_rng(41)
    x, k = orc.initial_packets(1000, q["L"], 4.0, q["f"], q["Cg"], rng)
    k = k * (1.0 + 0.3 * rng.standard_normal((1000, 1)))
    w = omega_of(k, q["f"], q["Cg"])
    src = w * (1.0 + 0.3 * rng.standard_normal(1000))
    for a in (x, k, w, src):
        a.setflags(write=False)
    return dict(q=q, x=x, k=k, w=w, src=src)


def _edges(st, ns, nw):
    return quantile_edges(st["w"], nw), quantile_edges(st["src"], ns)


def _begin(c, st, wedges, sedges, fb=FB):
    c.trans_series_begin(st["q"]["f"], st["q"]["Cg"], wedges, sedges, fb)


def _equal(got, want, what=""):
    for g, w, name in zip(got, want, ("counts", "sums", "stats")):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _planted(st, n):
    """The first n packets and source values with, where n allows, a NaN k, an
    over-range k, a NaN source, a source that puts d out of range and one that
    puts only d^2 out of range (|d| about 988: d * 2^20 < 2^38 <= d^2 * 2^20)."""
    x, k, src = st["x"][:n].copy(), st["k"][:n].copy(), st["src"][:n].copy()
    if n > 3:
        k[3, 1] = np.nan
    if n > 5:
        k[5] = [1e9, 0.0]
    if n > 7:
        src[7] = np.nan
    if n > 9:
        src[9] = 1e300
    if n > 11:
        src[11] = 1000.0
    return x, k, src


def _rejects(n):
    return sum(n > i for i in (3, 5, 7, 9, 11))


@pytest.mark.parametrize("ns,nw", SHAPES)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_device_against_the_restatement(ctx, state, n, ns, nw):
    """One packet, a workgroup's edge on both sides, and (1000) a grid stride
    with a partial last wave, through mark_values."""
    c, st, q = ctx, state, state["q"]
    x, k, src = _planted(st, n)
    c.packets_set(x, k)
    wedges, sedges = _edges(st, ns, nw)
    want = trans_frame_of(src, omega_of(k, q["f"], q["Cg"]), wedges, sedges, FB)
    print(f"n {n} ({ns}, {nw}): source row {want[0].sum(axis=1).tolist()} stats {want[2].tolist()}")
    assert want[2][0] == n and want[0].sum() == n - want[2][1] and want[2][1] == _rejects(n)
    if n == 1000:
        assert_populated(want[0], want[2], planted=True)
    _begin(c, st, wedges, sedges)
    c.trans_series_mark_values(src)
    c.trans_series_record()
    counts, sums, stats = c.trans_series_get()
    assert counts.shape == (1, ns + 2, nw + 2) and sums.shape == (1, ns + 2, 3) and stats.shape == (1, 3)
    _equal((counts[0], sums[0], stats[0]), want, f"n {n} ({ns}, {nw})")


@pytest.fixture()
def tctx(ctx):
    """The session context with the path key back at 0 afterwards."""
    yield ctx
    ctx.debug_set(DEBUG_TRANS_GLOBAL, 0)


def test_path_boundary(tctx, state):
    """16384 cells (the last LDS shape) and 16385 (the first global one), and
    1022 and 1023 source classes (the last shape with the sums in LDS, the
    first without, on either kernel) agree with the restatement; the forced
    global kernel gives the LDS kernel's integers on (4, 300), frac_bits 0
    and 32 included."""
    c, st, q = tctx, state, state["q"]
    x, k, src = _planted(st, 1000)
    c.packets_set(x, k)
    w = omega_of(k, q["f"], q["Cg"])
    for ns, nw in ((126, 126), (3, 3275), (1022, 5), (1023, 5), (1023, 60)):
        wedges, sedges = _edges(st, ns, nw)
        want = trans_frame_of(src, w, wedges, sedges, FB)
        if max(ns, nw) < 200:
            assert_populated(want[0], want[2], planted=True)
        else:  # (1000 packets cannot fill half of a thousand classes: both ends of both axes, and a spread)
            wrow, srow = want[0].sum(axis=0), want[0].sum(axis=1)
            assert wrow[0] > 0 and wrow[-1] > 0 and srow[0] > 0 and srow[-1] > 0 and want[2][1] > 0
            assert np.count_nonzero(wrow if nw > ns else srow) > 400
        _begin(c, st, wedges, sedges)
        c.trans_series_mark_values(src)
        c.trans_series_record()
        _equal([a[0] for a in c.trans_series_get()], want, f"({ns}, {nw})")
    assert 128 * 128 == 16384 and 5 * 3277 == 16385
    for fb in (0, FB, 32):
        wedges, sedges = _edges(st, 4, 300)
        want = trans_frame_of(src, w, wedges, sedges, fb)
        assert_populated(want[0], want[2], planted=True)
        _begin(c, st, wedges, sedges, fb)
        c.trans_series_mark_values(src)
        for forced in (0, 1):
            c.debug_set(DEBUG_TRANS_GLOBAL, forced)
            assert c.debug_get(DEBUG_TRANS_GLOBAL) == forced
            c.trans_series_record()
        c.debug_set(DEBUG_TRANS_GLOBAL, 0)
        got = c.trans_series_get()
        for i in (0, 1):
            _equal([a[i] for a in got], want, f"frac_bits {fb} forced {i}")
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
        c.debug_set(DEBUG_TRANS_GLOBAL, 2)


def test_one_shared_cell_and_source_class(tctx, state):
    """Every packet with one k and one source value: one cell holds all 1000
    and one row of sums takes every add (the wave merge of the per-class
    sums), on both paths; d is negative, so its sum is in two's complement."""
    c, st, q = tctx, state, state["q"]
    n = 1000
    x, k = np.tile(st["x"][:1], (n, 1)), np.tile(st["k"][:1], (n, 1))
    src = np.full(n, st["w"][0] + 0.37)
    c.packets_set(x, k)
    wedges, sedges = _edges(st, 4, 300)
    want = trans_frame_of(src, omega_of(k, q["f"], q["Cg"]), wedges, sedges, FB)
    assert np.count_nonzero(want[0]) == 1 and want[0].max() == n
    assert np.count_nonzero(want[1].any(axis=1)) == 1 and want[1].min() == n * int(np.rint(-0.37 * 2.0 ** FB)) < 0
    _begin(c, st, wedges, sedges)
    c.trans_series_mark_values(src)
    for forced in (0, 1):
        c.debug_set(DEBUG_TRANS_GLOBAL, forced)
        c.trans_series_record()
    got = c.trans_series_get()
    for i in (0, 1):
        _equal([a[i] for a in got], want, f"forced {i}")


def _fields(c, q, P=None):
    P = np.asarray(cbind.planes_of(q["flow"])) if P is None else P
    c.set_field_grid(0, P, q["nx"], q["L"])
    c.set_field_grid(1, 0.8 * P, q["nx"], q["L"])


def test_the_mark_survives_rebinning(state):
    """4096 spread packets marked, advanced 6 leapfrog steps in the
    two-snapshot blend while re-binned every 2 steps, recorded: the frame is
    the restatement's of (omega at the mark, omega now), both from
    swrt_packets_get in the original order.  With binning off, and with the
    per-packet kernel, the frames are byte-equal.  Condition on the inputs,
    checked with the CPU oracle's leapfrog: at least 5 % of the packets leave
    the diagonal of the 64 quantile classes."""
    st, q = state, state["q"]
    n, steps = 4096, 6
    rng = np.random.default_rng(42)
    x0, k0 = orc.initial_packets(n, q["L"], 4.0, q["f"], q["Cg"], rng)
    k0 = k0 * (1.0 + 0.3 * rng.standard_normal((n, 1)))
    w0 = omega_of(k0, q["f"], q["Cg"])
    edges = quantile_edges(w0, 64)
    phys = dict(alpha0=0.05, dalpha=0.1, bump=BUMP)
    flow1 = {name: 0.8 * np.asarray(v) for name, v in q["flow"].items()}
    dx = q["L"] / q["nx"]
    _, ko, _, _ = orc.leapfrog(x0, k0, q["dt"], steps, q["f"], q["Cg"] ** 2, orc.GridField(q["flow"], dx),
                               orc.GridField(flow1, dx), **phys)
    moved = np.mean(class_of(omega_of(ko, q["f"], q["Cg"]), edges) != class_of(w0, edges))
    print(f"the oracle: {100 * moved:.1f} % of the packets leave the diagonal")
    assert moved >= 0.05
    frames = {}
    for name, rebin, kernel in (("re-binned", 2, None), ("binning off", 0, None), ("per-packet kernel", 2, 1)):
        c = sw.Context(0)
        try:
            _fields(c, q)
            c.set_locality(rebin, 0)
            if kernel is not None:
                c.set_kernel(kernel)
            c.packets_set(x0, k0)
            _begin(c, st, edges, edges)
            c.trans_series_mark()
            _, kb = c.packets_get()
            c.advance(q["dt"], steps, q["f"], q["Cg"] ** 2, nslots=2, **phys)
            _, ka = c.packets_get()
            c.trans_series_record()
            got = c.trans_series_get()
        finally:
            c.close()
        np.testing.assert_array_equal(kb, k0)
        want = trans_frame_of(omega_of(kb, q["f"], q["Cg"]), omega_of(ka, q["f"], q["Cg"]), edges, edges, FB)
        off = want[0].sum() - np.trace(want[0])
        print(f"{name}: {off} of {n} off the diagonal, stats {want[2].tolist()}")
        assert want[2].tolist() == [n, 0, 1] and off >= 0.05 * n
        assert_populated(want[0])
        _equal([a[0] for a in got], want, name)
        frames[name] = got
    for name in ("binning off", "per-packet kernel"):
        assert [a.tobytes() for a in frames[name]] == [a.tobytes() for a in frames["re-binned"]], name


def test_advance_calls_and_packet_streams_do_not_change_a_frame(state):
    """swrt_advance_intervals against two swrt_advance calls, and one packet
    stream against two (65,536 packets: the tile launches split), give equal
    frames against a mark taken before the advance."""
    st, q = state, state["q"]
    P = np.asarray(cbind.planes_of(q["flow"]))
    rng = np.random.default_rng(43)
    xb, kb = orc.initial_packets(65536, q["L"], 4.0, q["f"], q["Cg"], rng)
    kb = kb * (1.0 + 0.3 * rng.standard_normal((65536, 1)))
    edges = quantile_edges(omega_of(kb, q["f"], q["Cg"]), 64)
    h, phys = q["dt"], dict(alpha0=0.1, dalpha=0.2, bump=BUMP)
    frames = []
    for form, streams in (("intervals", 2), ("calls", 2), ("calls", 1)):
        c = sw.Context(0)
        try:
            c.set_packet_streams(streams)
            c.packets_set(xb, kb)
            _begin(c, st, edges, edges)
            c.trans_series_mark()
            for s, scale in enumerate((1.0, 0.8, 0.9)):
                c.set_field_grid(s, scale * P, q["nx"], q["L"])
            if form == "intervals":
                c.advance_intervals([h, 1.1 * h], 5, q["f"], q["Cg"] ** 2, **phys)
            else:
                c.advance(h, 5, q["f"], q["Cg"] ** 2, nslots=2, **phys)
                c.set_field_grid(0, 0.8 * P, q["nx"], q["L"])
                c.set_field_grid(1, 0.9 * P, q["nx"], q["L"])
                c.advance(1.1 * h, 5, q["f"], q["Cg"] ** 2, nslots=2, **phys)
            c.trans_series_record()
            frames.append(c.trans_series_get())
        finally:
            c.close()
    counts, _, stats = frames[0]
    assert stats[0].tolist() == [65536, 0, 1] and counts.sum() == 65536
    assert counts[0].sum() - np.trace(counts[0]) > 0.05 * 65536  # (the packets moved between classes)
    _equal(frames[1], frames[0], "two advance calls against advance_intervals")
    _equal(frames[2], frames[0], "one packet stream against two")


def test_mark_then_record_is_diagonal(ctx, state):
    c, st = ctx, state
    c.packets_set(st["x"], st["k"])
    edges = quantile_edges(st["w"], 64)
    _begin(c, st, edges, edges)
    c.trans_series_mark()
    c.trans_series_record()
    counts, sums, stats = (a[0] for a in c.trans_series_get())
    want = trans_frame_of(st["w"], st["w"], edges, edges, FB)
    assert_populated(want[0])
    _equal((counts, sums, stats), want, "mark, record")
    assert np.array_equal(counts, np.diag(np.diag(counts))) and counts.sum() == 1000
    assert not sums[:, 1:].any() and (sums[:, 0] > 0).all() and stats.tolist() == [1000, 0, 1]


@pytest.mark.parametrize("count", [1, 3])
def test_record_history(fresh_ctx, state, count):
    """One frame per history frame, joined to the current mark: the bits of a
    record on packets set to that frame and marked alike.  The packets are
    re-binned before the frames are saved, so the storage order is not the
    original one."""
    c, st, q = fresh_ctx, state, state["q"]
    _fields(c, q)
    c.set_locality(2, 0)
    c.packets_set(st["x"], st["k"])
    c.history_reset()
    c.advance(q["dt"], 4 * count, q["f"], q["Cg"] ** 2, nslots=2, alpha0=0.05, dalpha=0.1, bump=BUMP, save_every=4)
    hx, hk = c.history()
    assert hx.shape[0] == count
    wedges, sedges = _edges(st, 4, 300)
    _begin(c, st, wedges, sedges)
    c.trans_series_mark_values(st["src"])
    c.trans_series_record_history(0, count)
    assert c.trans_series_frames() == count
    hist = c.trans_series_get()
    for i in range(count):
        x, k = np.ascontiguousarray(hx[i].T), np.ascontiguousarray(hk[i].T)
        want = trans_frame_of(st["src"], omega_of(k, q["f"], q["Cg"]), wedges, sedges, FB)
        assert_populated(want[0])
        _equal([a[i] for a in hist], want, f"history frame {i}")
        c.packets_set(x, k)
        c.trans_series_reset()
        c.trans_series_mark_values(st["src"])
        c.trans_series_record()
        rec = c.trans_series_get()
        _equal([rec[0][0], rec[1][0], rec[2][0][:2]], [hist[0][i], hist[1][i], hist[2][i][:2]], f"record on frame {i}")
        assert rec[2][0][2] == 2 + i  # (every mark counts)
    if count > 1:
        assert len({a.tobytes() for a in hist[0]}) == count  # the frames differ
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*history"):  # (packets_set began a new history)
            c.trans_series_record_history(0, 1)


def test_series_life(fresh_ctx, state):
    """4097 frames of a tiny shape grow the series past its first 4096;
    partial gets; reset keeps the mark and the edges; begin drops the mark."""
    c, st = fresh_ctx, state
    wedges, sedges = _edges(st, 1, 1)
    c.packets_set(st["x"][:1], st["k"][:1])
    _begin(c, st, wedges, sedges)
    c.trans_series_mark_values(st["src"][:1])
    for _ in range(4097):
        c.trans_series_record()
    assert c.trans_series_frames() == 4097 and c.trans_series_bins() == (1, 1)
    counts, sums, stats = c.trans_series_get()
    want = trans_frame_of(st["src"][:1], st["w"][:1], wedges, sedges, FB)
    for i in (0, 4095, 4096):
        _equal((counts[i], sums[i], stats[i]), want, f"frame {i}")
    assert (counts == counts[0]).all() and (sums == sums[0]).all() and (stats == stats[0]).all()
    part = c.trans_series_get(4090, 7)
    assert part[0].shape == (7, 3, 3) and np.array_equal(part[0], counts[4090:])
    i64 = ctypes.POINTER(ctypes.c_int64)
    only = [np.zeros_like(a[:2]) for a in (counts, sums, stats)]
    for j in range(3):
        args = [only[i].ctypes.data_as(i64) if i == j else None for i in range(3)]
        assert c._L.swrt_trans_series_get(c._h, 4095, 2, *args) == 0
    _equal(only, [a[4095:] for a in (counts, sums, stats)], "single outputs")
    c.trans_series_reset()
    assert c.trans_series_frames() == 0 and c.trans_series_bins() == (1, 1)
    assert c.trans_series_get()[0].shape == (0, 3, 3)
    c.trans_series_record()  # the mark and the edges stay
    _equal([a[0] for a in c.trans_series_get()], want, "after the reset")
    c.trans_series_mark()  # a second mark: the serial steps, the source is omega now
    c.trans_series_record()
    got = [a[1] for a in c.trans_series_get()]
    _equal(got, trans_frame_of(st["w"][:1], st["w"][:1], wedges, sedges, FB, serial=2), "after the second mark")
    _begin(c, st, *_edges(st, 3, 5))  # begin again: empty, the new shape, no mark, the serial from 0
    assert c.trans_series_frames() == 0 and c.trans_series_bins() == (5, 3)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*mark"):
        c.trans_series_record()
    c.trans_series_mark()
    c.trans_series_record()
    assert c.trans_series_get()[2][0].tolist() == [1, 0, 1]


def test_errors(fresh_ctx, state):
    """Every refusal returns before any launch."""
    c, st = fresh_ctx, state
    wedges, sedges = _edges(st, 3, 5)

    def refused(code, call):
        with pytest.raises(sw.SwrtError, match=code) as e:
            call()
        assert c._L.swrt_last_error(c._h), e.value  # a message, not only a code
        return str(e.value)

    for call in (c.trans_series_record, c.trans_series_mark, lambda: c.trans_series_mark_values(st["src"]),
                 lambda: c.trans_series_record_history(0, 0)):
        refused("SWRT_ERR_STATE.*begin", call)
    assert c.trans_series_frames() == 0 and c.trans_series_bins() == (0, 0)
    big = np.arange(301.0)
    refused("SWRT_ERR_ARG.*65536", lambda: c.trans_series_begin(3.0, 1.0, big + 3, big, FB))  # 302 x 302 cells
    refused("SWRT_ERR_ARG", lambda: c.trans_series_begin(3.0, 1.0, wedges, sedges[:1], FB))  # ns = 0
    refused("SWRT_ERR_ARG", lambda: c.trans_series_begin(3.0, 1.0, wedges[:1], sedges, FB))
    refused("SWRT_ERR_ARG.*4096", lambda: c.trans_series_begin(3.0, 1.0, np.arange(4098.0), sedges, FB))
    refused("SWRT_ERR_ARG.*4096", lambda: c.trans_series_begin(3.0, 1.0, wedges, np.arange(4098.0), FB))
    refused("SWRT_ERR_ARG.*increase", lambda: c.trans_series_begin(3.0, 1.0, wedges, sedges[::-1], FB))
    refused("SWRT_ERR_ARG.*increase", lambda: c.trans_series_begin(3.0, 1.0, wedges[::-1], sedges, FB))
    bad = sedges.copy()
    bad[2] = np.nan
    refused("SWRT_ERR_ARG.*finite", lambda: c.trans_series_begin(3.0, 1.0, wedges, bad, FB))
    refused("SWRT_ERR_ARG.*frac_bits", lambda: c.trans_series_begin(3.0, 1.0, wedges, sedges, 33))
    refused("SWRT_ERR_ARG.*frac_bits", lambda: c.trans_series_begin(3.0, 1.0, wedges, sedges, -1))
    refused("SWRT_ERR_STATE.*begin", c.trans_series_record)  # a refused begin opens nothing
    _begin(c, st, wedges, sedges)
    refused("SWRT_ERR_ARG.*no packets", c.trans_series_mark)
    refused("SWRT_ERR_ARG.*no packets", c.trans_series_record)
    c.packets_set(st["x"][:300], st["k"][:300])
    refused("SWRT_ERR_STATE.*mark", c.trans_series_record)  # no mark yet
    refused("SWRT_ERR_STATE.*mark", lambda: c.trans_series_record_history(0, 0))
    refused("SWRT_ERR_ARG.*packet count", lambda: c.trans_series_mark_values(st["src"][:299]))
    refused("SWRT_ERR_ARG.*packet count", lambda: c.trans_series_mark_values(st["src"][:301]))
    refused("SWRT_ERR_STATE.*mark", c.trans_series_record)  # a refused mark marks nothing
    c.trans_series_mark_values(st["src"][:300])
    c.trans_series_record()
    c.packets_set(st["x"][:300], st["k"][:300])  # the same N: the mark belongs to the old set all the same
    refused("SWRT_ERR_STATE.*mark", c.trans_series_record)
    assert c.trans_series_frames() == 1  # (the recorded frame stays)
    c.trans_series_mark()
    for first, count in ((-1, 1), (0, 2), (1, 1), (0, -1)):
        refused("SWRT_ERR_ARG.*range", lambda: c.trans_series_get(first, count))
    refused("SWRT_ERR_ARG.*history", lambda: c.trans_series_record_history(0, 1))  # no history frames
    c.trans_series_record()  # the open series is still usable
    assert c.trans_series_frames() == 2 and c.trans_series_get()[2][:, 2].tolist() == [1, 2]


def test_more_than_2_24_packets_are_refused(fresh_ctx, state):
    """The argument check alone: the packet buffers are never read (mark and
    record return before any launch)."""
    c, st = fresh_ctx, state
    n = (1 << 24) + 1
    z = np.zeros((n, 2))
    c.packets_set(z, z)
    _begin(c, st, *_edges(st, 3, 5))
    for call in (c.trans_series_mark, c.trans_series_record, lambda: c.trans_series_mark_values(np.zeros(n))):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*2\\^24"):
            call()
    assert c.trans_series_frames() == 0


# ---- the ensemble and the drivers ---------------------------------------------

TRANS_FILES = ("trans_hist.bin", "trans_sums.bin", "trans_stats.bin", "trans_time.bin", "trans_geom.bin")
SPEC_EDGES = np.linspace(9.0, 15.0, 13)  # the ring starts at omega = 12
SRC_EDGES = np.array([11.0, 11.9, 12.1, 13.0])  # (the mark sits in the middle class)


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


def _read_trans(files, src_edges, nw, by, fb=20):
    ns = len(src_edges) - 1
    frames = len(files["trans_stats.bin"]) // 24
    assert len(files["trans_hist.bin"]) == frames * (ns + 2) * (nw + 2) * 8
    assert len(files["trans_sums.bin"]) == frames * 3 * (ns + 2) * 8
    assert len(files["trans_stats.bin"]) == frames * 3 * 8
    assert len(files["trans_time.bin"]) == frames * 2 * 8
    geom = np.frombuffer(files["trans_geom.bin"], dtype=np.float64)
    assert geom.tolist() == [ns, nw, fb, by] + list(src_edges) + SPEC_EDGES.tolist()
    counts = np.frombuffer(files["trans_hist.bin"], dtype=np.int64).reshape(frames, ns + 2, nw + 2)
    sums = np.frombuffer(files["trans_sums.bin"], dtype=np.int64).reshape(frames, ns + 2, 3)
    stats = np.frombuffer(files["trans_stats.bin"], dtype=np.int64).reshape(frames, 3)
    times = np.frombuffer(files["trans_time.bin"], dtype=np.float64).reshape(frames, 2)
    return counts, sums, stats, times


def _check_driver_files(d, facts, n, lag=None, fb=20):
    """A transition frame beside every packet frame but the first, where the
    mark is taken: sizes, the count identity, the omega marginal, the times
    and the serials of the lag."""
    nw = SPEC_EDGES.size - 1
    frames = facts["packet_frames"] - 1
    assert facts["trans_frames"] == frames > 1
    files = _files(d)
    counts, sums, stats, times = _read_trans(files, SRC_EDGES, nw, 0, fb)
    assert counts.shape[0] == frames
    rows = sw.read_field(os.path.join(d, "omega_hist"), nw + 2, 1, 1).reshape(nw + 2, frames + 1).T
    ptime = sw.read_field(os.path.join(d, "packet_time"), 1, 1, 1).ravel()
    print(f"source rows {counts.sum(axis=2).tolist()} stats {stats.tolist()} times {times.tolist()}")
    assert (stats[:, 0] == n).all() and (stats[:, 1] == 0).all()  # nobody rejected: the run stayed finite
    np.testing.assert_array_equal(counts.sum(axis=(1, 2)), stats[:, 0] - stats[:, 1])
    np.testing.assert_array_equal(counts.sum(axis=1), rows[1:])  # packet frame i + 1
    np.testing.assert_array_equal(times[:, 0], ptime[1:])
    index = np.arange(1, frames + 1)
    marks = np.zeros(frames, dtype=np.int64) if lag is None else (index - 1) // lag  # re-marks before frame `index`
    np.testing.assert_array_equal(stats[:, 2], 1 + marks)
    np.testing.assert_array_equal(times[:, 1], ptime[marks * (lag or 0)])  # the mark's frame: the last multiple of lag
    mom = sw.trans_moments(counts, sums, fb)
    wstats = sw.read_field(os.path.join(d, "omega_stats"), 4, 1, 1).reshape(4, frames + 1).T
    mean = np.nansum(mom["omega_mean"] * mom["n"], axis=1) / n
    np.testing.assert_allclose(mean, wstats[1:, 1] / n, rtol=0, atol=2.0 ** -fb)  # exact to the quantum
    return files


def test_one_layer_driver(ctx, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    args = (64, 64, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0)
    kw = dict(ctx=ctx, max_steps=25, nsub=2, r_drag=0.0, spectrum_edges=SPEC_EDGES)
    facts = sw.qgsw_raytrace(*args, out_dir=a, trans_src_edges=SRC_EDGES, **kw)
    fa = _check_driver_files(a, facts, 64)
    counts = _read_trans(fa, SRC_EDGES, 12, 0)[0]
    assert (counts.sum(axis=2)[:, 2] == 64).all()  # never re-marked: every packet keeps the ring's class
    # with the new arguments left out: the same files without the five, the same bytes, the same facts
    plain = sw.qgsw_raytrace(*args, out_dir=b, **kw)
    fb = _files(b)
    assert plain["trans_frames"] == 0 and not set(TRANS_FILES) & set(fb)
    assert {n: v for n, v in fa.items() if n not in TRANS_FILES} == fb
    assert {k: v for k, v in facts.items() if k != "trans_frames"} == \
        {k: v for k, v in plain.items() if k != "trans_frames"}
    log_a, log_b = (open(os.path.join(d, "run.log")).read().splitlines() for d in (a, b))
    assert len(log_a) == len(log_b) and not any("Rings" in line for line in log_a)
    # re-marked every second frame, another frac_bits, no packet files
    facts = sw.qgsw_raytrace(*args, out_dir=b, trans_src_edges=SRC_EDGES, trans_lag=2, trans_frac_bits=8,
                             packet_files=False, **kw)
    assert facts["packet_frames"] == 6
    fl = _check_driver_files(b, facts, 64, lag=2, fb=8)
    assert "packet_x.bin" not in fl
    with pytest.raises(ValueError, match="spectrum_edges"):
        sw.qgsw_raytrace(*args, out_dir=b, ctx=ctx, max_steps=5, trans_src_edges=SRC_EDGES)
    with pytest.raises(ValueError, match="trans_lag"):
        sw.qgsw_raytrace(*args, out_dir=b, trans_by="ring", trans_lag=2, **kw)
    with pytest.raises(ValueError, match="trans_lag"):
        sw.qgsw_raytrace(*args, out_dir=b, trans_src_edges=SRC_EDGES, trans_lag=0, **kw)


def test_two_layer_driver(ctx, tmp_path):
    facts = sw.qg2layersw_raytrace(64, 64, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path), nsub=2, max_steps=80,
                                   seed=5, ctx=ctx, spectrum_edges=SPEC_EDGES, trans_src_edges=SRC_EDGES, trans_lag=2)
    _check_driver_files(str(tmp_path), facts, 64, lag=2)


@pytest.mark.parametrize("driver,args,kw", [
    ("qgsw_raytrace", (64, 65, [2.0, 4.0], 20.0, 0.0, 0.2, 3.0, 1.0), dict(max_steps=15, nsub=2, r_drag=0.0)),
    ("qg2layersw_raytrace", (64, 65, [2.0, 4.0], 40.0, 0.0, 0.2, 3.0, 1.0), dict(max_steps=80, nsub=2, seed=5)),
])
def test_rings_split_the_spectra(ctx, tmp_path, driver, args, kw):
    """Two rings in one run, trans_by="ring": source row r is the spectrum of
    ring r's packets.  The cheaper equivalent of a separate single-ring
    context: each row is compared with the class-binning of omega of that
    ring's block of the run's own packet_k.bin frames (the packets do not
    interact, so a single-ring context over the same snapshots holds exactly
    that block); the first frame's k is the two-ring layout of the ref."""
    d = str(tmp_path)
    edges = np.linspace(4.0, 15.0, 23)  # the rings start at omega = 6 and 12
    facts = getattr(sw, driver)(*args, out_dir=d, ctx=ctx, spectrum_edges=edges, trans_by="ring", **kw)
    n, f, Cg = args[1], args[6], args[7]
    frames = facts["packet_frames"] - 1
    assert facts["trans_frames"] == frames > 1
    files = _files(d)
    ns, nw = 2, edges.size - 1
    geom = np.frombuffer(files["trans_geom.bin"], dtype=np.float64)
    assert geom.tolist() == [ns, nw, 20, 1, -0.5, 0.5, 1.5] + edges.tolist()
    counts = np.frombuffer(files["trans_hist.bin"], dtype=np.int64).reshape(frames, ns + 2, nw + 2)
    stats = np.frombuffer(files["trans_stats.bin"], dtype=np.int64).reshape(frames, 3)
    assert (stats == [n, 0, 1]).all()
    kf = sw.read_field(os.path.join(d, "packet_k"), n, 2, 1).reshape(n, 2, frames + 1)
    np.testing.assert_array_equal(kf[:, :, 0], ring_k(n, [2.0, 4.0], f, Cg))
    ring = ring_of(n, 2)
    assert np.bincount(ring).tolist() == [32, 33]
    for i in range(frames):
        w = omega_of(kf[:, :, i + 1], f, Cg)
        assert not counts[i, 0].any() and not counts[i, 3].any()
        for r in (0, 1):
            row = np.bincount(class_of(w[ring == r], edges), minlength=nw + 2)
            np.testing.assert_array_equal(counts[i, r + 1], row, err_msg=f"frame {i} ring {r}")
    assert np.count_nonzero(counts[-1, 1]) > 1 and np.count_nonzero(counts[-1, 2]) > 1  # the rings have spread
    log = open(os.path.join(d, "run.log")).read()
    assert log.count("Rings:") == 1 and "omega0 = 6" in log and "omega0 = 12" in log


def test_record_trans_drains_a_large_series(fresh_ctx, state, tmp_path, monkeypatch):
    """The drain (get, combine, append, reset) at a lowered threshold: the same files as one write at the end."""
    import swraytracing_amd.integrate as integ
    st, q = state, state["q"]
    wedges, sedges = _edges(st, 3, 5)

    def run(d, threshold):
        monkeypatch.setattr(integ, "MAP_DRAIN_BYTES", threshold)
        os.makedirs(d)
        ens = sw.PacketEnsemble(st["x"], st["k"], q["L"], q["f"], q["Cg"], q["nx"], q["K_d2"], bump=BUMP, ctx=fresh_ctx)
        ens.begin_trans(wedges, sedges, FB, directory=d if threshold < 1 << 20 else None)
        with pytest.raises(sw.SwrtError, match="mark_trans"):
            ens.record_trans(0.0)
        for i in range(7):
            fresh_ctx.packets_set(st["x"], st["k"] * (1.0 + 0.02 * i))
            if i % 3 == 0:
                ens.mark_trans(st["src"], t=float(i))
            else:
                ens.mark_trans(t=float(i))
                fresh_ctx.packets_set(st["x"], st["k"] * (1.0 + 0.02 * i + 0.01))
                ens.mark_trans(st["src"], t=float(i))
            ens.record_trans(i + 0.5)
        if threshold >= 1 << 20:
            counts, sums, stats, times = ens.trans_series()
            assert counts.shape == (7, 5, 7) and times[:, 0].tolist() == [i + 0.5 for i in range(7)]
            assert times[:, 1].tolist() == [float(i) for i in range(7)]
            want = trans_frame_of(st["src"], omega_of(st["k"] * (1.0 + 0.02 * 6), q["f"], q["Cg"]), wedges, sedges, FB,
                                  serial=11)
            _equal((counts[6], sums[6], stats[6]), want, "the ensemble's last frame")
        assert ens.write_trans(d) == 7
        return _files(d)

    whole = run(str(tmp_path / "whole"), 256 << 20)
    drained = run(str(tmp_path / "drained"), 3 * 8 * (5 * 7 + 3 * 5 + 3) - 1)  # drains at every third frame
    assert set(whole) == set(TRANS_FILES) and whole == drained
    assert len(whole["trans_hist.bin"]) == 7 * 35 * 8 and len(whole["trans_stats.bin"]) == 7 * 3 * 8
