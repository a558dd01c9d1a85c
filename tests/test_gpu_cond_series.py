"""The conditional spectrum series on the device (swrt_cond_series_*;
swraytracing_amd/csrc/swrt_cond.hpp) and the drivers' cond_*.bin files.

Expected values are tests/cond_series_ref.py, the numpy restatement of the
contract in include/swrt.h on the oracle's interpolation, at the packets
swrt_packets_get returns; the fields are set as six planes, so both sides
gather the same numbers.  Every comparison is exact integer equality: integer
sums are order-free, so there is no tolerance.

The packets are 1000 on the qg_case ring after 40 leapfrog steps (their omega
has spread); a case with N packets takes the first N.  The omega edges span the
central 80 % of the restatement's omega of those 1000, the vorticity edges half
the gridded flow's largest |zeta| either way, the strain and Okubo-Weiss edges
the 10th to 90th percentile of the restatement's values at those 1000.  Where a
test says so it asserts on the restatement's frame (never the device's) that
below, above and half of the interior classes of both axes are populated; with
1000 packets every shape is, with fewer only the small shapes can be."""
import ctypes
import os

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import cbind, swrt_oracle as orc
from swraytracing_amd._lib import DEBUG_COND_GLOBAL
from tests.cond_series_ref import (assert_populated, central_edges, cond_frame, cond_frame_of, flow_scalars, omega_of,
                                   quantile_edges, zeta_edges)

pytestmark = pytest.mark.gpu

FB = 20
BUMP = orc.BUMP_QG
SHAPES = [(1, 1), (4, 7), (15, 300)]  # (nq, nw)


def _fields(c, q, nslots=2):
    planes = cbind.planes_of(q["flow"])
    c.set_field_grid(0, planes, q["nx"], q["L"])
    if nslots == 2:
        c.set_field_grid(1, 0.8 * np.asarray(planes), q["nx"], q["L"])


@pytest.fixture(scope="module")
def state(qg_case):
    """The evolved packets, the two snapshots in the oracle's form, and the
    restatement's scalars and omega at those packets (computed once, read-only)."""
    q = qg_case
    rng = np.random.default_rng(31)
    x0, k0 = orc.initial_packets(1000, q["L"], 4.0, q["f"], q["Cg"], rng)
    c = sw.Context(0)
    try:
        _fields(c, q)
        c.packets_set(x0, k0)
        c.advance(q["dt"], 40, q["f"], q["Cg"] ** 2, nslots=1, bump=BUMP)
        x, k = (np.ascontiguousarray(a) for a in c.packets_get())
    finally:
        c.close()
    assert np.isfinite(x).all() and np.isfinite(k).all()
    flows = [q["flow"], {n: 0.8 * np.asarray(v) for n, v in q["flow"].items()}]
    dx = q["L"] / q["nx"]
    scal = {1: flow_scalars(flows, 1, 0.0, x, dx, BUMP), 2: flow_scalars(flows, 2, 0.3, x, dx, BUMP)}
    w = omega_of(k, q["f"], q["Cg"])
    for a in (x, k, w, x0, k0):
        a.setflags(write=False)
    return dict(q=q, x0=x0, k0=k0, x=x, k=k, flows=flows, dx=dx, scal=scal, w=w)


def _edges(st, which, nq, nw):
    qedges = zeta_edges(st["q"]["flow"], nq) if which == 0 else quantile_edges(st["scal"][1][which], nq)
    return central_edges(st["w"], nw), qedges


def _begin(c, st, which, wedges, qedges, fb=FB):
    c.cond_series_begin(st["q"]["f"], st["q"]["Cg"], wedges, which, qedges, fb)


def _equal(got, want, what=""):
    for g, w, name in zip(got, want, ("counts", "sums", "stats")):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _planted(st, n):
    """The first n packets with a NaN k and k = 1e9 planted where n allows."""
    x, k = st["x"][:n].copy(), st["k"][:n].copy()
    if n > 3:
        k[3, 1] = np.nan
    if n > 5:
        k[5] = [1e9, 0.0]
    return x, k


@pytest.mark.parametrize("nslots,alpha", [(1, 0.0), (2, 0.3)])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_device_against_itself(fresh_ctx, state, which, nslots, alpha):
    """After an advance the frame is the class-binning of swrt_raydiag_sample's
    column and of omega from swrt_packets_get on the same context."""
    c, st, q = fresh_ctx, state, state["q"]
    _fields(c, q, nslots)
    c.packets_set(st["x0"], st["k0"])
    c.advance(q["dt"], 40, q["f"], q["Cg"] ** 2, nslots=nslots, alpha0=alpha, bump=BUMP)
    wedges, qedges = _edges(st, which, 15, 300)
    _begin(c, st, which, wedges, qedges)
    c.cond_series_record(nslots, alpha, BUMP)
    s4, _ = c.raydiag_sample(q["f"], q["Cg"] ** 2, nslots=nslots, alpha=alpha, bump=BUMP)
    _, k = c.packets_get()
    want = cond_frame_of(s4[:, 1 + which], omega_of(k, q["f"], q["Cg"]), wedges, qedges, FB)
    counts, sums, stats = c.cond_series_get()
    assert counts.shape == (1, 17, 302) and sums.shape == (1, 17) and stats.shape == (1, 2)
    print(f"which {which} nslots {nslots}: q row {want[0].sum(axis=1).tolist()} stats {want[2].tolist()}")
    assert_populated(want[0])
    assert want[2].tolist() == [1000, 0]
    _equal((counts[0], sums[0], stats[0]), want, f"which {which} nslots {nslots}")


@pytest.mark.parametrize("nq,nw", SHAPES)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_device_against_the_restatement(ctx, state, n, nq, nw):
    """One packet, a workgroup's edge on both sides, and (1000) a grid stride
    with a partial last wave; one snapshot, then two blended at 0.3."""
    c, st, q = ctx, state, state["q"]
    _fields(c, q)
    x, k = _planted(st, n)
    c.packets_set(x, k)
    w = omega_of(k, q["f"], q["Cg"])
    for which in (0, 1, 2):
        wedges, qedges = _edges(st, which, nq, nw)
        _begin(c, st, which, wedges, qedges)
        c.cond_series_record(1, 0.0, BUMP)
        c.cond_series_record(2, 0.3, BUMP)
        got = c.cond_series_get()
        for i, nslots in enumerate((1, 2)):
            want = cond_frame_of(st["scal"][nslots][which][:n], w, wedges, qedges, FB)
            what = f"n {n} ({nq}, {nw}) which {which} nslots {nslots}"
            print(f"{what}: q row {want[0].sum(axis=1).tolist()} stats {want[2].tolist()}")
            assert want[2][0] == n and want[0].sum() == n - want[2][1]
            assert want[2][1] == (n > 3) + (n > 5)
            if n == 1000:
                assert_populated(want[0], want[2], planted=True)
            _equal([a[i] for a in got], want, what)
    # the restatement end to end (its own interpolation) on the last shape
    want = cond_frame(st["flows"], 2, 0.3, x, k, st["dx"], BUMP, q["f"], q["Cg"], wedges, 2, qedges, FB)
    _equal([a[1] for a in got], want, "cond_frame")


@pytest.fixture()
def cctx(ctx):
    """The session context with the path key back at 0 afterwards."""
    yield ctx
    ctx.debug_set(DEBUG_COND_GLOBAL, 0)


def test_path_boundary(cctx, state):
    """16384 cells (the last LDS shape) and 16385 (the first global one) agree
    with the restatement; the forced global kernel gives the LDS kernel's
    integers on (15, 300), frac_bits 0 and 32 included."""
    c, st, q = cctx, state, state["q"]
    _fields(c, q)
    x, k = _planted(st, 1000)
    c.packets_set(x, k)
    w = omega_of(k, q["f"], q["Cg"])
    for nq, nw in ((126, 126), (3, 3275)):
        assert (nq + 2) * (nw + 2) == 16384 + (nq == 3)
        wedges, qedges = _edges(st, 0, nq, nw)
        want = cond_frame_of(st["scal"][2][0], w, wedges, qedges, FB)
        if nw < 1000:
            assert_populated(want[0], want[2], planted=True)
        else:  # (1000 packets cannot fill half of 3275 omega bins: both ends of both axes, and a spread)
            wrow, qrow = want[0].sum(axis=0), want[0].sum(axis=1)
            assert wrow[0] > 0 and wrow[-1] > 0 and np.count_nonzero(wrow) > 500 and (qrow > 0).all() and want[2][1] > 0
        _begin(c, st, 0, wedges, qedges)
        c.cond_series_record(2, 0.3, BUMP)
        _equal([a[0] for a in c.cond_series_get()], want, f"({nq}, {nw})")
    for fb in (0, FB, 32):
        wedges, qedges = _edges(st, 0, 15, 300)
        want = cond_frame_of(st["scal"][1][0], w, wedges, qedges, fb)
        assert_populated(want[0], want[2], planted=True)
        _begin(c, st, 0, wedges, qedges, fb)
        for forced in (0, 1):
            c.debug_set(DEBUG_COND_GLOBAL, forced)
            assert c.debug_get(DEBUG_COND_GLOBAL) == forced
            c.cond_series_record(1, 0.0, BUMP)
        c.debug_set(DEBUG_COND_GLOBAL, 0)
        got = c.cond_series_get()
        for i in (0, 1):
            _equal([a[i] for a in got], want, f"frac_bits {fb} forced {i}")
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
        c.debug_set(DEBUG_COND_GLOBAL, 2)


def test_one_shared_cell(cctx, state):
    """Every packet at one position with one k: one cell holds all 1000
    (the wave merge, the 32-bit LDS count), on both paths."""
    c, st, q = cctx, state, state["q"]
    _fields(c, q, 1)
    n = 1000
    x, k = np.tile(st["x"][:1], (n, 1)), np.tile(st["k"][:1], (n, 1))
    c.packets_set(x, k)
    wedges, qedges = _edges(st, 0, 15, 300)
    want = cond_frame_of(np.full(n, st["scal"][1][0][0]), omega_of(k, q["f"], q["Cg"]), wedges, qedges, FB)
    assert np.count_nonzero(want[0]) == 1 and want[0].max() == n
    assert want[1].max() == n * int(np.rint(st["w"][0] * 2.0 ** FB))
    _begin(c, st, 0, wedges, qedges)
    for forced in (0, 1):
        c.debug_set(DEBUG_COND_GLOBAL, forced)
        c.cond_series_record(1, 0.0, BUMP)
    got = c.cond_series_get()
    for i in (0, 1):
        _equal([a[i] for a in got], want, f"forced {i}")


def test_rebinning_does_not_change_a_frame(state):
    """Twin contexts with the same packets, one re-binning every 4 steps and
    one never: equal frames after 10 and after 13 steps (a re-binning between
    the two records), each the restatement's at that context's packets."""
    st, q = state, state["q"]
    wedges, qedges = _edges(st, 0, 15, 300)
    frames = {}
    for rebin in (4, 0):
        c = sw.Context(0)
        try:
            _fields(c, q)
            c.set_locality(rebin, 0)
            c.packets_set(st["x"], st["k"])
            _begin(c, st, 0, wedges, qedges)
            states = []
            for steps in (10, 3):
                c.advance(q["dt"], steps, q["f"], q["Cg"] ** 2, nslots=2, alpha0=0.05, dalpha=0.1, bump=BUMP)
                c.cond_series_record(2, 0.3, BUMP)
                states.append(c.packets_get())
            got = c.cond_series_get()
            for i, (x, k) in enumerate(states):
                want = cond_frame(st["flows"], 2, 0.3, x, k, st["dx"], BUMP, q["f"], q["Cg"], wedges, 0, qedges, FB)
                assert_populated(want[0])
                _equal([a[i] for a in got], want, f"rebin_every {rebin} record {i}")
            assert not np.array_equal(got[0][0], got[0][1])
            frames[rebin] = got
        finally:
            c.close()
    _equal(frames[4], frames[0], "re-binned against never re-binned")


def test_advance_calls_and_packet_streams_do_not_change_a_frame(state):
    """swrt_advance_intervals against two swrt_advance calls, and one packet
    stream against two (65,536 packets: the tile launches split), give equal
    frames."""
    st, q = state, state["q"]
    wedges, qedges = _edges(st, 0, 15, 300)
    P = np.asarray(cbind.planes_of(q["flow"]))
    rng = np.random.default_rng(32)
    xb, kb = orc.initial_packets(65536, q["L"], 4.0, q["f"], q["Cg"], rng)
    kb = kb * (1.0 + 0.3 * rng.standard_normal((65536, 1)))
    h, phys = q["dt"], dict(alpha0=0.1, dalpha=0.2, bump=BUMP)
    frames = []
    for form, streams in (("intervals", 2), ("calls", 2), ("calls", 1)):
        c = sw.Context(0)
        try:
            c.set_packet_streams(streams)
            c.packets_set(xb, kb)
            for s, scale in enumerate((1.0, 0.8, 0.9)):
                c.set_field_grid(s, scale * P, q["nx"], q["L"])
            if form == "intervals":
                c.advance_intervals([h, 1.1 * h], 5, q["f"], q["Cg"] ** 2, **phys)
            else:
                c.advance(h, 5, q["f"], q["Cg"] ** 2, nslots=2, **phys)
                c.set_field_grid(0, 0.8 * P, q["nx"], q["L"])
                c.set_field_grid(1, 0.9 * P, q["nx"], q["L"])
                c.advance(1.1 * h, 5, q["f"], q["Cg"] ** 2, nslots=2, **phys)
            c.set_field_grid(0, P, q["nx"], q["L"])
            c.set_field_grid(1, 0.8 * P, q["nx"], q["L"])
            _begin(c, st, 0, wedges, qedges)
            c.cond_series_record(2, 0.3, BUMP)
            frames.append(c.cond_series_get())
        finally:
            c.close()
    assert frames[0][2][0].tolist() == [65536, 0] and frames[0][0].sum() == 65536
    _equal(frames[1], frames[0], "two advance calls against advance_intervals")
    _equal(frames[2], frames[0], "one packet stream against two")


@pytest.mark.parametrize("count", [1, 3])
def test_record_history(fresh_ctx, state, count):
    """One frame per history frame with its own alpha: the bits of a record on
    packets set to that frame."""
    c, st, q = fresh_ctx, state, state["q"]
    _fields(c, q)
    c.packets_set(st["x"], st["k"])
    c.history_reset()
    c.advance(q["dt"], 4 * count, q["f"], q["Cg"] ** 2, nslots=2, alpha0=0.05, dalpha=0.1, bump=BUMP, save_every=4)
    hx, hk = c.history()
    assert hx.shape[0] == count
    alphas = np.array([0.3, 0.55, 0.9])[:count]
    wedges, qedges = _edges(st, 1, 15, 300)
    _begin(c, st, 1, wedges, qedges)
    c.cond_series_record_history(0, count, 2, alphas, BUMP)
    assert c.cond_series_frames() == count
    hist = c.cond_series_get()
    c.cond_series_record_history(0, count, 1, None, BUMP)  # one snapshot: no alphas
    one = c.cond_series_get(count, count)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*alphas"):  # two snapshots need them
        c._chk(c._L.swrt_cond_series_record_history(c._h, 0, count, 2, None, BUMP), "record_history")
    for i in range(count):
        x, k = np.ascontiguousarray(hx[i].T), np.ascontiguousarray(hk[i].T)
        want = cond_frame(st["flows"], 2, alphas[i], x, k, st["dx"], BUMP, q["f"], q["Cg"], wedges, 1, qedges, FB)
        assert_populated(want[0])
        _equal([a[i] for a in hist], want, f"history frame {i}")
        c.packets_set(x, k)
        c.cond_series_reset()
        c.cond_series_record(2, alphas[i], BUMP)
        c.cond_series_record(1, 0.0, BUMP)
        rec = c.cond_series_get()
        _equal([a[0] for a in rec], [a[i] for a in hist], f"record on frame {i}")
        _equal([a[1] for a in rec], [a[i] for a in one], f"record on frame {i}, one snapshot")
    if count > 1:
        assert len({a.tobytes() for a in hist[0]}) == count  # the frames differ
    for first, n in ((0, count + 1), (-1, 1), (count, 1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*history"):
            c.cond_series_record_history(first, n, 1, None, BUMP)


def test_series_life(fresh_ctx, state):
    """4097 frames of a tiny shape grow the series past its first 4096;
    reset keeps the edges, begin empties, another N keeps earlier frames."""
    c, st, q = fresh_ctx, state, state["q"]
    _fields(c, q, 1)
    wedges, qedges = _edges(st, 0, 1, 1)
    c.packets_set(st["x"][:1], st["k"][:1])
    _begin(c, st, 0, wedges, qedges)
    for _ in range(4097):
        c.cond_series_record(1, 0.0, BUMP)
    assert c.cond_series_frames() == 4097 and c.cond_series_bins() == (1, 1)
    counts, sums, stats = c.cond_series_get()
    want = cond_frame_of(st["scal"][1][0][:1], st["w"][:1], wedges, qedges, FB)
    for i in (0, 4095, 4096):
        _equal((counts[i], sums[i], stats[i]), want, f"frame {i}")
    assert (counts == counts[0]).all() and (sums == sums[0]).all() and (stats == stats[0]).all()
    part = c.cond_series_get(4090, 7)
    assert part[0].shape == (7, 3, 3) and np.array_equal(part[0], counts[4090:])
    # each output alone
    i64 = ctypes.POINTER(ctypes.c_int64)
    only = [np.zeros_like(a[:2]) for a in (counts, sums, stats)]
    for j in range(3):
        args = [only[i].ctypes.data_as(i64) if i == j else None for i in range(3)]
        assert c._L.swrt_cond_series_get(c._h, 4095, 2, *args) == 0
    _equal(only, [a[4095:] for a in (counts, sums, stats)], "single outputs")
    assert c._L.swrt_cond_series_get(c._h, 0, 1, None, None, None) == 0
    c.cond_series_reset()
    assert c.cond_series_frames() == 0 and c.cond_series_bins() == (1, 1)
    assert c.cond_series_get()[0].shape == (0, 3, 3)
    c.cond_series_record(1, 0.0, BUMP)  # the edges stay
    c.packets_set(st["x"][:300], st["k"][:300])  # another N keeps the frame
    assert c.cond_series_frames() == 1
    c.cond_series_record(1, 0.0, BUMP)
    got = c.cond_series_get()
    _equal([a[0] for a in got], want, "frame 0 after the reset")
    _equal([a[1] for a in got], cond_frame_of(st["scal"][1][0][:300], st["w"][:300], wedges, qedges, FB), "300 packets")
    wedges, qedges = _edges(st, 0, 4, 7)
    _begin(c, st, 0, wedges, qedges)  # begin again: empty, the new shape
    assert c.cond_series_frames() == 0 and c.cond_series_bins() == (7, 4)
    c.cond_series_record(1, 0.0, BUMP)
    want = cond_frame_of(st["scal"][1][0][:300], st["w"][:300], wedges, qedges, FB)
    assert_populated(want[0])
    _equal([a[0] for a in c.cond_series_get()], want, "after the second begin")


def test_errors(fresh_ctx, state):
    c, st, q = fresh_ctx, state, state["q"]
    wedges, qedges = _edges(st, 0, 4, 7)

    def refused(code, call):
        with pytest.raises(sw.SwrtError, match=code) as e:
            call()
        assert c._L.swrt_last_error(c._h), e.value  # a message, not only a code
        return str(e.value)

    refused("SWRT_ERR_STATE.*begin", lambda: c.cond_series_record(1, 0.0, BUMP))
    refused("SWRT_ERR_STATE.*begin", lambda: c.cond_series_record_history(0, 0, 1, None, BUMP))
    assert c.cond_series_frames() == 0 and c.cond_series_bins() == (0, 0)
    big = np.arange(301.0)
    refused("SWRT_ERR_ARG.*65536", lambda: c.cond_series_begin(3.0, 1.0, big + 3, 0, big, FB))  # 302 x 302 cells
    refused("SWRT_ERR_ARG", lambda: c.cond_series_begin(3.0, 1.0, wedges, 0, qedges[:1], FB))  # nq = 0
    refused("SWRT_ERR_ARG", lambda: c.cond_series_begin(3.0, 1.0, wedges[:1], 0, qedges, FB))
    refused("SWRT_ERR_ARG.*4096", lambda: c.cond_series_begin(3.0, 1.0, np.arange(4098.0), 0, qedges, FB))
    refused("SWRT_ERR_ARG.*increase", lambda: c.cond_series_begin(3.0, 1.0, wedges, 0, qedges[::-1], FB))
    refused("SWRT_ERR_ARG.*increase", lambda: c.cond_series_begin(3.0, 1.0, wedges[::-1], 0, qedges, FB))
    bad = qedges.copy()
    bad[2] = np.nan
    refused("SWRT_ERR_ARG.*finite", lambda: c.cond_series_begin(3.0, 1.0, wedges, 0, bad, FB))
    refused("SWRT_ERR_ARG.*which", lambda: c.cond_series_begin(3.0, 1.0, wedges, 3, qedges, FB))
    refused("SWRT_ERR_ARG.*which", lambda: c.cond_series_begin(3.0, 1.0, wedges, -1, qedges, FB))
    refused("SWRT_ERR_ARG.*frac_bits", lambda: c.cond_series_begin(3.0, 1.0, wedges, 0, qedges, 33))
    refused("SWRT_ERR_ARG.*frac_bits", lambda: c.cond_series_begin(3.0, 1.0, wedges, 0, qedges, -1))
    refused("SWRT_ERR_STATE.*begin", lambda: c.cond_series_record(1, 0.0, BUMP))  # a refused begin opens nothing
    _begin(c, st, "zeta", wedges, qedges)
    refused("SWRT_ERR_ARG.*nslots", lambda: c.cond_series_record(3, 0.0, BUMP))
    refused("SWRT_ERR_ARG.*nslots", lambda: c.cond_series_record(0, 0.0, BUMP))
    refused("SWRT_ERR_ARG.*slot", lambda: c.cond_series_record(1, 0.0, BUMP))  # an unset slot
    _fields(c, q, 1)
    refused("SWRT_ERR_ARG.*slot", lambda: c.cond_series_record(2, 0.3, BUMP))  # slot 1 unset
    refused("SWRT_ERR_ARG.*no packets", lambda: c.cond_series_record(1, 0.0, BUMP))
    c.packets_set(st["x"][:300], st["k"][:300])
    c.set_field_grid(1, cbind.planes_of({n: v[::2, ::2] for n, v in q["flow"].items()}), q["nx"] // 2, q["L"])
    refused("SWRT_ERR_ARG.*grids", lambda: c.cond_series_record(2, 0.3, BUMP))
    c.cond_series_record(1, 0.0, BUMP)
    for first, count in ((-1, 1), (0, 2), (1, 1), (0, -1)):
        refused("SWRT_ERR_ARG.*range", lambda: c.cond_series_get(first, count))
    refused("SWRT_ERR_ARG.*history", lambda: c.cond_series_record_history(0, 1, 1, None, BUMP))  # no history frames
    c.cond_series_record(1, 0.0, BUMP)  # the open series is still usable
    assert c.cond_series_frames() == 2


# ---- the ensemble and the drivers ---------------------------------------------

COND_FILES = ("cond_hist.bin", "cond_sums.bin", "cond_stats.bin", "cond_geom.bin")
SPEC_EDGES = np.linspace(9.0, 15.0, 13)  # the ring starts at omega = 12
Q_EDGES = np.array([-1.0, -0.3, 0.0, 0.3, 1.0])


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


def _check_driver_files(d, facts, n, which=0, fb=20):
    """A cond frame beside every packet frame but the first (written before
    any snapshot exists): sizes, the count identity, the omega marginal."""
    nq, nw = Q_EDGES.size - 1, SPEC_EDGES.size - 1
    frames = facts["packet_frames"] - 1
    assert facts["cond_frames"] == frames > 1
    files = _files(d)
    assert len(files["cond_hist.bin"]) == frames * (nq + 2) * (nw + 2) * 8
    assert len(files["cond_sums.bin"]) == frames * (nq + 2) * 8
    assert len(files["cond_stats.bin"]) == frames * 2 * 8
    geom = np.frombuffer(files["cond_geom.bin"], dtype=np.float64)
    assert geom.tolist() == [which, nq, nw, fb] + Q_EDGES.tolist() + SPEC_EDGES.tolist()
    counts = np.frombuffer(files["cond_hist.bin"], dtype=np.int64).reshape(frames, nq + 2, nw + 2)
    sums = np.frombuffer(files["cond_sums.bin"], dtype=np.int64).reshape(frames, nq + 2)
    stats = np.frombuffer(files["cond_stats.bin"], dtype=np.int64).reshape(frames, 2)
    rows = sw.read_field(os.path.join(d, "omega_hist"), nw + 2, 1, 1).reshape(nw + 2, frames + 1).T
    print(f"q rows {counts.sum(axis=2).tolist()} stats {stats.tolist()}")
    assert (stats[:, 0] == n).all() and (stats[:, 1] == 0).all()  # nobody rejected: the run stayed finite
    np.testing.assert_array_equal(counts.sum(axis=(1, 2)), stats[:, 0] - stats[:, 1])
    np.testing.assert_array_equal(counts.sum(axis=1), rows[1:])  # packet frame i + 1
    assert np.count_nonzero(counts.sum(axis=(0, 2))) >= 2  # more than one vorticity class is met
    spec = sw.cond_spectra(counts, sums, fb)
    mean = np.nansum(spec["omega_mean"] * spec["n"], axis=1) / n
    wstats = sw.read_field(os.path.join(d, "omega_stats"), 4, 1, 1).reshape(4, frames + 1).T
    np.testing.assert_allclose(mean, wstats[1:, 1] / n, rtol=0, atol=2.0 ** -fb)  # exact to the quantum
    return files


def test_one_layer_driver(ctx, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    args = (64, 64, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0)
    kw = dict(ctx=ctx, max_steps=15, nsub=2, r_drag=0.0, spectrum_edges=SPEC_EDGES)
    facts = sw.qgsw_raytrace(*args, out_dir=a, cond_by="zeta", cond_edges=Q_EDGES, **kw)
    fa = _check_driver_files(a, facts, 64)
    # with the new arguments left out: the same files without the four, the same bytes, the same facts
    plain = sw.qgsw_raytrace(*args, out_dir=b, **kw)
    fb = _files(b)
    assert plain["cond_frames"] == 0 and not set(COND_FILES) & set(fb)
    assert {n: v for n, v in fa.items() if n not in COND_FILES} == fb
    assert {k: v for k, v in facts.items() if k != "cond_frames"} == \
        {k: v for k, v in plain.items() if k != "cond_frames"}
    with pytest.raises(ValueError, match="spectrum_edges"):
        sw.qgsw_raytrace(*args, out_dir=b, ctx=ctx, max_steps=5, cond_by="zeta", cond_edges=Q_EDGES)
    # another scalar and frac_bits
    facts = sw.qgsw_raytrace(*args, out_dir=b, cond_by="D", cond_edges=Q_EDGES, cond_frac_bits=8, **kw)
    _check_driver_files(b, facts, 64, which=2, fb=8)


def test_two_layer_driver(ctx, tmp_path):
    facts = sw.qg2layersw_raytrace(64, 64, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path), nsub=2, max_steps=80,
                                   seed=5, ctx=ctx, spectrum_edges=SPEC_EDGES, cond_by="zeta", cond_edges=Q_EDGES)
    _check_driver_files(str(tmp_path), facts, 64)


def test_record_cond_drains_a_large_series(fresh_ctx, state, tmp_path, monkeypatch):
    """The drain (get, combine, append, reset) at a lowered threshold: the same files as one write at the end."""
    import swraytracing_amd.integrate as integ
    st, q = state, state["q"]
    wedges, qedges = _edges(st, 0, 4, 7)
    _fields(fresh_ctx, q)

    def run(d, threshold):
        monkeypatch.setattr(integ, "MAP_DRAIN_BYTES", threshold)
        os.makedirs(d)
        ens = sw.PacketEnsemble(st["x"], st["k"], q["L"], q["f"], q["Cg"], q["nx"], q["K_d2"], bump=BUMP, ctx=fresh_ctx)
        ens.begin_cond(wedges, "zeta", qedges, FB, directory=d if threshold < 1 << 20 else None)
        for i in range(7):
            fresh_ctx.packets_set(st["x"], st["k"] * (1.0 + 0.02 * i))
            ens.record_cond(0.3 if i % 2 == 0 else None)  # two snapshots blended, then slot 0 alone, in turn
        if threshold >= 1 << 20:
            counts, sums, stats = ens.cond_series()
            assert counts.shape == (7, 6, 9)
            want = cond_frame_of(st["scal"][2][0], omega_of(st["k"] * (1.0 + 0.02 * 6), q["f"], q["Cg"]), wedges, qedges,
                                 FB)
            _equal((counts[6], sums[6], stats[6]), want, "the ensemble's last frame")
        assert ens.write_conds(d) == 7
        return _files(d)

    whole = run(str(tmp_path / "whole"), 256 << 20)
    drained = run(str(tmp_path / "drained"), 3 * 8 * (6 * 9 + 6 + 2) - 1)  # drains at every third frame
    assert set(whole) == set(COND_FILES) and whole == drained
    assert len(whole["cond_hist.bin"]) == 7 * 54 * 8 and len(whole["cond_stats.bin"]) == 7 * 2 * 8
