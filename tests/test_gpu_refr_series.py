"""The refraction series on the device (swrt_refr_series_*;
swraytracing_amd/csrc/swrt_refr.hpp) and the drivers' refr_*.bin files.

Expected values are tests/refr_series_ref.py, the numpy restatement of the
contract in include/swrt.h on the oracle's interpolation; the fields are set as
six planes, so both sides gather the same numbers.  Every comparison is exact
integer equality: integer sums are order-free, so there is no tolerance.

The packets are 4099 on the initial ring spread by 300 leapfrog steps of the C
oracle (the device's bits), in the qg_case 64^2 flow and in a 32^2 flow built
the same way; a case with N packets takes the first N.  Bump 1e-10, alignment
edges linspace(-0.8, 0.8, na + 1), omega edges over the central 80 % of the
restatement's omega range of the 4099.  Where a test says so it asserts on the
restatement's frame (never the device's) that below, above and half of the
interior classes of both axes are populated."""
import ctypes
import os

import numpy as np
import pytest

import swraytracing_amd as sw
import swraytracing_amd.qg as qgmod
from oracle import cbind, swrt_oracle as orc
from swraytracing_amd._lib import DEBUG_REFR_GLOBAL
from tests.cond_series_ref import assert_populated, central_edges
from tests.refr_series_ref import a_edges_of, gradients, packet_values, refr_frame, refr_frame_of

pytestmark = pytest.mark.gpu

FB = 20
BUMP = 1e-10
NALL = 4099
SHAPES = [(1, 1), (8, 12), (126, 126), (127, 126), (200, 300)]  # (na, nw)
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]


def _flow32():
    """A 32^2 background built as conftest's qg_case builds its 64^2 one."""
    nx, L, f, Cg, Ug = 32, 2 * np.pi, 3.0, 1.0, 0.2
    rng = np.random.default_rng(147)
    K_d2 = f / Cg
    q = orc.initial_q(nx, L, Ug, K_d2, 5, 8, rng)
    kx_, ky_, K2 = orc.wavenumber_grids(nx)
    flow = orc.grid_U(orc.g2k(q), K_d2, K2, kx_, ky_)
    speed = np.sqrt(flow["u"] ** 2 + flow["v"] ** 2).max()
    return dict(nx=nx, L=L, f=f, Cg=Cg, K_d2=K_d2, flow=flow, dt=0.05 * (L / nx) / speed)


def _state(q, seed):
    """The spread packets, the two snapshots in the oracle's form, and the
    restatement's gradients at those packets (computed once, read-only)."""
    rng = np.random.default_rng(seed)
    x0, k0 = orc.initial_packets(NALL, q["L"], 4.0, q["f"], q["Cg"], rng)
    planes = cbind.planes_of(q["flow"])
    dx = q["L"] / q["nx"]
    x, k, _, _ = cbind.leapfrog(planes, None, 0.0, 0.0, q["nx"], q["nx"], dx, BUMP, x0, k0, q["dt"], 300, q["f"],
                                q["Cg"] ** 2)
    x, k = np.ascontiguousarray(x), np.ascontiguousarray(k)
    assert np.isfinite(x).all() and np.isfinite(k).all()
    flows = [q["flow"], {n: 0.8 * np.asarray(v) for n, v in q["flow"].items()}]
    grads = {1: gradients(flows, 1, 0.0, x, dx, BUMP), 2: gradients(flows, 2, 0.3, x, dx, BUMP)}
    w = packet_values(grads[1], k, q["f"], q["Cg"])[0]
    for a in (x, k, w) + grads[1] + grads[2]:
        a.setflags(write=False)
    return dict(q=q, x=x, k=k, flows=flows, dx=dx, grads=grads, w=w, planes=np.asarray(planes))


@pytest.fixture(scope="module")
def states(qg_case):
    return {64: _state(qg_case, 33), 32: _state(_flow32(), 34)}


@pytest.fixture(scope="module")
def state(states):
    return states[64]


def _fields(c, st, nslots=2):
    q = st["q"]
    c.set_field_grid(0, st["planes"], q["nx"], q["L"])
    if nslots == 2:
        c.set_field_grid(1, 0.8 * st["planes"], q["nx"], q["L"])


def _edges(st, na, nw):
    return central_edges(st["w"], nw), a_edges_of(na)


def _begin(c, st, wedges, aedges, fb=FB):
    c.refr_series_begin(st["q"]["f"], st["q"]["Cg"], wedges, aedges, fb)


def _equal(got, want, what=""):
    for g, w, name in zip(got, want, ("counts", "sums", "stats")):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _planted(st, n):
    """The first n packets with a NaN k, k = 0 and k = 1e9 planted where n allows."""
    x, k = st["x"][:n].copy(), st["k"][:n].copy()
    if n > 3:
        k[3, 1] = np.nan
    if n > 4:
        k[4] = [0.0, 0.0]
    if n > 5:
        k[5] = [1e9, 0.0]
    return x, k


def _assert_spread(counts):
    """The frame (the restatement's) of packets advanced past the spread state,
    whose omega range has moved against the edges: at least half of the
    interior classes of both axes are met."""
    for axis in (0, 1):
        row = counts.sum(axis=axis)
        assert 2 * np.count_nonzero(row[1:-1]) >= row.size - 2, row


def _want(st, nslots, k, wedges, aedges, fb=FB):
    n = k.shape[0]
    vals = packet_values(tuple(g[:n] for g in st["grads"][nslots]), k, st["q"]["f"], st["q"]["Cg"])
    return refr_frame_of(*vals, wedges, aedges, fb)


def test_the_inputs_fill_the_classes(states):
    """On the restatement alone: every shape's frame of the 4099 packets has
    below, above and half the interior classes of both axes, on both grids,
    with one snapshot and with two; nobody is rejected."""
    for nx, st in states.items():
        for na, nw in SHAPES:
            wedges, aedges = _edges(st, na, nw)
            for nslots in (1, 2):
                counts, sums, stats = _want(st, nslots, st["k"], wedges, aedges)
                print(f"{nx}^2 ({na}, {nw}) nslots {nslots}: stats {stats.tolist()}"
                      + (f" a row {counts.sum(axis=1).tolist()}" if na <= 8 else ""))
                assert stats.tolist() == [NALL, 0]
                assert_populated(counts)


@pytest.mark.parametrize("na,nw", SHAPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nx", [64, 32])
def test_device_against_the_restatement(ctx, states, nx, n, na, nw):
    """One packet, a wave's and a workgroup's edge on both sides, a grid
    stride with a partial last wave; one snapshot, then two blended at 0.3;
    planted NaN, zero and huge k are rejected as the restatement rejects them."""
    c, st = ctx, states[nx]
    _fields(c, st)
    x, k = _planted(st, n)
    c.packets_set(x, k)
    wedges, aedges = _edges(st, na, nw)
    _begin(c, st, wedges, aedges)
    c.refr_series_record(1, 0.0, BUMP)
    c.refr_series_record(2, 0.3, BUMP)
    got = c.refr_series_get()
    assert got[0].shape == (2, na + 2, nw + 2) and got[1].shape == (2, 3 * (nw + 2) + na + 2)
    for i, nslots in enumerate((1, 2)):
        want = _want(st, nslots, k, wedges, aedges)
        what = f"{nx}^2 n {n} ({na}, {nw}) nslots {nslots}"
        assert want[2][0] == n and want[0].sum() == n - want[2][1]
        assert want[2][1] == (n > 3) + (n > 4) + (n > 5)
        if n == NALL:
            assert_populated(want[0], want[2], planted=True)
        _equal([a[i] for a in got], want, what)
    if (na, nw) == (8, 12):  # the restatement end to end (its own interpolation)
        q = st["q"]
        want = refr_frame(st["flows"], 2, 0.3, x, k, st["dx"], BUMP, q["f"], q["Cg"], wedges, aedges, FB)
        _equal([a[1] for a in got], want, "refr_frame")


@pytest.fixture()
def rctx(ctx):
    """The session context with the path key back at 0 afterwards."""
    yield ctx
    ctx.debug_set(DEBUG_REFR_GLOBAL, 0)


def test_path_boundary(rctx, state):
    """(126, 126), 16384 cells, is the last LDS shape and (127, 126) the first
    global one; on the same packets the forced global kernel gives the LDS
    kernel's integers, frac_bits 0 and 32 included."""
    c, st = rctx, state
    _fields(c, st)
    x, k = _planted(st, NALL)
    c.packets_set(x, k)
    assert (126 + 2) * (126 + 2) == 16384
    for fb in (0, FB, 32):
        wedges, aedges = _edges(st, 126, 126)
        want = _want(st, 2, k, wedges, aedges, fb)
        assert_populated(want[0], want[2], planted=True)
        _begin(c, st, wedges, aedges, fb)
        for forced in (0, 1):
            c.debug_set(DEBUG_REFR_GLOBAL, forced)
            assert c.debug_get(DEBUG_REFR_GLOBAL) == forced
            c.refr_series_record(2, 0.3, BUMP)
        c.debug_set(DEBUG_REFR_GLOBAL, 0)
        got = c.refr_series_get()
        _equal([a[0] for a in got], [a[1] for a in got], f"frac_bits {fb}: LDS against global")
        _equal([a[0] for a in got], want, f"frac_bits {fb}")
    wedges, aedges = _edges(st, 127, 126)
    _begin(c, st, wedges, aedges)
    c.refr_series_record(2, 0.3, BUMP)
    _equal([a[0] for a in c.refr_series_get()], _want(st, 2, k, wedges, aedges), "(127, 126)")
    # few alignment rows over thousands of omega classes: the sums alone outgrow the LDS form's share
    wedges, aedges = _edges(st, 1, 4096)
    _begin(c, st, wedges, aedges)
    c.refr_series_record(1, 0.0, BUMP)
    _equal([a[0] for a in c.refr_series_get()], _want(st, 1, k, wedges, aedges), "(1, 4096)")
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
        c.debug_set(DEBUG_REFR_GLOBAL, 2)


def test_one_shared_cell(rctx, state):
    """Every packet at one position with one k: one cell holds all 1000 and
    every sum is 1000 times one packet's (the wave merge, the 32-bit LDS
    count, fully contended LDS sums), on both paths."""
    c, st, q = rctx, state, state["q"]
    _fields(c, st, 1)
    n = 1000
    x, k = np.tile(st["x"][:1], (n, 1)), np.tile(st["k"][:1], (n, 1))
    c.packets_set(x, k)
    wedges, aedges = _edges(st, 8, 12)
    one = _want(st, 1, k[:1], wedges, aedges)
    want = refr_frame(st["flows"], 1, 0.0, x, k, st["dx"], BUMP, q["f"], q["Cg"], wedges, aedges, FB)
    assert np.count_nonzero(want[0]) == 1 and want[0].max() == n
    np.testing.assert_array_equal(want[1], n * one[1])
    assert np.count_nonzero(want[1]) == 4
    _begin(c, st, wedges, aedges)
    for forced in (0, 1):
        c.debug_set(DEBUG_REFR_GLOBAL, forced)
        c.refr_series_record(1, 0.0, BUMP)
    got = c.refr_series_get()
    for i in (0, 1):
        _equal([a[i] for a in got], want, f"forced {i}")


def test_a_divergent_flow_lands_outside(ctx, state):
    """Six fields with v_y != -u_x: |c| exceeds 1 for some packets, which land
    in below or above of edges over [-1, 1]; nothing is rejected."""
    c, st, q = ctx, state, state["q"]
    flow = dict(q["flow"])
    flow["vy"] = 0.25 * np.asarray(flow["vy"])
    assert not np.array_equal(flow["vy"], -np.asarray(flow["ux"]))
    c.set_field_grid(0, cbind.planes_of(flow), q["nx"], q["L"])
    assert not c.field_div_free(0)
    c.packets_set(st["x"], st["k"])
    wedges, aedges = central_edges(st["w"], 12), sw.alignment_edges(8)
    _begin(c, st, wedges, aedges)
    c.refr_series_record(1, 0.0, BUMP)
    want = refr_frame([flow], 1, 0.0, st["x"], st["k"], st["dx"], BUMP, q["f"], q["Cg"], wedges, aedges, FB)
    arow = want[0].sum(axis=1)
    print(f"a row {arow.tolist()}")
    assert arow[0] > 10 and arow[-1] > 10 and want[2].tolist() == [NALL, 0]
    _equal([a[0] for a in c.refr_series_get()], want, "divergent flow")


def test_rebinning_does_not_change_a_frame(state):
    """An advance between set and record (the packets re-binned, stored in
    another order): the frame of a fresh context given the advanced packets,
    and the restatement's; re-binning every 4 steps against never."""
    st, q = state, state["q"]
    wedges, aedges = _edges(st, 8, 12)
    frames = {}
    for rebin in (4, 0):
        c = sw.Context(0)
        try:
            _fields(c, st)
            c.set_locality(rebin, 0)
            c.packets_set(st["x"], st["k"])
            _begin(c, st, wedges, aedges)
            states_ = []
            for steps in (10, 3):
                c.advance(q["dt"], steps, q["f"], q["Cg"] ** 2, nslots=2, alpha0=0.05, dalpha=0.1, bump=BUMP)
                c.refr_series_record(2, 0.3, BUMP)
                states_.append(c.packets_get())
            got = c.refr_series_get()
        finally:
            c.close()
        for i, (x, k) in enumerate(states_):
            want = refr_frame(st["flows"], 2, 0.3, x, k, st["dx"], BUMP, q["f"], q["Cg"], wedges, aedges, FB)
            _assert_spread(want[0])
            _equal([a[i] for a in got], want, f"rebin_every {rebin} record {i}")
        assert not np.array_equal(got[1][0], got[1][1])
        frames[rebin] = got
        if rebin == 4:  # a fresh context given the advanced packets
            f = sw.Context(0)
            try:
                _fields(f, st)
                f.packets_set(*states_[1])
                _begin(f, st, wedges, aedges)
                f.refr_series_record(2, 0.3, BUMP)
                _equal([a[0] for a in f.refr_series_get()], [a[1] for a in got], "fresh context")
            finally:
                f.close()
    _equal(frames[4], frames[0], "re-binned against never re-binned")


def test_advance_calls_and_packet_streams_do_not_change_a_frame(state):
    """swrt_advance_intervals against two swrt_advance calls, and one packet
    stream against two (65,536 packets: the tile launches split), give equal
    frames."""
    st, q = state, state["q"]
    wedges, aedges = _edges(st, 8, 12)
    P = st["planes"]
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
            _begin(c, st, wedges, aedges)
            c.refr_series_record(2, 0.3, BUMP)
            frames.append(c.refr_series_get())
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
    _fields(c, st)
    c.packets_set(st["x"][:1000], st["k"][:1000])
    c.history_reset()
    c.advance(q["dt"], 4 * count, q["f"], q["Cg"] ** 2, nslots=2, alpha0=0.05, dalpha=0.1, bump=BUMP, save_every=4)
    hx, hk = c.history()
    assert hx.shape[0] == count
    alphas = np.array([0.3, 0.55, 0.9])[:count]
    wedges, aedges = _edges(st, 8, 12)
    _begin(c, st, wedges, aedges)
    c.refr_series_record_history(0, count, 2, alphas, BUMP)
    assert c.refr_series_frames() == count
    hist = c.refr_series_get()
    c.refr_series_record_history(0, count, 1, None, BUMP)  # one snapshot: no alphas
    one = c.refr_series_get(count, count)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*alphas"):  # two snapshots need them
        c._chk(c._L.swrt_refr_series_record_history(c._h, 0, count, 2, None, BUMP), "record_history")
    for i in range(count):
        x, k = np.ascontiguousarray(hx[i].T), np.ascontiguousarray(hk[i].T)
        want = refr_frame(st["flows"], 2, alphas[i], x, k, st["dx"], BUMP, q["f"], q["Cg"], wedges, aedges, FB)
        _assert_spread(want[0])
        _equal([a[i] for a in hist], want, f"history frame {i}")
        c.packets_set(x, k)
        c.refr_series_reset()
        c.refr_series_record(2, alphas[i], BUMP)
        c.refr_series_record(1, 0.0, BUMP)
        rec = c.refr_series_get()
        _equal([a[0] for a in rec], [a[i] for a in hist], f"record on frame {i}")
        _equal([a[1] for a in rec], [a[i] for a in one], f"record on frame {i}, one snapshot")
    if count > 1:
        assert len({a.tobytes() for a in hist[1]}) == count  # the frames differ
    for first, n in ((0, count + 1), (-1, 1), (count, 1)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*history"):
            c.refr_series_record_history(first, n, 1, None, BUMP)


def test_record_history_across_the_frame_chunk(fresh_ctx, state):
    """258 history frames of 64 packets: two launches (256 frames, then 2);
    the frames on either side of the seam are the restatement's."""
    c, st, q = fresh_ctx, state, state["q"]
    _fields(c, st, 1)
    c.packets_set(st["x"][:64], st["k"][:64])
    c.history_reset()
    c.advance(q["dt"], 258, q["f"], q["Cg"] ** 2, nslots=1, bump=BUMP, save_every=1)
    hx, hk = c.history()
    assert hx.shape[0] == 258
    wedges, aedges = _edges(st, 8, 12)
    _begin(c, st, wedges, aedges)
    c.refr_series_record_history(0, 258, 1, None, BUMP)
    assert c.refr_series_frames() == 258
    counts, sums, stats = c.refr_series_get()
    assert (stats == [64, 0]).all() and (counts.sum(axis=(1, 2)) == 64).all()
    for i in (0, 255, 256, 257):
        x, k = np.ascontiguousarray(hx[i].T), np.ascontiguousarray(hk[i].T)
        want = refr_frame(st["flows"], 1, 0.0, x, k, st["dx"], BUMP, q["f"], q["Cg"], wedges, aedges, FB)
        _equal((counts[i], sums[i], stats[i]), want, f"history frame {i}")
    assert not np.array_equal(sums[255], sums[256])


def test_series_life(fresh_ctx, state):
    """4097 frames of a tiny shape grow the series past its first 4096;
    reset keeps the edges, begin empties, another N keeps earlier frames."""
    c, st = fresh_ctx, state
    _fields(c, st, 1)
    wedges, aedges = _edges(st, 1, 1)
    c.packets_set(st["x"][:1], st["k"][:1])
    _begin(c, st, wedges, aedges)
    for _ in range(4097):
        c.refr_series_record(1, 0.0, BUMP)
    assert c.refr_series_frames() == 4097 and c.refr_series_bins() == (1, 1)
    counts, sums, stats = c.refr_series_get()
    want = _want(st, 1, st["k"][:1], wedges, aedges)
    for i in (0, 4095, 4096):
        _equal((counts[i], sums[i], stats[i]), want, f"frame {i}")
    assert (counts == counts[0]).all() and (sums == sums[0]).all() and (stats == stats[0]).all()
    part = c.refr_series_get(4090, 7)
    assert part[0].shape == (7, 3, 3) and part[1].shape == (7, 12) and np.array_equal(part[1], sums[4090:])
    # each output alone
    i64 = ctypes.POINTER(ctypes.c_int64)
    only = [np.zeros_like(a[:2]) for a in (counts, sums, stats)]
    for j in range(3):
        args = [only[i].ctypes.data_as(i64) if i == j else None for i in range(3)]
        assert c._L.swrt_refr_series_get(c._h, 4095, 2, *args) == 0
    _equal(only, [a[4095:] for a in (counts, sums, stats)], "single outputs")
    assert c._L.swrt_refr_series_get(c._h, 0, 1, None, None, None) == 0
    c.refr_series_reset()
    assert c.refr_series_frames() == 0 and c.refr_series_bins() == (1, 1)
    assert c.refr_series_get()[0].shape == (0, 3, 3)
    c.refr_series_record(1, 0.0, BUMP)  # the edges stay
    c.packets_set(st["x"][:300], st["k"][:300])  # another N keeps the frame
    assert c.refr_series_frames() == 1
    c.refr_series_record(1, 0.0, BUMP)
    got = c.refr_series_get()
    _equal([a[0] for a in got], want, "frame 0 after the reset")
    _equal([a[1] for a in got], _want(st, 1, st["k"][:300], wedges, aedges), "300 packets")
    wedges, aedges = _edges(st, 8, 12)
    _begin(c, st, wedges, aedges)  # begin again: empty, the new shape
    assert c.refr_series_frames() == 0 and c.refr_series_bins() == (12, 8)
    c.refr_series_record(1, 0.0, BUMP)
    _equal([a[0] for a in c.refr_series_get()], _want(st, 1, st["k"][:300], wedges, aedges), "after the second begin")


def test_errors(fresh_ctx, state):
    c, st, q = fresh_ctx, state, state["q"]
    wedges, aedges = _edges(st, 8, 12)

    def refused(code, call):
        with pytest.raises(sw.SwrtError, match=code) as e:
            call()
        assert c._L.swrt_last_error(c._h), e.value  # a message, not only a code
        return str(e.value)

    refused("SWRT_ERR_STATE.*begin", lambda: c.refr_series_record(1, 0.0, BUMP))
    refused("SWRT_ERR_STATE.*begin", lambda: c.refr_series_record_history(0, 0, 1, None, BUMP))
    assert c.refr_series_frames() == 0 and c.refr_series_bins() == (0, 0)
    big = np.arange(301.0)
    refused("SWRT_ERR_ARG.*65536", lambda: c.refr_series_begin(3.0, 1.0, big + 3, big, FB))  # 302 x 302 cells
    refused("SWRT_ERR_ARG", lambda: c.refr_series_begin(3.0, 1.0, wedges, aedges[:1], FB))  # na = 0
    refused("SWRT_ERR_ARG", lambda: c.refr_series_begin(3.0, 1.0, wedges[:1], aedges, FB))
    refused("SWRT_ERR_ARG.*4096", lambda: c.refr_series_begin(3.0, 1.0, np.arange(4098.0), aedges, FB))
    refused("SWRT_ERR_ARG.*4096", lambda: c.refr_series_begin(3.0, 1.0, wedges, np.arange(4098.0), FB))
    refused("SWRT_ERR_ARG.*increase", lambda: c.refr_series_begin(3.0, 1.0, wedges, aedges[::-1], FB))
    refused("SWRT_ERR_ARG.*increase", lambda: c.refr_series_begin(3.0, 1.0, wedges[::-1], aedges, FB))
    bad = aedges.copy()
    bad[2] = np.nan
    refused("SWRT_ERR_ARG.*finite", lambda: c.refr_series_begin(3.0, 1.0, wedges, bad, FB))
    refused("SWRT_ERR_ARG.*frac_bits", lambda: c.refr_series_begin(3.0, 1.0, wedges, aedges, 33))
    refused("SWRT_ERR_ARG.*frac_bits", lambda: c.refr_series_begin(3.0, 1.0, wedges, aedges, -1))
    refused("SWRT_ERR_STATE.*begin", lambda: c.refr_series_record(1, 0.0, BUMP))  # a refused begin opens nothing
    _begin(c, st, wedges, aedges)
    refused("SWRT_ERR_ARG.*nslots", lambda: c.refr_series_record(3, 0.0, BUMP))
    refused("SWRT_ERR_ARG.*nslots", lambda: c.refr_series_record(0, 0.0, BUMP))
    refused("SWRT_ERR_ARG.*slot", lambda: c.refr_series_record(1, 0.0, BUMP))  # an unset slot
    _fields(c, st, 1)
    refused("SWRT_ERR_ARG.*slot", lambda: c.refr_series_record(2, 0.3, BUMP))  # slot 1 unset
    refused("SWRT_ERR_ARG.*no packets", lambda: c.refr_series_record(1, 0.0, BUMP))
    c.packets_set(st["x"][:300], st["k"][:300])
    c.set_field_grid(1, cbind.planes_of({n: v[::2, ::2] for n, v in q["flow"].items()}), q["nx"] // 2, q["L"])
    refused("SWRT_ERR_ARG.*grids", lambda: c.refr_series_record(2, 0.3, BUMP))
    c.refr_series_record(1, 0.0, BUMP)
    for first, count in ((-1, 1), (0, 2), (1, 1), (0, -1)):
        refused("SWRT_ERR_ARG.*range", lambda: c.refr_series_get(first, count))
    refused("SWRT_ERR_ARG.*history", lambda: c.refr_series_record_history(0, 1, 1, None, BUMP))  # no history frames
    c.refr_series_record(1, 0.0, BUMP)  # the open series is still usable
    assert c.refr_series_frames() == 2
    _equal([a[1] for a in c.refr_series_get()], _want(st, 1, st["k"][:300], wedges, aedges), "after the errors")


# ---- the ensemble and the drivers ---------------------------------------------

REFR_FILES = ("refr_hist.bin", "refr_sums.bin", "refr_stats.bin", "refr_geom.bin")
SPEC_EDGES = np.linspace(9.0, 15.0, 13)  # the ring starts at omega = 12
A_EDGES = sw.alignment_edges(4)


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


def _watch_frames(monkeypatch, ctx, seen):
    """Every packet frame the driver saves leaves the packets on the device,
    the device's gradients at them in slot 0 (swrt_eval: the record's I), slot
    0's planes, and the gradients at the positions of the frame just written
    (packet_x.bin holds them wrapped into the domain; None without the file)."""
    saved = qgmod._save_frame

    def save(ens, t, *args, **kw):
        out = saved(ens, t, *args, **kw)
        if kw.get("refrs") or (len(args) > 8 and args[8]):
            x, k = ctx.packets_get()
            wgrads = None
            if args[2]:  # packet_files
                px = sw.read_field(os.path.join(args[0], "packet_x"), x.shape[0], 2, 1, is_real=True)[:, :, -1]
                wgrads = ctx.eval(px[:, 0], px[:, 1], nslots=1, bump=orc.BUMP_QG)[2:]
            seen.append((np.array(x), np.array(k), ctx.eval(x[:, 0], x[:, 1], nslots=1, bump=orc.BUMP_QG)[2:],
                         ctx.get_field_grid(0), wgrads))
        return out

    monkeypatch.setattr(qgmod, "_save_frame", save)


def _check_driver_files(d, facts, n, seen, f, Cg, L, fb=20):
    """A frame beside every packet frame but the first (written before any
    snapshot exists): sizes, all three arrays against the restatement on the
    device's packets, refr_hist.bin against the restatement on the written
    packet frames, both in the snapshot at their time, the omega marginal."""
    na, nw = A_EDGES.size - 1, SPEC_EDGES.size - 1
    frames = facts["packet_frames"] - 1
    assert facts["refr_frames"] == frames == len(seen) > 1
    files = _files(d)
    nsum = 3 * (nw + 2) + na + 2
    assert len(files["refr_hist.bin"]) == frames * (na + 2) * (nw + 2) * 8
    assert len(files["refr_sums.bin"]) == frames * nsum * 8
    assert len(files["refr_stats.bin"]) == frames * 2 * 8
    geom = np.frombuffer(files["refr_geom.bin"], dtype=np.float64)
    assert geom.tolist() == [na, nw, fb] + A_EDGES.tolist() + SPEC_EDGES.tolist()
    counts = np.frombuffer(files["refr_hist.bin"], dtype=np.int64).reshape(frames, na + 2, nw + 2)
    sums = np.frombuffer(files["refr_sums.bin"], dtype=np.int64).reshape(frames, nsum)
    stats = np.frombuffer(files["refr_stats.bin"], dtype=np.int64).reshape(frames, 2)
    px = sw.read_field(os.path.join(d, "packet_x"), n, 2, 1, is_real=True)
    pk = sw.read_field(os.path.join(d, "packet_k"), n, 2, 1, is_real=True)
    assert px.shape[2] == frames + 1
    for i, (x, k, grads, _, wgrads) in enumerate(seen):
        # packet frame i + 1: the device's k, and its x wrapped into the domain
        assert np.array_equal(pk[:, :, i + 1], k)
        assert np.abs((px[:, :, i + 1] - x + L / 2) % L - L / 2).max() < 1e-9
        want = refr_frame_of(*packet_values(tuple(grads), k, f, Cg), SPEC_EDGES, A_EDGES, fb)
        _equal((counts[i], sums[i], stats[i]), want, f"driver frame {i}")
        want = refr_frame_of(*packet_values(tuple(wgrads), pk[:, :, i + 1], f, Cg), SPEC_EDGES, A_EDGES, fb)
        np.testing.assert_array_equal(counts[i], want[0], err_msg=f"driver frame {i} on the written frame")
    rows = sw.read_field(os.path.join(d, "omega_hist"), nw + 2, 1, 1).reshape(nw + 2, frames + 1).T
    print(f"a rows {counts.sum(axis=2).tolist()} stats {stats.tolist()}")
    assert (stats[:, 0] == n).all() and (stats[:, 1] == 0).all()
    np.testing.assert_array_equal(counts.sum(axis=1), rows[1:])
    assert np.count_nonzero(counts.sum(axis=(0, 2))) >= 2  # more than one alignment class is met
    rates = sw.refr_rates(counts, sums, fb)
    assert np.isfinite(rates["flux_share"]).any()
    return files


def test_one_layer_driver(ctx, tmp_path, monkeypatch):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    args = (64, 64, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0)
    kw = dict(ctx=ctx, max_steps=15, nsub=2, r_drag=0.0, spectrum_edges=SPEC_EDGES)
    seen = []
    _watch_frames(monkeypatch, ctx, seen)
    facts = sw.qgsw_raytrace(*args, out_dir=a, refr_edges=A_EDGES, **kw)
    fa = _check_driver_files(a, facts, 64, seen, 3.0, 1.0, 2 * np.pi)
    # every frame once more on the oracle's interpolation of slot 0's planes, the snapshot at the packets' time
    hist = np.frombuffer(fa["refr_hist.bin"], dtype=np.int64).reshape(-1, 6, 14)
    sums = np.frombuffer(fa["refr_sums.bin"], dtype=np.int64).reshape(-1, 48)
    for i, (x, k, _, P, _) in enumerate(seen):
        flow = {name: P[j].reshape(64, 64, order="F") for j, name in enumerate(orc.FIELD_ORDER)}
        want = refr_frame([flow], 1, 0.0, x, k, 2 * np.pi / 64, orc.BUMP_QG, 3.0, 1.0, SPEC_EDGES, A_EDGES, 20)
        np.testing.assert_array_equal(hist[i], want[0])
        np.testing.assert_array_equal(sums[i], want[1])
    # with the new arguments left out: the same files without the four, the same bytes, the same facts
    plain = sw.qgsw_raytrace(*args, out_dir=b, **kw)
    fb = _files(b)
    assert plain["refr_frames"] == 0 and not set(REFR_FILES) & set(fb)
    assert {n: v for n, v in fa.items() if n not in REFR_FILES} == fb
    assert {k_: v for k_, v in facts.items() if k_ != "refr_frames"} == \
        {k_: v for k_, v in plain.items() if k_ != "refr_frames"}
    # packet_files=False is allowed; another frac_bits
    seen.clear()
    facts = sw.qgsw_raytrace(*args, out_dir=b, refr_edges=A_EDGES, refr_frac_bits=8, packet_files=False, **kw)
    fb8 = _files(b)
    assert "packet_x.bin" not in fb8 and facts["refr_frames"] == facts["packet_frames"] - 1 == len(seen)
    assert fb8["refr_hist.bin"] == fa["refr_hist.bin"] and fb8["refr_sums.bin"] != fa["refr_sums.bin"]


def test_two_layer_driver(ctx, tmp_path, monkeypatch):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    args = (64, 64, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0)
    kw = dict(nsub=2, max_steps=80, seed=5, ctx=ctx, spectrum_edges=SPEC_EDGES)
    seen = []
    _watch_frames(monkeypatch, ctx, seen)
    facts = sw.qg2layersw_raytrace(*args, out_dir=a, refr_edges=A_EDGES, **kw)
    fa = _check_driver_files(a, facts, 64, seen, 3.0, 1.0, 20.0)
    plain = sw.qg2layersw_raytrace(*args, out_dir=b, **kw)
    assert plain["refr_frames"] == 0
    assert {n: v for n, v in fa.items() if n not in REFR_FILES} == _files(b)


def test_record_refr_drains_a_large_series(fresh_ctx, state, tmp_path, monkeypatch):
    """The drain (get, combine, append, reset) at a lowered threshold: the same files as one write at the end."""
    import swraytracing_amd.integrate as integ
    st, q = state, state["q"]
    wedges, aedges = _edges(st, 4, 7)
    _fields(fresh_ctx, st)
    x, k = st["x"][:1000], st["k"][:1000]

    def run(d, threshold):
        monkeypatch.setattr(integ, "MAP_DRAIN_BYTES", threshold)
        os.makedirs(d)
        ens = sw.PacketEnsemble(x, k, q["L"], q["f"], q["Cg"], q["nx"], q["K_d2"], bump=BUMP, ctx=fresh_ctx)
        ens.begin_refr(wedges, aedges, FB, directory=d if threshold < 1 << 20 else None)
        for i in range(7):
            fresh_ctx.packets_set(x, k * (1.0 + 0.02 * i))
            ens.record_refr(0.3 if i % 2 == 0 else None)  # two snapshots blended, then slot 0 alone, in turn
        if threshold >= 1 << 20:
            counts, sums, stats = ens.refr_series()
            assert counts.shape == (7, 6, 9) and sums.shape == (7, 33)
            want = _want(st, 2, k * (1.0 + 0.02 * 6), wedges, aedges)
            _equal((counts[6], sums[6], stats[6]), want, "the ensemble's last frame")
        assert ens.write_refrs(d) == 7
        return _files(d)

    whole = run(str(tmp_path / "whole"), 256 << 20)
    drained = run(str(tmp_path / "drained"), 3 * 8 * (6 * 9 + 33 + 2) - 1)  # drains at every third frame
    assert set(whole) == set(REFR_FILES) and whole == drained
    assert len(whole["refr_hist.bin"]) == 7 * 54 * 8 and len(whole["refr_sums.bin"]) == 7 * 33 * 8
