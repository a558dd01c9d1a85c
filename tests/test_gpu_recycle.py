"""Packet recycling on the device (swrt_recycle_*;
swraytracing_amd/csrc/swrt_recycle.hpp).

Expected values are tests/recycle_ref.py, the numpy restatement of the
contract in include/swrt.h, alternated with the C oracle's leapfrog (or the
library's own ode23 interval).  Every comparison is exact: the int64 and int32
arrays as they are, the float64 arrays viewed as uint64.  Conditions on the
inputs (how many packets an event absorbs) are asserted on the restatement,
never on the device's result."""
import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import cbind, swrt_oracle as orc
from swraytracing_amd import _lib as L_
from tests.recycle_ref import omega_of, recycle_event

pytestmark = pytest.mark.gpu

BUMP = orc.BUMP_QG
FB = 20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what=""):
    """x, k (bits), gen, born (int32) and the frame (int64)."""
    for g, w, name in zip(got, want, ("x", "k", "gen", "born", "frame")):
        if name in ("x", "k"):
            np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{what}: {name}")
        else:
            assert g.dtype == w.dtype, (name, g.dtype, w.dtype)
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


@pytest.fixture(scope="module")
def spread(qg_case):
    """1000 packets on the qg_case ring with |k| scaled by 1 + 0.3 N(0, 1)
    (computed once, read-only)."""
    q = qg_case
    rng = np.random.default_rng(41)
    x, k = orc.initial_packets(1000, q["L"], 4.0, q["f"], q["Cg"], rng)
    k = k * (1.0 + 0.3 * rng.standard_normal((1000, 1)))
    for a in (x, k):
        a.setflags(write=False)
    return dict(q=q, x=x, k=k)


def _planted(st, n, fb=FB):
    """The first n packets, their homes (0.3 k: inside the cut) and the cut,
    the omega of the packet at the 80th percentile: that packet sits exactly
    at the cut.  Where n allows three more are planted: the largest reachable
    omega below the cut, a NaN k and k = (1e9, 0).  At frac_bits 0 the
    contract does not reject 1e9 (it is below 2^38 quanta, hence absorbed), so
    there k = (1e12, 0) is planted as well and the rejected stay two.
    -> x, k, home, cut, (index at the cut, index just below it)."""
    q = st["q"]
    x, k = st["x"][:n].copy(), st["k"][:n].copy()
    w = omega_of(k, q["f"], q["Cg"])
    at = int(np.argsort(w)[int(0.8 * n)])
    cut = float(w[at])
    home = 0.3 * k
    below = None
    if n > 9:
        below, nan, big, bigger = [i for i in (3, 5, 7, 9, 11) if i != at][:4]
        kb = k[at].copy()
        j = int(np.argmax(np.abs(kb)))
        while omega_of(kb[None, :], q["f"], q["Cg"])[0] >= cut:
            kb[j] = np.nextafter(kb[j], 0.0)
        k[below] = kb
        k[nan, 1] = np.nan
        k[big] = [1e9, 0.0]
        home[[below, nan, big]] = 0.3 * st["k"][[below, nan, big]]
        if fb == 0:
            k[bigger] = [1e12, 0.0]
    return x, k, home, cut, (at, below)


def _event(c, q, x, k, home, cut, fb, seed=7, base=0):
    c.packets_set(x, k)
    c.recycle_begin(q["f"], q["Cg"], cut, q["L"], seed=seed, index_base=base, frac_bits=fb, home_k=home)
    c.recycle_apply()
    assert c.recycle_frames() == 1
    xg, kg = c.packets_get()
    gen, born = c.recycle_state()
    return xg, kg, gen, born, c.recycle_get()[0]


@pytest.mark.parametrize("n,fb", [(1, FB), (255, FB), (256, FB), (257, FB), (1000, FB), (1000, 0), (1000, 32)])
def test_one_event_against_the_restatement(ctx, spread, n, fb):
    """One packet, a workgroup's edge on both sides, four workgroups with a
    partial last wave; the packets planted at the cut's edge and the two
    rejected ones where n allows."""
    q = spread["q"]
    x, k, home, cut, (at, below) = _planted(spread, n, fb)
    zeros = np.zeros(n, dtype=np.int32)
    want = recycle_event(x, k, home, zeros, zeros, 1, q["f"], q["Cg"], cut, q["L"], 7, 0, fb)
    st = want[4]
    print(f"n {n} frac_bits {fb}: cut {cut!r} frame {st.tolist()}")
    assert want[2][at] == 1  # (exactly at the cut: absorbed)
    if n >= 255:
        assert st[1] > 0 and st[0] - st[1] - st[2] > 0 and st[2] == 2
        assert want[2][below] == 0 and np.array_equal(_bits(want[1][below]), _bits(k[below]))  # (just below: kept)
    _same(_event(ctx, q, x, k, home, cut, fb), want, f"n {n} frac_bits {fb}")


def _tile_setup(c, q, slots=1):
    P = np.asarray(cbind.planes_of(q["flow"]))
    c.set_field_grid(0, P, q["nx"], q["L"])
    if slots == 2:
        c.set_field_grid(1, 1.1 * P, q["nx"], q["L"])
    return P


def _tile_packets(q):
    return orc.initial_packets(5000, q["L"], 4.0, q["f"], q["Cg"], np.random.default_rng(7))


@pytest.fixture(scope="module")
def tile_want(qg_case):
    """The tile case's expected states after every round, per index_base
    (computed once by the oracle and the restatement)."""
    q = qg_case
    P = np.asarray(cbind.planes_of(q["flow"]))
    x0, k0 = _tile_packets(q)
    out = {}
    for base in (0, 1000):
        x, k = x0, k0
        gen = born = np.zeros(5000, dtype=np.int32)
        rounds = []
        for r in range(6):
            x, k, _, _ = cbind.leapfrog(P, None, 0, 0, 64, 64, q["L"] / 64, BUMP, x, k, q["dt"], 8, q["f"],
                                        q["Cg"] ** 2)
            x, k, gen, born, st = recycle_event(x, k, k0, gen, born, r + 1, q["f"], q["Cg"], 12.3, q["L"], 99, base,
                                                FB)
            rounds.append((x, k, gen, born, st))
        out[base] = rounds
    return out


def _tile_run(c, q, base, rounds=6):
    x0, k0 = _tile_packets(q)
    _tile_setup(c, q)
    c.packets_set(x0, k0)
    c.recycle_begin(q["f"], q["Cg"], 12.3, q["L"], seed=99, index_base=base, frac_bits=FB)  # (home: the packets' k now)
    got = []
    for r in range(rounds):
        c.advance(q["dt"], 8, q["f"], q["Cg"] ** 2, nslots=1, bump=BUMP)
        c.recycle_apply()
        got.append((*c.packets_get(), *c.recycle_state(), c.recycle_get(r, 1)[0]))
    return got


def test_tile_path_several_events(fresh_ctx, qg_case, tile_want):
    """5000 packets (binned and permuted), six rounds of 8 leapfrog steps and
    an event: every round's packets, marks and frame equal the oracle's
    leapfrog alternated with the restatement.  Every event absorbs between 5 %
    and 40 % of the packets and at least 500 end with gen >= 2 (asserted on
    the restatement), so re-injected packets are advanced and absorbed again."""
    q = qg_case
    want = tile_want[0]
    for r, w in enumerate(want):
        print(f"event {r + 1}: frame {w[4].tolist()}")
        assert 0.05 * 5000 <= w[4][1] <= 0.40 * 5000 and w[4][2] == 0
    assert np.count_nonzero(want[-1][2] >= 2) >= 500
    got = _tile_run(fresh_ctx, q, 0)
    for r, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"round {r + 1}")
    np.testing.assert_array_equal(fresh_ctx.recycle_get(), np.stack([w[4] for w in want]))


def test_tile_path_another_index_base(fresh_ctx, qg_case, tile_want):
    """index_base 1000: other positions than index_base 0's, the restatement's."""
    got = _tile_run(fresh_ctx, qg_case, 1000)
    for r, (g, w) in enumerate(zip(got, tile_want[1000])):
        _same(g, w, f"round {r + 1}")
    assert not np.array_equal(_bits(tile_want[1000][0][0]), _bits(tile_want[0][0][0]))
    np.testing.assert_array_equal(tile_want[1000][0][4], tile_want[0][0][4])  # (the first frame does not see the positions)


def test_tile_path_under_the_hazard_checker(fresh_ctx, qg_case, tile_want):
    """The same case with the happens-before checker on: no report, the same bits."""
    c = fresh_ctx
    c.debug_set(L_.DEBUG_HAZARD_CHECK, 1)
    try:
        got = _tile_run(c, qg_case, 0, rounds=3)
        assert c.debug_get(L_.DEBUG_HAZARD_CHECKS) > 0
    finally:
        c.debug_set(L_.DEBUG_HAZARD_CHECK, 0)
    for r, (g, w) in enumerate(zip(got, tile_want[0])):
        _same(g, w, f"round {r + 1}")


def test_two_snapshots(fresh_ctx, qg_case):
    """The two-snapshot blend (nslots = 2), two rounds: the oracle's blended
    leapfrog plus the restatement."""
    c, q = fresh_ctx, qg_case
    x0, k0 = _tile_packets(q)
    P = _tile_setup(c, q, slots=2)
    phys = dict(alpha0=0.05, dalpha=0.1)
    c.packets_set(x0, k0)
    c.recycle_begin(q["f"], q["Cg"], 12.3, q["L"], seed=99, frac_bits=FB)
    x, k = x0, k0
    gen = born = np.zeros(5000, dtype=np.int32)
    for r in range(2):
        c.advance(q["dt"], 8, q["f"], q["Cg"] ** 2, nslots=2, bump=BUMP, **phys)
        c.recycle_apply()
        x, k, _, _ = cbind.leapfrog(P, 1.1 * P, phys["alpha0"], phys["dalpha"], 64, 64, q["L"] / 64, BUMP, x, k,
                                    q["dt"], 8, q["f"], q["Cg"] ** 2)
        x, k, gen, born, st = recycle_event(x, k, k0, gen, born, r + 1, q["f"], q["Cg"], 12.3, q["L"], 99, 0, FB)
        assert 0 < st[1] < 5000
        _same((*c.packets_get(), *c.recycle_state(), c.recycle_get(r, 1)[0]), (x, k, gen, born, st), f"round {r + 1}")


def test_ode23_chain_is_dropped(qg_case):
    """An ode23 interval that queues the next one's stage 1 (the drivers'
    hook), an event, the next interval — against the interval, the
    restatement applied on the host through packets_get / packets_set, and the
    interval again.  A chained stage 1 left alive by the event would be that of
    the packets before it."""
    q = qg_case
    nx, Lx, f, Cg = q["nx"], q["L"], q["f"], q["Cg"]
    P = np.asarray(cbind.planes_of(q["flow"]))
    rng = np.random.default_rng(43)
    x0, k0 = orc.initial_packets(1000, Lx, 4.0, f, Cg, rng)
    k0 = k0 * (1.0 + 0.02 * rng.standard_normal((1000, 1)))
    cut = float(np.percentile(omega_of(k0, f, Cg), 70))
    home = 0.5 * k0
    tmax = 30 * q["dt"]

    def fields(c):
        for s, scale in enumerate((1.0, 1.3, -0.7)):
            c.set_field_grid(s, scale * P, nx, Lx)

    def interval(c, arm):
        hook = (lambda: c.ode23_chain_next(1, 2)) if arm else None
        c.ode23_run(0.0, tmax, tmax, f, Cg, 2, 1e-3, 1e-6, BUMP, hook=hook)

    a = sw.Context(0)
    try:
        fields(a)
        a.packets_set(x0, k0)
        a.recycle_begin(f, Cg, cut, Lx, seed=3, frac_bits=FB, home_k=home)
        taken0 = a.debug_get(L_.DEBUG_ODE23_CHAINED)
        interval(a, True)
        a.swap_slots(0, 1)
        a.swap_slots(1, 2)  # the armed slots 1 / 2 are now slots 0 / 1
        a.recycle_apply()
        interval(a, False)
        assert a.debug_get(L_.DEBUG_ODE23_CHAINED) == taken0  # (dropped, not taken)
        xa, ka = a.packets_get()
        frame = a.recycle_get()[0]
    finally:
        a.close()
    b = sw.Context(0)
    try:
        fields(b)
        b.packets_set(x0, k0)
        interval(b, False)
        b.swap_slots(0, 1)
        b.swap_slots(1, 2)
        x1, k1 = b.packets_get()
        zeros = np.zeros(1000, dtype=np.int32)
        x2, k2, _, _, st = recycle_event(x1, k1, home, zeros, zeros, 1, f, Cg, cut, Lx, 3, 0, FB)
        assert 50 < st[1] < 950 and st[2] == 0
        b.packets_set(x2, k2)
        interval(b, False)
        xb, kb = b.packets_get()
    finally:
        b.close()
    np.testing.assert_array_equal(frame, st)
    np.testing.assert_array_equal(_bits(xa), _bits(xb))
    np.testing.assert_array_equal(_bits(ka), _bits(kb))


def test_series_semantics(fresh_ctx, spread):
    c, q = fresh_ctx, spread["q"]
    n = 257
    x, k, home, cut, _ = _planted(spread, n)
    zeros = np.zeros(n, dtype=np.int32)
    f, Cg, Lx = q["f"], q["Cg"], q["L"]
    # before begin
    for call in (c.recycle_apply, c.recycle_get, c.recycle_state):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):
            call()
    assert c.recycle_frames() == 0
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*no packets"):
        c.recycle_begin(f, Cg, cut, Lx)
    c.packets_set(x, k)
    c.recycle_begin(f, Cg, cut, Lx, seed=7, frac_bits=FB, home_k=home)
    first = recycle_event(x, k, home, zeros, zeros, 1, f, Cg, cut, Lx, 7, 0, FB)
    second = recycle_event(first[0], first[1], home, first[2], first[3], 2, f, Cg, cut, Lx, 7, 0, FB)
    c.recycle_apply()
    c.recycle_apply()  # (nothing left at or above the cut: the rejected two stay)
    assert second[4].tolist() == [n, 0, 2, 0, 0, 0, 0, 2]
    # get: ranges and out-of-range errors
    assert c.recycle_frames() == 2
    np.testing.assert_array_equal(c.recycle_get(), np.stack([first[4], second[4]]))
    np.testing.assert_array_equal(c.recycle_get(1, 1)[0], second[4])
    assert c.recycle_get(2, 0).shape == (0, 8) and c.recycle_get(0, 0).shape == (0, 8)
    for first_, count in ((0, 3), (2, 1), (-1, 1), (1, -1), (3, 0)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*range"):
            c.recycle_get(first_, count)
    _same((*c.packets_get(), *c.recycle_state(), c.recycle_get(1, 1)[0]), second, "two events")
    # packets_set drops the state; the frames stay readable until the next begin
    c.packets_set(x, k)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE"):
        c.recycle_apply()
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE"):
        c.recycle_state()
    np.testing.assert_array_equal(c.recycle_get(), np.stack([first[4], second[4]]))
    c.recycle_begin(f, Cg, cut, Lx, seed=7, frac_bits=FB, home_k=home)
    assert c.recycle_frames() == 0
    c.recycle_apply()
    np.testing.assert_array_equal(c.recycle_get()[0], first[4])
    # end: everything released
    c.recycle_end()
    assert c.recycle_frames() == 0
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE.*begin"):
        c.recycle_get()


def test_reset_restarts_the_marks(fresh_ctx, qg_case, tile_want):
    """The tile case's first round, a reset, the second round: gen, born and
    the serial are back at 0 and home is kept, so the second event is a fresh
    begin's on the packets the first round left (re-injected packets that
    are absorbed again get generation 1 and age 1 once more)."""
    c, q = fresh_ctx, qg_case
    got = _tile_run(c, q, 0, rounds=1)
    _same(got[0], tile_want[0][0], "round 1")
    c.recycle_reset()
    assert c.recycle_frames() == 0
    gen, born = c.recycle_state()
    assert gen.dtype == np.int32 and not gen.any() and not born.any()
    c.advance(q["dt"], 8, q["f"], q["Cg"] ** 2, nslots=1, bump=BUMP)
    c.recycle_apply()
    P = np.asarray(cbind.planes_of(q["flow"]))
    x1, k1 = tile_want[0][0][:2]
    _, k0 = _tile_packets(q)
    x, k, _, _ = cbind.leapfrog(P, None, 0, 0, 64, 64, q["L"] / 64, BUMP, x1, k1, q["dt"], 8, q["f"], q["Cg"] ** 2)
    zeros = np.zeros(5000, dtype=np.int32)
    want = recycle_event(x, k, k0, zeros, zeros, 1, q["f"], q["Cg"], 12.3, q["L"], 99, 0, FB)
    again = np.count_nonzero((want[2] == 1) & (tile_want[0][0][2] == 1))
    print(f"after the reset: frame {want[4].tolist()}, {again} absorbed in both rounds")
    assert again >= 50 and want[4][6] == 1 and want[4][7] == 1
    _same((*c.packets_get(), *c.recycle_state(), c.recycle_get()[0]), want, "after the reset")


def test_argument_errors(fresh_ctx, spread):
    c, q = fresh_ctx, spread["q"]
    f, Cg, Lx = q["f"], q["Cg"], q["L"]
    x, k = spread["x"][:100], spread["k"][:100]
    c.packets_set(x, k)
    good = dict(f=f, Cg=Cg, omega_cut=50.0, L=Lx)
    for bad, msg in ((dict(L=0.0), "L must"), (dict(L=-1.0), "L must"), (dict(L=np.inf), "L must"),
                     (dict(L=np.nan), "L must"), (dict(f=np.nan), "finite"), (dict(Cg=np.inf), "finite"),
                     (dict(omega_cut=np.nan), "finite"), (dict(omega_cut=np.inf), "finite"),
                     (dict(omega_cut=f), "above"), (dict(omega_cut=0.5 * f), "above"),
                     (dict(f=-60.0), "above"), (dict(frac_bits=-1), "frac_bits"), (dict(frac_bits=33), "frac_bits")):
        with pytest.raises(sw.SwrtError, match=f"SWRT_ERR_ARG.*{msg}"):
            c.recycle_begin(**{**good, **bad})
    with pytest.raises(ValueError):
        c.recycle_begin(**good, home_k=k[:50])
    # a home at or above the cut, or one that would be rejected, is refused on the device
    w = omega_of(k, f, Cg)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*home"):
        c.recycle_begin(f, Cg, float(np.sort(w)[-1]), Lx)  # (the packets' own k: the largest omega is at the cut)
    for row in ([1e9, 0.0], [np.nan, 0.0]):
        home = 0.3 * k
        home[57] = row
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*home"):
            c.recycle_begin(f, Cg, 50.0, Lx, home_k=home)
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_STATE"):
        c.recycle_apply()  # (a refused begin leaves nothing begun)
    c.recycle_begin(f, Cg, float(np.nextafter(np.sort(w)[-1], np.inf)), Lx)  # (one ulp above every home: allowed)
    c.recycle_apply()
    assert c.recycle_get()[0].tolist() == [100, 0, 0, 0, 0, 0, 0, 1]
