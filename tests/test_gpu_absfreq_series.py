"""The absolute-frequency series on the device (swrt_absfreq_series_*;
swraytracing_amd/csrc/swrt_absfreq.hpp) and the drivers' absfreq_*.bin files.

Expected values are tests/absfreq_series_ref.py, the numpy restatement of the
contract in include/swrt.h, on the per-slot records A and B that
swrt_eval(nslots = 1) gives with each slot swapped into place 0.  Every
comparison with the restatement is exact integer equality: integer sums are
order-free, so there is no tolerance.

The fields are two different random non-divergent snapshots on 32^2 through
swrt_set_field_psi; the packets are 4099 spread over the domain with
wavevectors spread around the omega = 12 ring; a case with N packets takes the
first N.  Omega edges span the 10th to 90th percentile of the restatement's
values, so below, above and the interior fill."""
import ctypes
import os

import numpy as np
import pytest

import swraytracing_amd as sw
import swraytracing_amd.qg as qgmod
from oracle import swrt_oracle as orc
from swraytracing_amd._lib import DEBUG_ABSFREQ_GLOBAL
from tests.absfreq_series_ref import absfreq_frame, lds_bytes, lds_form, packet_values
from tests.cond_series_ref import omega_of

pytestmark = pytest.mark.gpu

NX, L, F, CG = 32, 2 * np.pi, 3.0, 1.0
FB = 20
BUMP = 1e-10
NALL = 4099
TAU = 0.37
DT = 0.05 * (L / NX) / 0.3


def _psi(seed):
    """A random smooth streamfunction with |U| of about 0.3."""
    rng = np.random.default_rng(seed)
    xs = np.arange(NX) * (L / NX)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    psi = np.zeros((NX, NX))
    for m in range(-3, 4):
        for n in range(0, 4):
            if (m, n) == (0, 0):
                continue
            psi += rng.standard_normal() / (1.0 + m * m + n * n) * np.cos(m * X + n * Y + rng.uniform(0, 2 * np.pi))
    gx, gy = np.gradient(psi, L / NX)
    return psi * (0.3 / np.sqrt(gx * gx + gy * gy).max())


@pytest.fixture(scope="module")
def state():
    rng = np.random.default_rng(52)
    x = rng.uniform(-L / 2, L / 2, (NALL, 2))
    th = rng.uniform(0, 2 * np.pi, NALL)
    k = (np.sqrt(135.0) * (1.0 + 0.3 * rng.standard_normal(NALL)))[:, None] * np.stack([np.cos(th), np.sin(th)], axis=1)
    psis = [_psi(61), _psi(62)]
    assert not np.array_equal(psis[0], psis[1])
    for a in (x, k, *psis):
        a.setflags(write=False)
    return dict(x=x, k=k, psi=psis, w=omega_of(k, F, CG))


def _fields(c, st, slots=(0, 1)):
    """psi[0] into slots[0] (the flow at alpha = 0), psi[1] into slots[1]."""
    for s, psi in zip(slots, st["psi"]):
        c.set_field_psi(s, psi, NX, L)


def _record_of(c, slot, x):
    """(u, v) of ``slot`` at x: swrt_eval(nslots = 1) with the slot in place 0."""
    if slot != 0:
        c.swap_slots(0, slot)
    try:
        out = c.eval(x[:, 0], x[:, 1], nslots=1, bump=BUMP)
    finally:
        if slot != 0:
            c.swap_slots(0, slot)
    return np.array(out[:2])


def _want(c, x, k, slots, alpha, tau, wedges, oedges, fb=FB):
    A = _record_of(c, slots[0], x)
    B = _record_of(c, slots[1], x) if slots[1] >= 0 else None
    return absfreq_frame(A, B, alpha, tau, k, F, CG, wedges, oedges, fb)


def _pct_edges(v, nb):
    lo, hi = np.percentile(v[np.isfinite(v)], [10.0, 90.0])
    return np.linspace(lo, hi, nb + 1)


def _edges(st, nw, no):
    """omega edges over the packets' omega; Omega edges over the same range (the
    Doppler shift |U.k| <= 0.3 * |k| is a fraction of it)."""
    return _pct_edges(st["w"], nw), _pct_edges(st["w"] + 1.0, no)


def _begin(c, wedges, oedges, fb=FB):
    c.absfreq_series_begin(F, CG, wedges, oedges, fb)


def _equal(got, want, what=""):
    for g, w, name in zip(got, want, ("counts", "sums", "stats")):
        assert np.asarray(g).dtype == np.int64
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _frame(got, i):
    return [a[i] for a in got]


def _shape_boundary(no):
    """The last LDS-form shape and the first global-form shape with ``no``
    Omega classes: computed from the rule, not written down."""
    nw = max(w for w in range(1, 4097) if lds_form(w, no))
    assert lds_form(nw, no) and not lds_form(nw + 1, no) and (no + 2) * (nw + 3) <= 65536
    return (nw, no), (nw + 1, no)


SHAPES = [(1, 1), (3, 2), (300, 8)]  # (nw, no)


@pytest.mark.parametrize("nw,no", SHAPES)
@pytest.mark.parametrize("n", [1, 63, 257, 1000, 4099])
def test_device_against_the_restatement(ctx, state, n, nw, no):
    """One packet, a partial wave, more than one workgroup, a grid stride: two
    snapshots at alpha 0, 0.3 and 1 with tau 0.37 and -0.37."""
    c, st = ctx, state
    _fields(c, st)
    x, k = st["x"][:n], st["k"][:n]
    c.packets_set(x, k)
    wedges, oedges = _edges(st, nw, no)
    _begin(c, wedges, oedges)
    cases = [(0.0, TAU), (0.3, TAU), (1.0, TAU), (0.3, -TAU)]
    for alpha, tau in cases:
        c.absfreq_series_record(0, 1, alpha, tau, BUMP)
    got = c.absfreq_series_get()
    assert got[0].shape == (4, no + 2, nw + 2) and got[1].shape == (4, 3 * (nw + 2) + 2 * (no + 2))
    A, B = _record_of(c, 0, x), _record_of(c, 1, x)
    for i, (alpha, tau) in enumerate(cases):
        want = absfreq_frame(A, B, alpha, tau, k, F, CG, wedges, oedges, FB)
        assert want[2].tolist() == [n, 0] and want[0].sum() == n
        if n == NALL:
            for axis in (0, 1):
                row = want[0].sum(axis=axis)
                assert row[0] > 0 and row[-1] > 0 and 2 * np.count_nonzero(row[1:-1]) >= row.size - 2, row
            assert np.count_nonzero(want[1]) > (nw + 2 + no + 2) // 2
        _equal(_frame(got, i), want, f"n {n} ({nw}, {no}) alpha {alpha} tau {tau}")
    # a negative tau turns the sign of every Omega-dot and leaves the rest
    nws = nw + 2
    np.testing.assert_array_equal(got[1][3][:nws], -got[1][1][:nws])
    np.testing.assert_array_equal(got[1][3][nws:3 * nws], got[1][1][nws:3 * nws])


@pytest.fixture()
def actx(ctx):
    """The session context with the path key back at 0 afterwards."""
    yield ctx
    ctx.debug_set(DEBUG_ABSFREQ_GLOBAL, 0)


def test_path_boundary(actx, state):
    """The last LDS shape and the first global one by the 80 KB rule; the
    forced global kernel gives the LDS kernel's integers, frac_bits 0 and 32
    included; a tail that alone outgrows the LDS form's share."""
    c, st = actx, state
    _fields(c, st)
    x, k = st["x"], st["k"]
    c.packets_set(x, k)
    A, B = _record_of(c, 0, x), _record_of(c, 1, x)
    # with 2 Omega classes the 80 KB rule ends the LDS form (the plane is far below 16384 cells, the kernel asks
    # for more than 64 KB); with 126 the cell limit does
    for no_, by_bytes in ((2, True), (126, False)):
        (nw, no), (nw2, no2) = _shape_boundary(no_)
        print(f"last LDS shape ({nw}, {no}): {lds_bytes(nw, no, True)} B; first global ({nw2}, {no2})")
        assert ((no2 + 2) * (nw2 + 2) <= 16384 and lds_bytes(nw, no, True) <= 80 << 10 < lds_bytes(nw2, no2, True)) \
            == by_bytes
        if by_bytes:  # (the kernel has to ask for its dynamic LDS limit)
            assert lds_bytes(nw, no, True) > 64 << 10
        for fb in (0, FB, 32) if by_bytes else (FB,):
            wedges, oedges = _edges(st, nw, no)
            want = absfreq_frame(A, B, 0.3, TAU, k, F, CG, wedges, oedges, fb)
            _begin(c, wedges, oedges, fb)
            for forced in (0, 1):
                c.debug_set(DEBUG_ABSFREQ_GLOBAL, forced)
                assert c.debug_get(DEBUG_ABSFREQ_GLOBAL) == forced
                c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
            c.debug_set(DEBUG_ABSFREQ_GLOBAL, 0)
            got = c.absfreq_series_get()
            _equal(_frame(got, 0), _frame(got, 1), f"({nw}, {no}) frac_bits {fb}: LDS against global")
            _equal(_frame(got, 0), want, f"({nw}, {no}) frac_bits {fb}")
        wedges, oedges = _edges(st, nw2, no2)
        _begin(c, wedges, oedges)
        c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
        _equal(_frame(c.absfreq_series_get(), 0), absfreq_frame(A, B, 0.3, TAU, k, F, CG, wedges, oedges, FB),
               f"({nw2}, {no2})")
    for nwt, not_ in ((4096, 1), (13, 4096)):  # the tail alone is 128 KB / 96 KB: one workgroup a CU
        assert not lds_form(nwt, not_) and lds_bytes(nwt, not_, False) > 64 << 10
        wedges, oedges = _edges(st, nwt, not_)
        _begin(c, wedges, oedges)
        c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
        _equal(_frame(c.absfreq_series_get(), 0), absfreq_frame(A, B, 0.3, TAU, k, F, CG, wedges, oedges, FB),
               f"({nwt}, {not_})")
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG"):
        c.debug_set(DEBUG_ABSFREQ_GLOBAL, 2)


def test_other_slots(fresh_ctx, state):
    """Slots (3, 1) instead of (0, 1): the same frame; the two swapped is the
    frame at 1 - alpha with -tau's rates."""
    c, st = fresh_ctx, state
    x, k = st["x"][:1000], st["k"][:1000]
    wedges, oedges = _edges(st, 12, 8)
    _fields(c, st, (0, 1))
    c.packets_set(x, k)
    _begin(c, wedges, oedges)
    c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
    ref = _frame(c.absfreq_series_get(), 0)
    _fields(c, st, (3, 1))
    c.set_field_psi(0, 2.0 * st["psi"][0], NX, L)  # (slot 0 now holds something else)
    c.absfreq_series_reset()
    c.absfreq_series_record(3, 1, 0.3, TAU, BUMP)
    got = _frame(c.absfreq_series_get(), 0)
    _equal(got, ref, "slots (3, 1) against (0, 1)")
    _equal(got, _want(c, x, k, (3, 1), 0.3, TAU, wedges, oedges), "slots (3, 1)")
    c.absfreq_series_record(1, 3, 0.3, TAU, BUMP)
    _equal(_frame(c.absfreq_series_get(), 1), _want(c, x, k, (1, 3), 0.3, TAU, wedges, oedges), "slots (1, 3)")


def test_two_layer_period(fresh_ctx, state):
    """The two-layer drivers' snapshots (ny_period = 2 nx) and packets with y
    in the upper period."""
    c, st = fresh_ctx, state
    _fields(c, st)
    planes = [np.array(c.get_field_grid(s)) for s in (0, 1)]
    for s in (0, 1):
        c.set_field_grid(s, planes[s], NX, L, 2 * NX)
    x = st["x"][:1000].copy()
    x[:, 1] += L  # y in [L/2, 3L/2): the upper period
    k = st["k"][:1000]
    c.packets_set(x, k)
    wedges, oedges = _edges(st, 12, 8)
    _begin(c, wedges, oedges)
    c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
    want = _want(c, x, k, (0, 1), 0.3, TAU, wedges, oedges)
    assert want[2].tolist() == [1000, 0] and np.count_nonzero(want[1]) > 10
    _equal(_frame(c.absfreq_series_get(), 0), want, "ny_period 2 nx")


def test_one_snapshot(ctx, state):
    """slot_b = -1: the rate sums are all zero and the counts are the
    two-snapshot counts at alpha = 0; alpha and tau are ignored."""
    c, st = ctx, state
    _fields(c, st)
    x, k = st["x"], st["k"]
    c.packets_set(x, k)
    wedges, oedges = _edges(st, 12, 8)
    _begin(c, wedges, oedges)
    c.absfreq_series_record(0, -1, 0.7, 0.0, BUMP)  # (tau 0 is no error here)
    c.absfreq_series_record(0, 1, 0.0, TAU, BUMP)
    c.absfreq_series_record(1, -1, np.nan, np.inf, BUMP)
    c.absfreq_series_record(0, 1, 1.0, TAU, BUMP)
    got = c.absfreq_series_get()
    nws = 14
    for one, two, slot in ((0, 1, 0), (2, 3, 1)):
        np.testing.assert_array_equal(got[0][one], got[0][two])
        np.testing.assert_array_equal(got[2][one], got[2][two])
        assert not got[1][one][:2 * nws].any() and not got[1][one][3 * nws:].any()
        np.testing.assert_array_equal(got[1][one][2 * nws:3 * nws], got[1][two][2 * nws:3 * nws])
        assert got[1][two][:nws].any()
        _equal(_frame(got, one), _want(c, x, k, (slot, -1), 0.0, 1.0, wedges, oedges), f"slot {slot} alone")


def test_planted_packets(actx, state):
    """A NaN k, k = 0 (accepted), an omega beyond 2^38 / S and an |Omega-dot|
    beyond 2^38 / S from a large k: stats[1] is the number planted as
    rejectable, on both paths, and the restatement agrees."""
    c, st = actx, state
    _fields(c, st)
    x, k = st["x"][:1000].copy(), st["k"][:1000].copy()
    k[3] = [np.nan, 1.0]
    k[4] = [0.0, 0.0]
    k[5] = [1e9, 0.0]      # omega = 1e9 > 2^18
    # omega = 1.5e5 and |D| <= 0.3 * 1.5e5 stay below 2^18; |Omega-dot| = |vt| * 1.5e5 with |vt| = |dv| / 0.05, at
    # the grid node where v = d psi / dx differs most between the snapshots (the others' |Omega-dot| is of
    # order |dU| |k| / 0.05 ~ 100, its square far below 2^18)
    dv = np.gradient(st["psi"][1] - st["psi"][0], L / NX, axis=0)
    i, j = np.unravel_index(np.argmax(np.abs(dv)), dv.shape)
    assert abs(dv[i, j]) > 0.2
    x[6] = [i * (L / NX), j * (L / NX)]
    k[6] = [0.0, 1.5e5]
    tau = 0.05
    c.packets_set(x, k)
    A, B = _record_of(c, 0, x), _record_of(c, 1, x)
    w, Om, D, Od = packet_values(A, B, 0.3, tau, k, F, CG)
    assert w[6] * 2.0 ** FB < 2.0 ** 38 and abs(D[6]) * 2.0 ** FB < 2.0 ** 38 and abs(Om[6]) * 2.0 ** FB < 2.0 ** 38
    assert abs(Od[6]) * 2.0 ** FB > 2.0 ** 38  # rejected for its rate alone
    wedges, oedges = _edges(st, 12, 8)
    want = absfreq_frame(A, B, 0.3, tau, k, F, CG, wedges, oedges, FB)
    assert want[2].tolist() == [1000, 3] and want[0].sum() == 997
    assert want[0][:, 1].sum() >= 1 or want[0][:, 0].sum() >= 1  # k = 0 sits at omega = f, in or below the first bin
    _begin(c, wedges, oedges)
    for forced in (0, 1):
        c.debug_set(DEBUG_ABSFREQ_GLOBAL, forced)
        c.absfreq_series_record(0, 1, 0.3, tau, BUMP)
    got = c.absfreq_series_get()
    for i in (0, 1):
        assert got[2][i].tolist() == [1000, 3]
        _equal(_frame(got, i), want, f"forced {i}")
    # the packet with k = 0 alone: accepted, w = f, D = 0
    c.packets_set(x[4:5], k[4:5])
    c.absfreq_series_reset()
    c.absfreq_series_record(0, 1, 0.3, tau, BUMP)
    counts, sums, stats = _frame(c.absfreq_series_get(), 0)
    assert stats.tolist() == [1, 0] and counts.sum() == 1 and not sums.any()


def test_rebinning_and_contexts_do_not_change_a_frame(state):
    """An advance between set and record (the packets re-binned, stored in
    another order) against never re-binning, a fresh context given the advanced
    packets, and the restatement."""
    st = state
    wedges, oedges = _edges(st, 12, 8)
    frames = {}
    for rebin in (4, 0):
        c = sw.Context(0)
        try:
            _fields(c, st)
            c.set_locality(rebin, 0)
            c.packets_set(st["x"], st["k"])
            _begin(c, wedges, oedges)
            states_ = []
            for steps in (10, 3):
                c.advance(DT, steps, F, CG ** 2, nslots=2, alpha0=0.05, dalpha=0.1, bump=BUMP)
                c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
                states_.append(c.packets_get())
            got = c.absfreq_series_get()
            for i, (x, k) in enumerate(states_):
                _equal(_frame(got, i), _want(c, x, k, (0, 1), 0.3, TAU, wedges, oedges), f"rebin {rebin} record {i}")
        finally:
            c.close()
        assert not np.array_equal(got[1][0], got[1][1])
        frames[rebin] = got
        if rebin == 4:  # a fresh context given the advanced packets
            f = sw.Context(0)
            try:
                _fields(f, st)
                f.packets_set(*states_[1])
                _begin(f, wedges, oedges)
                f.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
                _equal(_frame(f.absfreq_series_get(), 0), _frame(got, 1), "fresh context")
            finally:
                f.close()
    _equal(frames[4], frames[0], "re-binned against never re-binned")


def test_packet_streams_do_not_change_a_frame(state):
    """One packet stream against two (65,536 packets: the tile launches
    split) give equal frames."""
    st = state
    wedges, oedges = _edges(st, 12, 8)
    rng = np.random.default_rng(32)
    xb, kb = orc.initial_packets(65536, L, 4.0, F, CG, rng)
    kb = kb * (1.0 + 0.3 * rng.standard_normal((65536, 1)))
    frames = []
    for streams in (2, 1):
        c = sw.Context(0)
        try:
            c.set_packet_streams(streams)
            _fields(c, st)
            c.packets_set(xb, kb)
            c.advance(DT, 5, F, CG ** 2, nslots=2, alpha0=0.1, dalpha=0.2, bump=BUMP)
            _begin(c, wedges, oedges)
            c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
            frames.append(c.absfreq_series_get())
        finally:
            c.close()
    assert frames[0][2][0].tolist() == [65536, 0] and frames[0][0].sum() == 65536
    _equal(frames[1], frames[0], "one packet stream against two")


def test_consistency_with_the_ray_diagnostics(fresh_ctx, state):
    """Without the restatement: tau * sum(qO) / S against the change of
    swrt_raydiag_sample's Omega (gH = Cg^2) from alpha = 0 to alpha = 1, the
    omega marginal against swrt_omega_series_record's row, and sum(qD) / S
    against sum(Omega - omega).

    Bounds (derived, not measured).  Per packet qO / S is within the
    quantisation half-step 2^-(frac_bits + 1) of Od, and tau * Od, Omega_b -
    Omega_a and Omega - omega each come from a handful (< 16) of fp64 operations
    on numbers no larger than Omega_max, each within 2^-52 * Omega_max: n
    packets give n * (|tau| * 2^-(frac_bits + 1) + 16 * 2^-52 * Omega_max), and
    n * (2^-(frac_bits + 1) + 16 * 2^-52 * Omega_max) for the Doppler sum."""
    c, st = fresh_ctx, state
    _fields(c, st)
    x, k = st["x"], st["k"]
    n = NALL
    c.packets_set(x, k)
    Oa = c.raydiag_sample(F, CG * CG, nslots=2, alpha=0.0, bump=BUMP)[0][:, 0]
    Ob = c.raydiag_sample(F, CG * CG, nslots=2, alpha=1.0, bump=BUMP)[0][:, 0]
    Omax = max(np.abs(Oa).max(), np.abs(Ob).max())
    wedges = _pct_edges(st["w"], 12)
    wide = np.array([-1e4, 0.0, 1e4])  # every Omega inside
    nws = 14
    S = 2.0 ** FB
    for tau in (TAU, -TAU):
        _begin(c, wedges, wide)
        c.absfreq_series_record(0, 1, 0.0, tau, BUMP)
        c.absfreq_series_record(0, 1, 1.0, tau, BUMP)
        counts, sums, stats = c.absfreq_series_get()
        assert stats.tolist() == [[n, 0], [n, 0]] and counts[:, [0, 3]].sum() == 0
        qO = int(sums[0][:nws].sum())
        assert qO == int(sums[0][3 * nws:3 * nws + 4].sum()) == int(sums[1][:nws].sum())  # (the rate ignores alpha)
        lhs, rhs = tau * qO / S, float(np.sum(Ob - Oa))
        bound = n * (abs(tau) * 2.0 ** -(FB + 1) + 16 * 2.0 ** -52 * Omax)
        print(f"tau {tau}: tau * sum qO / S = {lhs!r}, sum(Omega_b - Omega_a) = {rhs!r}, |diff| {abs(lhs - rhs):.3e}, "
              f"bound {bound:.3e}")
        assert abs(lhs - rhs) <= bound
        for i, O in ((0, Oa), (1, Ob)):
            qD = int(sums[i][2 * nws:3 * nws].sum())
            rhs = float(np.sum(O - st["w"]))
            bound = n * (2.0 ** -(FB + 1) + 16 * 2.0 ** -52 * Omax)
            print(f"alpha {i}: sum qD / S = {qD / S!r}, sum(Omega - omega) = {rhs!r}, |diff| {abs(qD / S - rhs):.3e}, "
                  f"bound {bound:.3e}")
            assert abs(qD / S - rhs) <= bound
    # the marginal over the Omega classes is the spectrum series' row
    c.omega_series_begin(F, CG, wedges)
    c.omega_series_record()
    row = c.omega_series()[0][0]
    np.testing.assert_array_equal(counts[0].sum(axis=0), row)
    np.testing.assert_array_equal(counts[1].sum(axis=0), row)


def test_record_history(fresh_ctx, state):
    """One frame per history frame of a short advance (8 steps, save_every 2)
    with per-frame alphas: the bits of a record on packets set to that frame."""
    c, st = fresh_ctx, state
    _fields(c, st)
    c.packets_set(st["x"][:1000], st["k"][:1000])
    c.history_reset()
    c.advance(DT, 8, F, CG ** 2, nslots=2, alpha0=0.05, dalpha=0.1, bump=BUMP, save_every=2)
    hx, hk = c.history()
    count = 4
    assert hx.shape[0] == count
    alphas = np.array([0.2, 0.4, 0.6, 0.8])
    wedges, oedges = _edges(st, 12, 8)
    _begin(c, wedges, oedges)
    c.absfreq_series_record_history(0, count, 0, 1, alphas, TAU, BUMP)
    assert c.absfreq_series_frames() == count
    hist = c.absfreq_series_get()
    c.absfreq_series_record_history(0, count, 1, -1, None, 0.0, BUMP)  # one snapshot: no alphas
    one = c.absfreq_series_get(count, count)
    for i in range(count):
        x, k = np.ascontiguousarray(hx[i].T), np.ascontiguousarray(hk[i].T)
        c.packets_set(x, k)
        c.absfreq_series_reset()
        c.absfreq_series_record(0, 1, alphas[i], TAU, BUMP)
        c.absfreq_series_record(1, -1, 0.0, 0.0, BUMP)
        rec = c.absfreq_series_get()
        _equal(_frame(rec, 0), _frame(hist, i), f"record on frame {i}")
        _equal(_frame(rec, 1), _frame(one, i), f"record on frame {i}, one snapshot")
        _equal(_frame(rec, 0), _want(c, x, k, (0, 1), alphas[i], TAU, wedges, oedges), f"history frame {i}")
    assert len({a.tobytes() for a in hist[1]}) == count  # the frames differ


def test_series_life(fresh_ctx, state):
    """Reset keeps the edges, begin empties, another N drops the frames."""
    c, st = fresh_ctx, state
    _fields(c, st)
    wedges, oedges = _edges(st, 1, 1)
    c.packets_set(st["x"][:1], st["k"][:1])
    _begin(c, wedges, oedges)
    for _ in range(3):
        c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
    assert c.absfreq_series_frames() == 3 and c.absfreq_series_bins() == (1, 1)
    counts, sums, stats = c.absfreq_series_get()
    assert (counts == counts[0]).all() and (sums == sums[0]).all() and (stats == [1, 0]).all()
    part = c.absfreq_series_get(1, 2)
    assert part[0].shape == (2, 3, 3) and part[1].shape == (2, 15)
    i64 = ctypes.POINTER(ctypes.c_int64)
    only = [np.zeros_like(a[:2]) for a in (counts, sums, stats)]
    for j in range(3):  # each output alone
        args = [only[i].ctypes.data_as(i64) if i == j else None for i in range(3)]
        assert c._L.swrt_absfreq_series_get(c._h, 1, 2, *args) == 0
    _equal(only, [a[1:] for a in (counts, sums, stats)], "single outputs")
    c.absfreq_series_reset()
    assert c.absfreq_series_frames() == 0 and c.absfreq_series_bins() == (1, 1)
    assert c.absfreq_series_get()[0].shape == (0, 3, 3)
    c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)  # the edges stay
    c.packets_set(st["x"][:1], st["k"][:1])  # the same N keeps the frame
    assert c.absfreq_series_frames() == 1
    c.packets_set(st["x"][:300], st["k"][:300])  # another N drops it
    assert c.absfreq_series_frames() == 0 and c.absfreq_series_bins() == (1, 1)
    c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
    _equal(_frame(c.absfreq_series_get(), 0), _want(c, st["x"][:300], st["k"][:300], (0, 1), 0.3, TAU, wedges, oedges),
           "300 packets")
    wedges, oedges = _edges(st, 12, 8)
    _begin(c, wedges, oedges)  # begin again: empty, the new shape
    assert c.absfreq_series_frames() == 0 and c.absfreq_series_bins() == (12, 8)


def test_errors(fresh_ctx, state):
    c, st = fresh_ctx, state
    wedges, oedges = _edges(st, 12, 8)

    def refused(code, call):
        with pytest.raises(sw.SwrtError, match=code) as e:
            call()
        assert c._L.swrt_last_error(c._h), e.value  # a message, not only a code
        return str(e.value)

    refused("SWRT_ERR_STATE.*begin", lambda: c.absfreq_series_record(0, 1, 0.3, TAU, BUMP))
    refused("SWRT_ERR_STATE.*begin", lambda: c.absfreq_series_record_history(0, 0, 0, -1, None, TAU, BUMP))
    assert c.absfreq_series_frames() == 0 and c.absfreq_series_bins() == (0, 0)
    big = np.arange(301.0)
    refused("SWRT_ERR_ARG.*65536", lambda: c.absfreq_series_begin(F, CG, big + 3, big, FB))  # 302 x 302 cells
    refused("SWRT_ERR_ARG", lambda: c.absfreq_series_begin(F, CG, wedges, oedges[:1], FB))  # no = 0
    refused("SWRT_ERR_ARG.*4096", lambda: c.absfreq_series_begin(F, CG, wedges, np.arange(4098.0), FB))
    refused("SWRT_ERR_ARG.*increase", lambda: c.absfreq_series_begin(F, CG, wedges, oedges[::-1], FB))
    refused("SWRT_ERR_ARG.*frac_bits", lambda: c.absfreq_series_begin(F, CG, wedges, oedges, 33))
    refused("SWRT_ERR_STATE.*begin", lambda: c.absfreq_series_record(0, 1, 0.3, TAU, BUMP))  # a refused begin opens nothing
    _begin(c, wedges, oedges)
    refused("SWRT_ERR_ARG.*slot", lambda: c.absfreq_series_record(0, -1, 0.0, 1.0, BUMP))  # an unset slot
    c.set_field_psi(0, st["psi"][0], NX, L)
    refused("SWRT_ERR_ARG.*slot not set", lambda: c.absfreq_series_record(0, 1, 0.3, TAU, BUMP))  # slot 1 unset
    refused("SWRT_ERR_ARG.*no packets", lambda: c.absfreq_series_record(0, -1, 0.0, 1.0, BUMP))
    c.packets_set(st["x"][:300], st["k"][:300])
    for a, b in ((-1, 0), (5, 0), (0, 5), (0, -2)):
        refused("SWRT_ERR_ARG.*slot out of range", lambda: c.absfreq_series_record(a, b, 0.3, TAU, BUMP))
    refused("SWRT_ERR_ARG.*differ", lambda: c.absfreq_series_record(0, 0, 0.3, TAU, BUMP))  # slot_a == slot_b
    half = st["psi"][1][::2, ::2]
    c.set_field_psi(1, half, NX // 2, L)
    refused("SWRT_ERR_ARG.*grids", lambda: c.absfreq_series_record(0, 1, 0.3, TAU, BUMP))
    c.set_field_psi(1, st["psi"][1], NX, L)
    for tau in (0.0, np.inf, -np.inf, np.nan):
        refused("SWRT_ERR_ARG.*tau", lambda: c.absfreq_series_record(0, 1, 0.3, tau, BUMP))
        refused("SWRT_ERR_ARG.*tau", lambda: c.absfreq_series_record_history(0, 0, 0, 1, None, tau, BUMP))
    c.absfreq_series_record(0, 1, 0.3, -TAU, BUMP)  # a negative tau is allowed
    for first, count in ((-1, 1), (0, 2), (1, 1), (0, -1)):
        refused("SWRT_ERR_ARG.*range", lambda: c.absfreq_series_get(first, count))
    refused("SWRT_ERR_ARG.*history", lambda: c.absfreq_series_record_history(0, 1, 0, -1, None, TAU, BUMP))  # no frames
    c.history_reset()
    c.advance(DT, 2, F, CG ** 2, nslots=2, alpha0=0.0, dalpha=0.5, bump=BUMP, save_every=1)
    for first, count in ((0, 3), (-1, 1), (2, 1)):
        refused("SWRT_ERR_ARG.*history", lambda: c.absfreq_series_record_history(first, count, 0, -1, None, TAU, BUMP))
    with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*alphas"):  # two snapshots need them
        c._chk(c._L.swrt_absfreq_series_record_history(c._h, 0, 2, 0, 1, None, TAU, BUMP), "record_history")
    assert c.absfreq_series_frames() == 1
    c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)  # the open series is still usable
    assert c.absfreq_series_frames() == 2


def test_more_than_2_24_packets_are_refused(fresh_ctx, state):
    """The argument check alone: the packet buffers are never read (the
    records return before any launch)."""
    c, st = fresh_ctx, state
    n = (1 << 24) + 1
    z = np.zeros((n, 2))
    c.packets_set(z, z)
    _fields(c, st)
    _begin(c, *_edges(st, 3, 2))
    for call in (lambda: c.absfreq_series_record(0, 1, 0.3, TAU, BUMP),
                 lambda: c.absfreq_series_record(0, -1, 0.0, 1.0, BUMP)):
        with pytest.raises(sw.SwrtError, match="SWRT_ERR_ARG.*2\\^24"):
            call()
    assert c.absfreq_series_frames() == 0


# ---- the ensemble and the drivers ---------------------------------------------

ABS_FILES = ("absfreq_hist.bin", "absfreq_sums.bin", "absfreq_stats.bin", "absfreq_geom.bin")
SPEC_EDGES = np.linspace(9.0, 15.0, 13)  # the ring starts at omega = 12
O_EDGES = np.linspace(8.0, 16.0, 5)
NP = 512


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


def _watch(monkeypatch, ctx, seen, loops):
    """Every packet frame the driver saves with an absolute-frequency frame
    leaves: the packets on the device, layer 0 of the committed qk and of the
    one before it (the run's pv states either side of the last PDE step), the
    ensemble, and the two-layer loop (its dt)."""
    saved = qgmod._save_frame

    def save(ens, t, *args, **kw):
        if kw.get("absfreq") is not None or (len(args) > 9 and args[9] is not None):
            nh = 2 * ctx._qg_nhalf() + 1
            cur, prev = np.zeros(nh), np.zeros(nh)
            ctx.qg_export(cur, which=0, layer=0)
            ctx.qg_export(prev, which=1, layer=0)
            x, k = ctx.packets_get()
            seen.append(dict(x=np.array(x), k=np.array(k), cur=cur[:-1].copy(), prev=prev[:-1].copy(), ens=ens,
                             dt=loops[-1].dt if loops else None))
        return saved(ens, t, *args, **kw)

    monkeypatch.setattr(qgmod, "_save_frame", save)
    step = qgmod.TwoLayerLoop.step

    def watched_step(self):
        if not loops or loops[-1] is not self:
            loops.append(self)
        return step(self)

    monkeypatch.setattr(qgmod.TwoLayerLoop, "step", watched_step)


def _check_driver(ctx, d, facts, seen, nx, tau_of, fb=20):
    """A frame beside every packet frame but the first.  Each is recomputed
    through the same record call on snapshots rebuilt from the run's PV states
    (slot 0: the one before the last PDE step, slot 1: the one after it), at
    alpha = 1 with tau the last step's dt: all three arrays on the device's
    packets at the frame, and the counts and stats on the written
    packet_x/k.bin frame.  (packet_x.bin holds the positions wrapped into the
    domain: for a packet that left it that is another fp64 number, whose
    interpolated velocity may differ in its last bit, and with it a quantised
    sum by one; the classes do not move.)"""
    no, nw = O_EDGES.size - 1, SPEC_EDGES.size - 1
    frames = facts["packet_frames"] - 1
    assert facts["absfreq_frames"] == frames == len(seen) >= 11
    files = _files(d)
    nsum = 3 * (nw + 2) + 2 * (no + 2)
    assert len(files["absfreq_hist.bin"]) == frames * (no + 2) * (nw + 2) * 8
    assert len(files["absfreq_sums.bin"]) == frames * nsum * 8
    assert len(files["absfreq_stats.bin"]) == frames * 2 * 8
    geom = np.frombuffer(files["absfreq_geom.bin"], dtype=np.float64)
    assert geom.tolist() == [no, nw, fb] + O_EDGES.tolist() + SPEC_EDGES.tolist()
    counts = np.frombuffer(files["absfreq_hist.bin"], dtype=np.int64).reshape(frames, no + 2, nw + 2)
    sums = np.frombuffer(files["absfreq_sums.bin"], dtype=np.int64).reshape(frames, nsum)
    stats = np.frombuffer(files["absfreq_stats.bin"], dtype=np.int64).reshape(frames, 2)
    px = sw.read_field(os.path.join(d, "packet_x"), NP, 2, 1, is_real=True)
    pk = sw.read_field(os.path.join(d, "packet_k"), NP, 2, 1, is_real=True)
    assert px.shape[2] == frames + 1
    ctx.synchronize()
    for i, s in enumerate(seen):
        e = s["ens"]
        for slot, qk in ((0, s["prev"]), (1, s["cur"])):
            ctx.snapshot_qk(slot, qk, nx, e.L, e.K_d2, e.shear, e.k_scale, e.ny_period)
        tau = tau_of(s)
        ctx.absfreq_series_begin(e.f, e.Cg, SPEC_EDGES, O_EDGES, fb)
        ctx.packets_set(s["x"], s["k"])
        ctx.absfreq_series_record(0, 1, 1.0, tau, e.bump)
        assert np.array_equal(pk[:, :, i + 1], s["k"])
        ctx.packets_set(np.ascontiguousarray(px[:, :, i + 1]), np.ascontiguousarray(pk[:, :, i + 1]))
        ctx.absfreq_series_record(0, 1, 1.0, tau, e.bump)
        got = ctx.absfreq_series_get()
        _equal(_frame(got, 0), (counts[i], sums[i], stats[i]), f"driver frame {i}")
        np.testing.assert_array_equal(got[0][1], counts[i], err_msg=f"driver frame {i} on the written frame")
        np.testing.assert_array_equal(got[2][1], stats[i], err_msg=f"driver frame {i} on the written frame")
    rows = sw.read_field(os.path.join(d, "omega_hist"), nw + 2, 1, 1).reshape(nw + 2, frames + 1).T
    print(f"Omega rows {counts.sum(axis=2).tolist()} stats {stats.tolist()}")
    assert (stats[:, 0] == NP).all() and (stats[:, 1] == 0).all()
    np.testing.assert_array_equal(counts.sum(axis=1), rows[1:])
    assert sums[:, :nw + 2].any(axis=1).all()  # every frame has a rate: two snapshots were read
    assert np.count_nonzero(counts.sum(axis=(0, 2))) >= 2  # more than one Omega class is met
    rates = sw.absfreq_rates(counts, sums, stats, fb)
    assert np.isfinite(rates["abs_dot_sq_mean_abs"]).any() and (rates["accepted"] == NP).all()
    log = open(os.path.join(d, "run.log")).read()
    assert log.count("Absolute frequency: 4 classes over [8, 16], quantum 2^-20\n") == 1
    return files


TWO_LAYER = (32, NP, 4.0, 400.0, 0.0, 0.2, 3.0, 1.0)  # (T long enough for 300 PDE steps at 32^2)


@pytest.mark.parametrize("integrator,intervals,tracks", [("leapfrog", 1, False), ("leapfrog", 3, True),
                                                         ("ode23", 1, False)])
def test_two_layer_driver(ctx, tmp_path, monkeypatch, integrator, intervals, tracks):
    """A dozen frames; groups of 1 interval, of up to 3 (the track flushes cut
    them at 1, 2 and 3 intervals before a frame) and the ode23 path with its
    speculative snapshot slot."""
    a = str(tmp_path / "a")
    kw = dict(nsub=2, max_steps=300, seed=5, ctx=ctx, spectrum_edges=SPEC_EDGES, integrator=integrator,
              packet_intervals=intervals)
    if tracks:
        kw.update(track_ids=[0, 1], track_every=7)
    seen, loops = [], []
    _watch(monkeypatch, ctx, seen, loops)
    facts = sw.qg2layersw_raytrace(*TWO_LAYER, out_dir=a, absfreq_edges=O_EDGES, **kw)
    assert facts["steps"] == 300 and facts["packet_frames"] == 13, facts
    fa = _check_driver(ctx, a, facts, seen, 32, lambda s: s["dt"])
    if integrator == "leapfrog" and intervals == 1:
        # with the keyword off: the same files without the four, the same bytes, the same facts
        b = str(tmp_path / "b")
        plain = sw.qg2layersw_raytrace(*TWO_LAYER, out_dir=b, **kw)
        fb = _files(b)
        assert plain["absfreq_frames"] == 0 and not set(ABS_FILES) & set(fb)
        assert {n: v for n, v in fa.items() if n not in ABS_FILES} == fb
        assert {k_: v for k_, v in facts.items() if k_ not in ("absfreq_frames", "dts")} == \
            {k_: v for k_, v in plain.items() if k_ not in ("absfreq_frames", "dts")}
        assert "Absolute frequency" not in open(os.path.join(b, "run.log")).read()


def test_one_layer_driver(ctx, tmp_path, monkeypatch):
    """qgsw_raytrace saves every 5 steps: with packet_intervals = 3 every frame
    follows a group of 2 intervals."""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    args = (32, NP, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0)
    kw = dict(ctx=ctx, max_steps=60, nsub=2, r_drag=0.0, spectrum_edges=SPEC_EDGES, packet_intervals=3)
    seen, loops = [], []
    _watch(monkeypatch, ctx, seen, loops)
    facts = sw.qgsw_raytrace(*args, out_dir=a, absfreq_edges=O_EDGES, **kw)
    assert facts["steps"] == 60 and facts["packet_frames"] == 13, facts
    fa = _check_driver(ctx, a, facts, seen, 32, lambda s: facts["dt"])
    plain = sw.qgsw_raytrace(*args, out_dir=b, **kw)
    fb = _files(b)
    assert plain["absfreq_frames"] == 0 and not set(ABS_FILES) & set(fb)
    assert {n: v for n, v in fa.items() if n not in ABS_FILES} == fb
    # packet_files=False is allowed; another frac_bits moves the sums alone
    seen.clear()
    facts = sw.qgsw_raytrace(*args, out_dir=b, absfreq_edges=O_EDGES, absfreq_frac_bits=8, packet_files=False, **kw)
    fb8 = _files(b)
    assert "packet_x.bin" not in fb8 and facts["absfreq_frames"] == facts["packet_frames"] - 1 == len(seen)
    assert fb8["absfreq_hist.bin"] == fa["absfreq_hist.bin"] and fb8["absfreq_sums.bin"] != fa["absfreq_sums.bin"]


def test_record_absfreq_drains_a_large_series(fresh_ctx, state, tmp_path, monkeypatch):
    """The drain (get, combine, append, reset) at a lowered threshold: the same files as one write at the end."""
    import swraytracing_amd.integrate as integ
    st = state
    wedges, oedges = _edges(st, 7, 4)
    _fields(fresh_ctx, st)
    x, k = st["x"][:1000], st["k"][:1000]

    def run(d, threshold):
        monkeypatch.setattr(integ, "MAP_DRAIN_BYTES", threshold)
        os.makedirs(d)
        ens = sw.PacketEnsemble(x, k, L, F, CG, NX, F / CG, bump=BUMP, ctx=fresh_ctx)
        ens.begin_absfreq(wedges, oedges, FB, directory=d if threshold < 1 << 20 else None)
        for i in range(7):
            fresh_ctx.packets_set(x, k * (1.0 + 0.02 * i))
            if i % 2 == 0:
                ens.record_absfreq(0, 1, 0.3, TAU)
            else:
                ens.record_absfreq(1)  # slot 1 alone
        if threshold >= 1 << 20:
            counts, sums, stats = ens.absfreq_series()
            assert counts.shape == (7, 6, 9) and sums.shape == (7, 39)
            want = _want(fresh_ctx, x, k * (1.0 + 0.02 * 6), (0, 1), 0.3, TAU, wedges, oedges)
            _equal((counts[6], sums[6], stats[6]), want, "the ensemble's last frame")
        assert ens.write_absfreqs(d) == 7
        return _files(d)

    whole = run(str(tmp_path / "whole"), 256 << 20)
    drained = run(str(tmp_path / "drained"), 3 * 8 * (6 * 9 + 39 + 2) - 1)  # drains at every third frame
    assert set(whole) == set(ABS_FILES) and whole == drained
    assert len(whole["absfreq_hist.bin"]) == 7 * 54 * 8 and len(whole["absfreq_sums.bin"]) == 7 * 39 * 8
