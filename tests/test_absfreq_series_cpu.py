"""The absolute-frequency series off the device: the numpy restatement
(tests/absfreq_series_ref.py) on hand-made records (the omega marginal, each
rejection rule hit by one planted packet and no other, the class edges), the
package's host-side pieces (combine_absfreqs, absfreq_rates, the drivers'
argument check) and the names the built library exports."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import swraytracing_amd as sw
from swraytracing_amd import _lib
from swraytracing_amd.qg import _absfreq_args, _absfreq_line
from tests.absfreq_series_ref import absfreq_frame, absfreq_frame_of, hist_slot, lds_bytes, lds_form, packet_values
from tests.cond_series_ref import omega_of

F, CG, FB = 3.0, 1.0, 20
N = 300


@pytest.fixture(scope="module")
def case():
    """300 packets with spread wavevectors and hand-made per-slot (u, v)
    records of an O(0.2) flow that changes by a fifth between the snapshots."""
    rng = np.random.default_rng(91)
    th = rng.uniform(0, 2 * np.pi, N)
    k = (np.sqrt(135.0) * (1.0 + 0.3 * rng.standard_normal(N)))[:, None] * np.stack([np.cos(th), np.sin(th)], axis=1)
    A = 0.2 * rng.standard_normal((2, N))
    B = A + 0.04 * rng.standard_normal((2, N))
    vals = packet_values(A, B, 0.3, 0.37, k, F, CG)
    return dict(k=k, A=A, B=B, vals=vals)


def _edges(v, nb):
    lo, hi = np.percentile(v, [10.0, 90.0])
    return np.linspace(lo, hi, nb + 1)


def _spectrum_row(w, edges):
    """The spectrum series' row: [below, histcounts (last bin closed), above]."""
    return np.concatenate([[np.sum(w < edges[0])], np.histogram(w, edges)[0], [np.sum(w > edges[-1])]])


@pytest.mark.parametrize("nw,no", [(1, 1), (7, 4), (300, 15)])
def test_marginals_and_sums(case, nw, no):
    c = case
    w, Om, D, Od = c["vals"]
    wedges, oedges = _edges(w, nw), _edges(Om, no)
    counts, sums, stats = absfreq_frame(c["A"], c["B"], 0.3, 0.37, c["k"], F, CG, wedges, oedges, FB)
    assert stats.tolist() == [N, 0] and counts.sum() == N
    assert counts.shape == (no + 2, nw + 2) and sums.shape == (3 * (nw + 2) + 2 * (no + 2),)
    np.testing.assert_array_equal(counts.sum(axis=0), _spectrum_row(omega_of(c["k"], F, CG), wedges))
    np.testing.assert_array_equal(counts.sum(axis=1), _spectrum_row(Om, oedges))
    nws, nos = nw + 2, no + 2
    # the Omega classes carry the omega classes' totals of Omega-dot and its square
    assert sums[:nws].sum() == sums[3 * nws:3 * nws + nos].sum() == np.rint(Od * 2.0 ** FB).astype(np.int64).sum()
    assert sums[nws:2 * nws].sum() == sums[3 * nws + nos:].sum() == np.rint((Od * Od) * 2.0 ** FB).astype(np.int64).sum()
    assert sums[2 * nws:3 * nws].sum() == np.rint(D * 2.0 ** FB).astype(np.int64).sum()
    # the operation order, one packet in Python floats
    p = 5
    k1, k2 = (float(v) for v in c["k"][p])
    a0, a1, b0, b1 = (float(v) for v in (c["A"][0, p], c["A"][1, p], c["B"][0, p], c["B"][1, p]))
    oma = 1 - 0.3
    u, v = oma * a0 + 0.3 * b0, oma * a1 + 0.3 * b1
    wp = float(np.sqrt(F * F + (CG * CG) * (k1 * k1 + k2 * k2)))
    assert (w[p], D[p], Om[p]) == (wp, u * k1 + v * k2, wp + (u * k1 + v * k2))
    assert Od[p] == ((b0 - a0) / 0.37) * k1 + ((b1 - a1) / 0.37) * k2


def test_one_snapshot_has_zero_rates(case):
    c = case
    w = c["vals"][0]
    wedges = _edges(w, 7)
    two = absfreq_frame(c["A"], c["B"], 0.0, 0.37, c["k"], F, CG, wedges, [-40.0, 0.0, 40.0], FB)
    one = absfreq_frame(c["A"], None, 0.7, np.nan, c["k"], F, CG, wedges, [-40.0, 0.0, 40.0], FB)
    np.testing.assert_array_equal(one[0], two[0])  # alpha = 0 blends to slot a's bits: 1*a + 0*b
    nws = 9
    assert not one[1][:2 * nws].any() and not one[1][3 * nws:].any() and one[1][2 * nws:3 * nws].any()
    np.testing.assert_array_equal(one[1][2 * nws:3 * nws], two[1][2 * nws:3 * nws])
    assert two[1][:nws].any()


def test_each_rejection_rule_alone():
    """One planted packet per rule; the frame of the eight together rejects
    exactly the six planted as rejectable, and k = 0 is accepted."""
    S, lim = 2.0 ** FB, 2.0 ** 38
    wedges, oedges = np.array([1.0, 10.0, 100.0]), np.array([-1e3, 0.0, 1e3])
    # (k, A, B) with tau = 1, alpha = 0: u = A exactly, Od = (B - A) . k
    good = ([3.0, 4.0], [0.1, 0.2], [0.15, 0.1])
    plant = {
        "NaN k": ([np.nan, 1.0], [0.1, 0.2], [0.1, 0.2]),
        "omega * S alone": ([3e5, 0.0], [-0.25, 0.0], [-0.25, 0.0]),      # w = 3e5 > 2^18, D = -7.5e4, Om = 2.25e5
        "Omega * S alone": ([2e5, 0.0], [0.5, 0.0], [0.5, 0.0]),          # w = 2e5, D = 1e5, Om = 3e5
        "D * S alone": ([2e5, 0.0], [-1.5, 0.0], [-1.5, 0.0]),            # D = -3e5, Om = -1e5
        "Omega-dot * S": ([1e5, 0.0], [0.0, 0.0], [3.0, 0.0]),            # Od = 3e5 (its square too); w, D in range
        "Omega-dot^2 * S alone": ([1e4, 0.0], [0.0, 0.0], [0.1, 0.0]),    # Od = 1e3 < 2^18, Od^2 = 1e6 > 2^18
    }
    assert lim / S == 2.0 ** 18 and 2e5 < 2.0 ** 18 < 3e5 and 1e3 < 2.0 ** 18 < 1e6

    def frame(rows):
        k = np.array([r[0] for r in rows])
        A = np.array([r[1] for r in rows]).T
        B = np.array([r[2] for r in rows]).T
        return absfreq_frame(A, B, 0.0, 1.0, k, F, CG, wedges, oedges, FB), packet_values(A, B, 0.0, 1.0, k, F, CG)

    (counts, sums, stats), _ = frame([good])
    assert stats.tolist() == [1, 0] and counts.sum() == 1 and np.count_nonzero(sums) == 5
    for why, row in plant.items():
        (counts, sums, stats), (w, Om, D, Od) = frame([row])
        assert stats.tolist() == [1, 1], why
        assert counts.sum() == 0 and not sums.any(), why
        with np.errstate(all="ignore"):
            hit = [bool(np.isnan(Om[0]) or np.isnan(Od[0])), not abs(w[0] * S) < lim, not abs(Om[0] * S) < lim,
                   not abs(D[0] * S) < lim, not abs(Od[0] * S) < lim, not (Od[0] * Od[0]) * S < lim]
        want = {"NaN k": [True, True, True, True, True, True],  # (a NaN fails every comparison)
                "omega * S alone": [False, True, False, False, False, False],
                "Omega * S alone": [False, False, True, False, False, False],
                "D * S alone": [False, False, False, True, False, False],
                "Omega-dot * S": [False, False, False, False, True, True],
                "Omega-dot^2 * S alone": [False, False, False, False, False, True]}[why]
        assert hit == want, (why, hit)
    # k = 0 is accepted: w = f, D = 0
    zero = ([0.0, 0.0], [0.3, -0.2], [0.5, 0.1])
    (counts, sums, stats), (w, Om, D, Od) = frame([zero])
    assert stats.tolist() == [1, 0] and w[0] == F and D[0] == 0 and Om[0] == F and Od[0] == 0
    assert counts[2, 1] == 1 and not sums.any()  # omega bin 0 ([1, 10)), Omega bin 1 ([0, 1e3])
    (counts, sums, stats), _ = frame([good, zero] + list(plant.values()))
    assert stats.tolist() == [8, 6] and counts.sum() == 2


def test_class_edges():
    """[below, bins, above], bin i = [e_i, e_i+1), the last bin closed."""
    e = np.array([1.0, 2.0, 4.0])
    v = np.array([0.5, np.nextafter(1.0, 0.0), 1.0, np.nextafter(2.0, 0.0), 2.0, 3.0, 4.0, np.nextafter(4.0, 5.0), 9.0,
                  -np.inf, np.inf, np.nan])
    assert hist_slot(v, e).tolist() == [0, 0, 1, 1, 2, 2, 2, 3, 3, 0, 3, -1]
    # through a frame: Omega = w + D with D = 0 lands where w does
    k = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, np.sqrt(7.0)]])  # w = 3, 5, 4
    z = np.zeros((2, 3))
    w = omega_of(k, F, CG)
    assert w.tolist() == [3.0, 5.0, 4.0]
    counts, _, stats = absfreq_frame(z, z, 0.5, 2.0, k, F, CG, [3.0, 4.0, 5.0], [3.5, 5.0], FB)
    assert stats.tolist() == [3, 0]
    # omega classes: 3 -> bin 0 (class 1), 4 -> bin 1 (class 2), 5 -> the closed last bin (class 2)
    # Omega classes over [3.5, 5]: 3 below (0), 4 and 5 in the bin (1)
    assert counts.tolist() == [[0, 1, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0]]


def test_lds_form_rule():
    assert lds_bytes(300, 8, False) == 8 * (1200 + 24 + 13)
    assert lds_form(126, 126) and (126 + 2) ** 2 == 16384 and not lds_form(127, 126)
    # few Omega rows over thousands of omega classes: the tail alone breaks the 80 KB
    assert (1 + 2) * (4096 + 2) <= 16384 and not lds_form(4096, 1)
    assert lds_bytes(4096, 13, False) == 131488 <= 132 << 10


def test_combine_absfreqs(case):
    c = case
    w, Om = c["vals"][0], c["vals"][1]
    wedges, oedges = _edges(w, 7), _edges(Om, 4)
    whole = absfreq_frame_of(*c["vals"], wedges, oedges, FB)
    part_of = np.random.default_rng(5).integers(0, 3, N)
    parts = []
    for r in range(3):
        fr = absfreq_frame_of(*(v[part_of == r] for v in c["vals"]), wedges, oedges, FB)
        parts.append(tuple(a[None] for a in fr))  # one frame each
    got = sw.combine_absfreqs(parts)
    for g, want in zip(got, whole):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g[0], want)
    one = sw.combine_absfreqs(parts[:1])
    assert one[0].shape == (1, 6, 9) and one[1].shape == (1, 39) and one[2].shape == (1, 2)
    other = tuple(a[None] for a in absfreq_frame_of(*c["vals"], _edges(w, 8), oedges, FB))
    with pytest.raises(ValueError):
        sw.combine_absfreqs([parts[0], other])
    with pytest.raises(ValueError):
        sw.combine_absfreqs([(parts[1][0], parts[1][1][:, :3], parts[1][2])])
    with pytest.raises(ValueError):
        sw.combine_absfreqs([])


def test_absfreq_rates_on_a_hand_made_frame():
    # no = 1, nw = 2: Omega classes [below, bin, above], omega classes [below, b0, b1, above]
    counts = np.array([[0, 1, 0, 0], [0, 2, 4, 0], [0, 1, 0, 0]], dtype=np.int64)
    fb = 4
    sums = np.array([0, 4 * 3 * 16, -4 * 16, 0,          # Omega-dot per omega class: mean 3 in b0 (4 packets), -1 in b1
                     0, 4 * 10 * 16, 4 * 2 * 16 + 8, 0,  # Omega-dot^2: mean 10, 2.125
                     0, -4 * 16 // 2, 4 * 16, 0,         # U.k: mean -0.5, 1
                     32, 6 * 16, -32,                    # Omega-dot per Omega class: sums 2, 6, -2 over 1, 6, 1 packets
                     16, 12 * 16, 8], dtype=np.int64)    # Omega-dot^2 per Omega class: 1, 12, 0.5
    stats = np.array([9, 1], dtype=np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = sw.absfreq_rates(counts[None], sums[None], stats[None], fb)
    assert out["n"][0].tolist() == [0, 4, 4, 0] and out["n_abs"][0].tolist() == [1, 6, 1]
    assert out["accepted"].tolist() == [8.0] == [out["n"][0].sum()] == [out["n_abs"][0].sum()]
    assert out["abs_dot_mean"][0, 1:3].tolist() == [3.0, -1.0]
    assert out["abs_dot_sq_mean"][0, 1:3].tolist() == [10.0, 2.125]
    assert out["doppler_mean"][0, 1:3].tolist() == [-0.5, 1.0]
    for name in ("abs_dot_mean", "abs_dot_sq_mean", "doppler_mean"):
        assert np.isnan(out[name][0, [0, 3]]).all()
    assert out["abs_dot_mean_abs"][0].tolist() == [2.0, 1.0, -2.0]
    assert out["abs_dot_sq_mean_abs"][0].tolist() == [1.0, 2.0, 0.5]
    with warnings.catch_warnings():  # an empty frame: NaN means, no warning
        warnings.simplefilter("error")
        empty = sw.absfreq_rates(np.zeros((3, 4), dtype=np.int64), np.zeros(18, dtype=np.int64),
                                 np.zeros(2, dtype=np.int64), fb)
    assert np.isnan(empty["abs_dot_mean"]).all() and np.isnan(empty["abs_dot_mean_abs"]).all()
    assert empty["accepted"] == 0
    with pytest.raises(ValueError):
        sw.absfreq_rates(counts, sums[:17], stats, fb)
    with pytest.raises(ValueError):
        sw.absfreq_rates(counts, sums, stats[:1], fb)
    with pytest.raises(ValueError):
        sw.absfreq_rates(counts, sums, stats, 33)


def test_driver_arguments():
    spec = np.linspace(3.0, 20.0, 11)
    assert _absfreq_args(None, 20, None) is None and _absfreq_args(None, 20, spec) is None
    edges, fb = _absfreq_args([-1.0, 0.0, 1.0], 12, spec)
    assert edges.tolist() == [-1.0, 0.0, 1.0] and fb == 12
    assert _absfreq_line(edges, fb) == "Absolute frequency: 2 classes over [-1, 1], quantum 2^-12"
    with pytest.raises(ValueError, match="spectrum_edges"):
        _absfreq_args([-1.0, 1.0], 20, None)
    for bad in ([1.0, 0.0], [0.0, 0.0, 1.0], [0.0], [0.0, np.nan], [0.0, np.inf]):
        with pytest.raises(ValueError, match="absfreq_edges"):
            _absfreq_args(bad, 20, spec)
    for bad in (-1, 33, 1.5, True):
        with pytest.raises(ValueError, match="absfreq_frac_bits"):
            _absfreq_args([-1.0, 1.0], bad, spec)
    with pytest.raises(ValueError, match="65536"):
        _absfreq_args(np.arange(4001.0), 20, np.arange(301.0))
    # the drivers refuse before anything runs (no device is touched)
    with pytest.raises(ValueError, match="spectrum_edges"):
        sw.qgsw_raytrace(64, 10, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, absfreq_edges=[-1.0, 1.0])
    with pytest.raises(ValueError, match="absfreq_edges"):
        sw.qg2layersw_raytrace(64, 10, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0, absfreq_edges=[1.0, -1.0], spectrum_edges=spec)
    with pytest.raises(ValueError, match="absfreq_frac_bits"):
        sw.qg2layersw_raytrace(64, 10, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0, absfreq_edges=[-1.0, 1.0],
                               absfreq_frac_bits=40, spectrum_edges=spec)


NAMES = ["swrt_absfreq_series_begin", "swrt_absfreq_series_record", "swrt_absfreq_series_record_history",
         "swrt_absfreq_series_frames", "swrt_absfreq_series_bins", "swrt_absfreq_series_get",
         "swrt_absfreq_series_reset"]


def test_the_library_exports_the_names():
    """The built libswrt.so has every entry point, the ctypes table binds
    them, and Context and the package carry the Python side."""
    path = os.path.join(os.path.dirname(_lib.__file__), "libswrt.so")
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
    bound = sw.load()
    assert bound.swrt_absfreq_series_frames.restype is ctypes.c_int64
    assert len(bound.swrt_absfreq_series_record.argtypes) == 6
    assert len(bound.swrt_absfreq_series_record_history.argtypes) == 8
    for meth in ("begin", "record", "record_history", "frames", "bins", "get", "reset"):
        assert callable(getattr(sw.Context, "absfreq_series_" + meth))
    for meth in ("begin_absfreq", "record_absfreq", "absfreq_series", "write_absfreqs"):
        assert callable(getattr(sw.PacketEnsemble, meth))
    assert _lib.DEBUG_ABSFREQ_GLOBAL == 23
    # the header declares them, with the debug key
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "swrt.h")).read()
    for name in NAMES:
        assert name + "(" in header
    assert "#define SWRT_DEBUG_ABSFREQ_GLOBAL 23" in header
