"""The host side of the track series (CPU only): the numpy restatement of a
frame (tests/track_series_ref.py) against hand-computed values, combine_tracks
against plain indexing, and the drivers' argument checks.

The hand-computed case is one Fourier mode, psi = A sin(p x + q y) with
u = -psi_y, v = psi_x.  With s = sin(p x + q y), c = cos(p x + q y):

    u = -A q c,  v = A p c,  u_x = A p q s,  u_y = A q^2 s,
    v_x = -A p^2 s,  v_y = -A p q s

so zeta = v_x - u_y = -A (p^2 + q^2) s, the strain components are
2 A p q s and A (q^2 - p^2) s, hence sigma = A (p^2 + q^2) |s| = |zeta|, and
D = v_y^2 + v_x u_y = A^2 p^2 q^2 s^2 - A^2 p^2 q^2 s^2 = 0.

The packets sit on grid nodes, where the 6 x 6 Lagrange interpolation returns
the node value but for the bump: the offset a = 0 enters the weights as
a + bump, and a weight's slope is below 2 in magnitude, so each of the 36
products is off by at most about 4 * bump relative to the largest node value.
With bump = 1e-13 and |F| <= A (p^2 + q^2) = 0.25 that is below 4e-12 per
field; the four formulas multiply fields of that size by |k| = 3 at most and
add a handful of them: 1e-10 absolute bounds every column with room.
combine_tracks and the NaN frame are compared bit for bit."""
import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import swrt_oracle as orc
from tests.conftest import periodic_grid
from tests.track_series_ref import QUIET_NAN, track_frame

NX, L, F, GH = 64, 2 * np.pi, 3.0, 1.0
DX = L / NX
A, P, Q = 0.05, 1, 2
TOL = 1e-10


def _mode_fields(amp=A):
    X, Y = periodic_grid(NX, L)
    s, c = np.sin(P * X + Q * Y), np.cos(P * X + Q * Y)
    return dict(u=-amp * Q * c, v=amp * P * c, ux=amp * P * Q * s, uy=amp * Q * Q * s, vx=-amp * P * P * s,
                vy=-amp * P * Q * s)


def _node_packets(n, seed=1):
    rng = np.random.default_rng(seed)
    ij = rng.integers(-2 * NX, 3 * NX, (n, 2))  # nodes of several periods: the wrap is part of the case
    th = rng.uniform(0, 2 * np.pi, n)
    return ij * DX, 3.0 * np.stack([np.cos(th), np.sin(th)], axis=1)


def test_restatement_on_one_fourier_mode():
    x, k = _node_packets(200)
    ids = np.array([199, 0, 57, 3, 120])
    fr = track_frame(x, k, ids, [_mode_fields()], 0.0, F, GH, DX, orc.BUMP_SW)
    assert fr.shape == (5, 8)
    np.testing.assert_array_equal(fr[:, 0:2], x[ids])
    np.testing.assert_array_equal(fr[:, 2:4], k[ids])
    xs, ks = x[ids], k[ids]
    ph = P * xs[:, 0] + Q * xs[:, 1]
    s, c = np.sin(ph), np.cos(ph)
    Om = np.sqrt(F * F + GH * (ks ** 2).sum(axis=1)) + (-A * Q * c * ks[:, 0] + A * P * c * ks[:, 1])
    zeta = -A * (P * P + Q * Q) * s
    for name, got, want in (("Omega", fr[:, 4], Om), ("zeta", fr[:, 5], zeta), ("sigma", fr[:, 6], np.abs(zeta)),
                            ("D", fr[:, 7], np.zeros(5))):
        print(f"{name}: largest difference {np.abs(got - want).max():.3e} (bound {TOL:.0e})")
        np.testing.assert_allclose(got, want, rtol=0, atol=TOL, err_msg=name)
    assert np.abs(zeta).max() > 0.1  # the case is not the trivial one


def test_restatement_blends_two_snapshots():
    x, k = _node_packets(50, seed=2)
    ids = np.arange(49, -1, -7)
    f0, f1 = _mode_fields(A), _mode_fields(-2 * A)
    alpha = 0.37
    fr = track_frame(x, k, ids, [f0, f1], alpha, F, GH, DX, orc.BUMP_SW)
    amp = (1 - alpha) * A + alpha * (-2 * A)  # every field is linear in the amplitude
    one = track_frame(x, k, ids, [_mode_fields(amp)], 0.0, F, GH, DX, orc.BUMP_SW)
    np.testing.assert_array_equal(fr[:, 0:4], one[:, 0:4])
    np.testing.assert_allclose(fr[:, 4:8], one[:, 4:8], rtol=0, atol=TOL)
    assert np.abs(fr[:, 5]).max() > 0.01


def test_restatement_without_a_flow_is_the_quiet_nan():
    x, k = _node_packets(10)
    fr = track_frame(x, k, [9, 2], [], 0.0, F, GH, DX, orc.BUMP_SW)
    np.testing.assert_array_equal(fr[:, 0:2], x[[9, 2]])
    np.testing.assert_array_equal(fr[:, 2:4], k[[9, 2]])
    assert (fr[:, 4:8].view(np.uint64) == QUIET_NAN).all()


def test_combine_tracks_three_shards_one_empty_ids_out_of_order():
    n, T = 60, 4
    rng = np.random.default_rng(7)
    whole = rng.standard_normal((T, 8, n))  # the whole ensemble's columns, by original index
    whole[0, 4:8].view(np.uint64)[...] = QUIET_NAN  # a first frame without a flow
    whole[1, 2, 5] = -0.0
    ids = np.array([41, 3, 59, 20, 0, 19, 40, 5])
    bounds = [(0, 20), (20, 20), (20, 60)]  # the middle shard is empty
    parts = []
    for lo, hi in bounds:
        local = ids[(ids >= lo) & (ids < hi)] - lo
        parts.append(whole[:, :, lo:hi][:, :, local])
    assert [p.shape[2] for p in parts] == [4, 0, 4]
    got = sw.combine_tracks(parts, ids, bounds)
    assert got.shape == (T, 8, ids.size) and got.dtype == np.float64
    np.testing.assert_array_equal(got.view(np.uint64), np.ascontiguousarray(whole[:, :, ids]).view(np.uint64))
    # an empty shard may stand as None
    got2 = sw.combine_tracks([parts[0], None, parts[2]], ids, bounds)
    assert got2.tobytes() == got.tobytes()
    with pytest.raises(ValueError):
        sw.combine_tracks(parts[:2], ids, bounds)
    with pytest.raises(ValueError):
        sw.combine_tracks([parts[0], parts[1], parts[2][:2]], ids, bounds)
    with pytest.raises(ValueError):
        sw.combine_tracks(parts, ids, [(0, 20), (20, 20), (20, 50)])  # id 59 is in no shard


BAD = [dict(track_ids=[1.5, 2]), dict(track_ids=2.5), dict(track_ids=True), dict(track_ids=[3, 7, 3]),
       dict(track_ids=[0, 4001]), dict(track_ids=[-1, 5]), dict(track_ids=[]), dict(track_ids=4002),
       dict(track_ids=0), dict(track_ids=[1, 2], track_every=0), dict(track_ids=[1, 2], track_every=-3),
       dict(track_ids=[1, 2], track_every=2.5), dict(track_ids=[1, 2], track_every=True)]


@pytest.mark.parametrize("kw", BAD, ids=[str(b) for b in BAD])
def test_drivers_refuse_bad_track_arguments_before_anything_runs(tmp_path, kw):
    with pytest.raises(ValueError, match="track"):
        sw.qgsw_raytrace(64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path / "a"), max_steps=2, **kw)
    with pytest.raises(ValueError, match="track"):
        sw.qg2layersw_raytrace(64, 4001, 4.0, 10.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path / "b"), max_steps=2, **kw)
    x = np.zeros((4001, 2))
    with pytest.raises(ValueError, match="track"):
        sw.trace_stored(str(tmp_path / "no_such_pv"), 64, x, x, 3.0, 1.0, out_dir=str(tmp_path / "c"), **kw)
    assert not any((tmp_path / d).exists() for d in "abc")


def test_track_count_spreads_the_ids():
    from swraytracing_amd.qg import _track_args
    ids, every = _track_args(4, None, 1002, 5)
    assert ids.tolist() == [0, 250, 500, 750] and ids.dtype == np.int64 and every == 5
    ids, every = _track_args([7, 2], 3, 10, 5)
    assert ids.tolist() == [7, 2] and every == 3
    assert _track_args(None, None, 10, 5) is None
    # packet_files=False still needs a spectrum, tracked or not
    with pytest.raises(ValueError, match="no packet output"):
        sw.qgsw_raytrace(64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir="unused", packet_files=False,
                         track_ids=[1, 2])
