"""The host side of the map series (CPU only): the numpy restatement of the
contract (tests/map_series_ref.py) on its own edge cases, and combine_maps,
map_fields and the drivers' argument checks.

Every comparison is exact integer (or exact fp64) equality: the feature has no
tolerance.  Unless a case says otherwise f = 3, Cg = 1, frac_bits = 20."""
import numpy as np
import pytest

import swraytracing_amd as sw
from tests.map_series_ref import edge_positions, map_frame

F, CG, L = 3.0, 1.0, 2 * np.pi


def _packets(n, seed=3, span=40.0, kmax=6.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-span, span, (n, 2))
    th = rng.uniform(0, 2 * np.pi, n)
    r = kmax * rng.random(n)
    return x, np.stack([r * np.cos(th), r * np.sin(th)], axis=1)


@pytest.mark.parametrize("m", [1, 5, 64])
def test_restatement_is_shard_additive(m):
    x, k = _packets(1000)
    whole, ws = map_frame(x, k, L, m, F, CG)
    assert whole[0].sum() == 1000 and ws.tolist() == [1000, 0]
    for cut in (0, 1, 333, 1000):
        a, sa = map_frame(x[:cut], k[:cut], L, m, F, CG)
        b, sb = map_frame(x[cut:], k[cut:], L, m, F, CG)
        np.testing.assert_array_equal(a + b, whole)
        np.testing.assert_array_equal(sa + sb, ws)
    p = np.random.default_rng(4).permutation(1000)
    np.testing.assert_array_equal(map_frame(x[p], k[p], L, m, F, CG)[0], whole)


def test_restatement_places_the_edge_positions():
    m = 8
    e = edge_positions(L)
    # -0.0, 0, L, -L, 3L are the cell 0 (x/dxm is a multiple of m or a signed zero); L/2 the cell m/2;
    # -1e-17: mod gives m - 1e-17*m/L, which rounds to m, raw cell m, wrapped to 0
    want = [0, 0, 0, 0, m // 2, 0, 0]
    for pos, cell in zip(e, want):
        planes, stats = map_frame([[pos, 0.0]], [[1.0, 0.0]], L, m, F, CG)
        assert planes[0, cell, 0] == 1 and planes[0].sum() == 1 and stats.tolist() == [1, 0], pos
        planes, _ = map_frame([[0.3, pos]], [[1.0, 0.0]], L, m, F, CG)
        assert planes[0, 0, cell] == 1 and planes[0].sum() == 1, pos


def test_restatement_moments_and_rejection():
    fb = 20
    x = np.array([[0.1, 0.1]] * 9)
    big = 2.0 ** 18  # |k * 2^20| == 2^38: rejected; just below: kept
    k = np.array([[1.5, -2.25], [np.nan, 0.0], [0.0, np.inf], [big, 0.0], [np.nextafter(big, 0), 0.0],
                  [0.0, -big], [0.0, 0.0], [2.0 ** -21, 3 * 2.0 ** -21], [0.0, 0.0]])
    x[8, 0] = np.nan
    x[6, 1] = -np.inf
    planes, stats = map_frame(x, k, L, 4, F, CG, fb)
    # kept: packets 0, 7 (k = 2^-21 is half a unit: rint to even 0; 3*2^-21 = 1.5 units: 2).  Packet 4's k is
    # in range but its omega ~ 2^18 is not: rejected.
    assert stats.tolist() == [9, 7]
    assert planes[0, 0, 0] == 2 and planes[0].sum() == 2
    w0 = np.sqrt(F * F + CG * CG * (1.5 * 1.5 + 2.25 * 2.25))
    w7 = np.sqrt(F * F + CG * CG * (2.0 ** -42 + 9 * 2.0 ** -42))
    assert planes[1, 0, 0] == int(np.rint(w0 * 2 ** fb)) + int(np.rint(w7 * 2 ** fb))
    assert planes[2, 0, 0] == int(1.5 * 2 ** fb) + 0
    assert planes[3, 0, 0] == -int(2.25 * 2 ** fb) + 2
    # frac_bits 0: whole numbers, half to even
    planes, stats = map_frame([[0.0, 0.0]] * 2, [[0.5, 1.5], [2.5, -0.5]], L, 1, 0.0, 1.0, 0)
    assert planes[:, 0, 0].tolist() == [2, int(np.rint(np.sqrt(2.5))) + int(np.rint(np.sqrt(6.5))), 0 + 2, 2 + 0]


def test_combine_maps():
    x, k = _packets(600, seed=5)
    k[17, 0] = np.nan
    m, T = 6, 3
    whole = [map_frame(x + 0.1 * t, k, L, m, F, CG) for t in range(T)]
    wp, ws = np.stack([p for p, _ in whole]), np.stack([s for _, s in whole])
    parts = []
    for lo, hi in ((0, 250), (250, 600), (600, 600)):  # the last shard is empty: zeros
        fr = [map_frame(x[lo:hi] + 0.1 * t, k[lo:hi], L, m, F, CG) for t in range(T)]
        parts.append((np.stack([p for p, _ in fr]), np.stack([s for _, s in fr])))
    assert not parts[2][0].any() and not parts[2][1].any()
    gp, gs = sw.combine_maps(parts)
    assert gp.dtype == np.int64 and gs.dtype == np.int64
    np.testing.assert_array_equal(gp, wp)
    np.testing.assert_array_equal(gs, ws)
    assert (gs[:, 1] == 1).all()
    with pytest.raises(ValueError):
        sw.combine_maps([])
    with pytest.raises(ValueError):
        sw.combine_maps([parts[0], (parts[1][0][:2], parts[1][1][:2])])


def test_map_fields_exact():
    fb = 20
    x, k = _packets(500, seed=6)
    planes, _ = map_frame(x, k, L, 8, F, CG, fb)
    planes[:, 3, 3] = 0  # an empty cell for sure
    fields = sw.map_fields(planes, fb)
    n = planes[0]
    assert set(fields) == {"n", "energy", "k_mean", "l_mean"} and all(v.dtype == np.float64 for v in fields.values())
    np.testing.assert_array_equal(fields["n"], n)
    full = n > 0
    # energy * 2^frac_bits is the stored integer again: the conversion lost nothing
    np.testing.assert_array_equal((fields["energy"][full] * 2.0 ** fb).astype(np.int64), planes[1][full])
    np.testing.assert_array_equal(fields["k_mean"][full], planes[2][full] / n[full] * 2.0 ** -fb)
    np.testing.assert_array_equal(fields["l_mean"][full], planes[3][full] / n[full] * 2.0 ** -fb)
    for name in ("energy", "k_mean", "l_mean"):
        assert np.isnan(fields[name][~full]).all() and np.isfinite(fields[name][full]).all()
    assert np.isnan(fields["energy"][3, 3])
    # a series (T, 4, m, m) keeps its leading axes
    assert sw.map_fields(np.stack([planes, planes]), fb)["energy"].shape == (2, 8, 8)
    with pytest.raises(ValueError):
        sw.map_fields(planes[:3], fb)
    with pytest.raises(ValueError):
        sw.map_fields(planes, 33)


@pytest.mark.parametrize("kw", [dict(map_cells=0), dict(map_cells=4097), dict(map_cells=2.5), dict(map_cells=True),
                                dict(map_cells=32, map_frac_bits=-1), dict(map_cells=32, map_frac_bits=33)])
def test_drivers_refuse_bad_map_arguments_before_anything_runs(tmp_path, kw):
    with pytest.raises(ValueError, match="map_"):
        sw.qgsw_raytrace(64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path / "a"), max_steps=2, **kw)
    with pytest.raises(ValueError, match="map_"):
        sw.qg2layersw_raytrace(64, 5001, 4.0, 10.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path / "b"), max_steps=2, **kw)
    assert not (tmp_path / "a").exists() and not (tmp_path / "b").exists()
