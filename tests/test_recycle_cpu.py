"""Packet recycling without a GPU: the hash, the numpy restatement of the
contract (tests/recycle_ref.py) on hand-made packets, the shards' combine, the
flux arithmetic and the drivers' argument errors."""
import numpy as np
import pytest

from swraytracing_amd.integrate import combine_recycles, recycle_flux
from swraytracing_amd.qg import qg2layersw_raytrace, qgsw_raytrace
from tests.recycle_ref import mix, omega_of, positions, recycle_event, unit

F, CG, L = 3.0, 1.0, 2 * np.pi


def test_mix_known_answers():
    assert int(mix(0)) == 0xE220A8397B1DCDAF
    assert int(mix(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    assert mix(np.array([0, 0x9E3779B97F4A7C15], dtype=np.uint64)).tolist() == [0xE220A8397B1DCDAF,
                                                                                 0x6E789E6AA1B965F4]


def test_unit_interval_and_distinct_positions():
    """u in [0, 1), and no two of 1e5 (id, generation) pairs share a position."""
    assert unit(np.uint64(0)) == 0.0 and unit(np.uint64(2 ** 64 - 1)) == 1.0 - 2.0 ** -53
    gid, gen = np.meshgrid(np.arange(1000), np.arange(1, 101), indexing="ij")
    px, py = positions(99, gid.ravel(), gen.ravel(), 1.0)
    for u in (px + 0.5, py + 0.5):
        assert u.min() >= 0.0 and u.max() < 1.0
        assert np.unique(u).size == u.size
    assert abs(px.mean()) < 0.01 and abs(py.mean()) < 0.01  # (the mean of 1e5 uniform draws: sigma 0.0009)
    # another seed, another base: other positions
    qx, _ = positions(100, gid.ravel(), gen.ravel(), 1.0)
    rx, _ = positions(99, gid.ravel() + 1000, gen.ravel(), 1.0)
    assert not np.any(qx == px) and not np.any(rx == px)


def _hand_made():
    """Seven packets: below the cut, exactly at it, one ulp below it, well
    above it, a NaN k, k = (1e9, 0), and one more below."""
    kc = 5.0
    cut = float(omega_of(np.array([[kc, 0.0]]), F, CG)[0])
    k = np.array([[1.0, 2.0], [kc, 0.0], [kc, 0.0], [0.0, 9.0], [np.nan, 1.0], [1e9, 0.0], [2.0, -1.0]])
    # the largest k1 whose omega is still below the cut
    lo = kc
    while omega_of(np.array([[lo, 0.0]]), F, CG)[0] >= cut:
        lo = np.nextafter(lo, 0.0)
    k[2, 0] = lo
    x = np.arange(14, dtype=np.float64).reshape(7, 2) / 10.0
    home = np.array([[1.0, 1.0]] * 7) * np.arange(1, 8)[:, None] / 10.0
    return x, k, home, cut


def test_the_restatement_on_hand_made_packets():
    x, k, home, cut = _hand_made()
    w = omega_of(k, F, CG)
    assert w[1] == cut and w[2] < cut  # (exactly at the cut; the largest reachable omega below it)
    assert omega_of(np.array([[np.nextafter(k[2, 0], np.inf), 0.0]]), F, CG)[0] >= cut
    gen = np.zeros(7, dtype=np.int32)
    born = np.array([0, 2, 0, 1, 0, 0, 0], dtype=np.int32)
    fb = 20
    x1, k1, gen1, born1, st = recycle_event(x, k, home, gen, born, 3, F, CG, cut, L, 99, 40, fb)
    assert gen1.tolist() == [0, 1, 0, 1, 0, 0, 0] and born1.tolist() == [0, 3, 0, 3, 0, 0, 0]
    kept = [0, 2, 4, 5, 6]
    np.testing.assert_array_equal(x1[kept].view(np.uint64), x[kept].view(np.uint64))   # (NaN k included: untouched)
    np.testing.assert_array_equal(k1[kept].view(np.uint64), k[kept].view(np.uint64))
    np.testing.assert_array_equal(k1[[1, 3]], home[[1, 3]])
    px, py = positions(99, np.array([41, 43]), np.array([1, 1]), L)
    np.testing.assert_array_equal(x1[[1, 3], 0], px)
    np.testing.assert_array_equal(x1[[1, 3], 1], py)
    assert np.all(np.abs(x1[[1, 3]]) <= L / 2)
    q = lambda v: int(np.rint(v * 2.0 ** fb))
    wh = omega_of(home, F, CG)
    assert st.tolist() == [7, 2, 2, q(w[1]) + q(w[3]), q(wh[1]) + q(wh[3]), (3 - 2) + (3 - 1), 2, 3]
    # the inputs were not changed, and a second event absorbs nothing more
    assert gen.tolist() == [0] * 7
    _, _, gen2, born2, st2 = recycle_event(x1, k1, home, gen1, born1, 4, F, CG, cut, L, 99, 40, fb)
    assert st2.tolist() == [7, 0, 2, 0, 0, 0, 0, 4] and gen2.tolist() == gen1.tolist() and born2.tolist() == born1.tolist()
    # the same packets under a cut one ulp above packet 1's omega: it is kept
    up = recycle_event(x, k, home, gen, born, 3, F, CG, np.nextafter(cut, np.inf), L, 99, 40, fb)
    assert up[2].tolist() == [0, 0, 0, 1, 0, 0, 0] and up[4][1] == 1
    # frac_bits 32: 1e9 still rejected, and omega * 2^32 of the rest fits 2^38
    st32 = recycle_event(x, k, home, gen, born, 1, F, CG, cut, L, 0, 0, 32)[4]
    assert st32[1] == 2 and st32[2] == 2
    # frac_bits 0: 1e9 < 2^38 is representable, hence absorbed, not rejected
    st0 = recycle_event(x, k, home, gen, born, 1, F, CG, cut, L, 0, 0, 0)[4]
    assert st0[1] == 3 and st0[2] == 1


def test_combine_on_a_split_equals_the_whole():
    rng = np.random.default_rng(3)
    n = 600
    k = rng.normal(0, 4.0, (n, 2))
    x = rng.uniform(-L / 2, L / 2, (n, 2))
    home = 0.1 * k
    gen = np.zeros(n, dtype=np.int32)
    born = np.zeros(n, dtype=np.int32)
    cut = float(np.percentile(omega_of(k, F, CG), 70))
    whole = recycle_event(x, k, home, gen, born, 1, F, CG, cut, L, 5, 0, 20)
    assert 0 < whole[4][1] < n
    parts = []
    for lo, hi in ((0, 250), (250, 250), (250, 600)):  # (an empty shard in the middle stands as zeros)
        if hi == lo:
            parts.append(np.zeros((1, 8), dtype=np.int64))
            continue
        p = recycle_event(x[lo:hi], k[lo:hi], home[lo:hi], gen[lo:hi], born[lo:hi], 1, F, CG, cut, L, 5, lo, 20)
        np.testing.assert_array_equal(p[0].view(np.uint64), whole[0][lo:hi].view(np.uint64))
        np.testing.assert_array_equal(p[2], whole[2][lo:hi])
        parts.append(p[4][None, :])
    got = combine_recycles(parts)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, whole[4][None, :])
    bad = [parts[0], parts[2].copy()]
    bad[1][0, 7] = 2
    with pytest.raises(ValueError, match="serial"):
        combine_recycles(bad)
    with pytest.raises(ValueError):
        combine_recycles([])
    with pytest.raises(ValueError):
        combine_recycles([parts[0], np.zeros((2, 8), dtype=np.int64)])


def test_recycle_flux_arithmetic():
    fb = 4
    stats = np.array([[100, 10, 0, 10 * 13 * 16, 10 * 12 * 16, 10, 1, 1],
                      [100, 0, 0, 0, 0, 0, 0, 2],
                      [100, 25, 1, 25 * 14 * 16, 25 * 12 * 16, 60, 3, 3]], dtype=np.int64)
    out = recycle_flux(stats, [1.0, 1.5, 2.5], fb, t0=0.0)
    np.testing.assert_array_equal(out["fraction"], [0.1, 0.0, 0.25])
    np.testing.assert_array_equal(out["energy_out"], [130.0, 0.0, 350.0])
    np.testing.assert_array_equal(out["energy_in"], [120.0, 0.0, 300.0])
    np.testing.assert_array_equal(out["mean_age"][[0, 2]], [1.0, 2.4])
    assert np.isnan(out["mean_age"][1])
    first = recycle_flux(stats, [1.0, 1.5, 2.5], fb)
    assert np.isnan(first["energy_out"][0]) and first["energy_out"][2] == 350.0
    with pytest.raises(ValueError):
        recycle_flux(stats, [1.0, 2.0], fb)
    with pytest.raises(ValueError):
        recycle_flux(stats, [1.0, 1.5, 2.5], 33)


@pytest.mark.parametrize("driver,args", [(qgsw_raytrace, (64, 100, [2.0, 4.0], 20.0, 0.0, 0.2, 3.0, 1.0)),
                                         (qg2layersw_raytrace, (64, 100, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0))])
def test_driver_argument_errors(driver, args, tmp_path):
    """Each is raised before any context is made (there is no device here)."""
    out = dict(out_dir=str(tmp_path))
    with pytest.raises(ValueError, match="omega0"):
        driver(*args, recycle_omega=12.0, **out)  # (the largest ring's omega0 is 4 f = 12: not above it)
    with pytest.raises(ValueError, match="trans_src_edges"):
        driver(*args, recycle_omega=12.3, spectrum_edges=[4.0, 8.0, 12.3], trans_src_edges=[4.0, 8.0, 12.3], **out)
    with pytest.raises(ValueError, match="packets"):
        driver(args[0], 0, *args[2:], recycle_omega=12.3, **out)
    for bad in (dict(recycle_every=0), dict(recycle_seed=-1), dict(recycle_frac_bits=33), dict(recycle_omega=np.nan)):
        with pytest.raises(ValueError):
            driver(*args, **{"recycle_omega": 12.3, **bad}, **out)
    assert not list(tmp_path.iterdir())  # (nothing ran)
