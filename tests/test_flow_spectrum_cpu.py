"""The flow spectrum series without a GPU: the integer shell rule against the
reference's two masks, the three identities of the numpy restatement
(tests/flow_spectrum_ref.py) against the oracle's grid_U and k2g, the host
helpers and the files QGModel.write_flow_spectrum writes."""
import math

import numpy as np
import pytest

from oracle import swrt_oracle as orc
from tests.flow_spectrum_ref import flow_frame, nshells, shell_of


def test_integer_shell_rule_equals_both_reference_masks():
    """scratch/energy_spectrum.m:11: (j-0.5)^2 <= K2 & K2 < (j+0.5)^2;
    rsw/isospectrum.m:19: floor(K_ + .5) == j, both in doubles on index
    wavenumbers, for every (kx, ky) up to kmax = 511."""
    kmax = 511
    kx, ky = np.meshgrid(np.arange(-kmax, kmax + 1), np.arange(0, kmax + 1), indexing="ij")
    j = shell_of(kx, ky)
    K2 = (kx.astype(np.float64) ** 2 + ky.astype(np.float64) ** 2)
    jf = j.astype(np.float64)
    pos = j > 0
    assert np.array_equal(j == 0, K2 == 0)  # j = 0: the mean mode alone
    assert np.all(((jf - 0.5) ** 2 <= K2)[pos]) and np.all((K2 < (jf + 0.5) ** 2)[pos])
    assert np.array_equal(np.floor(np.sqrt(K2) + .5), jf)
    assert j.max() + 1 == nshells(2 * (kmax + 1))


def test_shell_counts():
    import swraytracing_amd.qg as qg
    assert [nshells(n) for n in (16, 64, 512)] == [11, 45, 362]
    assert [qg.flow_shell_count(n) for n in (8, 16, 64, 512, 4096)] == [nshells(n) for n in (8, 16, 64, 512, 4096)]


@pytest.mark.parametrize("nx,L", [(16, 2 * math.pi), (64, 20.0)])
def test_totals_are_half_the_domain_means(nx, L):
    """sum E = mean(u^2 + v^2)/2, sum Z = mean((v_x - u_y)^2)/2 and
    sum Q = mean(q^2)/2 (q = k2g(qk), the mean included) at 1e-13 relative,
    against the oracle's g2k / grid_U / k2g."""
    rng = np.random.default_rng(nx)
    K_d2 = 3.0
    q = rng.standard_normal((nx, nx)) + 0.3  # (a mean: the (0, 0) mode counts in Q)
    qk = orc.g2k(q)
    scale = L != 2 * math.pi
    k_scale = 2 * math.pi / L if scale else 1.0
    kx_, ky_, K2 = orc.wavenumber_grids(nx, L, scale=scale)
    U = orc.grid_U(qk, K_d2, K2, kx_, ky_)
    spectra, stats = flow_frame(qk, k_scale, K_d2, t=1.25)
    assert spectra.shape == (3, nshells(nx)) and stats[0] == 1.25
    qg = orc.k2g(qk)
    want = [0.5 * np.mean(U["u"] ** 2 + U["v"] ** 2), 0.5 * np.mean((U["vx"] - U["uy"]) ** 2), 0.5 * np.mean(qg ** 2)]
    for got, w in zip(stats[1:], want):
        assert abs(got - w) <= 1e-13 * abs(w), (got, w)
    # the skipped entries (ky = 0, kx < 0) change nothing, whatever they hold
    kmax = nx // 2 - 1
    bad = qk.copy()
    bad[:kmax, 0] = np.nan
    s2, t2 = flow_frame(bad, k_scale, K_d2, t=1.25)
    np.testing.assert_array_equal(s2, spectra)
    np.testing.assert_array_equal(t2, stats)
    # the mean mode sits in shell 0 alone, with weight 1/2
    assert spectra[2, 0] == 0.5 * (qk[kmax, 0].real ** 2 + qk[kmax, 0].imag ** 2)
    assert spectra[0, 0] == 0.0 and spectra[1, 0] == 0.0


def test_den_zero_at_the_mean_mode():
    qk = np.zeros((7, 4), dtype=complex)
    qk[3, 0] = 2.0 - 1.0j
    spectra, stats = flow_frame(qk, 1.0, 0.0)
    assert np.all(np.isfinite(spectra)) and np.all(spectra[:2] == 0.0)
    assert stats[3] == 2.5 and spectra[2, 0] == 2.5


def test_host_helpers():
    import swraytracing_amd as sw
    k = sw.flow_shells(64, 20.0)
    np.testing.assert_array_equal(k, np.arange(45) * (2 * math.pi / 20.0))
    np.testing.assert_array_equal(sw.flow_shells(16, 2 * math.pi), np.arange(11.0))
    spectra = np.arange(2 * 3 * 11, dtype=np.float64).reshape(2, 3, 11)
    stats = np.array([[0.5, 2.0, 8.0, 1.0], [1.5, 4.5, 18.0, 2.0]])
    f = sw.flow_spectrum_fields(spectra, stats, Cg=2.0)
    np.testing.assert_array_equal(f["t"], [0.5, 1.5])
    np.testing.assert_array_equal(f["E"], spectra[:, 0])
    np.testing.assert_array_equal(f["Z"], spectra[:, 1])
    np.testing.assert_array_equal(f["Q"], spectra[:, 2])
    np.testing.assert_array_equal(f["U_rms"], [2.0, 3.0])
    np.testing.assert_array_equal(f["zeta_rms"], [4.0, 6.0])
    np.testing.assert_array_equal(f["Fr"], [1.0, 1.5])
    # the files' flat layout reads the same; Fr only with Cg
    g = sw.flow_spectrum_fields(spectra.reshape(2, 33), stats.ravel())
    np.testing.assert_array_equal(g["Z"], spectra[:, 1])
    assert "Fr" not in g


class _FakeCtx:
    def __init__(self, spectra, stats):
        self.spectra, self.stats = spectra, stats

    def flow_spectrum_get(self):
        return self.spectra.copy(), self.stats.copy()

    def flow_spectrum_shells(self):
        return self.spectra.shape[2]


def test_file_layout(tmp_path):
    import swraytracing_amd.qg as qg
    ns = nshells(16)
    rng = np.random.default_rng(5)
    spectra, stats = rng.random((3, 3, ns)), rng.random((3, 4))
    m = object.__new__(qg.QGModel)
    m.ctx, m.nx, m.nlayers, m.L, m.flow_layer = _FakeCtx(spectra, stats), 16, 2, 20.0, 0
    m.params = qg.QGParams(nlayers=2, L=20.0, K_d2=3.0)
    for name in ("flow_spec", "flow_stats", "flow_geom"):
        (tmp_path / (name + ".bin")).write_bytes(b"stale")
    qg._fresh_outputs(str(tmp_path), True)  # the drivers clear the three names at start
    assert not list(tmp_path.glob("flow_*.bin"))
    assert m.write_flow_spectrum(str(tmp_path), first_time=-0.25) == 3
    got = np.fromfile(tmp_path / "flow_spec.bin").reshape(3, 3, ns)
    np.testing.assert_array_equal(got, spectra)
    st = np.fromfile(tmp_path / "flow_stats.bin").reshape(3, 4)
    np.testing.assert_array_equal(st[:, 1:], stats[:, 1:])
    np.testing.assert_array_equal(st[:, 0], [-0.25, stats[1, 0], stats[2, 0]])  # (the first frame's label)
    assert np.fromfile(tmp_path / "flow_geom.bin").tolist() == [16.0, float(ns), 2.0 * math.pi / 20.0, 3.0, 0.0]
    # frames append (write_field's way); the geometry is one record
    m.write_flow_spectrum(str(tmp_path))
    assert np.fromfile(tmp_path / "flow_stats.bin").size == 24 and np.fromfile(tmp_path / "flow_geom.bin").size == 5
    one = object.__new__(qg.QGModel)
    one.nlayers, one.L = 1, 2 * math.pi
    assert one.kscale == 1.0  # exactly, as QGDev.kscale


def test_driver_keyword_needs_packets():
    import swraytracing_amd.qg as qg
    with pytest.raises(ValueError, match="flow_spectrum"):
        qg._flow_args(True, 0)
    qg._flow_args(False, 0)
    qg._flow_args(True, 5)
