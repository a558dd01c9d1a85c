"""The staged packet step off the device: swrt_integrator_weights (no context,
no GPU call), the bindings, the convergence orders of the numpy restatement
(tests/integrator_ref.py) on the steady case, and the host path of
ode_symplectic(method=...) against the restatement."""
import ctypes
import os

import numpy as np
import pytest

import swraytracing_amd as sw
from oracle import swrt_oracle as orc
from swraytracing_amd import _lib
from swraytracing_amd.integrate import packet_method
from tests import integrator_ref as ref

W1 = 1.3512071919596578
S5 = 0.4144907717943757


@pytest.mark.parametrize("comp,stages", [(None, 1), ("yoshida", 3), ("suzuki", 5)])
def test_weights(comp, stages):
    w, off = sw.integrator_weights(comp)
    assert len(w) == len(off) == stages
    assert np.array_equal(w, w[::-1])  # exactly symmetric
    assert np.array_equal(off, -off[::-1]) and off[stages // 2] == 0.0 and not np.signbit(off[stages // 2])
    total = 0.0
    for v in w:
        total = total + float(v)
    assert abs(total - 1.0) <= 2 * np.spacing(1.0)
    if comp == "yoshida":
        assert w.tolist() == [W1, 1.0 - 2.0 * W1, W1]
        assert off[0] == W1 / 2 - 0.5 and abs(off[0] - 0.1756) < 1e-4
    elif comp == "suzuki":
        assert w.tolist() == [S5, S5, 1.0 - 4.0 * S5, S5, S5]
        assert off[0] == S5 / 2 - 0.5 and off[1] == (S5 + S5 / 2) - 0.5
        assert abs(off[0] + 0.2927) < 1e-4 and abs(off[1] - 0.1217) < 1e-4
    else:
        assert w.tolist() == [1.0] and off.tolist() == [0.0]
    # the integer codes name the same compositions
    w2, off2 = sw.integrator_weights({None: 0, "yoshida": 1, "suzuki": 2}[comp])
    assert np.array_equal(w, w2) and np.array_equal(off, off2)


def test_literals_are_within_an_ulp():
    """The literals against 1/(m - m^(1/3)), the root of g(v) = (m - 1/v)^3 - m (increasing in v),
    in exact rational arithmetic: the root lies between each literal's two neighbouring doubles."""
    from fractions import Fraction

    for lit, m in ((W1, 2), (S5, 4)):
        lo, hi = Fraction(float(np.nextafter(lit, 0.0))), Fraction(float(np.nextafter(lit, 2.0)))
        assert (m - 1 / lo) ** 3 - m < 0 < (m - 1 / hi) ** 3 - m


def test_bad_arguments_raise():
    with pytest.raises(sw.SwrtError):
        sw.integrator_weights(3)
    with pytest.raises(ValueError):
        sw.integrator_weights("ruth")
    L = _lib.load()
    w = np.zeros(5)
    n = ctypes.c_int(0)
    assert L.swrt_integrator_weights(1, None, _lib._p(w), ctypes.byref(n)) == 1  # SWRT_ERR_ARG
    assert L.swrt_set_integrator(None, 0, 1, 0) == 1 and L.swrt_get_integrator(None, None, None, None) == 1
    with pytest.raises(ValueError):
        packet_method("rk4")
    with pytest.raises(ValueError):
        packet_method("midpoint", 5)
    with pytest.raises(ValueError):
        packet_method("leapfrog", 2)
    assert packet_method("leapfrog") == ("euler", 1, None) and packet_method("midpoint") == ("midpoint", 2, None)
    assert packet_method("yoshida4") == ("midpoint", 4, "yoshida") and packet_method("suzuki4", 3) == ("midpoint", 3, "suzuki")


def test_header_and_bindings():
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "swrt.h")).read()
    L = _lib.load()
    for name in ("swrt_set_integrator", "swrt_get_integrator", "swrt_integrator_weights"):
        assert f"int {name}(" in header
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    doc = header[header.index("The packet step of swrt_advance"):header.index("int swrt_set_integrator(")]
    assert "ode_symplectic.m:18-21" in doc and "ode_symplectic.m:39-53" in doc
    for order in ("Order 1", "Order 2", "order 4"):
        assert order in doc
    for m in ("set_integrator", "get_integrator", "integrator_weights"):
        assert hasattr(sw.Context, m)


@pytest.fixture(scope="module")
def orders():
    """max|r| of the restatement on the steady case: T = 2 at dt = 0.2, 0.1, 0.05."""
    c = ref.steady_case()
    flow = ref.grid_flow(c["snap"])
    e = {}
    for name, kick, it, comp in (("euler", 0, 1, None), ("midpoint", 1, 2, None), ("yoshida", 1, 4, "yoshida")):
        w, off = sw.integrator_weights(comp)
        for dt, n in ((0.2, 10), (0.1, 20), (0.05, 40)):
            e[name, dt] = ref.omega_error(c["x0"], c["k0"], dt, n, ref.F, ref.GH, flow, w, off, kick, it)
    return e


def test_orders_of_the_restatement(orders):
    e = orders
    for name in ("euler", "midpoint", "yoshida"):
        print(name, [e[name, dt] for dt in (0.2, 0.1, 0.05)])
    assert 1.7 <= e["euler", 0.2] / e["euler", 0.1] <= 2.4     # first order
    assert e["midpoint", 0.2] / e["midpoint", 0.1] >= 3.5       # second
    assert e["yoshida", 0.2] / e["yoshida", 0.1] >= 10          # fourth, above the interpolation's floor
    assert e["midpoint", 0.05] < e["euler", 0.05] / 20


def test_default_weights_restate_the_oracle_leapfrog():
    """S = 1 with the Euler kick is oracle.leapfrog, bit for bit."""
    c = ref.steady_case(nx=32, npk=16)
    w, off = sw.integrator_weights(None)
    x, k, _, _ = ref.integrate(c["x0"], c["k0"], 0.1, 4, ref.F, ref.GH, ref.grid_flow(c["snap"]), w, off)
    xo, ko, _, _ = orc.leapfrog(c["x0"], c["k0"], 0.1, 4, ref.F, ref.GH, c["snap"], bump=ref.BUMP)
    assert np.array_equal(x, xo) and np.array_equal(k, ko)


@pytest.mark.parametrize("method", ["leapfrog", "midpoint", "yoshida4", "suzuki4"])
def test_host_path_equals_restatement(method):
    c = ref.steady_case(nx=32, npk=16)
    scheme = orc.SpectralSchemeOracle(c["L"], c["nx"], c["psi"], bump=ref.BUMP)
    dt, n = 0.1, 4
    x, k, t = sw.ode_symplectic(c["x0"].T[None], c["k0"].T[None], dt, (n + 1) * dt * (1 + 1e-12), ref.F, ref.GH, scheme,
                                method=method)
    assert x.shape == (n + 1, 2, 16)
    kick, it, comp = packet_method(method)
    w, off = sw.integrator_weights(comp)
    flow = ref.grid_flow(orc.GridField(scheme.fields, scheme.dx), None, ref.BUMP)
    _, _, hx, hk = ref.integrate(c["x0"], c["k0"], dt, n, ref.F, ref.GH, flow, w, off, _lib.KICKS[kick], it, save_every=1)
    assert np.array_equal(x[1:], np.array([a.T for a in hx]))
    assert np.array_equal(k[1:], np.array([a.T for a in hk]))
    if method == "leapfrog":  # ... and the default is the oracle's ode_symplectic
        xo, ko, _ = orc.ode_symplectic(c["x0"].T[None], c["k0"].T[None], dt, (n + 1) * dt * (1 + 1e-12), ref.F, ref.GH, scheme)
        assert np.array_equal(x, xo) and np.array_equal(k, ko)
