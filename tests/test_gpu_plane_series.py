"""The four class-plane series (cond, trans, refr, absfreq) open in one
context.  Their host side is shared code (swrt_host_diag.hpp's plane_*
functions over one PlaneSeriesState each), so this covers what the per-series
tests cannot: interleaved records on all four, each with its own raised
dynamic-LDS limit, its own edges and its own staged alphas.

Expected values are the series' restatements (tests/*_ref.py) on the oracle's
interpolation, compared as the per-series tests compare them: exact integer
equality, no tolerance.  The fields are set as six planes, so both sides
gather the same numbers; the absolute-frequency records are swrt_eval's, as in
tests/test_gpu_absfreq_series.py.

Shapes.  cond and trans: nw = 4094 with 2 classes on the second axis, 16384
cells, the LDS form's limit, under 33 KB of edges: about 98 KB of dynamic LDS,
past the 64 KB a kernel gets unasked.  refr and absfreq: 126 x 126 classes,
again 16384 cells, the most their *_lds_form admits (one more class on either
axis is refused); 71672 and 72696 bytes.  The restated byte counts are
asserted below, not assumed."""
import numpy as np
import pytest

from oracle import cbind, swrt_oracle as orc
from tests.absfreq_series_ref import absfreq_frame, lds_bytes as absfreq_lds_bytes, lds_form as absfreq_lds_form
from tests.cond_series_ref import central_edges, cond_frame, omega_of, zeta_edges
from tests.refr_series_ref import a_edges_of, refr_frame
from tests.trans_series_ref import trans_frame_of

pytestmark = pytest.mark.gpu

NX, L, F, CG, UG = 32, 2 * np.pi, 3.0, 1.0, 0.2
N = 300
FB = 20
BUMP = 1e-10
TAU = 0.37
LDS_CELLS = 16384       # kCondLdsCells: the LDS forms' count plane, at most
LDS_UNASKED = 64 << 10  # dynamic LDS a kernel may use without asking
REFR_FORM_BYTES = 80 << 10  # kRefrLdsFormBytes


def _cond_lds_bytes(nw, n2):
    """cond_kernel's LDS form: the two edge arrays, n2 + 2 sums, a word pair
    for the rejected count, the uint32 plane (swrt_cond.hpp)."""
    return 8 * ((nw + 1) + (n2 + 1) + (n2 + 2) + 1) + 4 * (n2 + 2) * (nw + 2)


def _refr_lds_bytes(nw, na):
    """refr_kernel's LDS form (swrt_refr.hpp's refr_lds_bytes)."""
    return 8 * ((nw + 1) + (na + 1) + 3 * (nw + 2) + (na + 2) + 1) + 4 * (na + 2) * (nw + 2)


def _refr_lds_form(nw, na):
    return (na + 2) * (nw + 2) <= LDS_CELLS and _refr_lds_bytes(nw, na) <= REFR_FORM_BYTES


def _equal(got, want, what):
    for g, w, name in zip(got, want, ("counts", "sums", "stats")):
        assert np.asarray(g).dtype == np.int64
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _frame(got, i):
    return [a[i] for a in got]


def test_four_series_in_one_context(fresh_ctx):
    c = fresh_ctx
    # a 32^2 background built as conftest's qg_case builds its 64^2 one; slot 1 is slot 0 scaled
    rng = np.random.default_rng(148)
    K_d2 = F / CG
    q = orc.initial_q(NX, L, UG, K_d2, 5, 8, rng)
    kx_, ky_, K2 = orc.wavenumber_grids(NX)
    flow = orc.grid_U(orc.g2k(q), K_d2, K2, kx_, ky_)
    flows = [flow, {n: 0.8 * np.asarray(v) for n, v in flow.items()}]
    planes = np.asarray(cbind.planes_of(flow))
    dx = L / NX
    dt = 0.05 * dx / np.sqrt(flow["u"] ** 2 + flow["v"] ** 2).max()
    c.set_field_grid(0, planes, NX, L)
    c.set_field_grid(1, 0.8 * planes, NX, L)
    # 300 packets of the initial ring, |k| spread so that omega covers many classes
    x, k = orc.initial_packets(N, L, 4.0, F, CG, rng)
    k = np.ascontiguousarray(k * (1.0 + 0.3 * rng.standard_normal(N))[:, None])
    x = np.ascontiguousarray(x)
    w = omega_of(k, F, CG)
    c.packets_set(x, k)

    big, square = (4094, 2), (126, 126)  # (nw, n2)
    assert (big[1] + 2) * (big[0] + 2) == LDS_CELLS and _cond_lds_bytes(*big) > LDS_UNASKED
    assert 8 * (big[0] + 1 + big[1] + 1) <= 33 << 10
    assert _refr_lds_form(*square) and not _refr_lds_form(127, 126) and not _refr_lds_form(126, 127)
    assert absfreq_lds_form(*square) and not absfreq_lds_form(127, 126) and not absfreq_lds_form(126, 127)
    assert _refr_lds_bytes(*square) == 71672 and absfreq_lds_bytes(*square, True) == 72696
    wbig, wsq = central_edges(w, big[0]), central_edges(w, square[0])
    qedges = zeta_edges(flow, big[1])
    sedges = central_edges(w, big[1])
    aedges = a_edges_of(square[1])
    oedges = central_edges(w + 1.0, square[1])
    src = [w * (1.0 + 0.05 * rng.standard_normal(N)), w * (1.0 + 0.02 * rng.standard_normal(N))]

    c.cond_series_begin(F, CG, wbig, 0, qedges, FB)
    c.trans_series_begin(F, CG, wbig, sedges, FB)
    c.refr_series_begin(F, CG, wsq, aedges, FB)
    c.absfreq_series_begin(F, CG, wsq, oedges, FB)
    assert (c.cond_series_bins(), c.trans_series_bins(), c.refr_series_bins(), c.absfreq_series_bins()) \
        == (big, big, square, square)

    def records_of(xs):
        """(u, v) of slot 0 and of slot 1 at xs: swrt_eval with the slot in place 0."""
        out = []
        for slot in (0, 1):
            if slot:
                c.swap_slots(0, slot)
            try:
                out.append(np.array(c.eval(xs[:, 0], xs[:, 1], nslots=1, bump=BUMP)[:2]))
            finally:
                if slot:
                    c.swap_slots(0, slot)
        return out

    def want(series, xs, ks, nslots, alpha, serial=None):
        if series == "cond":
            return cond_frame(flows, nslots, alpha, xs, ks, dx, BUMP, F, CG, wbig, 0, qedges, FB)
        if series == "trans":
            return trans_frame_of(src[serial - 1], omega_of(ks, F, CG), wbig, sedges, FB, serial)
        if series == "refr":
            return refr_frame(flows, nslots, alpha, xs, ks, dx, BUMP, F, CG, wsq, aedges, FB)
        A, B = records_of(xs)
        return absfreq_frame(A, B if nslots == 2 else None, alpha, TAU, ks, F, CG, wsq, oedges, FB)

    # one frame on each, one snapshot; then one more on each in the reverse order, two snapshots at 0.3
    c.trans_series_mark_values(src[0])
    c.cond_series_record(1, 0.0, BUMP)
    c.trans_series_record()
    c.refr_series_record(1, 0.0, BUMP)
    c.absfreq_series_record(0, -1, 0.0, 1.0, BUMP)
    c.trans_series_mark_values(src[1])
    c.absfreq_series_record(0, 1, 0.3, TAU, BUMP)
    c.refr_series_record(2, 0.3, BUMP)
    c.trans_series_record()
    c.cond_series_record(2, 0.3, BUMP)
    got = dict(cond=c.cond_series_get(), trans=c.trans_series_get(), refr=c.refr_series_get(),
               absfreq=c.absfreq_series_get())
    assert (c.cond_series_frames(), c.trans_series_frames(), c.refr_series_frames(), c.absfreq_series_frames()) \
        == (2, 2, 2, 2)
    for series, frames in got.items():
        for i, (nslots, alpha) in enumerate(((1, 0.0), (2, 0.3))):
            wanted = want(series, x, k, nslots, alpha, serial=i + 1)
            print(f"{series} frame {i}: stats {wanted[2].tolist()}, cells met {np.count_nonzero(wanted[0])}")
            assert wanted[2][0] == N and wanted[2][1] == 0 and np.count_nonzero(wanted[0]) > 50
            _equal(_frame(frames, i), wanted, f"{series} frame {i}")

    # three history frames with two snapshots on cond, refr and absfreq in turn: each stages its own alphas
    c.history_reset()
    c.advance(dt, 6, F, CG ** 2, nslots=2, alpha0=0.05, dalpha=0.1, bump=BUMP, save_every=2)
    hx, hk = c.history()
    assert hx.shape[0] == 3
    alphas = dict(cond=np.array([0.2, 0.5, 0.8]), refr=np.array([0.1, 0.4, 0.7]), absfreq=np.array([0.3, 0.6, 0.9]))
    c.cond_series_record_history(0, 3, 2, alphas["cond"], BUMP)
    c.refr_series_record_history(0, 3, 2, alphas["refr"], BUMP)
    c.absfreq_series_record_history(0, 3, 0, 1, alphas["absfreq"], TAU, BUMP)
    hist = dict(cond=c.cond_series_get(2, 3), refr=c.refr_series_get(2, 3), absfreq=c.absfreq_series_get(2, 3))
    assert (c.cond_series_frames(), c.trans_series_frames(), c.refr_series_frames(), c.absfreq_series_frames()) \
        == (5, 2, 5, 5)
    for series, frames in hist.items():
        for i in range(3):
            xs, ks = np.ascontiguousarray(hx[i].T), np.ascontiguousarray(hk[i].T)
            wanted = want(series, xs, ks, 2, alphas[series][i])
            assert wanted[2][0] == N
            _equal(_frame(frames, i), wanted, f"{series} history frame {i}")
    # what the history records left of the earlier frames, trans's included
    for series, get in (("cond", c.cond_series_get), ("trans", c.trans_series_get), ("refr", c.refr_series_get),
                        ("absfreq", c.absfreq_series_get)):
        _equal(get(0, 2), got[series], f"{series} after the history records")
