"""ctypes binding of libswrt.so (the C ABI in include/swrt.h).

There is no CPU fallback: if the HIP library is missing or the device call
fails, the error propagates.  Build it with
``python -c "import __graft_entry__ as g; g.build()"`` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

# One HIP runtime per process: torch wheels ship their own libamdhip64.so.7.
# Import torch (if present) before dlopen-ing libswrt so that our NEEDED
# libamdhip64.so.7 resolves to the runtime torch already loaded, instead of a
# second copy from /opt/rocm.
try:  # pragma: no cover - import side effect only
    import torch  # noqa: F401
except Exception:  # torch absent: the system HIP runtime is used
    pass

_HERE = os.path.dirname(os.path.abspath(__file__))
# SWRT_LIB_PATH: alternative build of the same ABI (tuning experiments only)
LIB_PATH = os.environ.get("SWRT_LIB_PATH") or os.path.join(_HERE, "libswrt.so")

SWRT_OK = 0
ERRORS = {1: "SWRT_ERR_ARG", 2: "SWRT_ERR_HIP", 3: "SWRT_ERR_STATE", 4: "SWRT_ERR_ALLOC"}

_D = ctypes.c_double
_I = ctypes.c_int64
_INT = ctypes.c_int
_P = ctypes.POINTER(ctypes.c_double)
_VP = ctypes.c_void_p
_HOOK = ctypes.CFUNCTYPE(None, ctypes.c_void_p)  # void (*)(void*)
_REDUCE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p)  # int (*)(double*, void*)

class QGParams(ctypes.Structure):
    """swrt_qg_params (include/swrt.h)."""
    _fields_ = [("nlayers", ctypes.c_int), ("filter", ctypes.c_int), ("L", _D), ("K_d2", _D), ("beta", _D),
                ("r_drag", _D), ("force_strength", _D), ("f", _D), ("Cg", _D), ("shear", _D), ("nu", _D),
                ("hyper_order", _D), ("r", _D)]


# name -> (restype, argtypes).  Kept in the order of include/swrt.h.
SIGNATURES = {
    "swrt_version": (_INT, []),
    "swrt_create": (_INT, [_INT, ctypes.POINTER(_VP)]),
    "swrt_destroy": (None, [_VP]),
    "swrt_last_error": (ctypes.c_char_p, [_VP]),
    "swrt_set_field_grid": (_INT, [_VP, _INT, _P, _I, _D, _I]),
    "swrt_set_field_psi": (_INT, [_VP, _INT, _P, _I, _D]),
    "swrt_set_field_qk": (_INT, [_VP, _INT, _P, _I, _D, _D, _D, _D, _I]),
    "swrt_set_field_q": (_INT, [_VP, _INT, _P, _I, _D, _D, _D, _D, _I]),
    "swrt_get_field_grid": (_INT, [_VP, _INT, _P]),
    "swrt_get_psi_grid": (_INT, [_VP, _INT, _P]),
    "swrt_field_grid": (_I, [_VP, _INT]),
    "swrt_g2k": (_INT, [_VP, _P, _I, _P]),
    "swrt_k2g": (_INT, [_VP, _P, _I, _P]),
    "swrt_interpolate": (_INT, [_VP, _P, _I, _I, _D, _D, _D, _P, _P, _I, _P]),
    "swrt_eval": (_INT, [_VP, _P, _P, _I, _INT, _D, _D, _P]),
    "swrt_packets_set": (_INT, [_VP, _P, _P, _I]),
    "swrt_packets_get": (_INT, [_VP, _P, _P]),
    "swrt_packets_get_device": (_INT, [_VP, _VP, _VP, ctypes.c_int64]),
    "swrt_packets_count": (_I, [_VP]),
    "swrt_set_locality": (_INT, [_VP, _I, _I]),
    "swrt_set_kernel": (_INT, [_VP, _INT]),
    "swrt_set_gather_mode": (_INT, [_VP, _INT]),
    "swrt_set_sparse_tiles": (_INT, [_VP, _INT]),
    "swrt_set_integrator": (_INT, [_VP, _INT, _INT, _INT]),
    "swrt_get_integrator": (_INT, [_VP, ctypes.POINTER(_INT), ctypes.POINTER(_INT), ctypes.POINTER(_INT)]),
    "swrt_integrator_weights": (_INT, [_INT, _P, _P, ctypes.POINTER(_INT)]),
    "swrt_set_packet_streams": (_INT, [_VP, _INT]),
    "swrt_advance": (_INT, [_VP, _D, _I, _D, _D, _INT, _D, _D, _D, _I]),
    "swrt_advance_intervals": (_INT, [_VP, _INT, _VP, _I, _D, _D, _D, _D, _D, _I]),
    "swrt_history_frames": (_I, [_VP]),
    "swrt_history_get": (_INT, [_VP, _I, _I, _P, _P]),
    "swrt_history_reset": (_INT, [_VP]),
    "swrt_leapfrog": (_INT, [_VP, _P, _P, _I, _D, _I, _D, _D, _INT, _D, _D, _D, _I, _P, _P]),
    "swrt_xka_set_fields": (_INT, [_VP, _P, _I, _D, _D]),
    "swrt_xka_set_rsw": (_INT, [_VP, _P, _I, _D, _D, _D]),
    "swrt_xka_get_fields": (_INT, [_VP, _P]),
    "swrt_xka_grid": (_I, [_VP]),
    "swrt_xka_step": (_INT, [_VP, _P, _I, _D, _D, _D, _I, _I, _P]),
    "swrt_spectral_set_modes": (_INT, [_VP, _P, _I, _I, _D, _D, _D]),
    "swrt_spectral_eval": (_INT, [_VP, _P, _P, _I, _INT, _P]),
    "swrt_spectral_leapfrog": (_INT, [_VP, _P, _P, _I, _D, _I, _D, _D, _INT]),
    "swrt_omega_histogram": (_INT, [_VP, _D, _D, _P, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(_D)]),
    "swrt_omega_series_begin": (_INT, [_VP, _D, _D, _P, _I]),
    "swrt_omega_series_record": (_INT, [_VP]),
    "swrt_omega_series_record_history": (_INT, [_VP, _I, _I]),
    "swrt_omega_series_frames": (_I, [_VP]),
    "swrt_omega_series_bins": (_I, [_VP]),
    "swrt_omega_series_get": (_INT, [_VP, _I, _I, ctypes.POINTER(ctypes.c_int64), _P]),
    "swrt_omega_series_reset": (_INT, [_VP]),
    "swrt_omega_ideal": (_INT, [_VP, _INT, _P, _I, _D, _P, _I, ctypes.POINTER(ctypes.c_int64)]),
    "swrt_map_series_begin": (_INT, [_VP, _D, _I, _D, _D, _INT]),
    "swrt_map_series_record": (_INT, [_VP]),
    "swrt_map_series_record_history": (_INT, [_VP, _I, _I]),
    "swrt_map_series_frames": (_I, [_VP]),
    "swrt_map_series_cells": (_I, [_VP]),
    "swrt_map_series_get": (_INT, [_VP, _I, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "swrt_map_series_reset": (_INT, [_VP]),
    "swrt_kmap_series_begin": (_INT, [_VP, _D, _I, _INT]),
    "swrt_kmap_series_record": (_INT, [_VP]),
    "swrt_kmap_series_record_history": (_INT, [_VP, _I, _I]),
    "swrt_kmap_series_frames": (_I, [_VP]),
    "swrt_kmap_series_cells": (_I, [_VP]),
    "swrt_kmap_series_get": (_INT, [_VP, _I, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "swrt_kmap_series_reset": (_INT, [_VP]),
    "swrt_cond_series_begin": (_INT, [_VP, _D, _D, _P, _I, _INT, _P, _I, _INT]),
    "swrt_cond_series_record": (_INT, [_VP, _INT, _D, _D]),
    "swrt_cond_series_record_history": (_INT, [_VP, _I, _I, _INT, _P, _D]),
    "swrt_cond_series_frames": (_I, [_VP]),
    "swrt_cond_series_bins": (_INT, [_VP, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "swrt_cond_series_get": (_INT, [_VP, _I, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                    ctypes.POINTER(ctypes.c_int64)]),
    "swrt_cond_series_reset": (_INT, [_VP]),
    "swrt_trans_series_begin": (_INT, [_VP, _D, _D, _P, _I, _P, _I, _INT]),
    "swrt_trans_series_mark": (_INT, [_VP]),
    "swrt_trans_series_mark_values": (_INT, [_VP, _P, _I]),
    "swrt_trans_series_record": (_INT, [_VP]),
    "swrt_trans_series_record_history": (_INT, [_VP, _I, _I]),
    "swrt_trans_series_frames": (_I, [_VP]),
    "swrt_trans_series_bins": (_INT, [_VP, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "swrt_trans_series_get": (_INT, [_VP, _I, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                     ctypes.POINTER(ctypes.c_int64)]),
    "swrt_trans_series_reset": (_INT, [_VP]),
    "swrt_refr_series_begin": (_INT, [_VP, _D, _D, _P, _I, _P, _I, _INT]),
    "swrt_refr_series_record": (_INT, [_VP, _INT, _D, _D]),
    "swrt_refr_series_record_history": (_INT, [_VP, _I, _I, _INT, _P, _D]),
    "swrt_refr_series_frames": (_I, [_VP]),
    "swrt_refr_series_bins": (_INT, [_VP, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "swrt_refr_series_get": (_INT, [_VP, _I, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                    ctypes.POINTER(ctypes.c_int64)]),
    "swrt_refr_series_reset": (_INT, [_VP]),
    "swrt_absfreq_series_begin": (_INT, [_VP, _D, _D, _P, _I, _P, _I, _INT]),
    "swrt_absfreq_series_record": (_INT, [_VP, _INT, _INT, _D, _D, _D]),
    "swrt_absfreq_series_record_history": (_INT, [_VP, _I, _I, _INT, _INT, _P, _D, _D]),
    "swrt_absfreq_series_frames": (_I, [_VP]),
    "swrt_absfreq_series_bins": (_INT, [_VP, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "swrt_absfreq_series_get": (_INT, [_VP, _I, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                       ctypes.POINTER(ctypes.c_int64)]),
    "swrt_absfreq_series_reset": (_INT, [_VP]),
    "swrt_tangent_begin": (_INT, [_VP]),
    "swrt_tangent_mark": (_INT, [_VP]),
    "swrt_tangent_get": (_INT, [_VP, _P, ctypes.POINTER(ctypes.c_int32)]),
    "swrt_tangent_end": (_INT, [_VP]),
    "swrt_tangent_live": (_INT, [_VP]),
    "swrt_tangent_serial": (_I, [_VP]),
    "swrt_tangent_series_begin": (_INT, [_VP, _D, _D, _P, _I, _P, _I]),
    "swrt_tangent_series_record": (_INT, [_VP]),
    "swrt_tangent_series_frames": (_I, [_VP]),
    "swrt_tangent_series_bins": (_INT, [_VP, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "swrt_tangent_series_get": (_INT, [_VP, _I, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                       ctypes.POINTER(ctypes.c_int64)]),
    "swrt_tangent_series_reset": (_INT, [_VP]),
    "swrt_recycle_begin": (_INT, [_VP, _D, _D, _D, _D, ctypes.c_uint64, _I, _INT, _P]),
    "swrt_recycle_apply": (_INT, [_VP]),
    "swrt_recycle_frames": (_I, [_VP]),
    "swrt_recycle_get": (_INT, [_VP, _I, _I, ctypes.POINTER(ctypes.c_int64)]),
    "swrt_recycle_state": (_INT, [_VP, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "swrt_recycle_reset": (_INT, [_VP]),
    "swrt_recycle_end": (_INT, [_VP]),
    "swrt_track_begin": (_INT, [_VP, ctypes.POINTER(ctypes.c_int64), _I]),
    "swrt_track_record": (_INT, [_VP, _D, _D, _INT, _D, _D]),
    "swrt_track_record_history": (_INT, [_VP, _I, _I, _D, _D, _INT, _P, _D]),
    "swrt_track_frames": (_I, [_VP]),
    "swrt_track_count": (_I, [_VP]),
    "swrt_track_ids": (_INT, [_VP, ctypes.POINTER(ctypes.c_int64)]),
    "swrt_track_get": (_INT, [_VP, _I, _I, _P]),
    "swrt_track_reset": (_INT, [_VP]),
    "swrt_flow_spectrum_begin": (_INT, [_VP, _I, _D, _D]),
    "swrt_flow_spectrum_record_qg": (_INT, [_VP, _INT]),
    "swrt_flow_spectrum_record_qk": (_INT, [_VP, _P, _I, _D]),
    "swrt_flow_spectrum_frames": (_I, [_VP]),
    "swrt_flow_spectrum_shells": (_I, [_VP]),
    "swrt_flow_spectrum_get": (_INT, [_VP, _I, _I, _P, _P]),
    "swrt_flow_spectrum_reset": (_INT, [_VP]),
    "swrt_raydiag_mark": (_INT, [_VP, _D, _D, _INT, _D, _D]),
    "swrt_raydiag_sample": (_INT, [_VP, _D, _D, _INT, _D, _D, _P, _P]),
    "swrt_raydiag_record": (_INT, [_VP, _D, _D, _INT, _D, _D]),
    "swrt_raydiag_record_history": (_INT, [_VP, _I, _I, _D, _D, _INT, _P, _D]),
    "swrt_raydiag_frames": (_I, [_VP]),
    "swrt_raydiag_series_get": (_INT, [_VP, _I, _I, _P]),
    "swrt_raydiag_series_reset": (_INT, [_VP]),
    "swrt_ode23_f1": (_INT, [_VP, _D, _D, _D, _D, _INT, _D, _D, ctypes.POINTER(_D)]),
    "swrt_ode23_attempt": (_INT, [_VP, _D, _D, _D, _D, _D, _D, _INT, _D, _D, ctypes.POINTER(_D)]),
    "swrt_ode23_accept": (_INT, [_VP]),
    "swrt_ode23_set_dense": (_INT, [_VP, _INT]),
    "swrt_ode23_ntrp": (_INT, [_VP, _D, _D, _P, _I]),
    "swrt_ode23_run": (_INT, [_VP, _D, _D, _D, _D, _D, _INT, _D, _D, _D, _P, _I, ctypes.POINTER(_I),
                              ctypes.POINTER(_I)]),
    "swrt_ode23_run_at": (_INT, [_VP, _P, _I, _D, _D, _D, _INT, _D, _D, _D, _P, _I, ctypes.POINTER(_I),
                                 ctypes.POINTER(_I)]),
    "swrt_ode23_run_hooked": (_INT, [_VP, _D, _D, _D, _D, _D, _INT, _D, _D, _D, _P, _I, ctypes.POINTER(_I),
                                     ctypes.POINTER(_I), _HOOK, _VP]),
    "swrt_ode23_run_sharded": (_INT, [_VP, _D, _D, _D, _D, _D, _INT, _D, _D, _D, _P, _I, ctypes.POINTER(_I),
                                      ctypes.POINTER(_I), _HOOK, _VP, _REDUCE, _VP]),
    "swrt_ode23_chain_next": (_INT, [_VP, _INT, _INT]),
    "swrt_ode23_replay": (_INT, [_D, _D, _D, _D, _INT, _P, _I, _P, _I, ctypes.POINTER(_I), _P, _I,
                                 ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "swrt_qg_init": (_INT, [_VP, ctypes.POINTER(QGParams), _I, _P]),
    "swrt_qg_step": (_INT, [_VP, _D, _I]),
    "swrt_qg_step_speculative": (_INT, [_VP, _D]),
    "swrt_qg_resolve": (_INT, [_VP, _INT]),
    "swrt_qg_set_stream": (_INT, [_VP, _INT]),
    "swrt_qg_set_fused": (_INT, [_VP, _INT]),
    "swrt_qg_max_speed": (_INT, [_VP, ctypes.POINTER(_D)]),
    "swrt_qg_max_speed_async": (_INT, [_VP]),
    "swrt_qg_max_speed_result": (_INT, [_VP, ctypes.POINTER(_D)]),
    "swrt_qg_get": (_INT, [_VP, _P, ctypes.POINTER(_D), ctypes.POINTER(ctypes.c_int64)]),
    "swrt_qg_get_q": (_INT, [_VP, _P]),
    "swrt_qg_grid": (_I, [_VP, ctypes.POINTER(_INT)]),
    "swrt_qg_snapshot": (_INT, [_VP, _INT, _INT, _INT, _I]),
    "swrt_qg_snapshot_speculative": (_INT, [_VP, _INT, _I]),
    "swrt_qg_export": (_INT, [_VP, _INT, _INT, _VP, _INT, _VP, _D]),
    "swrt_snapshot_qk": (_INT, [_VP, _INT, _VP, _INT, _VP, _I, _D, _D, _D, _D, _I]),
    "swrt_swap_slots": (_INT, [_VP, _INT, _INT]),
    "swrt_field_div_free": (_INT, [_VP, _INT]),
    "swrt_check_arith": (_INT, [_VP, _I, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int64)]),
    "swrt_synchronize": (_INT, [_VP]),
    "swrt_get_stream": (_INT, [_VP, ctypes.POINTER(_VP)]),
    "swrt_set_timing": (_INT, [_VP, _INT]),
    "swrt_kernel_time": (_INT, [_VP, _INT, ctypes.POINTER(_D), ctypes.POINTER(_I)]),
    "swrt_clock_stamp": (_INT, [_VP, _INT]),
    "swrt_clock_ghz": (_INT, [_VP, ctypes.POINTER(_D), ctypes.POINTER(_D)]),
    "swrt_clock_ghz_stamps": (_INT, [ctypes.POINTER(ctypes.c_uint64), _I, _D, ctypes.POINTER(_D),
                                     ctypes.POINTER(_D)]),
    "swrt_debug_set": (_INT, [_VP, _INT, _I]),
    "swrt_debug_get": (_INT, [_VP, _INT, ctypes.POINTER(_I)]),
}

# swrt_debug_set / swrt_debug_get keys (include/swrt.h)
DEBUG_HAZARD_CHECK = 1
DEBUG_SPIN_US = 2
DEBUG_LEGACY_PARK = 3
DEBUG_HAZARD_CHECKS = 4
DEBUG_QG_JFUSE = 5
DEBUG_QG_UPDATE_COLS = 7
DEBUG_SHARE_SKEW = 8
DEBUG_CORRUPT_COUNT = 9
DEBUG_ODE23_CHAINED = 10
DEBUG_ODE23_FIRST_TAKEN = 11
DEBUG_ODE23_GUESSES_TAKEN = 12
DEBUG_ODE23_SPLIT_RUNS = 13
DEBUG_ODE23_FIRST_CHAINED = 14
DEBUG_ODE23_DENSE_REBIN = 15
DEBUG_ODE23_DENSE_REBINS = 16
DEBUG_MAP_TILED_FRAMES = 17
DEBUG_MAP_STRAYS = 18
DEBUG_KMAP_GLOBAL = 19
DEBUG_COND_GLOBAL = 20
DEBUG_TRANS_GLOBAL = 21
DEBUG_REFR_GLOBAL = 22
DEBUG_ABSFREQ_GLOBAL = 23
DEBUG_TANGENT_GLOBAL = 24
COND_WHICH = {"zeta": 0, "sigma": 1, "D": 2}  # swrt_cond_series_begin's ``which``
# The class-plane series' tails (PlaneLayout, swrt_packet_state.hpp): sums per
# omega class, sums per class of the second axis, stats words.
PLANE_TAILS = {"cond": (0, 1, 2), "trans": (0, 3, 3), "refr": (3, 1, 2), "absfreq": (3, 2, 2),
               "tangent": (3, 1, 3)}


def plane_sums_shape(prefix, nw, n2):
    """A frame's ``sums`` as ``<prefix>_series_get`` shapes them: flat, per
    omega class first; trans's (ns + 2, 3), its three sums side by side."""
    wsums, csums, _ = PLANE_TAILS[prefix]
    return (n2 + 2, csums) if prefix == "trans" else (wsums * (nw + 2) + csums * (n2 + 2),)

_lib = None


class SwrtError(RuntimeError):
    pass


def device_code_sha256(path=None):
    """sha256 of the device code embedded in a libswrt build (its ELF
    .hip_fatbin section: every gfx950 kernel, none of the host code).  PMC
    records carry it (tools/pmc_merge.py), so counters collected on one
    build are never divided by the launch time of another (bench.py)."""
    import hashlib
    import struct
    with open(path or LIB_PATH, "rb") as fh:
        b = fh.read()
    if b[:4] != b"\x7fELF" or b[4] != 2 or b[5] != 1:
        raise ValueError("not a little-endian ELF64 file")
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)

    def sec(i):
        name, _, _, _, off, size = struct.unpack_from("<IIQQQQ", b, shoff + i * shentsize)
        return name, off, size
    _, stroff, _ = sec(shstrndx)
    for i in range(shnum):
        name, off, size = sec(i)
        end = b.index(b"\0", stroff + name)
        if b[stroff + name:end] == b".hip_fatbin":
            return hashlib.sha256(b[off:off + size]).hexdigest()
    raise ValueError("no .hip_fatbin section")


def load():
    """dlopen libswrt.so (no HIP call is made by loading)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(_P)


KICKS = {"euler": 0, "midpoint": 1}
COMPOSITIONS = {None: 0, "yoshida": 1, "suzuki": 2}


def _code(table, v, what):
    """A setting by name or by its integer code."""
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
        if v not in table:
            raise ValueError(f"{what} must be one of {list(table)}, got {v!r}")
        return table[v]
    return int(v)


def integrator_weights(composition=None):
    """swrt_integrator_weights: (w, off), the stage weights and blend offsets
    of a composition (None, "yoshida", "suzuki" or 0, 1, 2) as the exact
    doubles the device uses.  No context and no GPU call."""
    w, off, n = np.zeros(5), np.zeros(5), _INT(0)
    rc = load().swrt_integrator_weights(_code(COMPOSITIONS, composition, "composition"), _p(w), _p(off),
                                        ctypes.byref(n))
    if rc != SWRT_OK:
        raise SwrtError(f"swrt_integrator_weights: {ERRORS.get(rc, rc)}: unknown composition {composition!r}")
    return w[:n.value].copy(), off[:n.value].copy()


def _f64(a, order="C"):
    return np.require(np.asarray(a, dtype=np.float64), requirements=[order[0] + "_CONTIGUOUS", "ALIGNED"])


class Context:
    """Owns one swrt_ctx (device buffers + HIP stream) on one GPU."""

    def __init__(self, device: int = 0):
        self._L = load()
        h = _VP()
        rc = self._L.swrt_create(int(device), ctypes.byref(h))
        if rc != SWRT_OK:
            raise SwrtError(f"swrt_create(device={device}) failed: {ERRORS.get(rc, rc)}")
        self._h = h
        self.device = device
        self._ode23_cb = self._ode23_hook = self._ode23_raised = None  # ode23_run's hook callback
        self._ode23_red_cb = self._ode23_reduce = None  # ... and its reduce callback (sharded runs)
        self.timing_every = 1  # swrt_set_timing's setting (the library default)

    def close(self):
        if getattr(self, "_h", None):
            self._L.swrt_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != SWRT_OK:
            msg = self._L.swrt_last_error(self._h)
            raise SwrtError(f"{what}: {ERRORS.get(rc, rc)}: {msg.decode() if msg else ''}")

    # ---- fields ---------------------------------------------------------
    def set_field_grid(self, slot, planes6, nx, L, ny_period=0):
        planes6 = _f64(planes6)
        assert planes6.size == 6 * nx * nx
        self._chk(self._L.swrt_set_field_grid(self._h, slot, _p(planes6), nx, float(L), ny_period),
                  "swrt_set_field_grid")

    def set_field_psi(self, slot, psi_grid, nx, L):
        psi = _f64(np.asarray(psi_grid, dtype=np.float64).ravel(order="F"))
        assert psi.size == nx * nx
        self._chk(self._L.swrt_set_field_psi(self._h, slot, _p(psi), nx, float(L)), "swrt_set_field_psi")

    def set_field_qk(self, slot, qk, nx, L, K_d2, shear=0.0, k_scale=1.0, ny_period=0):
        qk = np.asarray(qk, dtype=np.complex128)
        kmax = nx // 2 - 1
        assert qk.shape == (2 * kmax + 1, kmax + 1), qk.shape
        buf = _f64(np.asfortranarray(qk).ravel(order="F").view(np.float64))
        self._chk(self._L.swrt_set_field_qk(self._h, slot, _p(buf), nx, float(L), float(K_d2),
                                            float(shear), float(k_scale), ny_period),
                  "swrt_set_field_qk")

    def set_field_q(self, slot, q, L, K_d2, shear=0.0, k_scale=1.0, ny_period=0):
        """grid_U(g2k(q)) into `slot` from a gridded PV frame (swrt_set_field_q)."""
        q = np.asarray(q, dtype=np.float64)
        nx = q.shape[0]
        if q.shape != (nx, nx):
            raise ValueError("q must be nx x nx")
        buf = _f64(q.ravel(order="F"))
        self._chk(self._L.swrt_set_field_q(self._h, slot, _p(buf), nx, float(L), float(K_d2), float(shear),
                                           float(k_scale), int(ny_period)), "swrt_set_field_q")

    def field_grid(self, slot):
        """nx of field slot `slot` (swrt_field_grid); raises if unset."""
        nx = int(self._L.swrt_field_grid(self._h, int(slot)))
        if nx < 0:
            raise SwrtError(f"field slot {slot} is not set")
        return nx

    def _slot_nx(self, slot, nx):
        have = self.field_grid(slot)
        if nx is not None and int(nx) != have:
            raise ValueError(f"slot {slot} holds a {have}^2 grid, not {nx}^2")
        return have

    def get_field_grid(self, slot, nx=None):
        nx = self._slot_nx(slot, nx)
        out = np.empty(6 * nx * nx)
        self._chk(self._L.swrt_get_field_grid(self._h, slot, _p(out)), "swrt_get_field_grid")
        return out.reshape(6, nx * nx)

    def field_div_free(self, slot=0):
        """True if slot's v_y is exactly -u_x (the packet kernels then carry
        five stencil sums; results are unchanged)."""
        rc = self._L.swrt_field_div_free(self._h, int(slot))
        if rc < 0:
            self._chk(rc, "swrt_field_div_free")
        return rc == 1

    def get_psi_grid(self, slot, nx=None):
        nx = self._slot_nx(slot, nx)
        out = np.empty(nx * nx)
        self._chk(self._L.swrt_get_psi_grid(self._h, slot, _p(out)), "swrt_get_psi_grid")
        return out.reshape((nx, nx), order="F")

    def g2k(self, fg):
        fg = np.asarray(fg, dtype=np.float64)
        nx = fg.shape[0]
        kmax = nx // 2 - 1
        src = _f64(fg.ravel(order="F"))
        out = np.empty(2 * (2 * kmax + 1) * (kmax + 1))
        self._chk(self._L.swrt_g2k(self._h, _p(src), nx, _p(out)), "swrt_g2k")
        return out.view(np.complex128).reshape((2 * kmax + 1, kmax + 1), order="F")

    def k2g(self, fk):
        fk = np.asarray(fk, dtype=np.complex128)
        nx = fk.shape[0] + 1
        src = _f64(np.asfortranarray(fk).ravel(order="F").view(np.float64))
        out = np.empty(nx * nx)
        self._chk(self._L.swrt_k2g(self._h, _p(src), nx, _p(out)), "swrt_k2g")
        return out.reshape((nx, nx), order="F")

    # ---- evaluation -------------------------------------------------------
    def interpolate(self, x, y, F, dx, dy, bump):
        F = np.asarray(F, dtype=np.float64)
        nx = F.shape[0]
        nyF = int(np.prod(F.shape[1:]))
        Fc = _f64(F.reshape(nx, -1, order="F")[:, :nx].ravel(order="F"))
        x = np.asarray(x, dtype=np.float64)
        shape = x.shape
        xf = _f64(x.ravel())
        yf = _f64(np.asarray(y, dtype=np.float64).ravel())
        out = np.empty(xf.size)
        self._chk(self._L.swrt_interpolate(self._h, _p(Fc), nx, nyF, float(dx), float(dy), float(bump),
                                           _p(xf), _p(yf), xf.size, _p(out)), "swrt_interpolate")
        return out.reshape(shape)

    def eval(self, x, y, nslots=1, alpha=0.0, bump=1e-13):
        xf = _f64(np.asarray(x, dtype=np.float64).ravel())
        yf = _f64(np.asarray(y, dtype=np.float64).ravel())
        out = np.empty((6, xf.size))
        self._chk(self._L.swrt_eval(self._h, _p(xf), _p(yf), xf.size, nslots, float(alpha), float(bump),
                                    _p(out)), "swrt_eval")
        return out

    # ---- packets ---------------------------------------------------------
    def packets_set(self, x, k):
        """x, k: N x 2 arrays (converted to column-major)."""
        x = np.asfortranarray(x, dtype=np.float64)
        k = np.asfortranarray(k, dtype=np.float64)
        assert x.shape == k.shape and x.ndim == 2 and x.shape[1] == 2
        self._chk(self._L.swrt_packets_set(self._h, _p(x), _p(k), x.shape[0]), "swrt_packets_set")

    def packets_get(self):
        n = self._L.swrt_packets_count(self._h)
        x = np.empty((n, 2), order="F")
        k = np.empty((n, 2), order="F")
        self._chk(self._L.swrt_packets_get(self._h, _p(x), _p(k)), "swrt_packets_get")
        return x, k

    def packets_count(self):
        return int(self._L.swrt_packets_count(self._h))

    def packets_get_device(self, x_ptr, k_ptr, ld):
        """swrt_packets_get_device: original-order state into device buffers
        (addresses, N x 2 column-major with leading dimension ld) on the
        packet stream, no host sync."""
        self._chk(self._L.swrt_packets_get_device(self._h, ctypes.c_void_p(int(x_ptr)), ctypes.c_void_p(int(k_ptr)),
                                                  int(ld)), "swrt_packets_get_device")

    def set_locality(self, rebin_every=4, tile=0):
        self._chk(self._L.swrt_set_locality(self._h, int(rebin_every), int(tile)), "swrt_set_locality")

    def set_kernel(self, variant=0):
        self._chk(self._L.swrt_set_kernel(self._h, int(variant)), "swrt_set_kernel")

    def set_gather_mode(self, mode=0):
        """swrt_set_gather_mode: 0 bit-exact mul-then-add stencil sums (default),
        1 fused multiply-add (tolerance parity, fewer VALU instructions)."""
        self._chk(self._L.swrt_set_gather_mode(self._h, int(mode)), "swrt_set_gather_mode")

    def set_sparse_tiles(self, mode=0):
        """swrt_set_sparse_tiles: 0 auto (below SWRT_SPARSE_BELOW packets per tile), 1 never, 2 always; same bits."""
        self._chk(self._L.swrt_set_sparse_tiles(self._h, int(mode)), "swrt_set_sparse_tiles")

    def set_integrator(self, kick="euler", iterations=2, composition=None):
        """swrt_set_integrator: the packet step of advance / advance_intervals /
        leapfrog.  kick "euler" (the reference's, first order; the default) or
        "midpoint" (implicit midpoint with `iterations` in 1..4 fixed-point
        passes, second order); composition None, "yoshida" or "suzuki" (fourth
        order over the midpoint kick).  The integer codes are accepted too."""
        self._chk(self._L.swrt_set_integrator(self._h, _code(KICKS, kick, "kick"), int(iterations),
                                              _code(COMPOSITIONS, composition, "composition")),
                  "swrt_set_integrator")

    def get_integrator(self):
        """(kick, iterations, composition) as integer codes (swrt_get_integrator)."""
        k, i, c = _INT(0), _INT(0), _INT(0)
        self._chk(self._L.swrt_get_integrator(self._h, ctypes.byref(k), ctypes.byref(i), ctypes.byref(c)),
                  "swrt_get_integrator")
        return k.value, i.value, c.value

    integrator_weights = staticmethod(integrator_weights)

    def set_packet_streams(self, streams=2):
        """swrt_set_packet_streams: 2 (default: tile launches split over two streams) or 1; same bits."""
        self._chk(self._L.swrt_set_packet_streams(self._h, int(streams)), "swrt_set_packet_streams")

    def advance(self, dt, nsteps, f, gH, nslots=1, alpha0=0.0, dalpha=0.0, bump=1e-13, save_every=0):
        self._chk(self._L.swrt_advance(self._h, float(dt), int(nsteps), float(f), float(gH), int(nslots),
                                       float(alpha0), float(dalpha), float(bump), int(save_every)),
                  "swrt_advance")

    def advance_intervals(self, dts, nsub, f, gH, alpha0=0.0, dalpha=0.0, bump=1e-13, save_every=0):
        """len(dts) PDE intervals of nsub steps, interval i blending slots i, i+1
        (swrt_advance_intervals)."""
        d = np.ascontiguousarray(dts, dtype=np.float64)
        self._chk(self._L.swrt_advance_intervals(self._h, int(d.size), _p(d), int(nsub), float(f), float(gH),
                                                 float(alpha0), float(dalpha), float(bump), int(save_every)),
                  "swrt_advance_intervals")

    def history(self, first=0, count=None):
        n = self._L.swrt_packets_count(self._h)
        total = self._L.swrt_history_frames(self._h)
        count = total - first if count is None else count
        hx = np.empty((count, 2, n))
        hk = np.empty((count, 2, n))
        self._chk(self._L.swrt_history_get(self._h, first, count, _p(hx), _p(hk)), "swrt_history_get")
        return hx, hk

    def history_reset(self):
        self._chk(self._L.swrt_history_reset(self._h), "swrt_history_reset")

    def leapfrog(self, x, k, dt, nsteps, f, gH, nslots=1, alpha0=0.0, dalpha=0.0, bump=1e-13,
                 save_every=0):
        x = np.array(x, dtype=np.float64, order="F")
        k = np.array(k, dtype=np.float64, order="F")
        n = x.shape[0]
        nfr = nsteps // save_every if save_every else 0
        hx = np.empty((nfr, 2, n)) if nfr else None
        hk = np.empty((nfr, 2, n)) if nfr else None
        self._chk(self._L.swrt_leapfrog(self._h, _p(x), _p(k), n, float(dt), int(nsteps), float(f),
                                        float(gH), int(nslots), float(alpha0), float(dalpha),
                                        float(bump), int(save_every) if nfr else 0, _p(hx), _p(hk)),
                  "swrt_leapfrog")
        return x, k, hx, hk

    # ---- wave action (step_packet_xka) -------------------------------------
    def xka_set_fields(self, U, GradU, H, dx, dy):
        nx = np.asarray(H).shape[0]
        planes = _f64(np.stack([np.asarray(a, dtype=np.float64).ravel(order="F") for a in
                                (U["u"], U["v"], GradU["u_x"], GradU["u_y"], GradU["v_x"], GradU["v_y"], H)]))
        self._chk(self._L.swrt_xka_set_fields(self._h, _p(planes), nx, float(dx), float(dy)),
                  "swrt_xka_set_fields")

    def xka_set_rsw(self, S, f, Cg, L=2 * np.pi):
        """Background from an RSW state S = [u v eta] (nx x nx x 3), built on
        the GPU as ray_trace_sw/raytrace_sw.m:16-52 does."""
        S = np.asarray(S, dtype=np.float64)
        if S.ndim != 3 or S.shape[2] != 3 or S.shape[0] != S.shape[1]:
            raise ValueError("S must be nx x nx x 3")
        st = _f64(np.stack([S[:, :, i].ravel(order="F") for i in range(3)]))
        self._chk(self._L.swrt_xka_set_rsw(self._h, _p(st), S.shape[0], float(f), float(Cg), float(L)),
                  "swrt_xka_set_rsw")

    def xka_get_fields(self):
        """The current background as (U, GradU, H) dicts/planes (nx x nx)."""
        nx = int(self._L.swrt_xka_grid(self._h))
        out = np.empty((7, nx * nx))
        self._chk(self._L.swrt_xka_get_fields(self._h, _p(out)), "swrt_xka_get_fields")
        p = [out[i].reshape((nx, nx), order="F") for i in range(7)]
        return ({"u": p[0], "v": p[1]}, {"u_x": p[2], "u_y": p[3], "v_x": p[4], "v_y": p[5]}, p[6])

    def xka_step(self, state, C0, f, dt, nsteps, save_every=0):
        """state: n x 5 [x y k l a]; returns (new state, history frames n x 5 or None)."""
        st = np.array(state, dtype=np.float64, order="F")
        n = st.shape[0]
        nfr = nsteps // save_every if save_every else 0
        hist = np.empty((nfr, 5, n)) if nfr else None
        self._chk(self._L.swrt_xka_step(self._h, _p(st), n, float(C0), float(f), float(dt), int(nsteps),
                                        int(save_every) if nfr else 0, _p(hist)), "swrt_xka_step")
        return st, (None if hist is None else hist.transpose(0, 2, 1))

    # ---- exact spectral evaluator -----------------------------------------
    def spectral_set_modes(self, C, kx0, ky0, s):
        C = np.asarray(C, dtype=np.complex128)
        nkx, nky = C.shape
        buf = _f64(np.asfortranarray(C).ravel(order="F").view(np.float64))
        self._chk(self._L.swrt_spectral_set_modes(self._h, _p(buf), nkx, nky, float(kx0), float(ky0), float(s)),
                  "swrt_spectral_set_modes")

    def spectral_eval(self, x, y, precision=64):
        xf = _f64(np.asarray(x, dtype=np.float64).ravel())
        yf = _f64(np.asarray(y, dtype=np.float64).ravel())
        out = np.empty((6, xf.size))
        self._chk(self._L.swrt_spectral_eval(self._h, _p(xf), _p(yf), xf.size, int(precision), _p(out)),
                  "swrt_spectral_eval")
        return out

    def spectral_leapfrog(self, x, k, dt, nsteps, f, gH, precision=64):
        x = np.array(x, dtype=np.float64, order="F")
        k = np.array(k, dtype=np.float64, order="F")
        self._chk(self._L.swrt_spectral_leapfrog(self._h, _p(x), _p(k), x.shape[0], float(dt), int(nsteps),
                                                 float(f), float(gH), int(precision)), "swrt_spectral_leapfrog")
        return x, k

    # ---- diagnostics (load_data.m) -----------------------------------------
    def omega_histogram(self, f, Cg, edges, counts=None):
        """Add this frame's omega histcounts to `counts` (int64); returns
        (counts, mean omega)."""
        edges = _f64(np.asarray(edges, dtype=np.float64))
        nb = edges.size - 1
        counts = np.zeros(nb, dtype=np.int64) if counts is None else counts
        assert counts.dtype == np.int64 and counts.size == nb and counts.flags["C_CONTIGUOUS"]
        mean = _D()
        self._chk(self._L.swrt_omega_histogram(self._h, float(f), float(Cg), _p(edges), nb,
                                               counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                               ctypes.byref(mean)), "swrt_omega_histogram")
        return counts, mean.value

    # ---- the spectrum series (swrt_omega_series_*, load_data.m:33-52,63) -------
    def omega_series_begin(self, f, Cg, edges):
        """Open a series over ``edges`` (nbins + 1 increasing values); empties it."""
        edges = _f64(np.asarray(edges, dtype=np.float64).ravel())
        self._chk(self._L.swrt_omega_series_begin(self._h, float(f), float(Cg), _p(edges), edges.size - 1),
                  "swrt_omega_series_begin")

    def omega_series_record(self):
        """Append the current packets' frame to the device-side series (queued; no host wait)."""
        self._chk(self._L.swrt_omega_series_record(self._h), "swrt_omega_series_record")

    def omega_series_record_history(self, first, count):
        """One series frame per history frame [first, first + count) (queued; no host wait)."""
        self._chk(self._L.swrt_omega_series_record_history(self._h, int(first), int(count)),
                  "swrt_omega_series_record_history")

    def omega_series_frames(self):
        return int(self._L.swrt_omega_series_frames(self._h))

    def omega_series(self, first=0, count=None):
        """Recorded frames [first, first + count) -> (counts (count, nbins + 2)
        int64 [below, bins, above]; stats (count, 4) [n, sum omega, min, max])."""
        count = self.omega_series_frames() - first if count is None else count
        nslot = int(self._L.swrt_omega_series_bins(self._h)) + 2
        counts = np.zeros((max(count, 0), nslot), dtype=np.int64)
        stats = np.zeros((max(count, 0), 4))
        self._chk(self._L.swrt_omega_series_get(self._h, int(first), int(count),
                                                counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _p(stats)),
                  "swrt_omega_series_get")
        return counts, stats

    def omega_series_reset(self):
        self._chk(self._L.swrt_omega_series_reset(self._h), "swrt_omega_series_reset")

    def omega_ideal(self, slot, ring_k, omega0, edges):
        """ideal_omega_distribution.m:3-11: counts [below, bins, above] of
        omega0 + U_g . k_j over every node g of ``slot`` and every row j of
        ``ring_k`` (m x 2).  Synchronous."""
        ring = np.asarray(ring_k, dtype=np.float64)
        if ring.ndim != 2 or ring.shape[1] != 2:
            raise ValueError("ring_k must be m x 2")
        ring = _f64(np.asfortranarray(ring).ravel(order="F"))
        edges = _f64(np.asarray(edges, dtype=np.float64).ravel())
        counts = np.zeros(edges.size + 1, dtype=np.int64)
        self._chk(self._L.swrt_omega_ideal(self._h, int(slot), _p(ring), ring.size // 2, float(omega0), _p(edges),
                                           edges.size - 1, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
                  "swrt_omega_ideal")
        return counts

    # ---- the map series (swrt_map_series_*: packet density and wave energy) ----
    def map_series_begin(self, L, m, f, Cg, frac_bits=20):
        """Open a series of m x m maps over the periodic square of side ``L``;
        moments quantised to 2^-frac_bits.  Empties the series."""
        self._chk(self._L.swrt_map_series_begin(self._h, float(L), int(m), float(f), float(Cg), int(frac_bits)),
                  "swrt_map_series_begin")

    def map_series_record(self):
        """Append the current packets' map frame to the device-side series (queued; no host wait)."""
        self._chk(self._L.swrt_map_series_record(self._h), "swrt_map_series_record")

    def map_series_record_history(self, first, count):
        """One map frame per history frame [first, first + count) (queued; no host wait)."""
        self._chk(self._L.swrt_map_series_record_history(self._h, int(first), int(count)),
                  "swrt_map_series_record_history")

    def map_series_frames(self):
        return int(self._L.swrt_map_series_frames(self._h))

    def map_series(self, first=0, count=None):
        """Recorded frames [first, first + count) -> (planes (count, 4, m, m)
        int64 [count, sum q(omega), sum q(k), sum q(l)], planes[t, p, i, j] the
        cell with x index i and y index j; stats (count, 2) int64 [n, rejected])."""
        count = self.map_series_frames() - first if count is None else count
        m = int(self._L.swrt_map_series_cells(self._h))
        planes = np.zeros((max(count, 0), 4, m, m), dtype=np.int64)
        stats = np.zeros((max(count, 0), 2), dtype=np.int64)
        i64 = ctypes.POINTER(ctypes.c_int64)
        self._chk(self._L.swrt_map_series_get(self._h, int(first), int(count), planes.ctypes.data_as(i64),
                                              stats.ctypes.data_as(i64)), "swrt_map_series_get")
        return planes.transpose(0, 1, 3, 2), stats  # (the device's planes are column-major)

    def map_series_reset(self):
        self._chk(self._L.swrt_map_series_reset(self._h), "swrt_map_series_reset")

    # ---- the wave-vector plane series (swrt_kmap_series_*: density over (k, l), moments) ----
    def kmap_series_begin(self, K, m, frac_bits=16):
        """Open a series of m x m count planes over [-K, K) x [-K, K) of the
        (k, l) plane; moments quantised to 2^-frac_bits.  Empties the series."""
        self._chk(self._L.swrt_kmap_series_begin(self._h, float(K), int(m), int(frac_bits)),
                  "swrt_kmap_series_begin")

    def kmap_series_record(self):
        """Append the current packets' k-plane frame to the device-side series (queued; no host wait)."""
        self._chk(self._L.swrt_kmap_series_record(self._h), "swrt_kmap_series_record")

    def kmap_series_record_history(self, first, count):
        """One k-plane frame per history frame [first, first + count) (queued; no host wait)."""
        self._chk(self._L.swrt_kmap_series_record_history(self._h, int(first), int(count)),
                  "swrt_kmap_series_record_history")

    def kmap_series_frames(self):
        return int(self._L.swrt_kmap_series_frames(self._h))

    def kmap_series_cells(self):
        return int(self._L.swrt_kmap_series_cells(self._h))

    def kmap_series_get(self, first=0, count=None):
        """Recorded frames [first, first + count) -> (planes (count, m, m)
        int64, planes[t, i, j] the cell with k index i and l index j; stats
        (count, 8) int64 [n, rejected, outside, sum q(k), sum q(l), sum q(k*k),
        sum q(l*l), sum q(k*l)])."""
        count = self.kmap_series_frames() - first if count is None else count
        m = self.kmap_series_cells()
        planes = np.zeros((max(count, 0), m, m), dtype=np.int64)
        stats = np.zeros((max(count, 0), 8), dtype=np.int64)
        i64 = ctypes.POINTER(ctypes.c_int64)
        self._chk(self._L.swrt_kmap_series_get(self._h, int(first), int(count), planes.ctypes.data_as(i64),
                                               stats.ctypes.data_as(i64)), "swrt_kmap_series_get")
        return planes.transpose(0, 2, 1), stats  # (the device's planes are column-major)

    def kmap_series_reset(self):
        self._chk(self._L.swrt_kmap_series_reset(self._h), "swrt_kmap_series_reset")

    # ---- what the four class-plane series (cond, trans, refr, absfreq) share ----
    def _plane_begin(self, prefix, f, Cg, omega_edges, edges2, frac_bits, *own):
        """swrt_<prefix>_series_begin; ``own`` goes between the two edge arrays."""
        wedges = _f64(np.asarray(omega_edges, dtype=np.float64).ravel())
        edges2 = _f64(np.asarray(edges2, dtype=np.float64).ravel())
        name = f"swrt_{prefix}_series_begin"
        self._chk(getattr(self._L, name)(self._h, float(f), float(Cg), _p(wedges), wedges.size - 1, *own,
                                         _p(edges2), edges2.size - 1, int(frac_bits)), name)

    def _plane_bins(self, prefix):
        nw, n2 = ctypes.c_int64(0), ctypes.c_int64(0)
        name = f"swrt_{prefix}_series_bins"
        self._chk(getattr(self._L, name)(self._h, ctypes.byref(nw), ctypes.byref(n2)), name)
        return int(nw.value), int(n2.value)

    def _plane_get(self, prefix, first, count):
        """Frames [first, first + count) -> counts (count, n2 + 2, nw + 2),
        sums (count, *plane_sums_shape) and stats, all int64."""
        if count is None:
            count = int(getattr(self._L, f"swrt_{prefix}_series_frames")(self._h)) - first
        nw, n2 = self._plane_bins(prefix)
        counts = np.zeros((max(count, 0), n2 + 2, nw + 2), dtype=np.int64)
        sums = np.zeros((max(count, 0),) + plane_sums_shape(prefix, nw, n2), dtype=np.int64)
        stats = np.zeros((max(count, 0), PLANE_TAILS[prefix][2]), dtype=np.int64)
        i64 = ctypes.POINTER(ctypes.c_int64)
        name = f"swrt_{prefix}_series_get"
        self._chk(getattr(self._L, name)(self._h, int(first), int(count), counts.ctypes.data_as(i64),
                                         sums.ctypes.data_as(i64), stats.ctypes.data_as(i64)), name)
        return counts, sums, stats

    @staticmethod
    def _history_alphas(alphas, count):
        """record_history's ``alphas`` as the library takes them (None stays)."""
        if alphas is None:
            return None
        alphas = np.ascontiguousarray(alphas, dtype=np.float64)
        if alphas.shape != (int(count),):
            raise ValueError("alphas must hold one value per frame")
        return alphas

    # ---- the conditional spectrum series (swrt_cond_series_*: omega classes by a flow scalar's classes) ----
    def cond_series_begin(self, f, Cg, omega_edges, which, q_edges, frac_bits=20):
        """Open a series of (nq + 2) x (nw + 2) count planes: omega classes
        over ``omega_edges`` (nw + 1 increasing values) by the classes of the
        flow scalar ``which`` (0 / "zeta", 1 / "sigma", 2 / "D") at the packets
        over ``q_edges`` (nq + 1 increasing values); the per-class omega sums
        quantised to 2^-frac_bits.  Empties the series."""
        which = COND_WHICH.get(which, which) if isinstance(which, str) else which
        self._plane_begin("cond", f, Cg, omega_edges, q_edges, frac_bits, int(which))

    def cond_series_record(self, nslots=1, alpha=0.0, bump=1e-13):
        """Append the current packets' frame in the flow of slot 0 (nslots 1)
        or slots 0 and 1 blended at ``alpha`` (queued; no host wait)."""
        self._chk(self._L.swrt_cond_series_record(self._h, int(nslots), float(alpha), float(bump)),
                  "swrt_cond_series_record")

    def cond_series_record_history(self, first, count, nslots=1, alphas=None, bump=1e-13):
        """One frame per history frame [first, first + count), frame i with
        the snapshot blend ``alphas[i]`` (None with one snapshot: 0)."""
        alphas = self._history_alphas(alphas, count)
        self._chk(self._L.swrt_cond_series_record_history(self._h, int(first), int(count), int(nslots), _p(alphas),
                                                          float(bump)), "swrt_cond_series_record_history")

    def cond_series_frames(self):
        return int(self._L.swrt_cond_series_frames(self._h))

    def cond_series_bins(self):
        """(nw, nq) of the open series, (0, 0) if none."""
        return self._plane_bins("cond")

    def cond_series_get(self, first=0, count=None):
        """Recorded frames [first, first + count) -> (counts (count, nq + 2,
        nw + 2) int64, counts[t, qc, wc]; sums (count, nq + 2) int64, the sum
        of rint(omega * 2^frac_bits) per q class; stats (count, 2) int64
        [n, rejected])."""
        return self._plane_get("cond", first, count)

    def cond_series_reset(self):
        self._chk(self._L.swrt_cond_series_reset(self._h), "swrt_cond_series_reset")

    # ---- the transition series (swrt_trans_series_*: omega classes by a per-packet source value's classes) ----
    def trans_series_begin(self, f, Cg, omega_edges, src_edges, frac_bits=20):
        """Open a series of (ns + 2) x (nw + 2) count planes: omega classes
        over ``omega_edges`` (nw + 1 increasing values) by the classes of each
        packet's source value over ``src_edges`` (ns + 1 increasing values);
        the per-class sums quantised to 2^-frac_bits.  Empties the series and
        drops the mark."""
        self._plane_begin("trans", f, Cg, omega_edges, src_edges, frac_bits)

    def trans_series_mark(self):
        """Source of every packet := its current omega (queued; no host wait)."""
        self._chk(self._L.swrt_trans_series_mark(self._h), "swrt_trans_series_mark")

    def trans_series_mark_values(self, values):
        """Source of the packet with original index i := ``values[i]``."""
        v = _f64(np.asarray(values, dtype=np.float64).ravel())
        self._chk(self._L.swrt_trans_series_mark_values(self._h, _p(v), v.size), "swrt_trans_series_mark_values")

    def trans_series_record(self):
        """Append the current packets' frame against the mark (queued; no host wait)."""
        self._chk(self._L.swrt_trans_series_record(self._h), "swrt_trans_series_record")

    def trans_series_record_history(self, first, count):
        """One frame per history frame [first, first + count), joined to the current mark."""
        self._chk(self._L.swrt_trans_series_record_history(self._h, int(first), int(count)),
                  "swrt_trans_series_record_history")

    def trans_series_frames(self):
        return int(self._L.swrt_trans_series_frames(self._h))

    def trans_series_bins(self):
        """(nw, ns) of the open series, (0, 0) if none."""
        return self._plane_bins("trans")

    def trans_series_get(self, first=0, count=None):
        """Recorded frames [first, first + count) -> (counts (count, ns + 2,
        nw + 2) int64, counts[t, sc, wc]; sums (count, ns + 2, 3) int64, per
        source class the sums of rint(omega * 2^frac_bits), rint(d * ...) and
        rint(d^2 * ...) with d = omega - source; stats (count, 3) int64
        [n, rejected, mark serial])."""
        return self._plane_get("trans", first, count)

    def trans_series_reset(self):
        self._chk(self._L.swrt_trans_series_reset(self._h), "swrt_trans_series_reset")

    # ---- the refraction series (swrt_refr_series_*: omega-dot and strain alignment per class) ----
    def refr_series_begin(self, f, Cg, omega_edges, a_edges, frac_bits=20):
        """Open a series of (na + 2) x (nw + 2) count planes: omega classes
        over ``omega_edges`` (nw + 1 increasing values) by the classes of the
        alignment c = 2 gamma / sigma over ``a_edges`` (na + 1 increasing
        values); the per-class sums of omega-dot, omega-dot^2 and gamma
        quantised to 2^-frac_bits.  Empties the series."""
        self._plane_begin("refr", f, Cg, omega_edges, a_edges, frac_bits)

    def refr_series_record(self, nslots=1, alpha=0.0, bump=1e-13):
        """Append the current packets' frame in the flow of slot 0 (nslots 1)
        or slots 0 and 1 blended at ``alpha`` (queued; no host wait)."""
        self._chk(self._L.swrt_refr_series_record(self._h, int(nslots), float(alpha), float(bump)),
                  "swrt_refr_series_record")

    def refr_series_record_history(self, first, count, nslots=1, alphas=None, bump=1e-13):
        """One frame per history frame [first, first + count), frame i with
        the snapshot blend ``alphas[i]`` (None with one snapshot: 0)."""
        alphas = self._history_alphas(alphas, count)
        self._chk(self._L.swrt_refr_series_record_history(self._h, int(first), int(count), int(nslots), _p(alphas),
                                                          float(bump)), "swrt_refr_series_record_history")

    def refr_series_frames(self):
        return int(self._L.swrt_refr_series_frames(self._h))

    def refr_series_bins(self):
        """(nw, na) of the open series, (0, 0) if none."""
        return self._plane_bins("refr")

    def refr_series_get(self, first=0, count=None):
        """Recorded frames [first, first + count) -> (counts (count, na + 2,
        nw + 2) int64, counts[t, ac, wc]; sums (count, 3 (nw + 2) + (na + 2))
        int64: per omega class the sums of rint(omega-dot * 2^frac_bits),
        rint(omega-dot^2 * ...) and rint(gamma * ...), then per alignment
        class the sum of rint(omega-dot * ...); stats (count, 2) int64
        [n, rejected])."""
        return self._plane_get("refr", first, count)

    def refr_series_reset(self):
        self._chk(self._L.swrt_refr_series_reset(self._h), "swrt_refr_series_reset")

    # ---- the absolute-frequency series (swrt_absfreq_series_*: Omega = omega + U.k and k.dU/dt per class) ----
    def absfreq_series_begin(self, f, Cg, omega_edges, abs_edges, frac_bits=20):
        """Open a series of (no + 2) x (nw + 2) count planes: omega classes
        over ``omega_edges`` (nw + 1 increasing values) by the classes of the
        absolute frequency Omega = omega + U.k over ``abs_edges`` (no + 1
        increasing values); the per-class sums of dOmega/dt, its square and
        the Doppler shift U.k quantised to 2^-frac_bits.  Empties the
        series."""
        self._plane_begin("absfreq", f, Cg, omega_edges, abs_edges, frac_bits)

    def absfreq_series_record(self, slot_a=0, slot_b=-1, alpha=0.0, tau=1.0, bump=1e-13):
        """Append the current packets' frame in the flow of ``slot_a``
        (alpha = 0) and ``slot_b`` (alpha = 1) blended at ``alpha``, the two
        snapshots ``tau`` apart; ``slot_b`` -1: one snapshot, zero rates
        (queued; no host wait)."""
        self._chk(self._L.swrt_absfreq_series_record(self._h, int(slot_a), int(slot_b), float(alpha), float(tau),
                                                     float(bump)), "swrt_absfreq_series_record")

    def absfreq_series_record_history(self, first, count, slot_a=0, slot_b=-1, alphas=None, tau=1.0, bump=1e-13):
        """One frame per history frame [first, first + count), frame i with
        the snapshot blend ``alphas[i]`` (None with one snapshot)."""
        alphas = self._history_alphas(alphas, count)
        self._chk(self._L.swrt_absfreq_series_record_history(self._h, int(first), int(count), int(slot_a), int(slot_b),
                                                             _p(alphas), float(tau), float(bump)),
                  "swrt_absfreq_series_record_history")

    def absfreq_series_frames(self):
        return int(self._L.swrt_absfreq_series_frames(self._h))

    def absfreq_series_bins(self):
        """(nw, no) of the open series, (0, 0) if none."""
        return self._plane_bins("absfreq")

    def absfreq_series_get(self, first=0, count=None):
        """Recorded frames [first, first + count) -> (counts (count, no + 2,
        nw + 2) int64, counts[t, oc, wc]; sums (count, 3 (nw + 2) + 2 (no + 2))
        int64: per omega class the sums of rint(Omega-dot * 2^frac_bits),
        rint(Omega-dot^2 * ...) and rint(U.k * ...), then per Omega class the
        sums of rint(Omega-dot * ...) and rint(Omega-dot^2 * ...); stats
        (count, 2) int64 [n, rejected])."""
        return self._plane_get("absfreq", first, count)

    def absfreq_series_reset(self):
        self._chk(self._L.swrt_absfreq_series_reset(self._h), "swrt_absfreq_series_reset")

    # ---- packet recycling (swrt_recycle_*: absorb at an omega cut, re-inject at home) ----
    def recycle_begin(self, f, Cg, omega_cut, L, seed=0, index_base=0, frac_bits=20, home_k=None):
        """Begin recycling the current packets: at every recycle_apply a packet
        whose omega has reached ``omega_cut`` gets its home wavevector back
        (``home_k``, n x 2 in the original order; None: the packets' k now) and
        a fresh uniform position in [-L/2, L/2)^2 from a hash of (``seed``,
        ``index_base`` + original index, generation)."""
        home = None
        if home_k is not None:
            home = np.asfortranarray(home_k, dtype=np.float64)
            if home.ndim != 2 or home.shape != (self.packets_count(), 2):
                raise ValueError("home_k must be n x 2, one home wavevector per packet")
        self._chk(self._L.swrt_recycle_begin(self._h, float(f), float(Cg), float(omega_cut), float(L),
                                             int(seed) & 0xFFFFFFFFFFFFFFFF, int(index_base), int(frac_bits),
                                             _p(home)), "swrt_recycle_begin")

    def recycle_apply(self):
        """One event on the current packets (queued; no host wait)."""
        self._chk(self._L.swrt_recycle_apply(self._h), "swrt_recycle_apply")

    def recycle_frames(self):
        return int(self._L.swrt_recycle_frames(self._h))

    def recycle_get(self, first=0, count=None):
        """Recorded frames [first, first + count) -> (count, 8) int64 [n,
        absorbed, rejected, sum q(omega_out), sum q(omega_home), sum age, max
        age, serial]."""
        count = self.recycle_frames() - first if count is None else count
        stats = np.zeros((max(count, 0), 8), dtype=np.int64)
        self._chk(self._L.swrt_recycle_get(self._h, int(first), int(count),
                                           stats.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), "swrt_recycle_get")
        return stats

    def recycle_state(self):
        """(gen, born), int32 per packet in the original order."""
        n = self.packets_count()
        gen = np.zeros(n, dtype=np.int32)
        born = np.zeros(n, dtype=np.int32)
        i32 = ctypes.POINTER(ctypes.c_int32)
        self._chk(self._L.swrt_recycle_state(self._h, gen.ctypes.data_as(i32), born.ctypes.data_as(i32)),
                  "swrt_recycle_state")
        return gen, born

    def recycle_reset(self):
        self._chk(self._L.swrt_recycle_reset(self._h), "swrt_recycle_reset")

    def recycle_end(self):
        self._chk(self._L.swrt_recycle_end(self._h), "swrt_recycle_end")

    # ---- the tangent map (swrt_tangent_*: the discrete step's derivative along every ray) ----
    def tangent_begin(self):
        """Allocate M (= I) and the caustic counters (0) for the current
        packets, mark serial 1.  Until ``tangent_end`` the leapfrog calls take
        the per-packet route and carry M; x and k keep their bits."""
        self._chk(self._L.swrt_tangent_begin(self._h), "swrt_tangent_begin")

    def tangent_mark(self):
        """M = I, counters 0, the next serial: a new window (queued; no host wait)."""
        self._chk(self._L.swrt_tangent_mark(self._h), "swrt_tangent_mark")

    def tangent_get(self):
        """(M (N, 16) float64 row-major, caustics (N,) int32) in the original packet order."""
        n = self.packets_count()
        M = np.zeros((n, 16), dtype=np.float64)
        caustics = np.zeros(n, dtype=np.int32)
        self._chk(self._L.swrt_tangent_get(self._h, _p(M), caustics.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                  "swrt_tangent_get")
        return M, caustics

    def tangent_end(self):
        self._chk(self._L.swrt_tangent_end(self._h), "swrt_tangent_end")

    def tangent_live(self):
        return bool(self._L.swrt_tangent_live(self._h) == 1)

    def tangent_serial(self):
        """The live set's mark serial (0: none)."""
        return int(self._L.swrt_tangent_serial(self._h))

    def tangent_series_begin(self, f, Cg, omega_edges, growth_edges):
        """Open a series of (ns + 2) x (nw + 2) count planes: the classes of
        s = |M|_F^2 / 4 over ``growth_edges`` (ns + 1 increasing values) by the
        omega classes over ``omega_edges`` (nw + 1).  Empties the series."""
        wedges = _f64(np.asarray(omega_edges, dtype=np.float64).ravel())
        gedges = _f64(np.asarray(growth_edges, dtype=np.float64).ravel())
        self._chk(self._L.swrt_tangent_series_begin(self._h, float(f), float(Cg), _p(wedges), wedges.size - 1,
                                                    _p(gedges), gedges.size - 1), "swrt_tangent_series_begin")

    def tangent_series_record(self):
        """Append the live set's frame (queued; no host wait)."""
        self._chk(self._L.swrt_tangent_series_record(self._h), "swrt_tangent_series_record")

    def tangent_series_frames(self):
        return int(self._L.swrt_tangent_series_frames(self._h))

    def tangent_series_bins(self):
        """(nw, ns) of the open series, (0, 0) if none."""
        return self._plane_bins("tangent")

    def tangent_series_get(self, first=0, count=None):
        """Recorded frames [first, first + count) -> (counts (count, ns + 2,
        nw + 2) int64, counts[t, gc, wc]; sums (count, 3 (nw + 2) + (ns + 2))
        int64: per omega class the sums of e(s), e(|J|) and the caustic
        counters, then per growth class the caustic counters; stats (count, 3)
        int64 [n, rejected, mark serial])."""
        return self._plane_get("tangent", first, count)

    def tangent_series_reset(self):
        self._chk(self._L.swrt_tangent_series_reset(self._h), "swrt_tangent_series_reset")

    # ---- the track series (swrt_track_*: trajectories of chosen packets) ------
    def track_begin(self, ids):
        """Track the packets with the original indices ``ids`` (distinct, in
        0..N-1); a frame's rows follow their order.  Empties the series."""
        ids = np.asarray(ids)
        if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
            raise ValueError("ids must be a one-dimensional sequence of integers")
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        ptr = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if ids.size else None
        self._chk(self._L.swrt_track_begin(self._h, ptr, ids.size), "swrt_track_begin")

    def track_record(self, f, gH, nslots=1, alpha=0.0, bump=1e-13):
        """Append the tracked packets' frame [x, y, k, l, Omega, zeta, sigma, D]
        to the device-side series (queued; no host wait).  ``nslots=0``: no
        flow, the last four columns are NaN."""
        self._chk(self._L.swrt_track_record(self._h, float(f), float(gH), int(nslots), float(alpha), float(bump)),
                  "swrt_track_record")

    def track_record_history(self, first, count, f, gH, nslots=1, alphas=None, bump=1e-13):
        """One track frame per history frame [first, first + count) (queued; no
        host wait), frame i with the snapshot blend ``alphas[i]`` (None: 0)."""
        alphas = self._history_alphas(alphas, count)
        self._chk(self._L.swrt_track_record_history(self._h, int(first), int(count), float(f), float(gH),
                                                    int(nslots), _p(alphas), float(bump)),
                  "swrt_track_record_history")

    def track_frames(self):
        return int(self._L.swrt_track_frames(self._h))

    def track_ids(self):
        """The ids of the open series, in the order given (empty if none)."""
        ids = np.zeros(max(int(self._L.swrt_track_count(self._h)), 0), dtype=np.int64)
        if ids.size:
            self._chk(self._L.swrt_track_ids(self._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
                      "swrt_track_ids")
        return ids

    def track_series(self, first=0, count=None):
        """Recorded frames [first, first + count) as (count, 8, m) float64:
        [t, c, j] is column c of packet ids[j] at frame t."""
        count = self.track_frames() - first if count is None else count
        m = max(int(self._L.swrt_track_count(self._h)), 0)
        out = np.empty((max(count, 0), 8, m))
        self._chk(self._L.swrt_track_get(self._h, int(first), int(count), _p(out)), "swrt_track_get")
        return out

    def track_reset(self):
        self._chk(self._L.swrt_track_reset(self._h), "swrt_track_reset")

    # ---- the flow spectrum series (swrt_flow_spectrum_*: shell spectra of the background flow) ----
    def flow_spectrum_begin(self, nx, k_scale=1.0, K_d2=0.0):
        """Open a series of shell spectra of nx^2 spectral PV half planes
        (k_scale = 2*pi/L; exactly 1 for the one-layer model).  Empties the series."""
        self._chk(self._L.swrt_flow_spectrum_begin(self._h, int(nx), float(k_scale), float(K_d2)),
                  "swrt_flow_spectrum_begin")

    def flow_spectrum_record_qg(self, layer=0):
        """Append the frame of the QG state's committed qk, layer ``layer``
        (queued on the QG stream; no host wait)."""
        self._chk(self._L.swrt_flow_spectrum_record_qg(self._h, int(layer)), "swrt_flow_spectrum_record_qg")

    def flow_spectrum_record_qk(self, qk, t=0.0):
        """Append the frame of a host half plane ``qk`` ((2kmax+1, kmax+1)
        complex, set_field_qk's layout), stamped with ``t``."""
        qk = np.asarray(qk, dtype=np.complex128)
        nx = qk.shape[0] + 1
        if qk.ndim != 2 or qk.shape != (nx - 1, nx // 2):
            raise ValueError("qk must be a (2kmax+1, kmax+1) half plane")
        buf = _f64(np.asfortranarray(qk).ravel(order="F").view(np.float64))
        self._chk(self._L.swrt_flow_spectrum_record_qk(self._h, _p(buf), nx, float(t)),
                  "swrt_flow_spectrum_record_qk")

    def flow_spectrum_frames(self):
        return int(self._L.swrt_flow_spectrum_frames(self._h))

    def flow_spectrum_shells(self):
        return int(self._L.swrt_flow_spectrum_shells(self._h))

    def flow_spectrum_get(self, first=0, count=None, spectra=True, stats=True):
        """Recorded frames [first, first + count) -> (spectra (count, 3, nshell)
        float64 [E, Z, Q] per shell; stats (count, 4) [t, sum E, sum Z, sum Q]);
        None in place of an output not asked for."""
        count = self.flow_spectrum_frames() - first if count is None else count
        ns = self.flow_spectrum_shells()
        sp = np.zeros((max(count, 0), 3, ns)) if spectra else None
        st = np.zeros((max(count, 0), 4)) if stats else None
        self._chk(self._L.swrt_flow_spectrum_get(self._h, int(first), int(count), _p(sp), _p(st)),
                  "swrt_flow_spectrum_get")
        return sp, st

    def flow_spectrum_reset(self):
        self._chk(self._L.swrt_flow_spectrum_reset(self._h), "swrt_flow_spectrum_reset")

    # ---- the invariant and the flow along the rays (swrt_raydiag_*) ----------
    def raydiag_mark(self, f, gH, nslots=1, alpha=0.0, bump=1e-13):
        """Keep Omega_0 = omega(k) + U(x).k of every packet at the current state
        (symplectic_full_fourier.m:41)."""
        self._chk(self._L.swrt_raydiag_mark(self._h, float(f), float(gH), int(nslots), float(alpha), float(bump)),
                  "swrt_raydiag_mark")

    def raydiag_sample(self, f, gH, nslots=1, alpha=0.0, bump=1e-13, values=True):
        """-> (N x 4 [Omega zeta sigma D] in the original packet order, or None
        without ``values``; the frame [n, max|r|, sum r, sum r^2, sum omega,
        sum zeta, sum sigma, sum D]).  Synchronous."""
        n = self.packets_count()
        s4 = np.empty((n, 4), order="F") if values else None
        fr = np.empty(8)
        self._chk(self._L.swrt_raydiag_sample(self._h, float(f), float(gH), int(nslots), float(alpha), float(bump),
                                              _p(s4), _p(fr)), "swrt_raydiag_sample")
        return s4, fr

    def raydiag_record(self, f, gH, nslots=1, alpha=0.0, bump=1e-13):
        """Append the current state's frame to the device-side series (queued; no host wait)."""
        self._chk(self._L.swrt_raydiag_record(self._h, float(f), float(gH), int(nslots), float(alpha), float(bump)),
                  "swrt_raydiag_record")

    def raydiag_record_history(self, first, count, f, gH, nslots=1, alphas=None, bump=1e-13):
        """swrt_raydiag_record_history: one series frame per history frame
        [first, first + count) (queued; no host wait), frame i with the
        snapshot blend ``alphas[i]`` (None with one snapshot: 0)."""
        alphas = self._history_alphas(alphas, count)
        self._chk(self._L.swrt_raydiag_record_history(self._h, int(first), int(count), float(f), float(gH),
                                                      int(nslots), _p(alphas), float(bump)),
                  "swrt_raydiag_record_history")

    def raydiag_frames(self):
        return int(self._L.swrt_raydiag_frames(self._h))

    def raydiag_series(self, first=0, count=None):
        """Recorded frames [first, first + count) as a (count, 8) array."""
        count = self.raydiag_frames() - first if count is None else count
        out = np.empty((max(count, 0), 8))
        self._chk(self._L.swrt_raydiag_series_get(self._h, int(first), int(count), _p(out)),
                  "swrt_raydiag_series_get")
        return out

    def raydiag_series_reset(self):
        self._chk(self._L.swrt_raydiag_series_reset(self._h), "swrt_raydiag_series_reset")

    # ---- ode23 device stages (swrt_ode23_*) --------------------------------
    def ode23_f1(self, t, tmax, f, Cg, nslots, thr, bump):
        r = _D()
        self._chk(self._L.swrt_ode23_f1(self._h, float(t), float(tmax), float(f), float(Cg), int(nslots),
                                        float(thr), float(bump), ctypes.byref(r)), "swrt_ode23_f1")
        return r.value

    def ode23_attempt(self, t, h, tnew, tmax, f, Cg, nslots, thr, bump):
        r = _D()
        self._chk(self._L.swrt_ode23_attempt(self._h, float(t), float(h), float(tnew), float(tmax), float(f),
                                             float(Cg), int(nslots), float(thr), float(bump), ctypes.byref(r)),
                  "swrt_ode23_attempt")
        return r.value

    def ode23_accept(self):
        self._chk(self._L.swrt_ode23_accept(self._h), "swrt_ode23_accept")

    def ode23_set_dense(self, on):
        """swrt_ode23_set_dense: ode23_attempt keeps F2 and F3 for ode23_ntrp."""
        self._chk(self._L.swrt_ode23_set_dense(self._h, int(on)), "swrt_ode23_set_dense")

    def ode23_ntrp(self, t, tnew, tout):
        """swrt_ode23_ntrp: between a dense attempt of the step from t to tnew
        and ode23_accept, append one history frame per time in ``tout``
        (ntrp23 inside the step; a time equal to tnew is ynew itself)."""
        tout = np.ascontiguousarray(tout, dtype=np.float64).reshape(-1)
        self._chk(self._L.swrt_ode23_ntrp(self._h, float(t), float(tnew), _p(tout), int(tout.size)),
                  "swrt_ode23_ntrp")

    def ode23_run_at(self, tspan, tmax, f, Cg, nslots, rtol, atol, bump, ts_cap=10_000):
        """swrt_ode23_run_at: ode23 over a vector ``tspan`` with the controller
        in the library; the solution at tspan[1:] is appended to the history
        (len(tspan) - 1 frames) and the packets are left at the last one.
        Returns (accepted times, {steps, failed, attempts, accepted}) as
        ode23_run."""
        tspan = np.ascontiguousarray(tspan, dtype=np.float64).reshape(-1)
        ts = np.empty(ts_cap)
        nts = _I()
        st = (_I * 3)()
        self._chk(self._L.swrt_ode23_run_at(self._h, _p(tspan), int(tspan.size), float(tmax), float(f), float(Cg),
                                            int(nslots), float(rtol), float(atol), float(bump), _p(ts),
                                            int(ts_cap), ctypes.byref(nts), st), "swrt_ode23_run_at")
        if nts.value > ts_cap:
            import warnings
            warnings.warn(f"swrt_ode23_run_at accepted {nts.value} times; only the first ts_cap={ts_cap} are returned",
                          RuntimeWarning, stacklevel=2)
        return ts[:min(nts.value, ts_cap)].copy(), {"steps": st[0], "failed": st[1], "attempts": st[2],
                                                    "accepted": nts.value}

    def ode23_run(self, t0, tfinal, tmax, f, Cg, nslots, rtol, atol, bump, ts_cap=10_000, hook=None, reduce=None):
        """swrt_ode23_run: the whole ode23 call with the controller in the
        library.  Returns (accepted times, {steps, failed, attempts,
        accepted}); `accepted` counts every accepted time, and a warning is
        raised when more than ts_cap were accepted (the list then holds the
        first ts_cap only).  ``hook``: a callable run once after the first
        launches are queued (swrt_ode23_run_hooked; QG calls only, never the
        packets).  ``reduce``: a callable float -> float, the max over the
        ranks of a sharded run (swrt_ode23_run_sharded; called once for stage
        1 and once per attempt, the same order on every rank).  An exception
        either raises is re-raised after the call."""
        ts = np.empty(ts_cap)
        nts = _I()
        st = (_I * 3)()
        args = (self._h, float(t0), float(tfinal), float(tmax), float(f), float(Cg), int(nslots), float(rtol),
                float(atol), float(bump), _p(ts), int(ts_cap), ctypes.byref(nts), st)
        if hook is None and reduce is None:
            self._chk(self._L.swrt_ode23_run(*args), "swrt_ode23_run")
        else:
            # one ctypes callback per context (made once), calling this call's hook
            if self._ode23_cb is None:
                def _call(_user):
                    h, self._ode23_hook = self._ode23_hook, None
                    try:
                        if h is not None:
                            h()
                    except BaseException as e:  # ctypes would print and drop it
                        self._ode23_raised = e
                self._ode23_cb = _HOOK(_call)
            self._ode23_hook, self._ode23_raised = hook, None
            if reduce is None:
                rc = self._L.swrt_ode23_run_hooked(*args, self._ode23_cb if hook is not None else _HOOK(), None)
                name = "swrt_ode23_run_hooked"
            else:
                if self._ode23_red_cb is None:
                    def _red(vp, _user):
                        try:
                            vp[0] = float(self._ode23_reduce(vp[0]))
                            return 0
                        except BaseException as e:
                            if self._ode23_raised is None:
                                self._ode23_raised = e
                            return 1
                    self._ode23_red_cb = _REDUCE(_red)
                self._ode23_reduce = reduce
                rc = self._L.swrt_ode23_run_sharded(*args, self._ode23_cb if hook is not None else _HOOK(), None,
                                                    self._ode23_red_cb, None)
                self._ode23_reduce = None
                name = "swrt_ode23_run_sharded"
            self._ode23_hook = None
            raised, self._ode23_raised = self._ode23_raised, None
            if raised is not None:
                raise raised
            self._chk(rc, name)
        # ts_cap bounds the recorded times only (the interval always completes)
        if nts.value > ts_cap:
            import warnings
            warnings.warn(f"swrt_ode23_run accepted {nts.value} times; only the first ts_cap={ts_cap} are returned",
                          RuntimeWarning, stacklevel=2)
        return ts[:min(nts.value, ts_cap)].copy(), {"steps": st[0], "failed": st[1], "attempts": st[2],
                                                    "accepted": nts.value}

    def ode23_chain_next(self, slot_a, slot_b):
        """swrt_ode23_chain_next: the running (or next) ode23_run queues the
        next call's stage 1 with slots (slot_a, slot_b) as its slots 0 / 1
        when it ends; the next call takes it only if it computes the same."""
        self._chk(self._L.swrt_ode23_chain_next(self._h, int(slot_a), int(slot_b)), "swrt_ode23_chain_next")

    # ---- owner-driver hand-off (swrt_qg_export / swrt_snapshot_qk) -----------
    def qg_export(self, dst, which=0, layer=0, stream=None, tail=0.0, fenced=False):
        """Layer `layer` of the current (0) / previous (1) qk in the device's
        half-plane order (ky fastest), then `tail`, into `dst`: a float64
        numpy array of 2*(2kmax+1)*(kmax+1) + 1 values (host copy, returns
        when done), or an int device address (queued; ordered after and
        before the work of the hipStream_t `stream`, default the packet
        stream — ``fenced``: only before it, the caller guarantees dst is
        free; swrt_qg_export dst_mode 2)."""
        if isinstance(dst, np.ndarray):
            if dst.dtype != np.float64 or not dst.flags["C_CONTIGUOUS"] or dst.size != 2 * self._qg_nhalf() + 1:
                raise ValueError("dst must be a contiguous float64 array of 2*(2kmax+1)*(kmax+1) + 1 values")
            self._chk(self._L.swrt_qg_export(self._h, int(which), int(layer), dst.ctypes.data_as(_VP), 0, None,
                                             float(tail)), "swrt_qg_export")
        else:
            self._chk(self._L.swrt_qg_export(self._h, int(which), int(layer), _VP(int(dst)), 2 if fenced else 1,
                                             None if stream is None else _VP(int(stream)), float(tail)),
                      "swrt_qg_export")

    def _qg_nhalf(self):
        kmax = self._qg_nx // 2 - 1
        return (2 * kmax + 1) * (kmax + 1)

    def snapshot_qk(self, slot, qk, nx, L, K_d2, shear=0.0, k_scale=1.0, ny_period=0, stream=None):
        """grid_U of a half plane in qg_export's order into `slot`
        (swrt_snapshot_qk): `qk` a float64 numpy array (host) or an int device
        address (read after / before `stream`'s work)."""
        kmax = int(nx) // 2 - 1
        nh = (2 * kmax + 1) * (kmax + 1)
        if isinstance(qk, np.ndarray):
            if qk.dtype != np.float64 or not qk.flags["C_CONTIGUOUS"] or qk.size != 2 * nh:
                raise ValueError("qk must be a contiguous float64 array of 2*(2kmax+1)*(kmax+1) values")
            src, on_dev, st = qk.ctypes.data_as(_VP), 0, None
        else:
            src, on_dev, st = _VP(int(qk)), 1, None if stream is None else _VP(int(stream))
        self._chk(self._L.swrt_snapshot_qk(self._h, int(slot), src, on_dev, st, int(nx), float(L), float(K_d2),
                                           float(shear), float(k_scale), int(ny_period)), "swrt_snapshot_qk")

    # ---- QG PDE stepper (swrt_qg_*) ---------------------------------------
    def qg_init(self, params: QGParams, nx, qk):
        """qk: (2kmax+1, kmax+1) complex, or (2kmax+1, kmax+1, nlayers)."""
        qk = np.asarray(qk, dtype=np.complex128)
        if qk.ndim == 2:
            qk = qk[:, :, None]
        kmax = nx // 2 - 1
        assert qk.shape == (2 * kmax + 1, kmax + 1, params.nlayers), qk.shape
        buf = _f64(np.asfortranarray(qk).ravel(order="F").view(np.float64))
        self._qg_shape = (2 * kmax + 1, kmax + 1, params.nlayers)
        self._qg_nx = nx
        self._chk(self._L.swrt_qg_init(self._h, ctypes.byref(params), nx, _p(buf)), "swrt_qg_init")

    def qg_step(self, dt, nsteps=1):
        self._chk(self._L.swrt_qg_step(self._h, float(dt), int(nsteps)), "swrt_qg_step")

    def qg_step_speculative(self, dt):
        """swrt_qg_step_speculative: the next step with dt, its transforms and CFL read-back queued into
        spare buffers; the committed state is kept until qg_resolve."""
        self._chk(self._L.swrt_qg_step_speculative(self._h, float(dt)), "swrt_qg_step_speculative")

    def qg_resolve(self, accept):
        """swrt_qg_resolve: accept (the speculative step becomes current) or drop it."""
        self._chk(self._L.swrt_qg_resolve(self._h, int(bool(accept))), "swrt_qg_resolve")

    def qg_set_stream(self, separate=True):
        """QG PDE on its own stream, overlapping the packet launches (swrt_qg_set_stream)."""
        self._chk(self._L.swrt_qg_set_stream(self._h, int(bool(separate))), "swrt_qg_set_stream")

    def qg_set_fused(self, on=True):
        """One batched transform per qk for the step, CFL speed and snapshot (swrt_qg_set_fused)."""
        self._chk(self._L.swrt_qg_set_fused(self._h, int(bool(on))), "swrt_qg_set_fused")
        self.qg_fused = bool(on)

    def qg_max_speed(self):
        u = _D()
        self._chk(self._L.swrt_qg_max_speed(self._h, ctypes.byref(u)), "swrt_qg_max_speed")
        return u.value

    def qg_max_speed_async(self):
        self._chk(self._L.swrt_qg_max_speed_async(self._h), "swrt_qg_max_speed_async")

    def qg_max_speed_result(self):
        u = _D()
        self._chk(self._L.swrt_qg_max_speed_result(self._h, ctypes.byref(u)), "swrt_qg_max_speed_result")
        return u.value

    def qg_get(self):
        """-> (qk (2kmax+1, kmax+1, nlayers) complex, t, steps)."""
        out = np.empty(2 * int(np.prod(self._qg_shape)))
        t = _D()
        s = ctypes.c_int64()
        self._chk(self._L.swrt_qg_get(self._h, _p(out), ctypes.byref(t), ctypes.byref(s)), "swrt_qg_get")
        qk = out.view(np.complex128).reshape(self._qg_shape, order="F")
        return qk, t.value, s.value

    def qg_get_q(self):
        """-> q grid (nx, nx, nlayers), column-major per layer (k2g of each layer)."""
        nx, nl = self._qg_nx, self._qg_shape[2]
        out = np.empty(nx * nx * nl)
        self._chk(self._L.swrt_qg_get_q(self._h, _p(out)), "swrt_qg_get_q")
        return out.reshape((nx, nx, nl), order="F")

    def qg_snapshot(self, slot, which=0, layer=0, ny_period=0):
        self._chk(self._L.swrt_qg_snapshot(self._h, int(slot), int(which), int(layer), int(ny_period)),
                  "swrt_qg_snapshot")

    def qg_snapshot_speculative(self, slot, ny_period=0):
        """swrt_qg_snapshot_speculative: layer 0's grid_U of the pending
        speculative step into `slot` (what qg_snapshot(slot) writes after
        accepting it)."""
        self._chk(self._L.swrt_qg_snapshot_speculative(self._h, int(slot), int(ny_period)),
                  "swrt_qg_snapshot_speculative")

    def swap_slots(self, a=0, b=1):
        self._chk(self._L.swrt_swap_slots(self._h, int(a), int(b)), "swrt_swap_slots")

    # ---- runtime ---------------------------------------------------------
    def synchronize(self):
        self._chk(self._L.swrt_synchronize(self._h), "swrt_synchronize")

    def check_arith(self, n=1 << 20, seed=1):
        """Bit-exactness of the hot loop's short sqrt / reciprocal / drift
        sequences against the device's IEEE operations over 16*n random
        operands (swrt_check_arith): mismatch counts (sqrt, 1/w, drift)."""
        out = (ctypes.c_int64 * 3)()
        self._chk(self._L.swrt_check_arith(self._h, int(n), int(seed), out), "swrt_check_arith")
        return tuple(out)

    def stream(self):
        s = _VP()
        self._chk(self._L.swrt_get_stream(self._h, ctypes.byref(s)), "swrt_get_stream")
        return s.value

    def set_timing(self, every=1):
        self._chk(self._L.swrt_set_timing(self._h, int(every)), "swrt_set_timing")
        self.timing_every = int(every)

    def kernel_time(self, reset=True):
        ms = _D()
        n = _I()
        self._chk(self._L.swrt_kernel_time(self._h, int(reset), ctypes.byref(ms), ctypes.byref(n)),
                  "swrt_kernel_time")
        return ms.value, n.value

    def clock_stamp(self, which):
        """swrt_clock_stamp: 0 before, 1 after a region of packet-stream work."""
        self._chk(self._L.swrt_clock_stamp(self._h, int(which)), "swrt_clock_stamp")

    def clock_ghz(self):
        """swrt_clock_ghz: (median observed shader clock in GHz, relative spread) between the stamps."""
        g, s = _D(), _D()
        self._chk(self._L.swrt_clock_ghz(self._h, ctypes.byref(g), ctypes.byref(s)), "swrt_clock_ghz")
        return g.value, s.value

    def debug_set(self, key, value):
        """swrt_debug_set: DEBUG_HAZARD_CHECK, DEBUG_SPIN_US, DEBUG_LEGACY_PARK (test infrastructure)."""
        self._chk(self._L.swrt_debug_set(self._h, int(key), int(value)), "swrt_debug_set")

    def debug_get(self, key):
        v = _I()
        self._chk(self._L.swrt_debug_get(self._h, int(key), ctypes.byref(v)), "swrt_debug_get")
        return v.value


def ode23_replay(t0, tfinal, raw, rtol=1e-3, atol=1e-6, dev_first=True, ts_cap=100_000):
    """swrt_ode23_replay: the library's ode23 controller (swrt_ode23_ctl.cpp)
    over a scripted raw-error sequence, on the host (no GPU, no context).
    raw[0] = stage 1's max, then one per attempt the controller consumes.
    Returns (status, attempts (n, 4) [t, h, tnew, raw], accepted times, stats
    dict); status is SWRT_OK, "below hmin" or "script exhausted"."""
    L = load()
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    cap = max(1, raw.size)
    log = np.empty(4 * cap)
    ts = np.empty(ts_cap)
    nlog, nts = _I(), _I()
    st = (_I * 9)()
    rc = L.swrt_ode23_replay(float(t0), float(tfinal), float(rtol), float(atol), int(bool(dev_first)), _p(raw),
                             raw.size, _p(log), cap, ctypes.byref(nlog), _p(ts), ts_cap, ctypes.byref(nts), st)
    status = {SWRT_OK: SWRT_OK, 3: "below hmin", 1: "script exhausted"}.get(rc, rc)
    keys = ("steps", "failed", "attempts", "first_taken", "guesses", "taken_maxstep", "taken_ramp_maxstep",
            "taken_ramp_5x", "gate_violations")
    return (status, log[:4 * min(nlog.value, cap)].reshape(-1, 4).copy(), ts[:min(nts.value, ts_cap)].copy(),
            {k: int(v) for k, v in zip(keys, st)})


def clock_ghz_stamps(stamps, realtime_hz=100e6):
    """swrt_clock_ghz_stamps: (GHz, spread) from probe stamps shaped (2, waves,
    3) = start/end x wave x {cycles, realtime ticks, CU id}; raises SwrtError
    when no CU holds both a start and an end wave (host only)."""
    L = load()
    a = np.ascontiguousarray(stamps, dtype=np.uint64)
    if a.ndim != 3 or a.shape[0] != 2 or a.shape[2] != 3:
        raise ValueError("stamps must be (2, waves, 3)")
    g, s = _D(), _D()
    rc = L.swrt_clock_ghz_stamps(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), a.shape[1], float(realtime_hz),
                                 ctypes.byref(g), ctypes.byref(s))
    if rc != SWRT_OK:
        raise SwrtError(f"swrt_clock_ghz_stamps: {ERRORS.get(rc, rc)}: no CU with both a start and an end stamp"
                        if rc == 3 else f"swrt_clock_ghz_stamps: {ERRORS.get(rc, rc)}")
    return g.value, s.value


def exported_symbols():
    """Names the header declares (for the ABI export test)."""
    return list(SIGNATURES)


if __name__ == "__main__":  # pragma: no cover
    load()
    print("libswrt loaded:", LIB_PATH, file=sys.stderr)
