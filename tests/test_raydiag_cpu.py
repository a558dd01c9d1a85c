"""Host side of the ray diagnostics (no GPU): combining the frames of shards,
and the C ABI's declarations (include/swrt.h, the ctypes table)."""
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT

CALLS = ("swrt_raydiag_mark", "swrt_raydiag_sample", "swrt_raydiag_record", "swrt_raydiag_frames",
         "swrt_raydiag_series_get", "swrt_raydiag_series_reset")


def _frame(n, rmax, *sums):
    return np.array([n, rmax, *sums], dtype=np.float64)


def test_combine_frames_by_hand():
    from swraytracing_amd import combine_frames
    a = _frame(3, 0.25, 0.5, 0.125, 12.0, -1.0, 2.0, 0.5)
    b = _frame(5, 0.75, -0.25, 0.625, 20.0, 3.0, 1.0, -1.5)
    z = np.zeros(8)  # a shard without packets
    want = _frame(8, 0.75, 0.25, 0.75, 32.0, 2.0, 3.0, -1.0)
    np.testing.assert_array_equal(combine_frames([a, b]), want)
    np.testing.assert_array_equal(combine_frames([z, a, b]), want)
    np.testing.assert_array_equal(combine_frames([b, z, a, z]), want)
    np.testing.assert_array_equal(combine_frames([a]), a)
    np.testing.assert_array_equal(combine_frames([z, z]), z)


def test_combine_series():
    from swraytracing_amd import combine_frames
    a = np.stack([_frame(2, 0.0, 0, 0, 8.0, 1, 1, 1), _frame(2, 0.5, 0.25, 0.25, 8.5, 2, 2, 2)])
    b = np.stack([_frame(1, 0.0, 0, 0, 4.0, 1, 1, 1), _frame(1, 0.125, -0.125, 0.015625, 4.5, -2, 0, 1)])
    got = combine_frames([a, b, np.zeros((2, 8))])
    assert got.shape == (2, 8)
    np.testing.assert_array_equal(got[0], _frame(3, 0.0, 0, 0, 12.0, 2, 2, 2))
    np.testing.assert_array_equal(got[1], _frame(3, 0.5, 0.125, 0.265625, 13.0, 0, 2, 3))
    for bad in (np.zeros(8), np.zeros((2, 7)), []):
        with pytest.raises(ValueError):
            combine_frames(bad)


def test_header_declares_the_calls_with_their_sources():
    src = open(os.path.join(ROOT, "include", "swrt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\b" + name + r"\s*\(\s*(const\s+)?swrt_ctx\*", code), name
    for cite in ("symplectic_full_fourier.m:41", "SW_zero_background_raytracing.m:57", "RaytracingScheme.m:30"):
        assert cite in src, cite


def test_ctypes_table_binds_the_calls():
    import swraytracing_amd._lib as L
    for name in CALLS:
        assert name in L.SIGNATURES, name
    for meth in ("raydiag_mark", "raydiag_sample", "raydiag_record", "raydiag_frames", "raydiag_series",
                 "raydiag_series_reset"):
        assert callable(getattr(L.Context, meth))
