"""CPU test of the packet-buffer hazard checker's model (swrt_hazard.hpp):
tests/hazard_model.cpp replays the multi-stream launch protocol of
swrt_host_packets.hpp abstractly and checks the checker's verdicts — silent on the
library's ordering (third buffers, joins before re-binnings and whole
launches), reporting the pre-third-buffer race, a whole launch or a
re-binning without a join, and round 4's skewed cycle-end share (its regions
are the band slots swrt_share.hpp's mapping gives each part).  The device-side counterpart is
tests/test_gpu_hazard.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hazard_checker_model(tmp_path):
    exe = tmp_path / "hazard_model"
    # hipcc: the model includes swrt_share.hpp (host/device mapping functions);
    # host code only, no GPU needed
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-std=c++17",
                    "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "hazard_model.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
    assert "legacy_park_reported_s2 ok" in r.stdout
    assert "skewed_cycle_end_reported ok" in r.stdout and "consistent_skew_silent ok" in r.stdout
    assert "share_partitions_slots ok" in r.stdout
    assert "sort launch" in r.stdout or "part" in r.stdout
    # the library's own packet-set rotation and Binning transitions (swrt_packet_state.hpp)
    for name in ("set_ring_rotations", "binning_source_gather_pending_not_tiled", "binning_tiled_after_launch",
                 "binning_keys_valid_after_counting_launch", "binning_keys_other_grid_or_bins",
                 "binning_keys_stale_0", "binning_keys_stale_1", "binning_keys_stale_2", "binning_keys_stale_3",
                 "binning_memset_guard_larger_count", "binning_memset_guard_after_rebin",
                 "binning_memset_skip_survives_invalidate", "binning_invalidate_as_constructed",
                 "binning_cadence", "binning_due_after_cycle"):
        assert name + " ok" in r.stdout, r.stdout
    # the frame series' counting (SeriesExtent): growth, the range query, clear / release, the history rule
    for name in ("series_empty_does_not_fit", "series_growth_from_empty_takes_minimum", "series_fits_up_to_capacity",
                 "series_growth_doubles", "series_growth_takes_needed", "series_extra_zero_never_grows",
                 "series_no_minimum_takes_needed", "series_range_inside", "series_range_past_end",
                 "series_range_negative", "series_cleared_keeps_capacity", "series_cleared_holds_nothing",
                 "series_released_drops_capacity", "series_history_smaller_frame_does_not_pass",
                 "series_history_growth_for_larger_frame"):
        assert name + " ok" in r.stdout, r.stdout
    # the class-plane series' frame layout (PlaneLayout) against each series' own formulas
    for name in ("plane_layout_cond", "plane_layout_trans", "plane_layout_refr", "plane_layout_absfreq"):
        assert name + " ok" in r.stdout, r.stdout
