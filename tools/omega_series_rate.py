"""Cost of one recorded spectrum frame (swrt_omega_series_record) at the
bench's shape: 512^2, two snapshots, 1e6 packets, 300 bins over [0, 15].
Within one session, after warm-up, the median of --reps of

  (a) one recorded frame between two events on the context's stream, for
      the initial ring (every packet in one or two bins) and for the packets
      after --spread-steps bench steps (spread over many bins)
  (b) one synchronous swrt_omega_histogram call (host time: it waits)
  (c) the only route to a driver spectrum before the series: packets_get
      plus the numpy omega and histogram (host time, --host-reps)
  (d) one leapfrog step of advance: 5 x --reps bench steps of --substeps
      steps each between two device synchronisations, divided by the steps
      (as tools/ray_diag_rate.py measures it)

and the shader clock observed over the event-timed part (swrt_clock_ghz).
Prints one JSON line; (a) < (b) and (a) < (c) for both distributions is the
condition; (a)/(d) and the ring/spread ratio of (a) are reported.  With
SWRT_LIB_PATH set to a build with -DSWRT_HIST_AGG_ROUNDS=0
(tools/build_variant.sh) the same run gives the ratio without the wave
aggregation.
usage: python tools/omega_series_rate.py [--packets N] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_path(ctx, f, Cg, edges):
    """Counts and mean omega through the calls that existed before the series."""
    _, k = ctx.packets_get()
    k1, k2 = k[:, 0], k[:, 1]
    om = np.sqrt(f * f + Cg * Cg * (k1 * k1 + k2 * k2))
    b = np.searchsorted(edges, om, "right") - 1
    b[om == edges[-1]] = edges.size - 2
    ok = (om >= edges[0]) & (om <= edges[-1])
    return np.bincount(b[ok], minlength=edges.size - 1), om.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--spread-steps", type=int, default=200, help="bench steps before the spread distribution is timed")
    ap.add_argument("--bins", type=int, default=300)
    a = ap.parse_args()
    import bench
    bench._imports()
    import torch

    import swraytracing_amd as sw
    args = bench.parse_args(["--packets", str(a.packets)])
    ctx = sw.Context(0)
    w = bench.build_workload(ctx, args, 0, a.packets, a.packets)
    ctx.set_locality(args.rebin_every, args.tile)
    ctx.set_timing(0)
    ctx.packets_set(w["x"], w["k"])
    f, Cg, sub = w["f"], float(np.sqrt(w["gH"])), args.substeps
    edges = np.linspace(0.0, 15.0, a.bins + 1)
    stream = torch.cuda.ExternalStream(ctx.stream())

    def events(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            fn()
            e1.record(stream)
        ctx.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in ev]  # ms

    def host(fn, reps):
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def warm():
        ctx.omega_series_reset()
        for _ in range(5):
            ctx.omega_series_record()
            ctx.omega_histogram(f, Cg, edges)
        ctx.synchronize()

    def host_side(rec):
        """(b), (c) at the current packets beside the event times `rec` of (a), and the frame's non-zero bins."""
        hist = host(lambda: ctx.omega_histogram(f, Cg, edges), a.reps)
        hp = host(lambda: host_path(ctx, f, Cg, edges), a.host_reps)
        counts, stats = ctx.omega_series(ctx.omega_series_frames() - 1, 1)
        hc, hm = host_path(ctx, f, Cg, edges)
        sc, sm = ctx.omega_histogram(f, Cg, edges)
        return dict(a_record_frame_ms=statistics.median(rec), a_min_ms=min(rec),
                    b_omega_histogram_ms=statistics.median(hist), c_host_path_ms=statistics.median(hp),
                    nonzero_bins=int(np.count_nonzero(counts[0, 1:-1])), largest_bin=int(counts[0, 1:-1].max()),
                    counts_equal_host=bool(np.array_equal(counts[0, 1:-1], hc)),
                    counts_equal_histogram=bool(np.array_equal(counts[0, 1:-1], sc)),
                    mean_omega=float(stats[0, 1] / stats[0, 0]), mean_omega_host=float(hm),
                    mean_omega_histogram=float(sm))

    for _ in range(5):  # warm-up: the kernels loaded, the clocks up; then the ring again
        bench.step(ctx, w, sub)
    ctx.packets_set(w["x"], w["k"])
    ctx.omega_series_begin(f, Cg, edges)
    warm()
    ring = host_side(events(ctx.omega_series_record, a.reps))
    for _ in range(a.spread_steps):
        bench.step(ctx, w, sub)
    warm()
    ctx.clock_stamp(0)  # the clock over the device-timed part only: (a) for the spread packets, then (d)
    rec = events(ctx.omega_series_record, a.reps)
    t0 = time.perf_counter()
    for _ in range(5 * a.reps):
        bench.step(ctx, w, sub)
    ctx.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / (5 * a.reps * sub)
    rec2 = events(ctx.omega_series_record, a.reps)
    ctx.clock_stamp(1)
    ctx.synchronize()
    try:
        ghz, clk_spread = ctx.clock_ghz()
    except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
        ghz = clk_spread = None
    spread = host_side(rec)
    spread["a_after_steps_ms"] = statistics.median(rec2)
    ctx.close()
    ok = all(d["a_record_frame_ms"] < d["b_omega_histogram_ms"] and d["a_record_frame_ms"] < d["c_host_path_ms"]
             for d in (ring, spread))
    print(json.dumps({
        "metric": "one recorded spectrum frame (1 x MI355X)", "nx": w["nx"], "packets": a.packets, "bins": a.bins,
        "rebin_every": args.rebin_every, "lib": os.environ.get("SWRT_LIB_PATH", "libswrt.so"),
        "ring": ring, "spread": spread, "spread_steps": a.spread_steps, "d_advance_step_ms": step_ms,
        "a_over_d_ring": ring["a_record_frame_ms"] / step_ms, "a_over_d_spread": spread["a_record_frame_ms"] / step_ms,
        "a_ring_over_spread": ring["a_record_frame_ms"] / spread["a_record_frame_ms"],
        "a_below_b_and_c": ok, "clock_ghz_observed": ghz, "clock_probe_spread": clk_spread}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
