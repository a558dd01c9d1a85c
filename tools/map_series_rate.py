"""Cost of one recorded map frame (swrt_map_series_record) at the bench's
shape: 512^2, two snapshots, 1e6 packets, spread by --spread-steps bench steps.
For each map size m in --cells, within one session, the median of --reps of

  (a) one recorded frame between two events on the context's stream with the
      packets binned for the LDS tile kernel: the tile path
  (b) the same on the same packets with binning switched off through
      swrt_set_locality(0, ..): the general path
  (c) the only route to a map before the series: packets_get plus the numpy
      restatement (tests/map_series_ref.py; host time, --host-reps)

repeated --rounds times (a bench step between the rounds re-bins the packets),
and the shader clock observed over the event-timed part (swrt_clock_ghz).
Prints one JSON line: per m the medians of every round, their spread
(max - min over the rounds) and whether (a) < (c), (b) < (c); for --decide-at
(m = 128) whether (a) beats (b) by more than the two spreads — the condition
under which the tile path stays in the tree.
usage: python tools/map_series_rate.py [--packets N] [--reps 20] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--spread-steps", type=int, default=200, help="bench steps before anything is timed")
    ap.add_argument("--cells", type=int, nargs="+", default=[512, 128, 32])
    ap.add_argument("--decide-at", type=int, default=128)
    ap.add_argument("--frac-bits", type=int, default=20)
    a = ap.parse_args()
    import bench
    bench._imports()
    import torch

    import swraytracing_amd as sw
    from swraytracing_amd._lib import DEBUG_MAP_STRAYS, DEBUG_MAP_TILED_FRAMES
    from tests.map_series_ref import map_frame
    args = bench.parse_args(["--packets", str(a.packets)])
    ctx = sw.Context(0)
    w = bench.build_workload(ctx, args, 0, a.packets, a.packets)
    ctx.set_locality(args.rebin_every, args.tile)
    ctx.set_timing(0)
    ctx.packets_set(w["x"], w["k"])
    f, Cg, sub, L = w["f"], float(np.sqrt(w["gH"])), args.substeps, w["L"]
    stream = torch.cuda.ExternalStream(ctx.stream())

    def events(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            fn()
            e1.record(stream)
        ctx.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in ev]  # ms

    def timed(m):
        """The median of --reps recorded frames at the current packets and locality; the last frame."""
        ctx.map_series_begin(L, m, f, Cg, a.frac_bits)
        for _ in range(3):
            ctx.map_series_record()
        ctx.synchronize()
        ms = statistics.median(events(ctx.map_series_record, a.reps))
        planes, stats = ctx.map_series(ctx.map_series_frames() - 1, 1)
        return ms, planes[0], stats[0]

    for _ in range(a.spread_steps):
        bench.step(ctx, w, sub)
    ctx.synchronize()
    res = {m: dict(a_tile_ms=[], b_general_ms=[], paths_equal=True) for m in a.cells}
    tiled0, strays0 = ctx.debug_get(DEBUG_MAP_TILED_FRAMES), ctx.debug_get(DEBUG_MAP_STRAYS)
    ctx.clock_stamp(0)
    for _ in range(a.rounds):
        bench.step(ctx, w, sub)  # (re-bins when due: the tile path's precondition)
        frames = {}
        for m in a.cells:
            before = ctx.debug_get(DEBUG_MAP_TILED_FRAMES)
            ms, frames[m], _ = timed(m)
            if ctx.debug_get(DEBUG_MAP_TILED_FRAMES) - before != a.reps + 3:
                raise SystemExit(f"m={m}: the tile path did not apply")
            res[m]["a_tile_ms"].append(ms)
        ctx.set_locality(0, args.tile)
        for m in a.cells:
            before = ctx.debug_get(DEBUG_MAP_TILED_FRAMES)
            ms, planes, _ = timed(m)
            if ctx.debug_get(DEBUG_MAP_TILED_FRAMES) != before:
                raise SystemExit(f"m={m}: the general path did not apply")
            res[m]["b_general_ms"].append(ms)
            res[m]["paths_equal"] &= bool(np.array_equal(planes, frames[m]))
        ctx.set_locality(args.rebin_every, args.tile)
    ctx.clock_stamp(1)
    ctx.synchronize()
    try:
        ghz, clk_spread = ctx.clock_ghz()
    except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
        ghz = clk_spread = None
    tiled = ctx.debug_get(DEBUG_MAP_TILED_FRAMES) - tiled0
    strays = ctx.debug_get(DEBUG_MAP_STRAYS) - strays0
    ok = True
    for m in a.cells:
        r = res[m]
        host = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            x, k = ctx.packets_get()
            want, _ = map_frame(x, k, L, m, f, Cg, a.frac_bits)
            host.append((time.perf_counter() - t0) * 1e3)
        ctx.map_series_begin(L, m, f, Cg, a.frac_bits)
        ctx.map_series_record()
        r["device_equals_host"] = bool(np.array_equal(ctx.map_series()[0][0], want))
        r["c_host_path_ms"] = statistics.median(host)
        for key in ("a_tile_ms", "b_general_ms"):
            r[key + "_median"] = statistics.median(r[key])
            r[key + "_spread"] = max(r[key]) - min(r[key])
        r["a_and_b_below_c"] = max(r["a_tile_ms"]) < r["c_host_path_ms"] and max(r["b_general_ms"]) < r["c_host_path_ms"]
        ok &= r["a_and_b_below_c"] and r["paths_equal"] and r["device_equals_host"]
    d = res.get(a.decide_at)
    keep = None
    if d is not None:
        keep = d["b_general_ms_median"] - d["a_tile_ms_median"] > d["a_tile_ms_spread"] + d["b_general_ms_spread"]
    ctx.close()
    print(json.dumps({
        "metric": "one recorded map frame (1 x MI355X)", "nx": w["nx"], "packets": a.packets,
        "rebin_every": args.rebin_every, "spread_steps": a.spread_steps, "reps": a.reps, "rounds": a.rounds,
        "frac_bits": a.frac_bits, "cells": {str(m): res[m] for m in a.cells},
        "tiled_frames": tiled, "strays_per_tiled_frame": strays / max(tiled, 1),
        "decide_at": a.decide_at, "tile_path_beats_general_beyond_spread": keep,
        "all_below_host_path_and_equal": ok, "clock_ghz_observed": ghz, "clock_probe_spread": clk_spread}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
