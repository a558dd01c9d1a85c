"""Cost of one recorded track frame (swrt_track_record) at the bench's shape:
512^2, two snapshots, 1e6 packets, spread by --spread-steps bench steps.  For
each number of tracked packets m in --tracked, within one session, the median
of --reps of

  (a) one recorded frame (two snapshots, alpha 0.5) between two events on the
      context's stream
  (b) the only route to those rows before the series: packets_get +
      raydiag_sample(values=True) + numpy indexing (host time, --host-reps)

repeated --rounds times with a bench step in between, one leapfrog step of
swrt_advance between two events in every round for scale, and the shader clock
observed over the event-timed part (swrt_clock_ghz).  Prints one JSON line:
per m the medians of every round, their spread (max - min over the rounds),
whether (a)'s frame equals (b)'s rows bit for bit, and for --decide-at
(m = 1024) whether (a) is shorter than (b) by more than the two spreads.
usage: python tools/track_series_rate.py [--packets N] [--reps 20] [--rounds 5]"""
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
    ap.add_argument("--tracked", type=int, nargs="+", default=[64, 1024, 16384])
    ap.add_argument("--decide-at", type=int, default=1024)
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
    f, gH, sub, bump = w["f"], w["gH"], args.substeps, sw.BUMP_QG
    phys = dict(nslots=2, alpha=0.5, bump=bump)
    stream = torch.cuda.ExternalStream(ctx.stream())
    rng = np.random.default_rng(7)
    ids = {m: rng.choice(a.packets, m, replace=False) for m in a.tracked}

    def events(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            fn()
            e1.record(stream)
        ctx.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in ev]  # ms

    def record():
        ctx.track_record(f, gH, **phys)

    def host_route(m):
        x, k = ctx.packets_get()
        s4, _ = ctx.raydiag_sample(f, gH, values=True, **phys)
        i = ids[m]
        return np.concatenate([x[i].T, k[i].T, s4[i].T])

    for _ in range(a.spread_steps):
        bench.step(ctx, w, sub)
    ctx.synchronize()
    res = {m: dict(a_record_ms=[], b_download_ms=[], record_equals_download=True) for m in a.tracked}
    step_ms = []
    ctx.clock_stamp(0)
    for _ in range(a.rounds):
        bench.step(ctx, w, sub)
        for m in a.tracked:
            ctx.track_begin(ids[m])
            for _ in range(3):
                record()
            ctx.synchronize()
            res[m]["a_record_ms"].append(statistics.median(events(record, a.reps)))
        step_ms.append(statistics.median(events(lambda: bench.step(ctx, w, sub), a.reps)) / sub)
    ctx.clock_stamp(1)
    ctx.synchronize()
    try:
        ghz, clk_spread = ctx.clock_ghz()
    except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
        ghz = clk_spread = None
    for _ in range(a.rounds):
        for m in a.tracked:
            host = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                want = host_route(m)
                host.append((time.perf_counter() - t0) * 1e3)
            res[m]["b_download_ms"].append(statistics.median(host))
            ctx.track_begin(ids[m])
            record()
            got = ctx.track_series()[0]
            res[m]["record_equals_download"] &= bool(np.array_equal(got.view(np.uint64),
                                                                    np.ascontiguousarray(want).view(np.uint64)))
        bench.step(ctx, w, sub)
    ok = True
    for m in a.tracked:
        r = res[m]
        for key in ("a_record_ms", "b_download_ms"):
            r[key + "_median"] = statistics.median(r[key])
            r[key + "_spread"] = max(r[key]) - min(r[key])
        r["a_below_b_beyond_spread"] = bool(r["b_download_ms_median"] - r["a_record_ms_median"]
                                            > r["a_record_ms_spread"] + r["b_download_ms_spread"])
        r["frame_bytes"] = 64 * m
        ok &= r["record_equals_download"]
    d = res.get(a.decide_at)
    ctx.close()
    print(json.dumps({
        "metric": "one recorded track frame (1 x MI355X)", "nx": w["nx"], "packets": a.packets,
        "rebin_every": args.rebin_every, "spread_steps": a.spread_steps, "reps": a.reps, "rounds": a.rounds,
        "nslots": 2, "tracked": {str(m): res[m] for m in a.tracked},
        "leapfrog_step_ms": step_ms, "leapfrog_step_ms_median": statistics.median(step_ms),
        "compulsory_bytes_per_frame": 8 * a.packets,
        "decide_at": a.decide_at,
        "record_shorter_than_download_beyond_spread": None if d is None else d["a_below_b_beyond_spread"],
        "all_frames_equal_the_download": ok, "clock_ghz_observed": ghz, "clock_probe_spread": clk_spread}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
