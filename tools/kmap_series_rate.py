"""Cost of one recorded wave-vector plane frame (swrt_kmap_series_record) at
the bench's shape: 512^2, two snapshots, 1e6 packets, K four times the ring's
radius.  Three ensembles, in one session:

  ring_as_set  the drivers' initial ring in the order it was set (neighbouring
               lanes hold neighbouring angles: a driver's first frame)
  ring_binned  the same ring after one bench step (the packets re-binned into
               spatial order: neighbouring lanes hold unrelated wavevectors)
  spread       after --spread-steps bench steps in the 512^2 blend

For each and each m in --cells the median of --reps frames between two events
on the context's stream, per kernel (SWRT_DEBUG_KMAP_GLOBAL):

  auto      what a record takes: the LDS kernel up to m = 128, the global beyond
  merged    the global kernel with its wave-level merge
  unmerged  the global kernel, one atomic per inside packet

repeated --rounds times, against the only route before the series:
packets_get plus numpy.histogram2d and the five moment sums on the host
(--host-reps).  Yardsticks of the same ensemble: one bench step and one map
series frame at m = 128.  The shader clock observed over each ensemble's
event-timed part is reported with it (swrt_clock_ghz).  Records; gates nothing
but the equality of the kernels' integers.  Prints one JSON line.
usage: python tools/kmap_series_rate.py [--packets N] [--reps 20] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = (("auto", 0), ("merged", 2), ("unmerged", 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--spread-steps", type=int, default=200, help="bench steps before the spread ensemble is timed")
    ap.add_argument("--cells", type=int, nargs="+", default=[64, 128, 512])
    ap.add_argument("--frac-bits", type=int, default=16)
    a = ap.parse_args()
    import bench
    bench._imports()
    import torch

    import swraytracing_amd as sw
    from swraytracing_amd._lib import DEBUG_KMAP_GLOBAL
    from tests.kmap_series_ref import kmap_frame
    args = bench.parse_args(["--packets", str(a.packets)])
    ctx = sw.Context(0)
    w = bench.build_workload(ctx, args, 0, a.packets, a.packets)
    ctx.set_locality(args.rebin_every, args.tile)
    ctx.set_timing(0)
    ctx.packets_set(w["x"], w["k"])
    f, Cg, sub, L = w["f"], float(np.sqrt(w["gH"])), args.substeps, w["L"]
    ring = float(np.hypot(w["k"][0, 0], w["k"][0, 1]))
    K = 4.0 * ring
    stream = torch.cuda.ExternalStream(ctx.stream())

    def events(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            fn()
            e1.record(stream)
        ctx.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in ev]  # ms

    def timed(m, path):
        """The median of --reps recorded frames of the current packets by one kernel; the last frame."""
        ctx.debug_set(DEBUG_KMAP_GLOBAL, path)
        ctx.kmap_series_begin(K, m, a.frac_bits)
        for _ in range(3):
            ctx.kmap_series_record()
        ctx.synchronize()
        ms = statistics.median(events(ctx.kmap_series_record, a.reps))
        planes, stats = ctx.kmap_series_get(ctx.kmap_series_frames() - 1, 1)
        ctx.debug_set(DEBUG_KMAP_GLOBAL, 0)
        return ms, planes[0], stats[0]

    def host_path(m):
        """packets_get, histogram2d over the plane and the five sums: (ms, count plane)."""
        t0 = time.perf_counter()
        _, k = ctx.packets_get()
        edges = np.linspace(-K, K, m + 1)
        plane, _, _ = np.histogram2d(k[:, 0], k[:, 1], bins=(edges, edges))
        sums = [k[:, 0].sum(), k[:, 1].sum(), (k[:, 0] * k[:, 0]).sum(), (k[:, 1] * k[:, 1]).sum(),
                (k[:, 0] * k[:, 1]).sum()]
        return (time.perf_counter() - t0) * 1e3, plane, sums

    def measure(name):
        """Every device-timed figure of the current ensemble between two clock stamps, then the host path."""
        out = dict(cells={})
        _, kk = ctx.packets_get()
        dev = {}
        ctx.clock_stamp(0)
        for m in a.cells:
            r = {key: [] for key, _ in KERNELS}
            equal = True
            for _ in range(a.rounds):
                frames = []
                for key, path in KERNELS:
                    ms, plane, stats = timed(m, path)
                    r[key].append(ms)
                    frames.append((plane, stats))
                equal &= all(np.array_equal(p, frames[0][0]) and np.array_equal(s, frames[0][1]) for p, s in frames)
            dev[m] = (r, equal, frames[0])
        # yardstick on the same ensemble: a map-series frame at m = 128
        ctx.map_series_begin(L, 128, f, Cg, 20)
        for _ in range(3):
            ctx.map_series_record()
        ctx.synchronize()
        out["map_series_frame_m128_ms"] = statistics.median(events(ctx.map_series_record, a.reps))
        ctx.map_series_reset()
        ctx.clock_stamp(1)
        ctx.synchronize()
        try:
            out["clock_ghz_observed"], out["clock_probe_spread"] = ctx.clock_ghz()
        except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
            out["clock_ghz_observed"] = out["clock_probe_spread"] = None
        for m in a.cells:
            r, equal, frame = dev[m]
            want_p, want_s = kmap_frame(kk, K, m, a.frac_bits)
            host = [host_path(m)[0] for _ in range(a.host_reps)]
            c = dict(kernel_of_auto="lds" if m <= 128 else "global")
            for key, _ in KERNELS:
                c[key + "_ms"] = r[key]
                c[key + "_ms_median"] = statistics.median(r[key])
                c[key + "_ms_spread"] = max(r[key]) - min(r[key])
            c["host_path_ms"] = statistics.median(host)
            c["kernels_equal"] = bool(equal)
            c["device_equals_restatement"] = bool(np.array_equal(frame[0], want_p) and np.array_equal(frame[1], want_s))
            c["occupied_cells"] = int(np.count_nonzero(want_p))
            c["largest_count"] = int(want_p.max())
            c["outside"] = int(want_s[2])
            out["cells"][str(m)] = c
        print(f"{name}: measured", file=sys.stderr, flush=True)
        return out

    res = {}
    res["ring_as_set"] = measure("ring_as_set")
    bench.step(ctx, w, sub)
    ctx.synchronize()
    res["ring_binned"] = measure("ring_binned")
    for _ in range(a.spread_steps):
        bench.step(ctx, w, sub)
    ctx.synchronize()
    res["spread"] = measure("spread")
    step_ms = statistics.median(events(lambda: bench.step(ctx, w, sub), a.reps))
    ok = all(c["kernels_equal"] and c["device_equals_restatement"] for e in res.values() for c in e["cells"].values())
    ratio = {m: {key: res["ring_binned"]["cells"][m][key + "_ms_median"] / res["spread"]["cells"][m][key + "_ms_median"]
                 for key, _ in KERNELS} for m in res["spread"]["cells"]}
    ctx.close()
    print(json.dumps({
        "metric": "one recorded k-plane frame (1 x MI355X)", "nx": w["nx"], "packets": a.packets, "K": K,
        "ring_radius": ring, "rebin_every": args.rebin_every, "spread_steps": a.spread_steps, "reps": a.reps,
        "rounds": a.rounds, "frac_bits": a.frac_bits, "ensembles": res, "ring_binned_over_spread": ratio,
        "bench_step_ms": step_ms, "bench_substeps": sub, "all_equal": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
