"""Cost of one recorded conditional spectrum frame (swrt_cond_series_record)
at the bench's shape: 512^2, two snapshots, 1e6 packets; omega classes over
[f, 2.5 omega_0] in 300 bins, vorticity classes over half the gridded flow's
largest |zeta| either way.  Two ensembles, in one session:

  ring_binned  the drivers' initial ring after one bench step (re-binned into
               spatial order; every omega still within a few bins)
  spread       after --spread-steps more bench steps in the 512^2 blend

For each and each shape (nq, nw) in --shapes the median of --reps frames
between two events on the context's stream (a frame is the memsets of its
planes and one launch) after 3 warm-up frames, by what a record takes by
itself ("auto": the LDS kernel up to 16384 cells, the global one beyond) and,
for the LDS shapes, by the global kernel forced with SWRT_DEBUG_COND_GLOBAL.
Yardsticks of the same ensemble, measured the same way and interleaved with
them over --rounds rounds:

  pair   swrt_raydiag_record and swrt_omega_series_record back to back: the
         device cost of the same two quantities without joining them
  step   one bench step (--substeps leapfrog steps)

and, once per ensemble, the only route before the series: packets_get,
raydiag_sample and numpy.histogram2d on the host (--host-reps).  The shader
clock observed over each ensemble's event-timed part is reported with it
(swrt_clock_ghz).  Records; gates nothing but the equality of the kernels'
integers with the binning of raydiag_sample's column on the host.  Prints one
JSON line.
usage: python tools/cond_series_rate.py [--packets N] [--reps 20] [--rounds 3]"""
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--spread-steps", type=int, default=200, help="bench steps before the spread ensemble is timed")
    ap.add_argument("--shapes", type=str, nargs="+", default=["8,300", "50,300", "200,300"], help="nq,nw")
    ap.add_argument("--frac-bits", type=int, default=20)
    a = ap.parse_args()
    import bench
    bench._imports()
    import torch

    import swraytracing_amd as sw
    from swraytracing_amd._lib import DEBUG_COND_GLOBAL
    from tests.cond_series_ref import cond_frame_of, omega_of
    args = bench.parse_args(["--packets", str(a.packets)])
    ctx = sw.Context(0)
    w = bench.build_workload(ctx, args, 0, a.packets, a.packets)
    ctx.set_locality(args.rebin_every, args.tile)
    ctx.set_timing(0)
    ctx.packets_set(w["x"], w["k"])
    f, gH, sub = w["f"], w["gH"], args.substeps
    Cg = float(np.sqrt(gH))
    bump, alpha = sw.BUMP_QG, 0.3
    p = ctx.get_field_grid(0, w["nx"])
    zmax = float(np.abs(p[4] - p[3]).max())
    omega0 = float(np.sqrt(f * f + gH * (w["k"][0, 0] ** 2 + w["k"][0, 1] ** 2)))
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shapes]
    stream = torch.cuda.ExternalStream(ctx.stream())

    def edges(nq, nw):
        return np.linspace(f, 2.5 * omega0, nw + 1), 0.5 * zmax * np.linspace(-1.0, 1.0, nq + 1)

    def events(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            fn()
            e1.record(stream)
        ctx.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in ev]  # ms

    def median_of(fn):
        for _ in range(3):
            fn()
        ctx.synchronize()
        return statistics.median(events(fn, a.reps))

    def cond_timed(nq, nw, forced):
        """The median of --reps recorded frames of the current packets; the last frame."""
        wedges, qedges = edges(nq, nw)
        ctx.debug_set(DEBUG_COND_GLOBAL, forced)
        ctx.cond_series_begin(f, Cg, wedges, 0, qedges, a.frac_bits)
        ms = median_of(lambda: ctx.cond_series_record(2, alpha, bump))
        frame = [v[0] for v in ctx.cond_series_get(ctx.cond_series_frames() - 1, 1)]
        ctx.debug_set(DEBUG_COND_GLOBAL, 0)
        ctx.cond_series_reset()
        return ms, frame

    def pair():
        ctx.raydiag_record(f, gH, nslots=2, alpha=alpha, bump=bump)
        ctx.omega_series_record()

    def host_path(nq, nw):
        wedges, qedges = edges(nq, nw)
        t0 = time.perf_counter()
        _, k = ctx.packets_get()
        s4, _ = ctx.raydiag_sample(f, gH, nslots=2, alpha=alpha, bump=bump)
        om = np.sqrt(f * f + gH * (k[:, 0] * k[:, 0] + k[:, 1] * k[:, 1]))
        np.histogram2d(s4[:, 1], om, bins=(qedges, wedges))
        return (time.perf_counter() - t0) * 1e3

    def measure(name):
        out = dict(shapes={})
        keys = [(s, forced) for s in shapes for forced in ((0, 1) if (s[0] + 2) * (s[1] + 2) <= 16384 else (0,))]
        ms = {key: [] for key in keys}
        frames = {}
        pair_ms = []
        ctx.omega_series_begin(f, Cg, edges(8, 300)[0])
        ctx.clock_stamp(0)
        for _ in range(a.rounds):
            pair_ms.append(median_of(pair))
            for key in keys:
                t, frame = cond_timed(*key[0], key[1])
                ms[key].append(t)
                frames.setdefault(key, []).append(frame)
        ctx.raydiag_series_reset()
        ctx.omega_series_reset()
        ctx.clock_stamp(1)
        ctx.synchronize()
        try:
            out["clock_ghz_observed"], out["clock_probe_spread"] = ctx.clock_ghz()
        except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
            out["clock_ghz_observed"] = out["clock_probe_spread"] = None
        out["pair_ms"] = pair_ms
        out["pair_ms_median"] = statistics.median(pair_ms)
        _, k = ctx.packets_get()
        s4, _ = ctx.raydiag_sample(f, gH, nslots=2, alpha=alpha, bump=bump)
        om = omega_of(k, f, Cg)
        for nq, nw in shapes:
            wedges, qedges = edges(nq, nw)
            want = cond_frame_of(s4[:, 1], om, wedges, qedges, a.frac_bits)
            c = dict(cells=(nq + 2) * (nw + 2), kernel_of_auto="lds" if (nq + 2) * (nw + 2) <= 16384 else "global")
            equal = True
            for forced, label in ((0, "auto"), (1, "forced_global")):
                if ((nq, nw), forced) not in ms:
                    continue
                r = ms[((nq, nw), forced)]
                c[label + "_ms"] = r
                c[label + "_ms_median"] = statistics.median(r)
                c[label + "_ms_spread"] = max(r) - min(r)
                c[label + "_over_pair"] = statistics.median(r) / out["pair_ms_median"]
                equal &= all(np.array_equal(g, v) for fr in frames[((nq, nw), forced)] for g, v in zip(fr, want))
            c["device_equals_host_binning"] = bool(equal)
            c["occupied_cells"] = int(np.count_nonzero(want[0]))
            c["largest_count"] = int(want[0].max())
            c["rejected"] = int(want[2][1])
            c["host_path_ms"] = statistics.median([host_path(nq, nw) for _ in range(a.host_reps)])
            out["shapes"][f"{nq},{nw}"] = c
        print(f"{name}: measured", file=sys.stderr, flush=True)
        return out

    res = {}
    bench.step(ctx, w, sub)
    ctx.synchronize()
    res["ring_binned"] = measure("ring_binned")
    for _ in range(a.spread_steps):
        bench.step(ctx, w, sub)
    ctx.synchronize()
    res["spread"] = measure("spread")
    step_ms = median_of(lambda: bench.step(ctx, w, sub))
    ok = all(c["device_equals_host_binning"] for e in res.values() for c in e["shapes"].values())
    ctx.close()
    print(json.dumps({
        "metric": "one recorded conditional spectrum frame (1 x MI355X)", "nx": w["nx"], "packets": a.packets,
        "which": "zeta", "nslots": 2, "alpha": alpha, "zeta_grid_max": zmax, "omega0": omega0,
        "rebin_every": args.rebin_every, "spread_steps": a.spread_steps, "reps": a.reps, "rounds": a.rounds,
        "frac_bits": a.frac_bits, "ensembles": res, "bench_step_ms": step_ms, "bench_substeps": sub,
        "leapfrog_step_ms": step_ms / sub, "all_equal": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
