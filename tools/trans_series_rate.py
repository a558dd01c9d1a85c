"""Cost of one recorded transition frame (swrt_trans_series_record) at the
bench's shape: 512^2, two snapshots, 1e6 packets re-binned every 20 steps;
omega classes over [f, 2.5 omega_0] in 300 bins, source classes (omega at the
mark) over the same range in ns bins.  Two ensembles, in one session:

  ring_binned  the drivers' initial ring, marked, after one bench step
               (re-binned into spatial order; every packet still in one
               source class and a few omega bins: the per-class sums' and the
               count plane's worst case)
  spread       after --spread-steps bench steps in the 512^2 blend, marked
               --lag-steps bench steps before the end

For each and each ns in --sources the median of --reps frames between two
events on the context's stream (a frame is the memsets of its planes and one
launch) after 3 warm-up frames, by what a record takes by itself ("auto": the
LDS kernel up to 16384 cells, the global one beyond) and, for the LDS shapes,
by the global kernel forced with SWRT_DEBUG_TRANS_GLOBAL.  Yardsticks of the
same ensemble, measured the same way and interleaved with them over --rounds
rounds:

  omega  swrt_omega_series_record: the spectrum series' frame of the same k
  step   one bench step (--substeps leapfrog steps)

and, once per ensemble and shape, the only route before the series:
packets_get at the mark and now, omega of both and numpy.histogram2d on the
host (--host-reps; the download at the mark is timed where it is taken).  The
shader clock observed over each ensemble's event-timed part is reported with
it (swrt_clock_ghz).  Records; gates nothing but the equality of every recorded
frame with the host binning of the two downloads.  Prints one JSON line.
usage: python tools/trans_series_rate.py [--packets N] [--reps 20] [--rounds 3]"""
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
    ap.add_argument("--lag-steps", type=int, default=20, help="bench steps between the spread ensemble's mark and its frames")
    ap.add_argument("--sources", type=int, nargs="+", default=[4, 50, 200], help="ns")
    ap.add_argument("--omega-bins", type=int, default=300)
    ap.add_argument("--frac-bits", type=int, default=20)
    a = ap.parse_args()
    import bench
    bench._imports()
    import torch

    import swraytracing_amd as sw
    from swraytracing_amd._lib import DEBUG_TRANS_GLOBAL
    from tests.trans_series_ref import omega_of, trans_frame_of
    args = bench.parse_args(["--packets", str(a.packets)])
    ctx = sw.Context(0)
    w = bench.build_workload(ctx, args, 0, a.packets, a.packets)
    ctx.set_locality(args.rebin_every, args.tile)
    ctx.set_timing(0)
    ctx.packets_set(w["x"], w["k"])
    f, gH, sub = w["f"], w["gH"], args.substeps
    Cg = float(np.sqrt(gH))
    omega0 = float(np.sqrt(f * f + gH * (w["k"][0, 0] ** 2 + w["k"][0, 1] ** 2)))
    nw = a.omega_bins
    shapes = [(ns, nw) for ns in a.sources]
    stream = torch.cuda.ExternalStream(ctx.stream())

    def edges(ns):
        return np.linspace(f, 2.5 * omega0, nw + 1), np.linspace(f, 2.5 * omega0, ns + 1)

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

    def mark():
        """The source values of the frames that follow, and the host route's download at the mark."""
        t0 = time.perf_counter()
        _, k = ctx.packets_get()
        return omega_of(k, f, Cg), (time.perf_counter() - t0) * 1e3

    def trans_timed(ns, forced, src):
        """The median of --reps recorded frames of the current packets; all the frames."""
        wedges, sedges = edges(ns)
        ctx.debug_set(DEBUG_TRANS_GLOBAL, forced)
        ctx.trans_series_begin(f, Cg, wedges, sedges, a.frac_bits)
        ctx.trans_series_mark_values(src)  # (the mark's omega, bit for bit: begin dropped the device's mark)
        ms = median_of(ctx.trans_series_record)
        frames = ctx.trans_series_get()
        ctx.debug_set(DEBUG_TRANS_GLOBAL, 0)
        ctx.trans_series_reset()
        return ms, frames

    def host_path(ns, src, mark_ms):
        wedges, sedges = edges(ns)
        t0 = time.perf_counter()
        _, k = ctx.packets_get()
        om = np.sqrt(f * f + gH * (k[:, 0] * k[:, 0] + k[:, 1] * k[:, 1]))
        np.histogram2d(src, om, bins=(sedges, wedges))
        return mark_ms + (time.perf_counter() - t0) * 1e3

    def measure(name, src, mark_ms):
        out = dict(shapes={})
        keys = [(s, forced) for s in shapes for forced in ((0, 1) if (s[0] + 2) * (s[1] + 2) <= 16384 else (0,))]
        ms = {key: [] for key in keys}
        equal = {key: True for key in keys}
        omega_ms = []
        _, k = ctx.packets_get()
        om = omega_of(k, f, Cg)
        want = {ns: trans_frame_of(src, om, *edges(ns), a.frac_bits) for ns, _ in shapes}
        ctx.omega_series_begin(f, Cg, edges(4)[0])
        ctx.clock_stamp(0)
        for _ in range(a.rounds):
            omega_ms.append(median_of(ctx.omega_series_record))
            for key in keys:
                t, frames = trans_timed(key[0][0], key[1], src)
                ms[key].append(t)
                for g, v in zip(frames, want[key[0][0]]):  # every recorded frame against the host binning
                    equal[key] &= bool((g == v[None]).all())
        ctx.omega_series_reset()
        ctx.clock_stamp(1)
        ctx.synchronize()
        try:
            out["clock_ghz_observed"], out["clock_probe_spread"] = ctx.clock_ghz()
        except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
            out["clock_ghz_observed"] = out["clock_probe_spread"] = None
        out["omega_ms"] = omega_ms
        out["omega_ms_median"] = statistics.median(omega_ms)
        for ns, _ in shapes:
            c = dict(cells=(ns + 2) * (nw + 2), kernel_of_auto="lds" if (ns + 2) * (nw + 2) <= 16384 else "global")
            ok = True
            for forced, label in ((0, "auto"), (1, "forced_global")):
                if ((ns, nw), forced) not in ms:
                    continue
                r = ms[((ns, nw), forced)]
                c[label + "_ms"] = r
                c[label + "_ms_median"] = statistics.median(r)
                c[label + "_ms_spread"] = max(r) - min(r)
                c[label + "_over_omega"] = statistics.median(r) / out["omega_ms_median"]
                ok &= equal[((ns, nw), forced)]
            c["device_equals_host_binning"] = bool(ok)
            c["occupied_cells"] = int(np.count_nonzero(want[ns][0]))
            c["occupied_source_classes"] = int(np.count_nonzero(want[ns][0].sum(axis=1)))
            c["largest_count"] = int(want[ns][0].max())
            c["rejected"] = int(want[ns][2][1])
            c["host_path_ms"] = statistics.median([host_path(ns, src, mark_ms) for _ in range(a.host_reps)])
            out["shapes"][f"{ns},{nw}"] = c
        print(f"{name}: measured", file=sys.stderr, flush=True)
        return out

    res = {}
    src, mark_ms = mark()  # the initial ring: one source class
    bench.step(ctx, w, sub)
    ctx.synchronize()
    res["ring_binned"] = measure("ring_binned", src, mark_ms)
    for i in range(a.spread_steps):
        if i == a.spread_steps - a.lag_steps:
            ctx.synchronize()
            src, mark_ms = mark()
        bench.step(ctx, w, sub)
    ctx.synchronize()
    res["spread"] = measure("spread", src, mark_ms)
    step_ms = median_of(lambda: bench.step(ctx, w, sub))
    ok = all(c["device_equals_host_binning"] for e in res.values() for c in e["shapes"].values())
    ctx.close()
    print(json.dumps({
        "metric": "one recorded transition frame (1 x MI355X)", "nx": w["nx"], "packets": a.packets,
        "omega0": omega0, "omega_bins": nw, "rebin_every": args.rebin_every, "spread_steps": a.spread_steps,
        "lag_steps": a.lag_steps, "reps": a.reps, "rounds": a.rounds, "frac_bits": a.frac_bits, "ensembles": res,
        "bench_step_ms": step_ms, "bench_substeps": sub, "leapfrog_step_ms": step_ms / sub, "all_equal": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
