"""Cost of one recycle event (swrt_recycle_apply) and of the re-binning it
forces, at the bench's shape: 512^2, two snapshots, 1e6 packets re-binned
every 20 steps (4 bench steps of 5 leapfrog steps).  The ensemble is spread by
--spread-steps bench steps first; home is half the initial wavevector (omega
about 6.7, inside every cut used), and the cuts are the spread ensemble's
omega quantiles that absorb about 0 %, 1 % and 20 % of the packets.

An event changes the packets, so every timed repetition starts from the same
saved state: packets_set, recycle_begin and bench steps (untimed) that re-bin
the packets into spatial order and a host synchronisation, then the timed part
between two events on the context's stream (so every figure, the yardsticks'
too, includes the host's launch latency of its first launch).  Per cut,
medians of --reps repetitions after 3 warm-ups, over --rounds rounds
interleaved with the yardsticks:

  apply          swrt_recycle_apply alone (the frame's memset and one launch),
                 after one bench step
  next_mid       the bench step after an apply in mid-cycle (5 of 20 steps
                 done: without the apply it would not re-bin), and the same
                 step without an apply
  next_boundary  the bench step after an apply at a cycle boundary (20 of 20
                 steps done: it re-bins either way), and without

Yardsticks of the same state, measured the same way:

  omega  swrt_omega_series_record: the same 16 B-per-packet pass, reading only
  step   one bench step in mid-cycle (--substeps leapfrog steps), both part
         launches inside the timed interval
  host   the only route before: packets_get, the numpy restatement of the
         event, packets_set (wall clock, --host-reps)

The shader clock observed over the event-timed part is reported with it
(swrt_clock_ghz).  Records; gates nothing but the equality of one event per
cut with the numpy restatement (packets, generations and frame).  Prints one
JSON line.
usage: python tools/recycle_rate.py [--packets N] [--reps 20] [--rounds 3]"""
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
    ap.add_argument("--spread-steps", type=int, default=200, help="bench steps before the ensemble is saved")
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.0, 0.01, 0.2], help="absorbed, about")
    ap.add_argument("--frac-bits", type=int, default=20)
    a = ap.parse_args()
    import bench
    bench._imports()
    import torch

    import swraytracing_amd as sw
    from tests.recycle_ref import omega_of, recycle_event
    args = bench.parse_args(["--packets", str(a.packets)])
    ctx = sw.Context(0)
    w = bench.build_workload(ctx, args, 0, a.packets, a.packets)
    ctx.set_locality(args.rebin_every, args.tile)
    ctx.set_timing(0)
    f, gH, sub, L = w["f"], w["gH"], args.substeps, w["L"]
    Cg = float(np.sqrt(gH))
    cycle = args.rebin_every // sub  # bench steps per re-binning cycle
    home = 0.5 * w["k"]
    stream = torch.cuda.ExternalStream(ctx.stream())
    ctx.packets_set(w["x"], w["k"])
    for _ in range(a.spread_steps):
        bench.step(ctx, w, sub)
    xs, ks = ctx.packets_get()
    om = omega_of(ks, f, Cg)
    cuts = {fr: (2.0 * float(om.max()) if fr <= 0 else float(np.quantile(om, 1.0 - fr))) for fr in a.fractions}
    n = a.packets
    zeros = np.zeros(n, dtype=np.int32)

    def restore(cut, steps):
        """The saved ensemble, recycling begun, `steps` bench steps into a cycle (re-binned at its start)."""
        ctx.packets_set(xs, ks)
        ctx.recycle_begin(f, Cg, cut, L, seed=1, frac_bits=a.frac_bits, home_k=home)
        for _ in range(steps):
            bench.step(ctx, w, sub)

    def timed(prepare, fn):
        prepare()
        ctx.synchronize()  # (the extra packet stream's parts too: the timed call would wait for them)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        ctx.synchronize()
        return e0.elapsed_time(e1)  # ms

    def median_of(prepare, fn):
        for _ in range(3):
            timed(prepare, fn)
        return statistics.median(timed(prepare, fn) for _ in range(a.reps))

    def step():
        """One bench step, the extra packet stream's part joined into the timed stream (a get of no frame
        queues nothing else), so that the closing event covers both parts."""
        bench.step(ctx, w, sub)
        ctx.recycle_get(0, 0)

    def applied(cut, steps):
        def prepare():
            restore(cut, steps)
            ctx.recycle_apply()
        return prepare

    def check(cut):
        """One event after one bench step against the restatement of it."""
        restore(cut, 1)
        x1, k1 = ctx.packets_get()  # (drops nothing: the state stays)
        ctx.recycle_apply()
        x2, k2 = ctx.packets_get()
        gen, born = ctx.recycle_state()
        frame = ctx.recycle_get()[0]
        want = recycle_event(x1, k1, home, zeros, zeros, 1, f, Cg, cut, L, 1, 0, a.frac_bits)
        ok = all(np.array_equal(np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(v).view(np.uint64))
                 for g, v in ((x2, want[0]), (k2, want[1])))
        return bool(ok and np.array_equal(gen, want[2]) and np.array_equal(born, want[3])
                    and np.array_equal(frame, want[4])), frame

    def host_route(cut):
        restore(cut, 1)
        ctx.synchronize()
        t0 = time.perf_counter()
        x1, k1 = ctx.packets_get()
        x2, k2, _, _, _ = recycle_event(x1, k1, home, zeros, zeros, 1, f, Cg, cut, L, 1, 0, a.frac_bits)
        ctx.packets_set(x2, k2)
        return (time.perf_counter() - t0) * 1e3

    res = {}
    omega_ms, step_ms = [], []
    keys = ("apply", "next_mid_after_apply", "next_mid_plain", "next_boundary_after_apply", "next_boundary_plain")
    ms = {fr: {key: [] for key in keys} for fr in a.fractions}
    equal, frames = {}, {}
    for fr in a.fractions:
        equal[fr], frames[fr] = check(cuts[fr])
    ctx.omega_series_begin(f, Cg, np.linspace(f, 2.0 * float(om.max()), 301))
    ctx.clock_stamp(0)
    for _ in range(a.rounds):
        omega_ms.append(median_of(lambda: restore(cuts[a.fractions[0]], 1), ctx.omega_series_record))
        ctx.omega_series_reset()
        step_ms.append(median_of(lambda: restore(cuts[a.fractions[0]], 1), step))
        for fr in a.fractions:
            cut = cuts[fr]
            ms[fr]["apply"].append(median_of(lambda: restore(cut, 1), ctx.recycle_apply))
            ms[fr]["next_mid_after_apply"].append(median_of(applied(cut, 1), step))
            ms[fr]["next_mid_plain"].append(median_of(lambda: restore(cut, 1), step))
            ms[fr]["next_boundary_after_apply"].append(median_of(applied(cut, cycle), step))
            ms[fr]["next_boundary_plain"].append(median_of(lambda: restore(cut, cycle), step))
        print("round measured", file=sys.stderr, flush=True)
    ctx.clock_stamp(1)
    ctx.synchronize()
    try:
        clock, clock_spread = ctx.clock_ghz()
    except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
        clock = clock_spread = None
    omega_med, step_med = statistics.median(omega_ms), statistics.median(step_ms)
    for fr in a.fractions:
        c = dict(omega_cut=cuts[fr], frame=frames[fr].tolist(), absorbed_fraction=float(frames[fr][1]) / n,
                 device_equals_restatement=equal[fr])
        for key in keys:
            r = ms[fr][key]
            c[key + "_ms"] = r
            c[key + "_ms_median"] = statistics.median(r)
            c[key + "_ms_spread"] = max(r) - min(r)
        c["apply_over_omega"] = c["apply_ms_median"] / omega_med
        c["rebin_extra_mid_ms"] = c["next_mid_after_apply_ms_median"] - c["next_mid_plain_ms_median"]
        c["rebin_extra_boundary_ms"] = c["next_boundary_after_apply_ms_median"] - c["next_boundary_plain_ms_median"]
        c["host_route_ms"] = statistics.median([host_route(cuts[fr]) for _ in range(a.host_reps)])
        res[f"{fr:g}"] = c
    ok = all(equal.values())
    ctx.close()
    print(json.dumps({
        "metric": "one recycle event and the re-binning it forces (1 x MI355X)", "nx": w["nx"], "packets": n,
        "rebin_every": args.rebin_every, "bench_substeps": sub, "spread_steps": a.spread_steps, "reps": a.reps,
        "rounds": a.rounds, "frac_bits": a.frac_bits, "omega_min_max": [float(om.min()), float(om.max())],
        "cuts": res, "omega_ms": omega_ms, "omega_ms_median": omega_med, "bench_step_ms": step_ms,
        "bench_step_ms_median": step_med, "leapfrog_step_ms": step_med / sub, "clock_ghz_observed": clock,
        "clock_probe_spread": clock_spread, "all_equal": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
