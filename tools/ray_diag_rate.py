"""Cost of one recorded ray-diagnostics frame (swrt_raydiag_record) at the
bench's shape: 512^2, two snapshots, 1e6 packets, re-binned every 20 steps.
Within one session, after warm-up:

  (a) one recorded frame: median of --reps, each between two events on the
      context's stream
  (b) the same numbers without the device pass: packets_get, swrt_eval on the
      downloaded positions, the numpy arithmetic (tools/fp32_study.py:44-80);
      median host time of --host-reps (every call in it is synchronous)
  (c) one leapfrog step of advance: 5 x --reps bench steps of --substeps
      steps each between two device synchronisations (as bench.py times
      them: a split launch's second stream is not ordered before an event on
      the first), divided by the steps

and the shader clock observed over the event-timed part (swrt_clock_ghz).
Prints one JSON line; (a) < (b) is the condition, (a)/(c) is reported.
usage: python tools/ray_diag_rate.py [--packets N] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_path(ctx, w, alpha, Om0):
    """The frame through the calls that existed before swrt_raydiag_*."""
    f, gH = w["f"], w["gH"]
    x, k = ctx.packets_get()
    u, v, ux, uy, vx, vy = ctx.eval(x[:, 0], x[:, 1], nslots=2, alpha=alpha, bump=1e-10)
    k1, k2 = k[:, 0], k[:, 1]
    om = np.sqrt(f * f + gH * (k1 * k1 + k2 * k2))
    Om = om + (u * k1 + v * k2)
    if Om0 is None:
        return Om
    r = (Om - Om0) / Om0
    s1, s2 = ux - vy, vx + uy
    return np.array([r.size, np.abs(r).max(), r.sum(), (r * r).sum(), om.sum(), (vx - uy).sum(),
                     np.sqrt(s1 * s1 + s2 * s2).sum(), (vy * vy + vx * uy).sum()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--warm-steps", type=int, default=40, help="bench steps before anything is timed")
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
    sub, alpha = args.substeps, 0.5
    phys = dict(nslots=2, alpha=alpha, bump=sw.BUMP_QG)
    stream = torch.cuda.ExternalStream(ctx.stream())

    def events(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            fn()
            e1.record(stream)
        ctx.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in ev]  # ms

    for _ in range(a.warm_steps):  # the packets spread over the tiles, re-binned twice
        bench.step(ctx, w, sub)
    ctx.raydiag_mark(w["f"], w["gH"], **phys)
    Om0 = host_path(ctx, w, alpha, None)
    for _ in range(10):
        bench.step(ctx, w, sub)
    for _ in range(5):
        ctx.raydiag_record(w["f"], w["gH"], **phys)
    ctx.synchronize()

    ctx.clock_stamp(0)
    rec_ms = events(lambda: ctx.raydiag_record(w["f"], w["gH"], **phys), a.reps)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(5 * a.reps):
        bench.step(ctx, w, sub)
    ctx.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / (5 * a.reps * sub)
    rec2_ms = events(lambda: ctx.raydiag_record(w["f"], w["gH"], **phys), a.reps)
    ctx.clock_stamp(1)
    ctx.synchronize()
    try:
        ghz, spread = ctx.clock_ghz()
    except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
        ghz = spread = None

    host = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        fr_host = host_path(ctx, w, alpha, Om0)
        host.append((time.perf_counter() - t0) * 1e3)
    host_ms = statistics.median(host)
    fr_dev = ctx.raydiag_sample(w["f"], w["gH"], values=False, **phys)[1]
    ctx.close()
    # the median of --reps after the warm-up; the second set (behind the timed steps) is reported beside it
    a_ms, rec_ms, rec2_ms = statistics.median(rec_ms), min(rec_ms), statistics.median(rec2_ms)
    print(json.dumps({
        "metric": "one recorded ray-diagnostics frame (1 x MI355X)", "nx": w["nx"], "packets": a.packets,
        "rebin_every": args.rebin_every, "nslots": 2,
        "a_record_frame_ms": a_ms, "a_min_ms": rec_ms, "a_after_steps_ms": rec2_ms,
        "b_host_path_ms": host_ms, "b_all_ms": host, "c_advance_step_ms": step_ms,
        "a_over_c": a_ms / step_ms, "a_below_b": a_ms < host_ms,
        "clock_ghz_observed": ghz, "clock_probe_spread": spread,
        "frame_device": fr_dev.tolist(), "frame_host": fr_host.tolist(),
        "max_abs_r_same_bits": bool(fr_dev[1] == fr_host[1])}))
    return 0 if a_ms < host_ms else 1


if __name__ == "__main__":
    sys.exit(main())
