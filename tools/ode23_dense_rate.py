"""Cost of ode23's output at requested times at the bench's shape: 512^2, two
snapshots, 1e6 packets on the binned tile path.  Within one session, after
warm-up, each number the median of --reps between two events on the
context's stream:

  (a) one plain attempt (swrt_ode23_attempt: the fused stages 2-4, its max
      copied back) against one dense attempt (swrt_ode23_set_dense 1: the same
      launch also stores F2 and F3, 64 B per packet), alternating
  (b) swrt_ode23_ntrp of that step for 1, 2, 4, 8 frames (one launch) and 16
      (two launches): from bytes alone a launch reads y, F1..F4, ynew and the
      permutation (196 B per packet) once and writes 32 B per packet and frame

and the shader clock observed over the timed part (swrt_clock_ghz).  The
attempts are never accepted, so every repetition does the same work.  Prints
one JSON line.
usage: python tools/ode23_dense_rate.py [--packets N] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
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
    stream = torch.cuda.ExternalStream(ctx.stream())
    f, Cg, dt = w["f"], float(np.sqrt(w["gH"])), w["dt"]
    thr, bump = 1e-6 / 1e-3, sw.BUMP_QG

    def events(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            fn()
            e1.record(stream)
        ctx.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in ev]  # ms

    for _ in range(a.warm_steps):  # the packets spread over the tiles
        bench.step(ctx, w, args.substeps)
    ctx.history_reset()
    # one driver interval [0, dt] with alpha = t/dt; the step a tenth of it (MaxStep)
    t, h = 0.0, 0.1 * dt
    tnew = t + h
    ctx.ode23_f1(t, dt, f, Cg, 2, thr, bump)  # (re-bins into the ode23 tiles, sorts, F1)

    def attempt(dense):
        ctx.ode23_set_dense(dense)
        return ctx.ode23_attempt(t, h, tnew, dt, f, Cg, 2, thr, bump)

    for _ in range(5):
        attempt(0)
        attempt(1)
    frame_counts = (1, 2, 4, 8, 16)
    touts = {nf: t + h * (np.arange(nf) + 0.5) / nf for nf in frame_counts}
    ctx.ode23_ntrp(t, tnew, touts[16])  # (the history's capacity)
    ctx.synchronize()

    ctx.clock_stamp(0)
    plain, dense = [], []
    for _ in range(a.reps):
        plain += events(lambda: attempt(0), 1)
        dense += events(lambda: attempt(1), 1)
    raw_plain, raw_dense = attempt(0), attempt(1)
    ntrp = {}
    for nf in frame_counts:
        def one(nf=nf):
            ctx.history_reset()
            ctx.ode23_ntrp(t, tnew, touts[nf])
        one()
        ntrp[nf] = events(one, a.reps)
    ctx.clock_stamp(1)
    ctx.synchronize()
    try:
        ghz, spread = ctx.clock_ghz()
    except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
        ghz = spread = None
    ctx.ode23_set_dense(0)
    ctx.close()
    n = a.packets
    med = statistics.median
    out = {
        "metric": "ode23 dense attempt and ntrp launches (1 x MI355X)", "nx": w["nx"], "packets": n, "nslots": 2,
        "reps": a.reps, "plain_attempt_ms": med(plain), "plain_min_ms": min(plain), "plain_max_ms": max(plain),
        "dense_attempt_ms": med(dense), "dense_min_ms": min(dense), "dense_max_ms": max(dense),
        "dense_over_plain": med(dense) / med(plain), "same_error_max": bool(raw_plain == raw_dense),
        "ntrp_ms": {str(nf): med(v) for nf, v in ntrp.items()},
        "ntrp_min_ms": {str(nf): min(v) for nf, v in ntrp.items()},
        "ntrp_gb_per_s": {str(nf): ((196 * -(-nf // 8) + 32 * nf) * n) / (med(v) * 1e-3) / 1e9 for nf, v in ntrp.items()},
        "clock_ghz_observed": ghz, "clock_probe_spread": spread,
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
