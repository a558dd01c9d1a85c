"""Cost of carrying the tangent map (swrt_tangent_*) at the bench's shape:
512^2, two snapshots, 1e6 packets, re-binned every 20 steps.  In one session,
alternating over --rounds rounds, the median of --reps bench steps (--substeps
leapfrog steps each) between two events on the context's stream after 3
warm-up steps, by

  tile        the default route (the LDS-tiled kernel)
  per_packet  swrt_set_kernel(1): leapfrog_kernel, the tangent kernel's model
  tangent     a live tangent set: leapfrog_tangent_kernel (M re-marked before
              every timed batch, so it never overflows)

then one recorded tangent frame (swrt_tangent_series_record, shapes --shapes
as ns,nw; "auto" and, for the LDS shapes, the global kernel forced) against
swrt_omega_series_record, and the only route without the feature: five
ensembles (the packets themselves and +-eps in x0 and in y0, the least J's
2 x 2 block needs by central differences; all of M takes nine) advanced and
downloaded, timed here as one packets_set + advance + packets_get of the same
steps, times five.  The final x and k of the three routes are compared
bit for bit.  Records; gates nothing but that equality and the frames'
equality with the numpy restatement of the device's own M.  Prints one JSON
line.
usage: python tools/tangent_rate.py [--packets N] [--reps 20] [--rounds 3]"""
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
    ap.add_argument("--shapes", type=str, nargs="+", default=["8,300", "40,300", "200,300"], help="ns,nw")
    a = ap.parse_args()
    import bench
    bench._imports()
    import torch

    import swraytracing_amd as sw
    from swraytracing_amd._lib import DEBUG_TANGENT_GLOBAL
    from tests.cond_series_ref import omega_of
    from tests.tangent_ref import tangent_frame_of
    args = bench.parse_args(["--packets", str(a.packets)])
    ctx = sw.Context(0)
    w = bench.build_workload(ctx, args, 0, a.packets, a.packets)
    ctx.set_locality(args.rebin_every, args.tile)
    ctx.set_timing(0)
    f, gH, sub = w["f"], w["gH"], args.substeps
    Cg = float(np.sqrt(gH))
    omega0 = float(np.sqrt(f * f + gH * (w["k"][0, 0] ** 2 + w["k"][0, 1] ** 2)))
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shapes]
    stream = torch.cuda.ExternalStream(ctx.stream())

    def lds_form(ns, nw):  # refr_lds_form (swrt_refr.hpp): the tangent frame has the refraction frame's tail
        return (ns + 2) * (nw + 2) <= 16384 and 8 * (4 * nw + 2 * ns + 11) + 4 * (ns + 2) * (nw + 2) <= 80 << 10

    def events(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            fn()
            e1.record(stream)
        ctx.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in ev]  # ms

    def median_of(fn, before=None):
        for _ in range(3):
            fn()
        ctx.synchronize()
        if before:
            before()
        return statistics.median(events(fn, a.reps))

    def one_step():
        bench.step(ctx, w, sub)

    def route(name):
        """The context on route `name`, the packets at the start again."""
        if ctx.tangent_live():
            ctx.tangent_end()
        ctx.set_kernel(1 if name == "per_packet" else 0)
        ctx.packets_set(w["x"], w["k"])
        if name == "tangent":
            ctx.tangent_begin()

    routes = ("tile", "per_packet", "tangent")
    step_ms = {r: [] for r in routes}
    finals = {}
    ctx.clock_stamp(0)
    for _ in range(a.rounds):
        for r in routes:
            route(r)
            step_ms[r].append(median_of(one_step, ctx.tangent_mark if r == "tangent" else None))
            finals[r] = ctx.packets_get()  # (3 + reps steps from the same start on every route)
    ctx.clock_stamp(1)
    ctx.synchronize()
    try:
        ghz, spread = ctx.clock_ghz()
    except sw.SwrtError:
        ghz = spread = None
    same = all(np.array_equal(finals[r][i], finals["tile"][i]) for r in routes for i in (0, 1))

    # frames of the set as the last round left it (reps steps of M since the mark before the timed batch)
    M, caus = ctx.tangent_get()
    _, k = ctx.packets_get()
    wv = omega_of(k, f, Cg)
    s = (M * M).sum(axis=1) / 4
    frames = {}
    equal = True
    ctx.omega_series_begin(f, Cg, np.linspace(f, 2.5 * omega0, 301))
    omega_ms = median_of(ctx.omega_series_record)
    ctx.omega_series_reset()
    for ns, nw in shapes:
        wedges = np.linspace(f, 2.5 * omega0, nw + 1)
        gedges = 2.0 ** np.linspace(0.0, max(1.0, float(np.ceil(np.log2(s[np.isfinite(s)].max())))), ns + 1)
        want = tangent_frame_of(M, caus, wv, wedges, gedges, ctx.tangent_serial())
        c = dict(cells=(ns + 2) * (nw + 2), kernel_of_auto="lds" if lds_form(ns, nw) else "global")
        for forced, label in ((0, "auto"), (1, "forced_global")):
            if forced and not lds_form(ns, nw):
                continue
            ctx.debug_set(DEBUG_TANGENT_GLOBAL, forced)
            ctx.tangent_series_begin(f, Cg, wedges, gedges)
            c[label + "_ms_median"] = median_of(ctx.tangent_series_record)
            got = [v[0] for v in ctx.tangent_series_get(ctx.tangent_series_frames() - 1, 1)]
            equal &= all(np.array_equal(g, v) for g, v in zip(got, want))
            c[label + "_over_omega_record"] = c[label + "_ms_median"] / omega_ms
            ctx.debug_set(DEBUG_TANGENT_GLOBAL, 0)
        c["occupied_cells"] = int(np.count_nonzero(want[0]))
        c["rejected"] = int(want[2][1])
        frames[f"{ns},{nw}"] = c
    J = M[:, 0] * M[:, 5] - M[:, 1] * M[:, 4]
    facts = dict(steps_since_mark=a.reps * sub, folded_share=float((J < 0).mean()),
                 caustics_per_packet=float(caus.mean()), log2_s_max=float(np.log2(s[np.isfinite(s)].max())),
                 det_minus_one_max=float(np.abs(np.linalg.det(M.reshape(-1, 4, 4)) - 1).max()))

    # the route without the feature: five ensembles advanced and downloaded, then differenced on the host
    ctx.tangent_end()
    ctx.set_kernel(0)
    t0 = time.perf_counter()
    ctx.packets_set(w["x"], w["k"])
    for _ in range(3 + a.reps):
        one_step()
    x1, k1 = ctx.packets_get()
    one_ensemble_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    _ = ((x1 - finals["tile"][0]) / 2e-6, (k1 - finals["tile"][1]) / 2e-6)  # (one column's difference quotient)
    host_diff_ms = (time.perf_counter() - t0) * 1e3
    ctx.close()

    med = {r: statistics.median(step_ms[r]) for r in routes}
    print(json.dumps({
        "metric": "tangent map: time per leapfrog step and per recorded frame (1 x MI355X)", "nx": w["nx"],
        "packets": a.packets, "nslots": 2, "rebin_every": args.rebin_every, "substeps": sub, "reps": a.reps,
        "rounds": a.rounds, "bench_step_ms": step_ms, "bench_step_ms_median": med,
        "leapfrog_step_ms": {r: med[r] / sub for r in routes},
        "tangent_over_per_packet": med["tangent"] / med["per_packet"], "tangent_over_tile": med["tangent"] / med["tile"],
        "per_packet_over_tile": med["per_packet"] / med["tile"],
        "clock_ghz_observed": ghz, "clock_probe_spread": spread,
        "routes_equal_bits": bool(same), "omega_record_ms": omega_ms, "frames": frames, "window": facts,
        "download_and_difference": dict(one_ensemble_ms=one_ensemble_ms, ensembles=5,
                                        five_ensembles_ms=5 * one_ensemble_ms, host_difference_ms_per_column=host_diff_ms,
                                        tangent_same_steps_ms=med["tangent"] * (3 + a.reps)),
        "frames_equal_restatement": bool(equal)}))
    return 0 if (same and equal) else 1


if __name__ == "__main__":
    sys.exit(main())
