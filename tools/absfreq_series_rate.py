"""Cost of one recorded absolute-frequency frame (swrt_absfreq_series_record)
at the bench's shape: 512^2, two snapshots, 1e6 packets; omega classes over
[f, 2.5 omega_0] in 300 bins, Omega classes over [f - omega_0 / 2, 3 omega_0].
Two ensembles, in one session:

  ring_binned  the drivers' initial ring after one bench step (re-binned into
               spatial order; every omega still within a few bins)
  spread       after --spread-steps more bench steps in the 512^2 blend

For each and each shape (no, nw) in --shapes the median of --reps frames
between two events on the context's stream (a frame is the memsets of its
planes and one launch) after 3 warm-up frames, by what a record takes by
itself ("auto": the LDS kernel for absfreq_lds_form's shapes, the global one
beyond) and, for the LDS shapes, by the global kernel forced with
SWRT_DEBUG_ABSFREQ_GLOBAL.  Yardsticks of the same ensemble, measured the same
way and alternating with them over --rounds rounds:

  refr   swrt_refr_series_record at the same shape: the same gather with six
         fields a snapshot instead of two, four 64-bit LDS adds per packet
         instead of five, three divisions and a square root more
  step   one bench step (--substeps leapfrog steps)

and, once per ensemble and shape, the only route before the series:
packets_get, swrt_eval on each slot and the numpy restatement on the host
(--host-reps).  The shader clock observed over each ensemble's event-timed
part is reported with it (swrt_clock_ghz).  Records; gates nothing but the
equality of the kernels' integers with the restatement on swrt_eval's records.
Prints one JSON line.
usage: python tools/absfreq_series_rate.py [--packets N] [--reps 20] [--rounds 3]"""
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
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--spread-steps", type=int, default=200, help="bench steps before the spread ensemble is timed")
    ap.add_argument("--shapes", type=str, nargs="+", default=["8,300", "50,300", "200,300"], help="no,nw")
    ap.add_argument("--frac-bits", type=int, default=20)
    a = ap.parse_args()
    import bench
    bench._imports()
    import torch

    import swraytracing_amd as sw
    from swraytracing_amd._lib import DEBUG_ABSFREQ_GLOBAL
    from tests.absfreq_series_ref import absfreq_frame_of, lds_form as ref_lds_form, packet_values
    args = bench.parse_args(["--packets", str(a.packets)])
    ctx = sw.Context(0)
    w = bench.build_workload(ctx, args, 0, a.packets, a.packets)
    ctx.set_locality(args.rebin_every, args.tile)
    ctx.set_timing(0)
    ctx.packets_set(w["x"], w["k"])
    f, gH, sub = w["f"], w["gH"], args.substeps
    Cg = float(np.sqrt(gH))
    bump, alpha, tau = sw.BUMP_QG, 0.3, 0.37
    omega0 = float(np.sqrt(f * f + gH * (w["k"][0, 0] ** 2 + w["k"][0, 1] ** 2)))
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shapes]
    stream = torch.cuda.ExternalStream(ctx.stream())

    def lds_form(no, nw):  # absfreq_lds_form (swrt_absfreq.hpp)
        return ref_lds_form(nw, no)

    def edges(no, nw):
        return np.linspace(f, 2.5 * omega0, nw + 1), np.linspace(f - 0.5 * omega0, 3.0 * omega0, no + 1)

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

    def absfreq_timed(no, nw, forced):
        """The median of --reps recorded frames of the current packets; the last frame."""
        wedges, oedges = edges(no, nw)
        ctx.debug_set(DEBUG_ABSFREQ_GLOBAL, forced)
        ctx.absfreq_series_begin(f, Cg, wedges, oedges, a.frac_bits)
        ms = median_of(lambda: ctx.absfreq_series_record(0, 1, alpha, tau, bump))
        frame = [v[0] for v in ctx.absfreq_series_get(ctx.absfreq_series_frames() - 1, 1)]
        ctx.debug_set(DEBUG_ABSFREQ_GLOBAL, 0)
        ctx.absfreq_series_reset()
        return ms, frame

    def refr_timed(na, nw):
        ctx.refr_series_begin(f, Cg, edges(na, nw)[0], np.linspace(-1.0, 1.0, na + 1), a.frac_bits)
        ms = median_of(lambda: ctx.refr_series_record(2, alpha, bump))
        ctx.refr_series_reset()
        return ms

    def host_values():
        x, k = ctx.packets_get()
        A = np.array(ctx.eval(x[:, 0], x[:, 1], nslots=1, bump=bump)[:2])
        ctx.swap_slots(0, 1)
        try:
            B = np.array(ctx.eval(x[:, 0], x[:, 1], nslots=1, bump=bump)[:2])
        finally:
            ctx.swap_slots(0, 1)
        return packet_values(A, B, alpha, tau, k, f, Cg)

    def host_path(no, nw):
        wedges, oedges = edges(no, nw)
        t0 = time.perf_counter()
        absfreq_frame_of(*host_values(), wedges, oedges, a.frac_bits)
        return (time.perf_counter() - t0) * 1e3

    def measure(name):
        out = dict(shapes={})
        keys = [(s, forced) for s in shapes for forced in ((0, 1) if lds_form(*s) else (0,))]
        ms = {key: [] for key in keys}
        refr_ms = {s: [] for s in shapes}
        frames = {}
        ctx.clock_stamp(0)
        for _ in range(a.rounds):
            for key in keys:  # (a shape's refraction and absolute-frequency records next to each other)
                if key[1] == 0:
                    refr_ms[key[0]].append(refr_timed(*key[0]))
                t, frame = absfreq_timed(*key[0], key[1])
                ms[key].append(t)
                frames.setdefault(key, []).append(frame)
        ctx.clock_stamp(1)
        ctx.synchronize()
        try:
            out["clock_ghz_observed"], out["clock_probe_spread"] = ctx.clock_ghz()
        except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
            out["clock_ghz_observed"] = out["clock_probe_spread"] = None
        vals = host_values()
        for na, nw in shapes:
            wedges, oedges = edges(na, nw)
            want = absfreq_frame_of(*vals, wedges, oedges, a.frac_bits)
            c = dict(cells=(na + 2) * (nw + 2), kernel_of_auto="lds" if lds_form(na, nw) else "global")
            c["refr_ms"] = refr_ms[(na, nw)]
            c["refr_ms_median"] = statistics.median(refr_ms[(na, nw)])
            equal = True
            for forced, label in ((0, "auto"), (1, "forced_global")):
                if ((na, nw), forced) not in ms:
                    continue
                r = ms[((na, nw), forced)]
                c[label + "_ms"] = r
                c[label + "_ms_median"] = statistics.median(r)
                c[label + "_ms_spread"] = max(r) - min(r)
                c[label + "_over_refr"] = statistics.median(r) / c["refr_ms_median"]
                # the ratio round by round (the two records alternate): its spread over the alternations
                c[label + "_over_refr_rounds"] = [t / q for t, q in zip(r, c["refr_ms"])]
                equal &= all(np.array_equal(g, v) for fr in frames[((na, nw), forced)] for g, v in zip(fr, want))
            c["device_equals_host_restatement"] = bool(equal)
            c["occupied_cells"] = int(np.count_nonzero(want[0]))
            c["occupied_omega_classes"] = int(np.count_nonzero(want[0].sum(axis=0)))
            c["largest_count"] = int(want[0].max())
            c["rejected"] = int(want[2][1])
            c["abs_row"] = want[0].sum(axis=1).tolist() if na <= 8 else None
            c["host_path_ms"] = statistics.median([host_path(na, nw) for _ in range(a.host_reps)])
            out["shapes"][f"{na},{nw}"] = c
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
    ok = all(c["device_equals_host_restatement"] for e in res.values() for c in e["shapes"].values())
    ctx.close()
    print(json.dumps({
        "metric": "one recorded absolute-frequency frame (1 x MI355X)", "nx": w["nx"], "packets": a.packets,
        "slots": [0, 1], "alpha": alpha, "tau": tau, "omega0": omega0,
        "rebin_every": args.rebin_every, "spread_steps": a.spread_steps, "reps": a.reps, "rounds": a.rounds,
        "frac_bits": a.frac_bits, "ensembles": res, "bench_step_ms": step_ms, "bench_substeps": sub,
        "leapfrog_step_ms": step_ms / sub, "all_equal": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
