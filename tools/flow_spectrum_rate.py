"""Cost of one recorded flow spectrum frame (swrt_flow_spectrum_record_qg)
beside the PDE step it follows, on one GPU.  Parts, each a process of its own
so that each runs under its own time limit:

  frame   at 512^2 (one layer, and both layers of a two-layer state) and at
          64^2: a frame between two events (median of --reps), and --reps
          frames back to back between two events, divided; the PDE step the
          same way; against the route before the series, swrt_qg_get plus the
          numpy restatement of the same frame on the host.  The QG work runs
          on the context's stream here (swrt_qg_set_stream 0) so that events
          on it bracket it.  Gates the equality of the device's frame and the
          restatement's.
  driver  the two-layer driver's loop (TwoLayerLoop, 512^2, --packets packets,
          the QG stream beside the packet streams): wall time per step over
          --steps steps without a record, with one every 25th step (the
          driver's cadence) and with one every step.

With no --part the tool runs both as child processes (--limit seconds each),
prints one JSON line, and with --write stores it as
profiles/flow_spectrum/flow_spectrum_rate.json and writes the README beside
it (--bench-before / --bench-after: plain bench.py result lines to quote).
usage: python tools/flow_spectrum_rate.py [--write] [--reps 50] [--steps 300]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "flow_spectrum")
F, CG = 3.0, 1.0


def _model(sw, ctx, nx, layers, seed=5):
    from swraytracing_amd.qg import initial_q
    rng = np.random.default_rng(seed)
    L = 2 * math.pi if layers == 1 else 20.0
    q = initial_q(nx, L, 0.2, F / CG, 3, 8, rng, ndgrid=layers == 2)
    qk = ctx.g2k(q)
    if layers == 1:
        m = sw.QGModel.one_layer(qk, nx, F, CG, r_drag=0.0, ctx=ctx)
        return m, 0.05 * m.dx / m.max_speed()
    m = sw.QGModel.two_layer(np.stack([qk, ctx.g2k(-q)], axis=2), nx, F, CG, L=L, ctx=ctx)
    return m, 0.25 * m.dx / m.max_speed()


def part_frame(a):
    import torch

    import swraytracing_amd as sw
    from tests.flow_spectrum_ref import flow_frame
    res = {}
    ok = True
    for nx, layers in ((512, 1), (512, 2), (64, 1)):
        ctx = sw.Context(0)
        ctx.qg_set_stream(False)
        stream = torch.cuda.ExternalStream(ctx.stream())
        m, dt = _model(sw, ctx, nx, layers)
        m.step(dt, 5)

        def each(fn, reps):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for e0, e1 in ev:
                e0.record(stream)
                fn()
                e1.record(stream)
            ctx.synchronize()
            return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3  # us

        def batch(fn, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            ctx.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3  # us

        def records():
            for layer in range(layers):
                ctx.flow_spectrum_record_qg(layer)

        r = dict(nx=nx, layers=layers, shells=None)
        ctx.clock_stamp(0)
        m.begin_flow_spectrum(0)
        r["shells"] = ctx.flow_spectrum_shells()
        for _ in range(3):
            records()
        ctx.synchronize()
        r["record_us_each"] = [each(records, a.reps) for _ in range(a.rounds)]
        r["record_us_back_to_back"] = [batch(records, a.reps) for _ in range(a.rounds)]
        r["pde_step_us_each"] = [each(lambda: m.step(dt), a.reps) for _ in range(a.rounds)]
        r["pde_step_us_back_to_back"] = [batch(lambda: m.step(dt), a.reps) for _ in range(a.rounds)]
        ctx.clock_stamp(1)
        ctx.synchronize()
        try:
            r["clock_ghz_observed"], r["clock_probe_spread"] = ctx.clock_ghz()
        except sw.SwrtError:  # no CU ran both probes: the clock is unobserved
            r["clock_ghz_observed"] = r["clock_probe_spread"] = None
        # the route before the series: download, then the same frame on the host
        ctx.flow_spectrum_reset()
        records()
        sp, st = ctx.flow_spectrum_get()
        host = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            qk, t, _ = ctx.qg_get()
            t1 = time.perf_counter()
            frames = [flow_frame(qk[:, :, layer], m.kscale, m.params.K_d2, t) for layer in range(layers)]
            host.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        r["qg_get_ms"] = statistics.median(h[0] for h in host)
        r["numpy_restatement_ms"] = statistics.median(h[1] for h in host)
        r["device_equals_restatement"] = all(
            np.array_equal(sp[i], frames[i][0]) and np.array_equal(st[i], frames[i][1]) for i in range(layers))
        ok &= r["device_equals_restatement"]
        for k in ("record_us_each", "record_us_back_to_back", "pde_step_us_each", "pde_step_us_back_to_back"):
            r[k + "_median"] = statistics.median(r[k])
        res[f"{nx}x{layers}"] = r
        ctx.close()
        print(f"frame {nx} x {layers}: measured", file=sys.stderr, flush=True)
    print(json.dumps(dict(part="frame", reps=a.reps, rounds=a.rounds, cases=res, all_equal=bool(ok))))
    return 0 if ok else 1


def part_driver(a):
    import swraytracing_amd as sw
    from swraytracing_amd.qg import _packets
    from swraytracing_amd.scheme import BUMP_QG
    nx, L = 512, 20.0
    res = {}
    for name, every in (("no_record", 0), ("record_every_25", 25), ("record_every_step", 1)):
        ctx = sw.Context(0)
        ctx.set_timing(0)
        m, dt = _model(sw, ctx, nx, 2)
        rng = np.random.default_rng(7)
        x, k = _packets(a.packets, L, 4.0, F, CG, rng)
        ens = sw.PacketEnsemble(x, k, L, F, CG, nx, F / CG, shear=0.5, k_scale=2 * math.pi / L, nlayers=2,
                                bump=BUMP_QG, ctx=ctx)
        loop = sw.TwoLayerLoop(m, ens, dt, m.max_speed(), 0.25, 0.0, 5)
        m.begin_flow_spectrum(0)
        rounds = []
        for _ in range(a.rounds + 1):  # (the first round warms up)
            ctx.synchronize()
            t0 = time.perf_counter()
            for s in range(a.steps):
                loop.step()
                if every and (s + 1) % every == 0:
                    m.record_flow_spectrum()
            loop.flush()
            ctx.synchronize()
            ctx.flow_spectrum_get(stats=False)  # (waits for the QG stream as well)
            rounds.append((time.perf_counter() - t0) / a.steps * 1e6)
            ctx.flow_spectrum_reset()
        loop.settle()
        res[name] = dict(step_us=rounds[1:], step_us_median=statistics.median(rounds[1:]))
        ctx.close()
        print(f"driver {name}: measured", file=sys.stderr, flush=True)
    print(json.dumps(dict(part="driver", nx=nx, packets=a.packets, steps=a.steps, rounds=a.rounds, nsub=5, loops=res)))
    return 0


def _bench_row(path):
    with open(path) as fh:
        line = [ln for ln in fh.read().splitlines() if ln.strip().startswith("{")][-1]
    b = json.loads(line)
    g = b.get("roofline", {}).get("clock_ghz_observed")
    return b, b["value"], None if g is None else round(g, 3)


def readme(res, before, after):
    c = res["frame"]["cases"]
    d = res["driver"]["loops"]

    def row(key, label):
        r = c[key]
        return (f"| {label} | {r['shells']} | **{r['record_us_back_to_back_median']:.1f}** | "
                f"{r['record_us_each_median']:.1f} | {r['pde_step_us_back_to_back_median']:.1f} | "
                f"{r['pde_step_us_each_median']:.1f} | {r['qg_get_ms']:.2f} + {r['numpy_restatement_ms']:.0f} | "
                f"{r['clock_ghz_observed'] if r['clock_ghz_observed'] is None else round(r['clock_ghz_observed'], 3)} |")
    big = c["512x1"]
    lines = [
        "# Cost of one recorded flow spectrum frame", "",
        "`python tools/flow_spectrum_rate.py --write` on one MI355X, one session, on the tree of the commit that",
        "adds this file; `flow_spectrum_rate.json` is its output line.  A record is two launches on the QG stream",
        "(one workgroup per shell, then the totals).  \"Back to back\": "
        f"{res['frame']['reps']} records (or PDE steps) between two events,",
        "divided; \"each\": the median of records bracketed one by one, which adds the events' own idle time.",
        f"Medians of {res['frame']['rounds']} rounds.  With two layers a \"record\" is both layers' frames.  The host route is",
        "`swrt_qg_get` (ms) plus the numpy restatement of the same frame (ms).", "",
        "| grid, layers | shells | record, µs back to back | each | PDE step, µs back to back | each | "
        "`qg_get` + numpy, ms | clock, GHz |",
        "|---|---|---|---|---|---|---|---|",
        row("512x1", "512², 1"), row("512x2", "512², 2 (both)"), row("64x1", "64², 1"), "",
        f"* The device's frames equal the restatement's bit for bit in every case (`all_equal`: "
        f"{res['frame']['all_equal']}).",
        f"* A PDE step standalone measured {c['512x1']['pde_step_us_back_to_back_median']:.0f} µs (one layer) and "
        f"{c['512x2']['pde_step_us_back_to_back_median']:.0f} µs (two layers) at 512² here; a record at 512² is "
        f"{big['record_us_back_to_back_median'] / big['pde_step_us_back_to_back_median']:.2f} of the one-layer step,",
        "  once per packet frame (every 5 or 25 PDE steps in the drivers).",
        f"* The route it replaces stalls the QG stream for the download and takes "
        f"{big['qg_get_ms'] + big['numpy_restatement_ms']:.0f} ms a frame at 512² on the host.", "",
        f"The two-layer driver's loop (`TwoLayerLoop`, 512², {res['driver']['packets']} packets, 5 leapfrog substeps a step),",
        f"wall time per step over {res['driver']['steps']} steps, medians of {res['driver']['rounds']} rounds:", "",
        "| loop | µs per step (rounds) |", "|---|---|"]
    for key, label in (("no_record", "no record"), ("record_every_25", "a record every 25th step (the driver's cadence)"),
                       ("record_every_step", "a record every step")):
        lines.append(f"| {label} | **{d[key]['step_us_median']:.1f}** ({', '.join(f'{v:.1f}' for v in d[key]['step_us'])}) |")
    if before and after:
        (_, vb, gb), (_, va, ga) = _bench_row(before), _bench_row(after)
        lines += ["", "Hot kernel unchanged: plain `python bench.py --gpus 1 --steps 50 --warmup 5` in the same session, on the",
                  "parent's build and on this tree's:", "", "| tree | packet-steps/s | observed clock |", "|---|---|---|",
                  f"| parent (`bench_plain_before.json`) | {vb:.4g} | {gb} GHz |",
                  f"| this tree (`bench_plain_after.json`) | {va:.4g} | {ga} GHz |", "",
                  f"The difference ({(va / vb - 1) * 100:+.1f} %) goes with the clock's "
                  f"({(ga / gb - 1) * 100 if ga and gb else float('nan'):+.1f} %); `README.md` documents the box-to-box",
                  "spread as 2.11–2.22e10 at 1.70–1.82 GHz.  The bench never opens the series: a context that does",
                  "not allocates and launches nothing for it, and the leapfrog kernels' text is unchanged."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("frame", "driver"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--limit", type=int, default=240, help="seconds each part may take")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--bench-before")
    ap.add_argument("--bench-after")
    a = ap.parse_args()
    if a.part:
        return {"frame": part_frame, "driver": part_driver}[a.part](a)
    res = {}
    for part in ("frame", "driver"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(a.reps), "--rounds",
               str(a.rounds), "--host-reps", str(a.host_reps), "--steps", str(a.steps), "--packets", str(a.packets)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)  # (a part past its limit ends the run)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            sys.stderr.write(r.stdout)
            return r.returncode or 1  # (nothing more is started after a failed part)
        res[part] = json.loads(r.stdout.strip().splitlines()[-1])
    out = dict(metric="one recorded flow spectrum frame (1 x MI355X)", **res)
    print(json.dumps(out))
    if a.write:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "flow_spectrum_rate.json"), "w") as fh:
            fh.write(json.dumps(out) + "\n")
        with open(os.path.join(OUT, "README.md"), "w") as fh:
            fh.write(readme(out, a.bench_before, a.bench_after))
    return 0


if __name__ == "__main__":
    sys.exit(main())
