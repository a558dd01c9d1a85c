"""Cost and accuracy of the packet-step schemes (swrt_set_integrator) on the
device, in one process.

Rate, at the bench's shape (512^2, two snapshots, 1e6 packets, fp64): the time
of a composite step under the Euler kick (today's step), the midpoint kick
with 1, 2 and 4 iterations, Yoshida (2 and 4) and Suzuki (4).  Each figure is
the HIP-event time of --bench-steps bench steps of --substeps composite steps
(at least 100 steps) after --warmup bench steps, from the same initial
ensemble, the schemes alternating over --rounds rounds; each is reported as a
multiple of the Euler step of the same run beside its operation count,
(full gathers + u,v gathers) per step = S*(1 + it).

Accuracy: max|Omega - Omega0|/Omega0 of the device's own raydiag series on the
steady case of tests/integrator_ref.py (nx = 64, 64 packets, T = 2), and, for
a flow blended between two snapshots (nx = 32, alpha 0 -> 1 over T = 4), the
distance of the final k from a fine Suzuki run — one field at one resolution
each.  Records; gates nothing.  Prints one JSON line.
usage: python tools/integrator_rate.py [--packets N] [--rounds 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (kick, iterations, composition)
SCHEMES = {"euler": (0, 1, 0), "midpoint_it1": (1, 1, 0), "midpoint_it2": (1, 2, 0), "midpoint_it4": (1, 4, 0),
           "yoshida_it2": (1, 2, 1), "yoshida_it4": (1, 4, 1), "suzuki_it4": (1, 4, 2),
           "yoshida_over_euler": (0, 1, 1)}


def gathers(kick, it, comp):
    S = (1, 3, 5)[comp]
    return S, S * (it if kick else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import bench
    bench._imports()
    import torch

    import swraytracing_amd as sw
    from tests import integrator_ref as ref
    args = bench.parse_args(["--packets", str(a.packets)])
    ctx = sw.Context(0)
    w = bench.build_workload(ctx, args, 0, a.packets, a.packets)
    ctx.set_locality(args.rebin_every, args.tile)
    ctx.set_timing(0)
    sub = args.substeps
    stream = torch.cuda.ExternalStream(ctx.stream())

    def timed(integ):
        """ms per composite step: --bench-steps bench steps from the initial ensemble."""
        ctx.set_integrator(*integ)
        ctx.packets_set(w["x"], w["k"])
        for _ in range(a.warmup):
            bench.step(ctx, w, sub)
        ctx.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.bench_steps):
            bench.step(ctx, w, sub)
        ctx.synchronize()  # (joins the second packet stream into the context's)
        e1.record(stream)
        e1.synchronize()
        x, k = ctx.packets_get()
        assert np.isfinite(x).all() and np.isfinite(k).all()
        return e0.elapsed_time(e1) / (a.bench_steps * sub * w.get("intervals", 1))

    ms = {n: [] for n in SCHEMES}
    for _ in range(a.rounds):
        for n, integ in SCHEMES.items():
            ms[n].append(timed(integ))
        print("round done", file=sys.stderr, flush=True)
    rate = {}
    for n, integ in SCHEMES.items():
        full, uv = gathers(*integ)
        rate[n] = dict(integrator=list(integ), full_gathers=full, uv_gathers=uv, ms_per_step=ms[n],
                       ms_per_step_median=statistics.median(ms[n]),
                       over_euler=statistics.median(ms[n]) / statistics.median(ms["euler"]),
                       over_euler_rounds=[t / e for t, e in zip(ms[n], ms["euler"])])
    ctx.set_integrator(0, 1, 0)

    # accuracy, steady: the device's own Omega series
    methods = {"leapfrog": "euler", "midpoint": "midpoint_it2", "yoshida4": "yoshida_it4", "suzuki4": "suzuki_it4"}
    c = ref.steady_case()
    sch = sw.SpectralScheme(c["L"], c["nx"], c["psi"], bump=ref.BUMP, ctx=ctx)
    x0, k0 = c["x0"].T[None], c["k0"].T[None]
    steady = {}
    for m, rn in methods.items():
        rows = []
        for n in (5, 10, 20, 40, 80):
            dt = 2.0 / n
            d = sw.ode_symplectic(x0, k0, dt, (n + 1) * dt * (1 + 1e-12), ref.F, ref.GH, sch, diagnostics=True, method=m)[3]
            rows.append(dict(dt=dt, max_r=float(d[:, 1].max()), cost=rate[rn]["over_euler"] / dt))
        steady[m] = rows

    # accuracy, blended: distance of the final k from a fine Suzuki run
    c = ref.steady_case(nx=32)
    ctx.set_field_psi(0, c["psi"], 32, c["L"])
    ctx.set_field_psi(1, np.roll(c["psi"], 5, axis=0), 32, c["L"])
    T = 4.0

    def final_k(integ, nsub):
        ctx.set_integrator(*integ)
        return ctx.leapfrog(c["x0"], c["k0"], T / nsub, nsub, ref.F, ref.GH, nslots=2, alpha0=0.5 / nsub,
                            dalpha=1.0 / nsub, bump=ref.BUMP)[1]

    fine = final_k(SCHEMES["suzuki_it4"], 1280)
    blended = {}
    for m, rn in methods.items():
        blended[m] = [dict(nsub=n, dt=T / n, err=float(np.abs(final_k(SCHEMES[rn], n) - fine).max()),
                           cost=rate[rn]["over_euler"] * n / T) for n in (10, 20, 40, 80)]
    ctx.set_integrator(0, 1, 0)
    ctx.close()
    out = {"metric": "packet-step schemes: ms per composite step and accuracy (1 x MI355X)", "nx": w["nx"],
           "packets": a.packets, "substeps": sub, "bench_steps": a.bench_steps, "rounds": a.rounds,
           "steps_timed": a.bench_steps * sub, "rate": rate,
           "cost_unit": "Euler steps of the same run per unit of simulated time",
           "steady_nx64_T2_max_r": steady, "blended_nx32_T4_final_k_error": blended}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
