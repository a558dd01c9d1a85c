"""The staged packet step in a sharded driver run: the single-layer driver with
packet_method="yoshida4" over two ranks sharing GPU 0 (gloo, as
tests/test_dist_gpu.py) writes the single process's bytes — packets are
independent, so sharding needs nothing new — and those bytes are not the
leapfrog run's."""
import os
import subprocess
import sys

import pytest

from tests.test_dist_gpu import ROOT, _free_port, _rank_report

pytestmark = pytest.mark.gpu

ARGS = "64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0"
KW = 'nsub=2, max_steps=24, r_drag=0.0, packet_method="yoshida4"'

DRIVER = rf"""
import os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, os.environ["SWRT_ROOT"])
import swraytracing_amd as sw
torch.cuda.set_device(0)
dist.init_process_group("gloo")
ctx = sw.Context(0)
sw.qgsw_raytrace({ARGS}, out_dir=sys.argv[1], {KW}, ctx=ctx, pde="owner", owner_weight=0.5, link_buffers="host")
assert ctx.get_integrator() == (0, 1, 0)
ctx.close()
dist.destroy_process_group()
"""

FILES = ("packet_x.bin", "packet_k.bin", "packet_time.bin", "pv.bin")


def test_sharded_yoshida_driver_files_equal_single_process(fresh_ctx, tmp_path):
    import swraytracing_amd as sw
    ctx = fresh_ctx
    ref, plain = tmp_path / "single", tmp_path / "plain"
    sw.qgsw_raytrace(64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(ref), nsub=2, max_steps=24, r_drag=0.0,
                     packet_method="yoshida4", ctx=ctx)
    assert ctx.get_integrator() == (0, 1, 0)  # the driver restores the context's setting
    log = (ref / "run.log").read_text()
    assert "Packet step: yoshida4 (midpoint kick, 4 iterations, yoshida composition)" in log
    sw.qgsw_raytrace(64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(plain), nsub=2, max_steps=24, r_drag=0.0, ctx=ctx)
    assert "Packet step" not in (plain / "run.log").read_text()
    assert (ref / "packet_k.bin").read_bytes() != (plain / "packet_k.bin").read_bytes()
    assert (ref / "pv.bin").read_bytes() == (plain / "pv.bin").read_bytes()
    with pytest.raises(ValueError, match="packet_method"):
        sw.qgsw_raytrace(64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(tmp_path / "bad"), integrator="ode23",
                         packet_method="midpoint", ctx=ctx)
    (tmp_path / "driver.py").write_text(DRIVER)
    out = tmp_path / "sharded"
    env = dict(os.environ, SWRT_ROOT=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(tmp_path / "driver.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, _rank_report(r.stderr)
    for name in FILES:
        a, b = (ref / name).read_bytes(), (out / name).read_bytes()
        assert len(a) > 0 and a == b, name


def test_loops_take_the_packet_method(fresh_ctx):
    """TwoLayerLoop(packet_method=) sets the ensemble's step: four PDE steps
    equal those of an ensemble built with method=, and differ from the
    leapfrog's; ode23 rejects it."""
    import numpy as np
    import swraytracing_amd as sw
    ctx = fresh_ctx
    nx, L, f, Cg, N = 64, 20.0, 3.0, 1.0, 2049
    rng = np.random.default_rng(3)
    q1 = sw.qg.initial_q(nx, L, 0.2, f / Cg, 10, 30, rng, ndgrid=True)
    qk0 = np.stack([ctx.g2k(q1), ctx.g2k(-q1)], axis=2)
    x, k = sw.qg._packets(N, L, 4.0, f, Cg, rng)

    def run(ens_kw, loop_kw):
        model = sw.QGModel.two_layer(qk0, nx, f, Cg, L=L, ctx=ctx)
        ens = sw.PacketEnsemble(x, k, L, f, Cg, nx, f / Cg, shear=0.5, k_scale=2 * np.pi / L, nlayers=2,
                                bump=sw.BUMP_QG, ctx=ctx, **ens_kw)
        U0 = model.max_speed()
        loop = sw.TwoLayerLoop(model, ens, 0.25 * (L / nx) / U0, U0, 0.25, 0.0, nsub=2, **loop_kw)
        for _ in range(4):
            loop.step()
        loop.flush()
        loop.settle()
        out = ens.state()
        ctx.set_integrator(0, 1, 0)
        return out

    xa, ka = run(dict(method="midpoint", iterations=1), {})
    xb, kb = run({}, dict(packet_method="midpoint", packet_iterations=1))
    xc, kc = run({}, {})
    assert np.array_equal(xa, xb) and np.array_equal(ka, kb)
    assert not np.array_equal(ka, kc)
    with pytest.raises(ValueError, match="packet_method"):
        run({}, dict(integrator="ode23", packet_method="midpoint"))
