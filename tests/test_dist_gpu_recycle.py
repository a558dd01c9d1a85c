"""The drivers' packet recycling sharded over two ranks (gloo, both on GPU 0,
as tests/test_dist_gpu_trans_series.py launches them) against a single
process.

Every rank recycles its shard's packets on its own device with index_base =
its first global id, so a re-injected packet's position depends on its global
id and generation alone; PacketEnsemble gathers the shards' frames and
generations, rank 0 combines (combine_recycles) and writes.  The four
recycle_*.bin files, the packet files and the spectrum are byte-equal to the
single-process run's: the one-layer driver in the replicated form with two
rings (and the ring transition series beside it), the two-layer driver in the
owner form with rank 0 holding no packets, with either integrator.

The cut is 12.3 in every case (omega0 = 12 on the largest ring): the
single-process runs meet the conditions below at that value.  On an MI355X the
one-layer run's five events absorb 36, 117, 71, 57 and 54 of the 1001 packets,
the two-layer run's three 465, 272 and 180 (467, 272 and 184 with ode23)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_dist_gpu import ROOT, _free_port, _rank_report

pytestmark = pytest.mark.gpu

N = 1001
CUT = 12.3
SPEC = "np.linspace(4.0, 12.3, 23)"
CASES = {
    "one": ("qgsw_raytrace", (64, N, [2.0, 4.0], 20.0, 0.0, 0.2, 3.0, 1.0),
            dict(nsub=2, max_steps=24, r_drag=0.0, trans_by="ring", recycle_omega=CUT, recycle_seed=5)),
    "two": ("qg2layersw_raytrace", (64, N, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0),
            dict(nsub=2, max_steps=80, seed=5, recycle_omega=CUT)),
    "two-ode23": ("qg2layersw_raytrace", (64, N, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0),
                  dict(nsub=2, max_steps=80, seed=5, recycle_omega=CUT, integrator="ode23")),
}
RECYCLE_FILES = ("recycle_stats.bin", "recycle_time.bin", "recycle_geom.bin", "recycle_gen.bin")

DRIVER = rf"""
import os, sys
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, os.environ["SWRT_ROOT"])
import swraytracing_amd as sw
torch.cuda.set_device(0)
dist.init_process_group("gloo")
ctx = sw.Context(0)
driver, args, kw = eval(sys.argv[4])
out = getattr(sw, driver)(*args, out_dir=sys.argv[1], ctx=ctx, pde=sys.argv[2], owner_weight=float(sys.argv[3]),
                          link_buffers="host", spectrum_edges={SPEC}, **kw)
assert out["recycle_events"] == out["packet_frames"] - 1
ctx.close()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("case,pde,w0", [("one", "replicated", 1.0), ("two", "owner", 0.0), ("two-ode23", "owner", 0.0)])
def test_sharded_recycling_equals_single_process(ctx, tmp_path, case, pde, w0):
    import swraytracing_amd as sw
    driver, args, kw = CASES[case]
    ref_dir = tmp_path / "single"
    facts = getattr(sw, driver)(*args, out_dir=str(ref_dir), ctx=ctx, spectrum_edges=eval(SPEC), **kw)
    ref = {n: (ref_dir / n).read_bytes() for n in os.listdir(ref_dir) if n.endswith(".bin")}
    # the single-process files: a cascade that is absorbed and re-injected
    stats = np.frombuffer(ref["recycle_stats.bin"], dtype=np.int64).reshape(-1, 8)
    times = np.frombuffer(ref["recycle_time.bin"], dtype=np.float64)
    gen = np.frombuffer(ref["recycle_gen.bin"], dtype=np.int32)
    geom = np.frombuffer(ref["recycle_geom.bin"], dtype=np.float64)
    hist = np.frombuffer(ref["omega_hist.bin"], dtype=np.float64).reshape(-1, 24)
    print(f"{case}: events {stats.tolist()} above {hist[:, -1].tolist()} gen sum {int(gen.sum())}")
    assert facts["recycle_events"] == stats.shape[0] == times.size == facts["packet_frames"] - 1
    assert geom.tolist() == [CUT, 2 * np.pi if case == "one" else 20.0, kw.get("recycle_seed", 0), 20.0, 3.0, 1.0, 1.0]
    assert (stats[:, 0] == N).all() and stats[:, 7].tolist() == list(range(1, stats.shape[0] + 1))
    assert np.count_nonzero(stats[:, 1] > 0) >= 3 and (stats[:, 1] < N).all() and not stats[:, 2].any()
    assert hist.shape[0] == facts["packet_frames"] and not hist[1:, -1].any()  # (no packet at or above the cut is saved)
    assert gen.size == N and int(gen.sum()) == int(stats[:, 1].sum())
    # the sharded run
    (tmp_path / "driver.py").write_text(DRIVER)
    out = tmp_path / "sharded"
    env = dict(os.environ, SWRT_ROOT=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(tmp_path / "driver.py"), str(out),
           pde, str(w0), repr(CASES[case])]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, _rank_report(r.stderr)
    got = {n: (out / n).read_bytes() for n in os.listdir(out) if n.endswith(".bin")}
    names = RECYCLE_FILES + ("packet_x.bin", "packet_k.bin", "packet_time.bin", "omega_hist.bin")
    for name in names + (("trans_hist.bin",) if case == "one" else ()):
        assert len(ref[name]) > 0 and got[name] == ref[name], name
