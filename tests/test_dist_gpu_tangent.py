"""The drivers' tangent series sharded over two ranks (gloo, both on GPU 0, as
tests/test_dist_gpu_refr_series.py launches them) against a single process.

Every rank carries the tangent maps of its own packets and records its shard's
frames on its own device; PacketEnsemble gathers the shards' int64 frames, rank
0 adds them (combine_tangents) and writes.  A frame is integer sums over the
packet set, exact and order-free, and M depends on its own ray alone, so the
five tangent_*.bin files are byte-equal to the single-process run's: the
one-layer driver in the replicated form, the two-layer driver in the owner form
with rank 0 holding no packets."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_dist_gpu import ROOT, _free_port, _rank_report

pytestmark = pytest.mark.gpu

N = 1001
SPEC = "np.linspace(9.0, 15.0, 13)"
GE = "2.0 ** np.arange(5)"
CASES = {
    "one": ("qgsw_raytrace", (64, N, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0), dict(nsub=2, max_steps=24, r_drag=0.0)),
    "two": ("qg2layersw_raytrace", (64, N, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0), dict(nsub=2, max_steps=80, seed=5)),
}
TANGENT_FILES = ("tangent_hist.bin", "tangent_sums.bin", "tangent_stats.bin", "tangent_time.bin", "tangent_geom.bin")

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
                          link_buffers="host", spectrum_edges={SPEC}, tangent_edges={GE}, tangent_lag=2, **kw)
assert out["tangent_frames"] == out["packet_frames"] - 1
ctx.close()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("case,pde,w0", [("one", "replicated", 1.0), ("two", "owner", 0.0)])
def test_sharded_tangents_equal_single_process(ctx, tmp_path, case, pde, w0):
    import swraytracing_amd as sw
    driver, args, kw = CASES[case]
    ref_dir = tmp_path / "single"
    getattr(sw, driver)(*args, out_dir=str(ref_dir), ctx=ctx, spectrum_edges=eval(SPEC), tangent_edges=eval(GE),
                        tangent_lag=2, **kw)
    ref = {n: (ref_dir / n).read_bytes() for n in os.listdir(ref_dir) if n.endswith(".bin")}
    (tmp_path / "driver.py").write_text(DRIVER)
    out = tmp_path / "sharded"
    env = dict(os.environ, SWRT_ROOT=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(tmp_path / "driver.py"), str(out),
           pde, str(w0), repr(CASES[case])]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, _rank_report(r.stderr)
    got = {n: (out / n).read_bytes() for n in os.listdir(out) if n.endswith(".bin")}
    for name in TANGENT_FILES + ("packet_time.bin", "omega_hist.bin", "packet_x.bin", "packet_k.bin"):
        assert len(ref[name]) > 0 and got[name] == ref[name], name
    stats = np.frombuffer(got["tangent_stats.bin"], dtype=np.int64).reshape(-1, 3)
    counts = np.frombuffer(got["tangent_hist.bin"], dtype=np.int64).reshape(stats.shape[0], 6, 14)
    assert stats.shape[0] > 1 and (stats[:, :2] == [N, 0]).all() and (counts.sum(axis=(1, 2)) == N).all()
    assert stats[:, 2].tolist() == [1 + i // 2 for i in range(stats.shape[0])]
    assert np.count_nonzero(counts.sum(axis=(0, 2))) >= 2  # the shards' packets meet several growth classes
