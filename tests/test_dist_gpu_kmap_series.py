"""The drivers' wave-vector plane series sharded over two ranks (gloo, both on
GPU 0, as tests/test_dist_gpu_map_series.py launches them) against a single
process.

Every rank records its shard's frames on its own device; PacketEnsemble sums
the shards' int64 frames (all_reduce) and rank 0 writes.  A frame is integer
sums over the packet set, exact and order-free, so the three k-plane files are
byte-equal to the single-process run's, the moment sums included."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_dist_gpu import ROOT, _free_port, _rank_report

pytestmark = pytest.mark.gpu

N, M = 4001, 32
ARGS = "64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0"
KW = "nsub=2, max_steps=24, r_drag=0.0, kmap_cells=32"
KMAP_FILES = ("kmap_n.bin", "kmap_stats.bin", "kmap_geom.bin")

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
out = sw.qgsw_raytrace({ARGS}, out_dir=sys.argv[1], {KW}, ctx=ctx, pde=sys.argv[2],
                       owner_weight=float(sys.argv[3]), link_buffers="host")
assert out["kmap_frames"] == out["packet_frames"]
ctx.close()
dist.destroy_process_group()
"""

_REF = {}


def _single(ctx, tmp_path):
    import swraytracing_amd as sw
    if not _REF:
        ref = tmp_path / "single"
        sw.qgsw_raytrace(64, N, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(ref), nsub=2, max_steps=24, r_drag=0.0,
                         kmap_cells=M, ctx=ctx)
        for n in os.listdir(ref):
            if n.endswith(".bin"):
                _REF[n] = (ref / n).read_bytes()
    return _REF


@pytest.mark.parametrize("pde,w0", [("replicated", 1.0), ("owner", 0.0)])  # owner, 0.0: rank 0 holds no packets
def test_sharded_kmaps_equal_single_process(ctx, tmp_path, pde, w0):
    ref = _single(ctx, tmp_path)
    (tmp_path / "driver.py").write_text(DRIVER)
    out = tmp_path / "sharded"
    env = dict(os.environ, SWRT_ROOT=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(tmp_path / "driver.py"), str(out),
           pde, str(w0)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, _rank_report(r.stderr)
    got = {n: (out / n).read_bytes() for n in os.listdir(out) if n.endswith(".bin")}
    for name in KMAP_FILES + ("packet_time.bin", "packet_x.bin", "packet_k.bin"):
        assert len(ref[name]) > 0 and got[name] == ref[name], name
    stats = np.frombuffer(got["kmap_stats.bin"], dtype=np.int64).reshape(-1, 8)
    assert stats.shape[0] > 1 and stats.shape[0] * M * M * 8 == len(got["kmap_n.bin"])
    assert (stats[:, :3] == [N, 0, 0]).all()
    counts = np.frombuffer(got["kmap_n.bin"], dtype=np.int64).reshape(stats.shape[0], M * M)
    assert (counts.sum(axis=1) == N).all()
    ring = np.sqrt(15.0 * 9.0)
    assert np.frombuffer(got["kmap_geom.bin"]).tolist() == [4.0 * ring, M, 16]
