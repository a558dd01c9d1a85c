"""The drivers' transition series sharded over two ranks (gloo, both on GPU 0,
as tests/test_dist_gpu_cond_series.py launches them) against a single process.

Every rank marks and records its shard's packets on its own device;
PacketEnsemble gathers the shards' int64 frames, rank 0 combines them
(combine_transitions: counts and sums add, the mark serials must agree) and
writes.  A frame is integer sums over the packet set, exact and order-free, so
the five trans_*.bin files are byte-equal to the single-process run's: the
one-layer driver in the replicated form with two rings split by ring, the
two-layer driver in the owner form with rank 0 holding no packets, the source
omega at a mark renewed every second frame."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_dist_gpu import ROOT, _free_port, _rank_report

pytestmark = pytest.mark.gpu

N = 1001
SPEC = "np.linspace(4.0, 15.0, 23)"
CASES = {
    "one": ("qgsw_raytrace", (64, N, [2.0, 4.0], 20.0, 0.0, 0.2, 3.0, 1.0),
            dict(nsub=2, max_steps=24, r_drag=0.0, trans_by="ring")),
    "two": ("qg2layersw_raytrace", (64, N, 4.0, 40.0, 0.0, 0.2, 3.0, 1.0),
            dict(nsub=2, max_steps=80, seed=5, trans_src_edges=[9.0, 11.0, 11.9, 12.1, 13.0, 15.0], trans_lag=2)),
}
TRANS_FILES = ("trans_hist.bin", "trans_sums.bin", "trans_stats.bin", "trans_time.bin", "trans_geom.bin")

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
assert out["trans_frames"] == out["packet_frames"] - 1
ctx.close()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("case,pde,w0", [("one", "replicated", 1.0), ("two", "owner", 0.0)])
def test_sharded_transitions_equal_single_process(ctx, tmp_path, case, pde, w0):
    import swraytracing_amd as sw
    driver, args, kw = CASES[case]
    ref_dir = tmp_path / "single"
    getattr(sw, driver)(*args, out_dir=str(ref_dir), ctx=ctx, spectrum_edges=eval(SPEC), **kw)
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
    for name in TRANS_FILES + ("packet_time.bin", "omega_hist.bin"):
        assert len(ref[name]) > 0 and got[name] == ref[name], name
    stats = np.frombuffer(got["trans_stats.bin"], dtype=np.int64).reshape(-1, 3)
    ns = 2 if case == "one" else 5
    counts = np.frombuffer(got["trans_hist.bin"], dtype=np.int64).reshape(stats.shape[0], ns + 2, 24)
    assert stats.shape[0] > 1 and (stats[:, :2] == [N, 0]).all() and (counts.sum(axis=(1, 2)) == N).all()
    if case == "one":  # the rings' blocks, split across the two ranks' shards
        assert (stats[:, 2] == 1).all() and (counts.sum(axis=2) == [0, 500, 501, 0]).all()
    else:  # re-marked after every second frame: the last source row is spread over several classes
        assert stats[:, 2].tolist() == [1 + i // 2 for i in range(stats.shape[0])]
        assert np.count_nonzero(counts[-1].sum(axis=1)) >= 3
