"""The drivers' track series sharded over two ranks (gloo, both on GPU 0, as
tests/test_dist_gpu.py launches them) against a single process.

Every rank records the tracked packets inside its bounds on its own device;
PacketEnsemble gathers the shards' series and rank 0 puts the rows back in the
caller's id order (combine_tracks) and writes.  A row is a function of its
packet alone, so all five track files are byte-equal to the single-process
run's.  The ids: one of them on rank 0 in every split below, standing in the
middle of the list, the others on rank 1 and not in increasing order.  With
owner_weight 0 rank 0 holds no packets at all and records nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_dist_gpu import ROOT, _free_port, _rank_report

pytestmark = pytest.mark.gpu

N = 4001
IDS = [3000, 4000, 500, 2500, 2100]
ARGS = "64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0"
KW = f"nsub=2, max_steps=14, r_drag=0.0, track_ids={IDS}, track_every=2"
TRACK_FILES = ("track_x.bin", "track_k.bin", "track_diag.bin", "track_time.bin", "track_ids.bin")

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
assert out["track_frames"] == 8, out["track_frames"]
ctx.close()
dist.destroy_process_group()
"""

_REF = {}


def _single(ctx, tmp_path):
    import swraytracing_amd as sw
    if not _REF:
        ref = tmp_path / "single"
        facts = sw.qgsw_raytrace(64, N, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(ref), nsub=2, max_steps=14,
                                 r_drag=0.0, track_ids=IDS, track_every=2, ctx=ctx)
        assert facts["track_frames"] == 8
        for n in os.listdir(ref):
            if n.endswith(".bin"):
                _REF[n] = (ref / n).read_bytes()
    return _REF


@pytest.mark.parametrize("pde,w0", [("replicated", 1.0), ("owner", 0.5), ("owner", 0.0)])
def test_sharded_tracks_equal_single_process(ctx, tmp_path, pde, w0):
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
    for name in TRACK_FILES + ("packet_time.bin", "packet_x.bin", "packet_k.bin"):
        assert len(ref[name]) > 0 and got[name] == ref[name], name
    m = len(IDS)
    assert np.frombuffer(got["track_ids.bin"]).tolist() == [float(i) for i in IDS]
    tx = np.frombuffer(got["track_x.bin"]).reshape(8, 2, m)
    diag = np.frombuffer(got["track_diag.bin"]).reshape(8, 4, m)
    assert np.isnan(diag[0]).all() and np.isfinite(diag[1:]).all()
    assert len({tx[-1, 0, j] for j in range(m)}) == m  # five different packets
