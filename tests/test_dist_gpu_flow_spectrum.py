"""The drivers' flow spectrum series in a sharded run (two gloo ranks, both on
GPU 0, as tests/test_dist_gpu_kmap_series.py launches them) against a single
process.

Rank 0 steps the PDE in both sharded forms and records layer 0's committed qk
at every packet frame, whether it holds packets (replicated) or none (the
owner with weight 0); the frame is a function of qk alone, so the three flow
files are byte-equal to the single-process run's, beside the packet files."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.flow_spectrum_ref import nshells
from tests.test_dist_gpu import ROOT, _free_port, _rank_report

pytestmark = pytest.mark.gpu

N = 4001
ARGS = "64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0"
KW = "nsub=2, max_steps=24, r_drag=0.0, flow_spectrum=True"
FLOW_FILES = ("flow_spec.bin", "flow_stats.bin", "flow_geom.bin")

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
assert out["flow_frames"] == out["packet_frames"]
ctx.close()
dist.destroy_process_group()
"""

_REF = {}


def _single(ctx, tmp_path):
    import swraytracing_amd as sw
    if not _REF:
        ref = tmp_path / "single"
        sw.qgsw_raytrace(64, N, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(ref), nsub=2, max_steps=24, r_drag=0.0,
                         flow_spectrum=True, ctx=ctx)
        for n in os.listdir(ref):
            if n.endswith(".bin"):
                _REF[n] = (ref / n).read_bytes()
    return _REF


@pytest.mark.parametrize("pde,w0", [("replicated", 1.0), ("owner", 0.0)])  # owner, 0.0: rank 0 holds no packets
def test_sharded_flow_spectra_equal_single_process(ctx, tmp_path, pde, w0):
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
    for name in FLOW_FILES + ("packet_time.bin", "packet_x.bin", "packet_k.bin"):
        assert len(ref[name]) > 0 and got[name] == ref[name], name
    stats = np.frombuffer(got["flow_stats.bin"]).reshape(-1, 4)
    ns = nshells(64)
    assert stats.shape[0] > 1 and stats.shape[0] * 3 * ns * 8 == len(got["flow_spec.bin"])
    assert stats[:, 0].tobytes() == got["packet_time.bin"] and (stats[:, 1:] > 0).all()
    assert np.frombuffer(got["flow_geom.bin"]).tolist() == [64, ns, 1.0, 3.0, 0.0]
