"""The drivers' spectrum series sharded over two ranks (gloo, both on GPU 0, as
tests/test_dist_gpu.py launches them) against a single process.

Every rank records its shard's frames on its own device; PacketEnsemble.
spectrum_series gathers them and rank 0 combines (combine_spectra) and writes.
Counts, n, min and max do not depend on how the packets are split, so
omega_hist.bin and omega_edges.bin are byte-equal and those columns of
omega_stats.bin are equal.  sum omega is a different summation order (two
shard sums added): any two orders of N positive terms differ by at most
2*N*2^-53*sum, which is the tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_dist_gpu import ROOT, _free_port, _rank_report

pytestmark = pytest.mark.gpu

N, NB = 4001, 300
ARGS = "64, 4001, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0"
KW = "nsub=2, max_steps=24, r_drag=0.0, spectrum_edges=np.linspace(0, 15, 301)"

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
                       owner_weight=float(sys.argv[3]), link_buffers="host", packet_files=sys.argv[4] == "files")
assert out["spectrum_frames"] == out["packet_frames"]
ctx.close()
dist.destroy_process_group()
"""

_REF = {}


def _single(ctx, tmp_path):
    import swraytracing_amd as sw
    if not _REF:
        ref = tmp_path / "single"
        sw.qgsw_raytrace(64, N, 4.0, 20.0, 0.0, 0.2, 3.0, 1.0, out_dir=str(ref), nsub=2, max_steps=24, r_drag=0.0,
                         spectrum_edges=np.linspace(0, 15, 301), ctx=ctx)
        for n in os.listdir(ref):
            if n.endswith(".bin"):
                _REF[n] = (ref / n).read_bytes()
    return _REF


@pytest.mark.parametrize("pde,w0,files", [("replicated", 1.0, "files"),
                                          ("owner", 0.0, "nofiles")])  # rank 0 holds no packets
def test_sharded_spectrum_equals_single_process(ctx, tmp_path, pde, w0, files):
    ref = _single(ctx, tmp_path)
    (tmp_path / "driver.py").write_text(DRIVER)
    out = tmp_path / "sharded"
    env = dict(os.environ, SWRT_ROOT=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(tmp_path / "driver.py"), str(out),
           pde, str(w0), files]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, _rank_report(r.stderr)
    got = {n: (out / n).read_bytes() for n in os.listdir(out) if n.endswith(".bin")}
    for name in ("omega_hist.bin", "omega_edges.bin", "packet_time.bin"):
        assert len(ref[name]) > 0 and got[name] == ref[name], name
    if files == "files":
        assert got["packet_k.bin"] == ref["packet_k.bin"] and got["packet_x.bin"] == ref["packet_x.bin"]
    else:
        assert "packet_k.bin" not in got and "packet_x.bin" not in got
    a = np.frombuffer(got["omega_stats.bin"]).reshape(-1, 4)
    b = np.frombuffer(ref["omega_stats.bin"]).reshape(-1, 4)
    assert a.shape == b.shape and a.shape[0] * (NB + 2) * 8 == len(ref["omega_hist.bin"]) and a.shape[0] > 1
    np.testing.assert_array_equal(a[:, [0, 2, 3]], b[:, [0, 2, 3]])
    assert (a[:, 0] == N).all()
    bound = 2 * N * 2.0 ** -53 * b[:, 1]
    print("sum omega: sharded - single", a[:, 1] - b[:, 1], "bound", bound)
    assert (np.abs(a[:, 1] - b[:, 1]) <= bound).all()
