"""bench.py's launcher logic (CPU): `--gpus N` without a torch.distributed
environment runs the ranks as a child torch.distributed.run; inside one,
WORLD_SIZE must agree with --gpus.  Importing bench does not import torch."""
import sys

import pytest

import bench


def test_import_is_light():
    assert "torch" not in vars(bench) or vars(bench)["torch"] is None


def test_one_gpu_runs_in_process():
    a = bench.parse_args([])
    assert bench.launcher_cmd(a, [], {}) is None
    a = bench.parse_args(["--gpus", "1"])
    assert bench.launcher_cmd(a, ["--gpus", "1"], {}) is None


def test_n_gpus_launches_child_torchrun():
    argv = ["--gpus", "4", "--steps", "7"]
    cmd = bench.launcher_cmd(bench.parse_args(argv), argv, {})
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--master-addr=127.0.0.1" in cmd
    assert cmd[-3:] == ["--gpus", "4", "--steps", "7"][-3:] and cmd[-4] == "--gpus"
    assert cmd[cmd.index("--master-addr=127.0.0.1") + 2].endswith("bench.py")


def test_rank_checks_world_size():
    a = bench.parse_args(["--gpus", "8"])
    assert bench.launcher_cmd(a, [], {"WORLD_SIZE": "8"}) is None
    with pytest.raises(SystemExit):
        bench.launcher_cmd(a, [], {"WORLD_SIZE": "2"})
    # no --gpus under torch.distributed.run: WORLD_SIZE decides
    assert bench.launcher_cmd(bench.parse_args([]), [], {"WORLD_SIZE": "2"}) is None


def test_strong_scaling_is_default():
    a = bench.parse_args([])
    assert a.scaling == "strong" and a.packets == 1_000_000
    assert bench.parse_args(["--scaling", "weak"]).scaling == "weak"


def test_relay_forwards_only_the_metric_line(capfd):
    code = ("import json,sys;print('noise');print(json.dumps({'metric':'m','value':1}));"
            "print('more', file=sys.stderr);sys.exit(3)")
    rc = bench.relay([sys.executable, "-c", code])
    out, err = capfd.readouterr()
    assert rc == 3
    assert out.strip() == '{"metric": "m", "value": 1}'
    assert "noise" in err and "more" in err


def test_plain_run_times_only_the_metric():
    """Without --full every measurement beside the metric is switched off;
    --full leaves each to its own switch."""
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None
    bench.metric_only(a)
    assert a.no_fma and a.no_forecast and a.no_cpu_baseline and a.driver_steps == 0 and a.ode23_steps == 0
    assert a.steps == 7 and a.warmup == 2
    f = bench.parse_args(["--full", "--no-fma"])
    assert f.full and f.no_fma and not f.no_forecast and not f.no_cpu_baseline
    assert f.driver_steps > 0 and f.ode23_steps > 0


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import numpy as np
    rng = np.random.default_rng(1)
    x, k = rng.random((1000, 2)), rng.random((1000, 2))
    info = bench.dump_outputs(str(tmp_path / "a"), x, k, seed=146)
    assert info["rows"] == info["of"] == 1000 and sorted(info["files"]) == ["k.npy", "x.npy"]
    xs, ks = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "k.npy")
    assert xs.dtype == np.float64 and np.array_equal(xs, x) and np.array_equal(ks, k)
    # above the size limit: the same seeded sample of rows every time, within the limit
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4000)
    for d in ("b", "c"):
        info = bench.dump_outputs(str(tmp_path / d), x, k, seed=146)
    assert info["rows"] == 100 and info["of"] == 1000 and "rows.npy" in info["files"]
    rows = np.load(tmp_path / "c" / "rows.npy")
    assert rows.dtype == np.float64 and np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))
    r = rows.astype(np.int64)
    assert np.all(np.diff(r) > 0) and np.array_equal(np.load(tmp_path / "c" / "x.npy"), x[r])
    assert np.array_equal(np.load(tmp_path / "c" / "k.npy"), k[r])
    assert sum(p.stat().st_size for p in (tmp_path / "c").iterdir()) <= 4000 + 3 * 128
    # several ranks: one set of files each, the limit shared
    info = bench.dump_outputs(str(tmp_path / "d"), x, k, seed=146, rank=1, world=2)
    assert info["rows"] == 50 and sorted(info["files"]) == ["k_rank1.npy", "rows_rank1.npy", "x_rank1.npy"]


@pytest.mark.parametrize("world", [1, 2, 8])
def test_shards_cover_the_ensemble(world):
    from swraytracing_amd.dist import shard_range
    n = 1_000_000
    r = [shard_range(n, world, i) for i in range(world)]
    assert r[0][0] == 0 and r[-1][1] == n
    assert all(r[i][1] == r[i + 1][0] for i in range(world - 1))
    assert r[0][1] - r[0][0] == -(-n // world)
