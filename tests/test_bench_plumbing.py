"""bench.py's multi-rank plumbing on the CPU (gloo): how the job's world is
resolved from --gpus and the launcher's environment, the ranks bench.py
starts itself when no launcher did, and each rank's e-row slabs
(main_MIDASPOM_MPI.c:361-368: the remainder rows go to rank 0)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _bench():
    import bench
    return bench


def _args(gpus):
    return argparse.Namespace(gpus=gpus)


def test_resolve_world():
    b = _bench()
    assert b.resolve_world(_args(None), {}) == (1, 0, 0, False)
    assert b.resolve_world(_args(1), {}) == (1, 0, 0, False)
    assert b.resolve_world(_args(4), {}) == (4, 0, 0, True)  # no launcher: bench.py starts the ranks
    env = {"WORLD_SIZE": "8", "RANK": "5", "LOCAL_RANK": "5"}
    assert b.resolve_world(_args(8), env) == (8, 5, 5, False)
    assert b.resolve_world(_args(None), env) == (8, 5, 5, False)
    with pytest.raises(SystemExit):
        b.resolve_world(_args(2), env)  # --gpus contradicts the launcher
    with pytest.raises(SystemExit):
        b.resolve_world(_args(0), {})


def _clean_env():
    return {k: v for k, v in os.environ.items()
            if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def _check_slabs(res, n):
    assert res["n_gpus"] == n and [r["rank"] for r in res["ranks"]] == list(range(n))
    for cfg, s in (("2", 512), ("3", 1024)):
        rows = [r["strong_cols"][cfg] for r in res["ranks"]]
        assert rows[0][0] == 0 and rows[-1][1] == s
        assert all(a[1] == b[0] for a, b in zip(rows, rows[1:]))  # contiguous, in rank order
        assert rows[0][1] - rows[0][0] == s // n + s % n      # the remainder on rank 0
        assert all(r[1] - r[0] == s // n for r in rows[1:])
    assert [r["weak_rows"] for r in res["ranks"]] == [[512 * i, 512 * (i + 1)] for i in range(n)]


def test_gpus_n_starts_n_ranks():
    """`bench.py --gpus 3` with no launcher: three ranks, one process group."""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "3", "--dry-run", "--backend", "gloo"],
                       capture_output=True, text=True, timeout=240, env=_clean_env(), cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    _check_slabs(_json_line(r.stdout), 3)


def test_torchrun_launch_unchanged():
    """Under torchrun the launcher's ranks are the job (no second spawn)."""
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29731", str(ROOT / "bench.py"),
                        "--gpus", "2", "--dry-run", "--backend", "gloo"],
                       capture_output=True, text=True, timeout=240, env=_clean_env(), cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    _check_slabs(_json_line(r.stdout), 2)


def test_projection_record():
    """The one-GPU strong-scaling projection (bench.project_likelihood /
    project_dieoff): per N the slowest rank's slab against the one-GPU pass,
    and the bytes rank 0 receives in the job's one gather."""
    b = _bench()
    p = b._project(10.0, {2: [5.5, 5.0], 4: [3.0, 2.5, 2.5, 2.5], 8: [2.0] + [1.25] * 7}, 1024 * 1024 * 8)
    assert set(p) == {"2", "4", "8"}
    assert p["2"]["max_slab_ms"] == 5.5 and p["2"]["projected_speedup"] == pytest.approx(10 / 5.5)
    assert p["8"]["projected_speedup"] == pytest.approx(5.0)
    assert p["4"]["gather_bytes_to_rank0"] == 1024 * 1024 * 8 * 3 // 4
    assert b.PROJ_NS == (2, 4, 8)


def test_coll_name():
    b = _bench()
    assert b._coll_name(argparse.Namespace(backend="nccl")) == "RCCL"
    assert b._coll_name(argparse.Namespace(backend="gloo")) == "gloo"


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: an array within the cap is written whole in float64; a
    larger one as the elements at a fixed, ascending set of distinct flat
    indices, the same set on every call."""
    import numpy as np
    b = _bench()
    small = np.arange(12, dtype=np.int64).reshape(3, 4)
    b.dump_outputs(tmp_path / "a", {"small": small})
    got = np.load(tmp_path / "a" / "small.npy")
    assert got.dtype == np.float64 and np.array_equal(got, small)
    assert b.DUMP_CAP_BYTES <= 32 << 20  # a run's arrays share it: under 64 MB in all
    with pytest.raises(SystemExit):  # the files hold finite numbers only
        b.dump_outputs(tmp_path / "a", {"bad": np.array([1.0, np.nan])})
    lik = np.array([[-np.inf, -3.0], [-700.5, -np.inf]])
    arrs = b.loglik_arrays(lik)
    assert np.array_equal(arrs["loglik"], [[-700.5, -3.0], [-700.5, -700.5]])
    assert np.array_equal(arrs["loglik_zero"], [[1.0, 0.0], [0.0, 1.0]])
    assert np.isnan(b.loglik_arrays(np.array([np.nan, -1.0]))["loglik"][0])  # a NaN stays, to be refused
    monkeypatch.setattr(b, "DUMP_CAP_BYTES", 80)  # ten float64
    big = np.random.default_rng(5).standard_normal((7, 9))
    b.dump_outputs(tmp_path / "a", {"big": big})
    b.dump_outputs(tmp_path / "b", {"big": big})
    s1, s2 = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert s1.dtype == np.float64 and s1.shape == (10,) and np.array_equal(s1, s2)
    idx = np.sort(np.random.default_rng(b.DUMP_SEED).choice(big.size, size=10, replace=False))
    assert np.unique(idx).size == 10 and np.array_equal(s1, big.ravel()[idx])


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`:
    one line with the headline keys and none of the --full blocks, K timed
    steps, and DIR/loglik.npy equal bit for bit to the slab the same engine
    calls give here (config 2, 512 x 512, [c][e]) wherever that is finite;
    the L = 0 points (log L = -inf) are marked in DIR/loglik_zero.npy."""
    import numpy as np
    import torch
    import midaspom_amd as mdp
    from midaspom_amd import synth
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "dump")],
                       capture_output=True, text=True, timeout=240, env=_clean_env(), cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    res = _json_line(r.stdout)
    assert res["metric"] == "grid-point x timestep likelihood evals/sec"
    assert res["unit"] == "grid-point-timestep evals/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["ms_per_step"] > 0
    assert res["config"]["years"] == 50
    assert res["value"] == pytest.approx(512 * 512 * 49 / (res["ms_per_step"] * 1e-3))
    assert not {"job", "kernel_ms", "roofline", "projection", "parity", "strong"} & set(res)
    assert sorted(p.name for p in (tmp_path / "dump").iterdir()) == ["loglik.npy", "loglik_zero.npy"]
    got, zero = np.load(tmp_path / "dump" / "loglik.npy"), np.load(tmp_path / "dump" / "loglik_zero.npy")
    assert got.dtype == zero.dtype == np.float64 and got.shape == zero.shape == (512, 512)
    assert np.isfinite(got).all() and set(np.unique(zero)) == {0.0, 1.0}
    model = mdp.Model.load(synth.write(tmp_path / "in.txt", **synth.CONFIG2), m=400.0, p=0.5, d=100.0)
    g, _ = mdp.grid(512, 0.0, 1.0)
    with mdp.Engine(model, devices=[0]) as eng:
        eng.set_grid(g, g)
        eng.set_layout("ce")
        out = torch.empty((512, 512), dtype=torch.float64, device="cuda")
        eng.run(out.data_ptr(), 512, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ref = out.cpu().numpy()
    # L = 0 exactly where e = 0, e = 1 or c = 0: marked, and stored as the smallest finite log L
    edge = np.zeros((512, 512), dtype=bool)
    edge[0, :] = edge[:, 0] = edge[:, -1] = True
    assert np.array_equal(np.isneginf(ref), edge) and np.array_equal(zero == 1.0, edge)
    assert np.array_equal(got[~edge], ref[~edge]) and (got[edge] == ref[~edge].min()).all()


@pytest.mark.gpu
def test_projection_legs_on_gpu():
    """The projection legs the default N = 1 line carries, on config 2 (both
    splits) and a small die-off grid: every rank's slab timed, speedups > 0."""
    import torch
    b = _bench()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = b.projection_block(argparse.Namespace(grid4=32), dev, stream, [2, 4])
    for key, splits in (("config2", ("split_e", "split_c")), ("config4", ("split_e",))):
        r = res[key]
        assert "error" not in r, r
        assert r["one_gpu_ms"] > 0
        for sp in splits:
            for n in b.PROJ_NS:
                rec = r[sp][str(n)]
                assert len(rec["slab_ms"]) == n and rec["projected_speedup"] > 0
