"""k_scnsim<NM> (mdp_scenario_sim) on the GPU: every table bit for bit, hist
and match, cell for cell, against the numpy restatement tests/scnsim_ref.py,
which tests/test_scnsim_host.py holds to the reference-pinned oracle."""
from __future__ import annotations

import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import midaspom_amd as mdp
import scnsim_ref as ref
from midaspom_amd import _lib
from test_scnsim_host import C, DSRC, E, KS, R, ROW4, SEED, TDIS, TS, anchor_tables

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = ("dieoff", "loss")
NMS = (8, 16, 32, 64)


def expect_nm(n):
    return next(nm for nm in NMS if nm >= n)


def gpu_tables(row, kind, e, c, K, dsrc, options=None, **kw):
    """(hist, match, kernel) in the restatement's shape (nd = 1 for die-off)."""
    with mdp.ScenarioSim(row, KIND[kind], options=options) as sim:
        h, m = sim.tables(e, c, K, dsrc if kind else None, **kw)
        name = sim.kernel
    if kind == 0:
        h, m = h[:, :, :, None, :], m[:, :, :, None, :]
    return h, m, name


def same(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    assert np.array_equal(got[0], want[0]), f"{what}: hist differs in {int((got[0] != want[0]).sum())} cells"
    assert np.array_equal(got[1], want[1]), f"{what}: match differs in {int((got[1] != want[1]).sum())} cells"


# ---------------------------------------------------------------------------
# 1. sizes: every instantiation's boundary, both kinds, every larger NM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 16, 17, 26, 33, 63, 64])
def test_sizes(n, kind):
    row = ref.synthetic_row(n, min(n, n % 4))
    e, c, K, dsrc = [0.2, 0.5], [0.3, 0.9], [0.4, 1.0, 3.0], [200.0, 900.0]
    kw = dict(ts=3, tdis=2, nrep=300, seed=7 + n)
    want = ref.tables(row, kind, e, c, K, dsrc, **kw)
    assert (want[0].sum(axis=-1) == 300).all()
    h, m, name = gpu_tables(row, kind, e, c, K, dsrc, **kw)
    assert name == f"k_scnsim<{expect_nm(n)}>"
    same((h, m), want, f"n {n} {name}")
    for nm in NMS:
        if nm > expect_nm(n):
            h, m, name = gpu_tables(row, kind, e, c, K, dsrc, options=f"MDP_SIM_NM={nm}", **kw)
            assert name == f"k_scnsim<{nm}>"
            same((h, m), want, f"n {n} {name}")


# ---------------------------------------------------------------------------
# 2. clamps and absorbing paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [7, 9, 26])
@pytest.mark.parametrize("ts,tdis", [(3, 2), (0, 3), (3, 0), (0, 0)])
def test_clamps_and_absorbing(n, kind, ts, tdis):
    """e/K > 1 at (e 0.5, K 0.1): everything dies in the first scenario year
    -- through the extinct-wave shortcut for die-off, past it for loss, whose
    source recolonises; c s1 K > 1 at K = 100; e = 0; c = 0."""
    row = ref.synthetic_row(n, 2)
    e, c, K, dsrc = [0.0, 0.5, 1.5], [0.0, 0.5], [0.1, 100.0], [100.0]
    kw = dict(ts=ts, tdis=tdis, nrep=200, seed=11)
    want = ref.tables(row, kind, e, c, K, dsrc, **kw)
    if kind == 0 and ts > 0:
        assert want[0][1, :, 0, 0, 0].tolist() == [200, 200]  # the absorbing point is in the case
    if kind == 1 and ts > 0 and tdis == 0:
        assert want[0][2, 1, 0, 0, 0] < 200  # e > 1 kills everything each year; the source recolonises
    if kind == 1 and tdis > 0:
        assert want[0][2, :, :, 0, 0].min() == 200  # and nothing does in the baseline years
    h, m, name = gpu_tables(row, kind, e, c, K, dsrc, **kw)
    same((h, m), want, f"n {n} ts {ts} tdis {tdis}")


# ---------------------------------------------------------------------------
# 3. launch and tile boundaries
# ---------------------------------------------------------------------------
ROW9 = (1, 0, -1, 1, 0, 1, -1, 0, 1)


@pytest.mark.parametrize("nrep", [1, 63, 64, 257, 64 * 4096 + 777])
def test_replicate_tiles_one_point(nrep):
    kw = dict(ts=2, tdis=1, nrep=nrep, seed=5)
    want = ref.tables(ROW9, 1, 0.3, 0.6, [2.0], [150.0], **kw)
    h, m, _ = gpu_tables(ROW9, 1, 0.3, 0.6, [2.0], [150.0], **kw)
    same((h, m), want, f"{nrep} replicates")


def test_more_tiles_than_workgroups():
    """4352 points of one tile each: the grid-stride loop wraps (4096 workgroups)."""
    row = (1, -1, 0, 1, 0)
    e, c, K = np.linspace(0.05, 0.9, 17), np.linspace(0.1, 1.6, 16), np.geomspace(0.2, 20.0, 16)
    kw = dict(ts=1, tdis=1, nrep=40, seed=2)
    want = ref.tables(row, 0, e, c, K, None, **kw)
    h, m, _ = gpu_tables(row, 0, e, c, K, None, **kw)
    same((h, m), want, "4352 points")


@pytest.mark.parametrize("kind", [0, 1])
def test_launch_points_split_accumulate_device(kind):
    import torch
    row = ref.synthetic_row(17, 3)
    e, c, K, dsrc = 0.3, 0.5, [0.2, 0.7, 1.0, 2.0, 9.0], [250.0]
    rep0 = (1 << 32) - 100  # replicate indices across 2^32
    kw = dict(ts=2, tdis=2, seed=3)
    want = ref.tables(row, kind, e, c, K, dsrc, nrep=300, rep0=rep0, **kw)
    for pts in (1, 2):
        h, m, _ = gpu_tables(row, kind, e, c, K, dsrc, options=f"MDP_SIM_LAUNCH_PTS={pts}", nrep=300, rep0=rep0, **kw)
        same((h, m), want, f"MDP_SIM_LAUNCH_PTS={pts}")
    with mdp.ScenarioSim(row, KIND[kind]) as sim:
        d = dsrc if kind else None
        # two calls accumulate into the caller's tables
        h, m = sim.tables(e, c, K, d, nrep=100, rep0=rep0, **kw)
        h2, m2 = sim.tables(e, c, K, d, nrep=200, rep0=rep0 + 100, hist=h, match=m, **kw)
        assert h2 is h and m2 is m
        same((h.reshape(want[0].shape), m.reshape(want[1].shape)), want, "two calls")
        # either table alone
        h1, none = sim.tables(e, c, K, d, nrep=300, rep0=rep0, match=False, **kw)
        assert none is None and np.array_equal(h1.reshape(want[0].shape), want[0])
        none, m1 = sim.tables(e, c, K, d, nrep=300, rep0=rep0, hist=False, **kw)
        assert none is None and np.array_equal(m1.reshape(want[1].shape), want[1])
        # the device form overwrites, and equals the host form
        st = torch.cuda.current_stream().cuda_stream
        dh = torch.full(want[0].shape, 7, dtype=torch.int64, device="cuda:0")
        dm = torch.full(want[1].shape, 7, dtype=torch.int64, device="cuda:0")
        for _ in range(2):
            sim.tables_device(dh.data_ptr(), dm.data_ptr(), e, c, K, d, nrep=300, rep0=rep0, stream=st, **kw)
        torch.cuda.synchronize()
        same((dh.cpu().numpy().astype(np.uint64), dm.cpu().numpy().astype(np.uint64)), want, "device form")
        # lik of these counts: the host formula
        assert np.array_equal(sim.lik(want[1], 300), ref.lik(row, 0.5, want[1], 300))
        assert sim.time_kernel(e, c, K, d, ts=2, tdis=2, nrep=300, reps=2) > 0


# ---------------------------------------------------------------------------
# 4. the statistical anchor of the CPU file, once on the GPU: equal tables
#    carry the oracle bound over exactly
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_anchor_equals_restatement(kind):
    want = anchor_tables(kind)
    h, m, name = gpu_tables(ROW4, kind, [E], [C], list(KS), list(DSRC), ts=TS, tdis=TDIS, nrep=R, seed=SEED)
    assert name == "k_scnsim<8>"
    same((h, m), want, "anchor")


# ---------------------------------------------------------------------------
# 5. the drop-ins: -R / -r / -H at 26 patches, compiled and Python, -g 1 and
#    -g 3 and two torchrun ranks: the same bytes
# ---------------------------------------------------------------------------
ROW26 = ref.synthetic_row(26, 2, seed=4)
CLI_GRID = {"dieoff": ["-s", "7"], "loss": ["-s", "3", "-v", "2"]}
CLI_FLAGS = ["-a", "2", "-b", "3", "-e", "0.4", "-c", "0.5", "-p", "0.3", "-R", "2000", "-r", "5"]


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    return env


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _input(tmp_path):
    path = tmp_path / "row26.txt"
    path.write_text(" ".join(str(int(v)) for v in ROW26) + "\n")
    return str(path)


def _exe(kind):
    return str(_lib.DIEOFF_CLI_PATH if kind == "dieoff" else _lib.LOSS_CLI_PATH)


@pytest.mark.parametrize("kind", ["dieoff", "loss"])
def test_dropins_same_bytes(tmp_path, kind):
    inp = _input(tmp_path)
    files = {}
    for tag, cmd in {"c1": [_exe(kind), "-g", "1"], "c3": [_exe(kind), "-g", "3"],
                     "py1": [sys.executable, "-m", "midaspom_amd.scenario", kind, "-g", "1"],
                     "py3": [sys.executable, "-m", "midaspom_amd.scenario", kind, "-g", "3"]}.items():
        lh, hh = tmp_path / f"{tag}.txt", tmp_path / f"{tag}.hist"
        r = subprocess.run([*cmd, *CLI_FLAGS, *CLI_GRID[kind], "-i", inp, "-o", str(lh), "-H", str(hh)],
                           capture_output=True, text=True, timeout=180, env=_env(), cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        at = lines.index("Starting likelihood computation")
        assert lines[at + 1] == "Simulated likelihood: 2000 replicates per grid point, seed 5"
        files[tag] = (lh.read_bytes(), hh.read_bytes())
    assert files["c1"] == files["c3"] == files["py1"] == files["py3"]
    # and they hold the restatement's tables
    k = 1 if kind == "loss" else 0
    K = mdp.kgrid(int(CLI_GRID[kind][1]), 0.1, 100.0)
    dv = mdp.dgrid(2, 200.0, 4000.0) if k else None
    hist, match = ref.tables(ROW26, k, 0.4, 0.5, K, dv, ts=3, tdis=2, nrep=2000, seed=5)
    want_h = "".join("".join(f"{int(v)}\t" for v in g) + "\n" for g in hist.reshape(-1, 27))
    assert files["c1"][1].decode() == want_h
    L = ref.lik(ROW26, np.float32(0.3), match, 2000)[0, 0]
    want_l = "".join("".join(f"{v:.20f}\t" for v in Lrow) + ("\n" if k else "") for Lrow in L)
    assert files["c1"][0].decode() == want_l


@pytest.mark.parametrize("kind", ["dieoff", "loss"])
def test_dropins_torchrun_two_ranks(tmp_path, kind):
    inp = _input(tmp_path)
    single, multi = tmp_path / "single.txt", tmp_path / "multi.txt"
    r1 = subprocess.run([_exe(kind), *CLI_FLAGS, *CLI_GRID[kind], "-i", inp, "-o", str(single)],
                        capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert r1.returncode == 0, r1.stderr
    launch = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
              "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
              "-m", "midaspom_amd.scenario", kind, "--backend", "gloo", *CLI_FLAGS, *CLI_GRID[kind], "-i", inp]
    r2 = subprocess.run([*launch, "-o", str(multi)], capture_output=True, text=True, timeout=240, env=_env(), cwd=ROOT)
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert multi.read_bytes() == single.read_bytes()
    assert "Simulated likelihood: 2000 replicates per grid point, seed 5" in r2.stdout


def test_dropin_refusals(tmp_path):
    inp = _input(tmp_path)
    plain = [f for f in CLI_FLAGS if f not in ("-R", "2000", "-r", "5")]
    # without -R the 26-patch row is refused as before
    for cmd in ([_exe("dieoff")], [sys.executable, "-m", "midaspom_amd.scenario", "dieoff"]):
        r = subprocess.run([*cmd, *plain, "-s", "3", "-i", inp, "-o", str(tmp_path / "no.txt")],
                           capture_output=True, text=True, timeout=180, env=_env(), cwd=ROOT)
        assert r.returncode == 1 and "26 patches: the scenario engine takes n <= 16" in r.stderr
        assert "Simulated likelihood" not in r.stdout
    # -H under a launcher is refused with a message (the launcher's environment, one process)
    env = _env()
    env.update(RANK="0", WORLD_SIZE="2", LOCAL_RANK="0", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, "-m", "midaspom_amd.scenario", "dieoff", *CLI_FLAGS, "-s", "3", "-i", inp,
                        "-o", str(tmp_path / "no.txt"), "-H", str(tmp_path / "no.hist")],
                       capture_output=True, text=True, timeout=180, env=env, cwd=ROOT)
    assert r.returncode == 1 and "-H is not available under torchrun" in r.stderr
