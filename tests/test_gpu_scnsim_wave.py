"""k_scnsim_wave<NP> (mdp_scenario_sim under MDP_SIM_WAVE) on the GPU: every
table bit for bit, hist and match, cell for cell, against the numpy
restatements tests/scnsim_ref.py (n <= 64, held to the reference-pinned oracle
by tests/test_scnsim_host.py) and tests/scnsim_wave_ref.py (any n: the same
year on the initial state of include/midaspom.h), and one anchor that shares
no loop with either: isolated patches against exact Poisson-binomial
probabilities (tests/fut_exact.py)."""
from __future__ import annotations

import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import fut_exact as fx
import midaspom_amd as mdp
import scnsim_ref as ref
import scnsim_wave_ref as wref
from midaspom_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = ("dieoff", "loss")
NPS = (1, 2, 4, 8)


def need_np(n):
    return next(np_ for np_ in NPS if n <= 128 * np_)


def gpu_tables(row, kind, e, c, K, dsrc, options="MDP_SIM_WAVE=auto", **kw):
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
# 1. MDP_SIM_WAVE=1 on rows the lane kernel holds: its tables, and with them
#    the oracle anchor of test_scnsim_host.py; every larger NP
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 9, 33, 64])
def test_forced_wave_equals_lane_kernel(n, kind):
    row = ref.synthetic_row(n, min(n, n % 4))
    e, c, K, dsrc = [0.2, 0.5], [0.3, 0.9], [0.4, 1.0, 3.0], [200.0, 900.0]  # test_gpu_scnsim.test_sizes' grid
    kw = dict(ts=3, tdis=2, nrep=300, seed=7 + n)
    want = ref.tables(row, kind, e, c, K, dsrc, **kw)
    assert (want[0].sum(axis=-1) == 300).all()
    lane = gpu_tables(row, kind, e, c, K, dsrc, options=None, **kw)
    assert lane[2].startswith("k_scnsim<")
    same(lane[:2], want, f"n {n} {lane[2]}")
    h, m, name = gpu_tables(row, kind, e, c, K, dsrc, options="MDP_SIM_WAVE=1", **kw)
    assert name == "k_scnsim_wave<1>"
    same((h, m), want, f"n {n} {name}")
    same((h, m), lane[:2], f"n {n} {name} against {lane[2]}")
    for np_ in NPS[1:]:
        h, m, name = gpu_tables(row, kind, e, c, K, dsrc, options=f"MDP_SIM_WAVE=1;MDP_SIM_NP={np_}", **kw)
        assert name == f"k_scnsim_wave<{np_}>"
        same((h, m), want, f"n {n} {name}")


# ---------------------------------------------------------------------------
# 2. auto past 64 patches: every instantiation's boundary, both kinds
# ---------------------------------------------------------------------------
def _auto_case(n, kind):
    """Arguments of wref.tables_cached: 130 replicates = 32 full wave quartets
    and a ragged one."""
    row = tuple(int(v) for v in ref.synthetic_row(n, 3))
    if n <= 256:
        return (row, kind, (0.1, 0.3), (0.3,), (0.5, 3.0), (250.0,), 3, 2, 130, 40 + n)
    return (row, kind, (0.2,), (0.3,), (0.5, 3.0), (250.0,), 2, 1, 130, 40 + n)


def _run_case(case, options):
    row, kind, e, c, K, dsrc, ts, tdis, nrep, seed = case
    return gpu_tables(row, kind, list(e), list(c), list(K), list(dsrc), options=options, ts=ts, tdis=tdis, nrep=nrep,
                      seed=seed)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [65, 127, 128, 129, 255, 256, 257, 513, 1024])
def test_auto_sizes(n, kind):
    case = _auto_case(n, kind)
    want = wref.tables_cached(*case)
    # from the restatement alone: the case is not a degenerate one
    assert (want[0].sum(axis=-1) == 130).all()
    assert ((want[0] != 0).sum(axis=-1) >= 3).all()
    h, m, name = _run_case(case, "MDP_SIM_WAVE=auto")
    assert name == f"k_scnsim_wave<{need_np(n)}>"
    same((h, m), want, f"n {n} {name}")


@pytest.mark.parametrize("kind", [0, 1])
def test_65_patches_under_np_8(kind):
    case = _auto_case(65, kind)
    h, m, name = _run_case(case, "MDP_SIM_WAVE=auto;MDP_SIM_NP=8")
    assert name == "k_scnsim_wave<8>"
    same((h, m), wref.tables_cached(*case), "n 65 k_scnsim_wave<8>")


# ---------------------------------------------------------------------------
# 3. a match table that is not empty past 64 patches: a colonisation front
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,k0", [(65, 40), (129, 100), (257, 200), (1024, 600), (1024, 1000)])
def test_match_on_a_front(n, k0):
    """Loss, e = 1 (nothing survives a year), c = 1, two scenario years and
    no baseline year, the source at dsrc = 0.3 m and K = exp(0.3 (k0 + 1)):
    pC_k = min(1, exp(0.3 (k0 - k))) -- 1 up to k0, falling by 0.74 per patch
    through the ten missing ones, small beyond.  The row is that front."""
    m_ = 400.0
    row = np.zeros(n, dtype=np.int32)
    row[:k0 + 1] = 1
    row[k0 + 1:k0 + 11] = -1
    K, dsrc = [math.exp(0.3 * (k0 + 1))], [0.3 * m_]
    kw = dict(ts=2, tdis=0, nrep=200, seed=31 + n + k0)
    want = wref.tables(row, 1, 1.0, 1.0, K, dsrc, m=m_, **kw)
    matched, distinct = int(want[1].sum()), int((want[1] != 0).sum())
    print(f"n {n} k0 {k0}: {matched} of 200 replicates match over {distinct} completions")
    assert matched >= 100 and distinct >= 30
    h, mt, name = gpu_tables(row, 1, 1.0, 1.0, K, dsrc, **kw)
    assert name == f"k_scnsim_wave<{need_np(n)}>"
    same((h, mt), want, f"front n {n} k0 {k0}")


# ---------------------------------------------------------------------------
# 4. absorbing paths and clamps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("ts,tdis", [(3, 2), (0, 3), (3, 0), (0, 0)])
def test_clamps_and_absorbing(n, kind, ts, tdis):
    """e/K > 1 at (e 0.5, K 0.1): everything dies in the first scenario year
    -- through the extinct-replicate shortcut for die-off, past it for loss,
    whose source recolonises; c s1 K > 1 at K = 100; e = 0; c = 0; e > 1."""
    row = ref.synthetic_row(n, 2)
    e, c, K, dsrc = [0.0, 0.5, 1.5], [0.0, 0.5], [0.1, 100.0], [100.0]
    kw = dict(ts=ts, tdis=tdis, nrep=70, seed=11)
    want = wref.tables(row, kind, e, c, K, dsrc, **kw)
    if kind == 0 and ts > 0:
        assert want[0][1, :, 0, 0, 0].tolist() == [70, 70]  # the absorbing point is in the case
    if kind == 1 and ts > 0 and tdis == 0:
        assert want[0][2, 1, 0, 0, 0] < 70  # e > 1 kills everything each year; the source recolonises
    if kind == 1 and tdis > 0:
        assert want[0][2, :, :, 0, 0].min() == 70  # and nothing does in the baseline years
    h, m, name = gpu_tables(row, kind, e, c, K, dsrc, **kw)
    same((h, m), want, f"n {n} ts {ts} tdis {tdis}")


# ---------------------------------------------------------------------------
# 5. launch, tile and call boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_launch_points_split_accumulate_device(kind):
    import torch
    row = ref.synthetic_row(65, 3)
    e, c, K, dsrc = 0.3, 0.5, [0.2, 0.7, 1.0, 2.0, 9.0], [250.0]
    rep0 = (1 << 32) - 60  # replicate indices across 2^32
    kw = dict(ts=2, tdis=2, seed=3)
    want = wref.tables(row, kind, e, c, K, dsrc, nrep=130, rep0=rep0, **kw)
    for pts in (1, 2):
        h, m, _ = gpu_tables(row, kind, e, c, K, dsrc, options=f"MDP_SIM_WAVE=auto;MDP_SIM_LAUNCH_PTS={pts}", nrep=130,
                             rep0=rep0, **kw)
        same((h, m), want, f"MDP_SIM_LAUNCH_PTS={pts}")
    with mdp.ScenarioSim(row, KIND[kind], options="MDP_SIM_WAVE=auto") as sim:
        d = dsrc if kind else None
        # nrep 1, 3, 4 and 5 (a ragged quartet, a full one, one past it), accumulated
        # into the caller's tables with the rest: 1 + 3 + 4 + 5 + 117 = 130
        h = m = True
        at = rep0
        for cnt in (1, 3, 4, 5, 117):
            h, m = sim.tables(e, c, K, d, nrep=cnt, rep0=at, hist=h, match=m, **kw)
            if cnt == 1:
                assert h.sum() == 5  # one replicate in each of the 5 points
            at += cnt
        same((h.reshape(want[0].shape), m.reshape(want[1].shape)), want, "five calls")
        # either table alone
        h1, none = sim.tables(e, c, K, d, nrep=130, rep0=rep0, match=False, **kw)
        assert none is None and np.array_equal(h1.reshape(want[0].shape), want[0])
        none, m1 = sim.tables(e, c, K, d, nrep=130, rep0=rep0, hist=False, **kw)
        assert none is None and np.array_equal(m1.reshape(want[1].shape), want[1])
        # the device form overwrites, and equals the host form
        st = torch.cuda.current_stream().cuda_stream
        dh = torch.full(want[0].shape, 7, dtype=torch.int64, device="cuda:0")
        dm = torch.full(want[1].shape, 7, dtype=torch.int64, device="cuda:0")
        for _ in range(2):
            sim.tables_device(dh.data_ptr(), dm.data_ptr(), e, c, K, d, nrep=130, rep0=rep0, stream=st, **kw)
        torch.cuda.synchronize()
        same((dh.cpu().numpy().astype(np.uint64), dm.cpu().numpy().astype(np.uint64)), want, "device form")
        assert sim.time_kernel(e, c, K, d, ts=2, tdis=2, nrep=130, reps=2) > 0


def test_more_tiles_than_workgroups():
    """4100 points of one replicate, so one tile, each: the grid-stride loop wraps (4096 workgroups)."""
    row = ref.synthetic_row(65, 2)
    K = np.geomspace(0.2, 20.0, 4100)
    kw = dict(ts=1, tdis=0, nrep=1, seed=2)
    want = wref.tables(row, 0, 0.3, 0.5, K, None, **kw)
    assert (want[0].sum(axis=-1) == 1).all() and (want[0].sum(axis=(0, 1, 2, 3)) != 0).sum() >= 3
    h, m, name = gpu_tables(row, 0, 0.3, 0.5, K, None, **kw)
    assert name == "k_scnsim_wave<1>"
    same((h, m), want, "4100 points")


# ---------------------------------------------------------------------------
# 6. an anchor with no shared loop: isolated patches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 1024])
def test_isolated_patches_poisson_binomial(n):
    """d / m = 1000: every M[l][k] underflows to 0.0, so each patch is its own
    two-state chain -- started at 1/2; in each of the ts = 3 loss years it
    survives with 1 - E, E = min(1, e), and an empty one is colonised with
    pC_k = min(1, c src_k K); in each of the tdis = 2 baseline years it
    survives with 1 - E and nothing colonises.  hist is then Poisson-binomial
    in the patches' final probabilities; every cell is held to its exact
    binomial p-value at alpha / cells, alpha = 1e-5 (fut_exact.check)."""
    N, m_, d_, e, c, K, dsrc, ts, tdis = 200_000, 400.0, 400_000.0, 0.3, 0.5, 2.0, 4.0, 3, 2
    assert math.exp(-(1.0 / m_) * 1.0 * d_) == 0.0
    src = np.exp(-(1.0 / m_) * (np.arange(n) + 1.0) * dsrc)
    pc = np.minimum(1.0, c * src * K)
    p = np.full(n, 0.5)
    for _ in range(ts):
        p = p * (1.0 - e)
        p = p + (1.0 - p) * pc
    for _ in range(tdis):
        p = p * (1.0 - e)
    probs = fx.poisson_binomial(p)
    assert abs(probs.sum() - 1.0) < 1e-12
    assert int(fx.informative(N, probs).sum()) >= 20  # non-vacuity, from the probabilities alone
    row = np.zeros(n, dtype=np.int32)
    with mdp.ScenarioSim(row, "loss", m=m_, d=d_, options="MDP_SIM_WAVE=auto") as sim:
        hist, _ = sim.tables(e, c, [K], [dsrc], ts=ts, tdis=tdis, nrep=N, seed=20261020, match=False)
        assert sim.kernel == f"k_scnsim_wave<{need_np(n)}>"
    counts = hist.reshape(n + 1)
    assert int(counts.sum()) == N
    assert (counts[probs == 0.0] == 0).all()
    fx.check(counts, N, probs, alpha=1e-5, label=f"isolated patches n {n}")


# ---------------------------------------------------------------------------
# 7. the drop-ins at 130 patches: -R / -r / -H, compiled and Python, -g 1 and
#    -g 3 and two torchrun ranks: the same bytes, and the restatement's counts
# ---------------------------------------------------------------------------
ROW130 = ref.synthetic_row(130, 2, seed=4)
CLI_GRID = {"dieoff": ["-s", "7"], "loss": ["-s", "3", "-v", "2"]}
CLI_FLAGS = ["-a", "2", "-b", "3", "-e", "0.4", "-c", "0.5", "-p", "0.3", "-R", "200", "-r", "5"]


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    return env


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _input(tmp_path, row=ROW130):
    path = tmp_path / f"row{len(row)}.txt"
    path.write_text(" ".join(str(int(v)) for v in row) + "\n")
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
        assert lines[at + 1] == "Simulated likelihood: 200 replicates per grid point, seed 5"
        files[tag] = (lh.read_bytes(), hh.read_bytes(), r.stdout[:r.stdout.index("Starting likelihood")])
    assert files["c1"][:2] == files["c3"][:2] == files["py1"][:2] == files["py3"][:2]
    assert files["c1"][2] == files["py1"][2]  # the log up to the computation: the matrix and the four completions
    # and they hold the restatement's tables
    k = 1 if kind == "loss" else 0
    K = mdp.kgrid(int(CLI_GRID[kind][1]), 0.1, 100.0)
    dv = mdp.dgrid(2, 200.0, 4000.0) if k else None
    hist, match = wref.tables(ROW130, k, 0.4, 0.5, K, dv, ts=3, tdis=2, nrep=200, seed=5)
    assert (hist.sum(axis=-1) == 200).all() and ((hist != 0).sum(axis=-1) >= 3).any()
    want_h = "".join("".join(f"{int(v)}\t" for v in g) + "\n" for g in hist.reshape(-1, 131))
    assert files["c1"][1].decode() == want_h
    L = ref.lik(ROW130, np.float32(0.3), match, 200)[0, 0]
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
    assert "Simulated likelihood: 200 replicates per grid point, seed 5" in r2.stdout


def test_dropin_refusals(tmp_path):
    inp = _input(tmp_path, np.ones(1025, dtype=np.int32))
    for cmd in ([_exe("loss")], [sys.executable, "-m", "midaspom_amd.scenario", "loss"]):
        r = subprocess.run([*cmd, *CLI_FLAGS, "-s", "3", "-v", "2", "-i", inp, "-o", str(tmp_path / "no.txt")],
                           capture_output=True, text=True, timeout=180, env=_env(), cwd=ROOT)
        assert r.returncode == 1 and "1025 patches in the first row: -R takes at most 1024" in r.stderr
        assert "Simulated likelihood" not in r.stdout
    # without -R the 130-patch row is refused as before
    plain = [f for f in CLI_FLAGS if f not in ("-R", "200", "-r", "5")]
    r = subprocess.run([_exe("dieoff"), *plain, "-s", "3", "-i", _input(tmp_path), "-o", str(tmp_path / "no.txt")],
                       capture_output=True, text=True, timeout=180, env=_env(), cwd=ROOT)
    assert r.returncode == 1 and "130 patches: the scenario engine takes n <= 16" in r.stderr
