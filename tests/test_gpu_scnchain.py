"""k_scnchain<NM> and k_chain_eval (mdp_scenario_chain) on the GPU: every count
cell for cell against the numpy restatement tests/scnchain_ref.py, which
tests/test_scnchain_host.py holds to the reference-pinned oracle; the device
evaluation bit for bit against the host evaluation, which that file holds to
numpy."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import midaspom_amd as mdp
import scnchain_ref as ref
import scnsim_ref
from midaspom_amd import _lib
from test_gpu_streams import Side, no_sentinel
from test_scnchain_host import (AC, AE, AKS, AN, ATDIS, ATS, C, DSRC, E, EVAL_DURATIONS, KS, M_, R, SEED, anchor_check,
                                anchor_counts, anchor_exact)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = ("dieoff", "loss")
NMS = (8, 16, 32, 64)


def expect_nm(n):
    return next(nm for nm in NMS if nm >= n)


def row_of(n):
    return scnsim_ref.synthetic_row(n, min(n, n % 4))


def gpu_counts(n, kind, e, c, K=None, dsrc=None, baseline=False, options=None, row=None, d=200.0, **kw):
    """(counts, kernel) in the restatement's shape (nd = 1 for die-off)."""
    with mdp.ScenarioChain(row_of(n) if row is None else row, KIND[kind], d=d, options=options) as ch:
        cnt = ch.counts(e, c, K, dsrc if kind else None, baseline=baseline, **kw)
        name = ch.kernel
    if kind == 0 and not baseline:
        cnt = cnt[:, :, :, None]
    return cnt, name


def same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} cells differ"


# ---------------------------------------------------------------------------
# 1. sizes: every instantiation's boundary, both kinds, both tables, every
#    larger NM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 16, 17, 26, 33, 63, 64])
def test_sizes(n, kind):
    e, c, K, dsrc = [0.2, 0.5], [0.3, 0.9], [0.4, 1.0, 3.0], [200.0, 900.0]
    kw = dict(nrep=300, seed=7 + n)
    want = ref.counts(n, kind, e, c, K, dsrc, **kw)
    want_b = ref.counts(n, kind, e, c, baseline=True, **kw)
    assert (want.sum(axis=-1) == 300).all() and (want_b.sum(axis=-1) == 300).all()
    for nm in NMS:
        if nm < expect_nm(n):
            continue
        opts = None if nm == expect_nm(n) else f"MDP_CHAIN_NM={nm}"
        got, name = gpu_counts(n, kind, e, c, K, dsrc, options=opts, **kw)
        assert name == f"k_scnchain<{nm}>"
        same(got, want, f"n {n} {name} scenario")
        got, _ = gpu_counts(n, kind, e, c, baseline=True, options=opts, **kw)
        same(got, want_b, f"n {n} {name} baseline")


# ---------------------------------------------------------------------------
# 2. clamps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [7, 26])
def test_clamps(n, kind):
    """e/K > 1 at (e 0.5, K 0.1); c s1 K > 1 at K = 100; e = 0; c = 0; e > 1:
    under loss the source refills class 0, which is simulated like the rest."""
    e, c, K, dsrc = [0.0, 0.5, 1.5], [0.0, 0.5], [0.1, 100.0], [100.0]
    kw = dict(nrep=200, seed=11)
    want = ref.counts(n, kind, e, c, K, dsrc, **kw)
    want_b = ref.counts(n, kind, e, c, baseline=True, **kw)
    if kind == 0:
        assert (want[1, :, 0, 0, :, 0] == 200).all()   # e/K > 1: every class ends empty
        assert (want[:, :, :, :, 0, 0] == 200).all()   # class 0 is absorbing
        assert want[0, 1, 1, 0, n, n] == 200           # e = 0 and pC clamped to 1: full stays full
    else:
        assert (want[2, 1, :, 0, :, 0] < 200).all()    # e > 1 kills everything; the source recolonises
        assert (want[:, 1, :, 0, 0, 0] < 200).all()    # class 0 is not absorbing
        assert (want[:, 0, :, 0, 0, 0] == 200).all()   # but for c = 0
    assert (want_b[:, :, 0, 0] == 200).all() and (want_b[2, :, :, 0] == 200).all()
    got, _ = gpu_counts(n, kind, e, c, K, dsrc, **kw)
    same(got, want, f"n {n} scenario")
    got, _ = gpu_counts(n, kind, e, c, baseline=True, **kw)
    same(got, want_b, f"n {n} baseline")


# ---------------------------------------------------------------------------
# 3. tile, flush and launch boundaries
# ---------------------------------------------------------------------------
N9 = 9
GRID9 = (0.3, 0.6, [0.5, 2.0, 7.0], [150.0])


@pytest.mark.parametrize("nrep", [1, 63, 64, 257, 1000])
def test_replicate_tiles(nrep):
    want = ref.counts_cached(N9, 1, (0.3,), (0.6,), (0.5, 2.0, 7.0), (150.0,), nrep, 5)
    got, _ = gpu_counts(N9, 1, *GRID9, nrep=nrep, seed=5)
    same(got, want, f"{nrep} replicates")
    want_b = ref.counts_cached(N9, 1, (0.3,), (0.6,), None, None, nrep, 5, 0, True)
    got, _ = gpu_counts(N9, 1, 0.3, 0.6, baseline=True, nrep=nrep, seed=5)  # one point: many workgroups share it
    same(got, want_b, f"{nrep} replicates, baseline")


@pytest.mark.parametrize("option", ["MDP_CHAIN_PARTS=1", "MDP_CHAIN_PARTS=2", "MDP_CHAIN_PARTS=3",
                                    "MDP_CHAIN_LAUNCH_PTS=1", "MDP_CHAIN_LAUNCH_PTS=2",
                                    "MDP_CHAIN_PARTS=3;MDP_CHAIN_LAUNCH_PTS=2"])
def test_flush_and_launch_boundaries(option):
    """1000 replicates: 4 tiles per class, the last one partial; 40 tiles per
    point in 1, 2 or 3 runs, each flushed on its own."""
    want = ref.counts_cached(N9, 1, (0.3,), (0.6,), (0.5, 2.0, 7.0), (150.0,), 1000, 5)
    got, _ = gpu_counts(N9, 1, *GRID9, nrep=1000, seed=5, options=option)
    same(got, want, option)
    want_b = ref.counts_cached(N9, 1, (0.3,), (0.6,), None, None, 1000, 5, 0, True)
    got, _ = gpu_counts(N9, 1, 0.3, 0.6, baseline=True, nrep=1000, seed=5, options=option)
    same(got, want_b, option + " baseline")


def test_more_units_than_workgroups():
    """4352 points of one run each: the grid-stride loop wraps (4096 workgroups)."""
    e, c, K = np.linspace(0.05, 0.9, 17), np.linspace(0.1, 1.6, 16), np.geomspace(0.2, 20.0, 16)
    want = ref.counts(5, 0, e, c, K, None, nrep=40, seed=2)
    got, _ = gpu_counts(5, 0, e, c, K, None, nrep=40, seed=2)
    same(got, want, "4352 points")


@pytest.mark.parametrize("kind", [0, 1])
def test_rep0_across_2_32_and_accumulation(kind):
    n, rep0 = 17, (1 << 32) - 100
    e, c, K, dsrc = 0.3, 0.5, [0.2, 1.0, 9.0], [250.0]
    want = ref.counts(n, kind, e, c, K, dsrc, nrep=300, seed=3, rep0=rep0)
    got, _ = gpu_counts(n, kind, e, c, K, dsrc, nrep=300, seed=3, rep0=rep0)
    same(got, want, "rep0 across 2^32")
    assert not np.array_equal(want, ref.counts(n, kind, e, c, K, dsrc, nrep=300, seed=3, rep0=0))
    with mdp.ScenarioChain(row_of(n), KIND[kind]) as ch:
        d = dsrc if kind else None
        a = ch.counts(e, c, K, d, nrep=100, seed=3, rep0=rep0)
        b = ch.counts(e, c, K, d, nrep=200, seed=3, rep0=rep0 + 100, out=a)
        assert b is a
        same(a.reshape(want.shape), want, "two calls")
        assert all(v > 0 for v in ch.time_kernels(e, c, K, d, ts=2, tdis=2, nrep=300, nbase=300, reps=2).values())


@pytest.mark.parametrize("kind", [0, 1])
def test_anchor_equals_restatement(kind):
    """The n = 4 tables the CPU file holds to the exact lumped matrices: equal
    tables carry that bound over exactly."""
    got, name = gpu_counts(4, kind, [E], [C], list(KS), [DSRC], row=[0, 1, 1, 0], nrep=R, seed=SEED)
    assert name == "k_scnchain<8>"
    same(got, anchor_counts(kind, False), "anchor scenario")
    got, _ = gpu_counts(4, kind, [E], [C], baseline=True, row=[0, 1, 1, 0], nrep=R, seed=SEED)
    same(got, anchor_counts(kind, True), "anchor baseline")


# ---------------------------------------------------------------------------
# 4. the evaluation on the device: the host evaluation's bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64])
def test_lik_equals_host_eval_of_counts(n, kind):
    e, c, K, dsrc = [0.2, 0.5], [0.4], [0.4, 3.0], [200.0, 900.0]
    d = dsrc if kind else None
    nrep, nbase = 100, 200
    with mdp.ScenarioChain(row_of(n), KIND[kind], p=0.3, options="MDP_CHAIN_LAUNCH_PTS=3") as ch:
        scn = ch.counts(e, c, K, d, nrep=nrep, seed=9)
        base = ch.counts(e, c, baseline=True, nrep=nbase, seed=9)
        for ts, tdis in EVAL_DURATIONS:
            for start in ("uniform", "states"):
                want, want_by = ch.eval(scn, nrep, base, nbase, ts=ts, tdis=tdis, start=start, by_class=True)
                got, by = ch.lik(e, c, K, d, ts=ts, tdis=tdis, nrep=nrep, nbase=nbase, seed=9, start=start,
                                 by_class=True)
                assert np.isfinite(want).all() and (want >= 0).all()
                assert np.array_equal(got, want), (ts, tdis, start)
                assert np.array_equal(by, want_by), (ts, tdis, start)
                assert np.array_equal(ch.lik(e, c, K, d, ts=ts, tdis=tdis, nrep=nrep, nbase=nbase, seed=9, start=start),
                                      want)
        # the evaluation moves with its inputs
        assert not np.array_equal(ch.eval(scn, nrep, base, nbase, ts=3, tdis=2), ch.eval(scn, nrep, base, nbase, ts=3, tdis=0))


@pytest.mark.parametrize("kind", ["dieoff", "loss"])
def test_lik_device_is_ordered_on_the_stream(kind):
    """delay, sentinel fill, lik_device, copy -- all on a side stream: the
    result equals lik's and holds no sentinel; then the other grid into the
    same buffer, which is overwritten."""
    row = row_of(26)
    a = ([0.05, 0.4], [0.1, 0.7], [0.8, 2.5], [250.0, 1500.0] if kind == "loss" else None)
    b = tuple(None if x is None else x[::-1] for x in a)
    kw = dict(ts=4, tdis=3, nrep=300, nbase=500, seed=11)
    with mdp.ScenarioChain(row, kind) as fresh:
        want_a, want_b = fresh.lik(*a, **kw), fresh.lik(*b, **kw)
    assert not np.array_equal(want_a, want_b)
    side = Side()
    with mdp.ScenarioChain(row, kind) as ch:
        ch.lik(*b, **kw)  # the device side exists and holds the other grid
        out = side.out(want_a.shape)
        side.delay()
        ch.lik_device(out.data_ptr(), *a, stream=side.h, **kw)
        side.still_delayed(f"chain lik_device {kind}")
        got = side.fetch()[0]
        assert no_sentinel(got)
        assert np.array_equal(got, want_a)
        ch.lik_device(out.data_ptr(), *b, stream=side.h, **kw)
        assert np.array_equal(side.fetch()[0], want_b)


# ---------------------------------------------------------------------------
# 5. the exact-lumping anchor through the device path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_exact_lumping_anchor_on_the_device(kind):
    with mdp.ScenarioChain(np.zeros(AN, dtype=np.int32), KIND[kind], m=M_, d=0.0) as ch:
        got = np.array([ch.lik(AE, AC, list(AKS), [0.0] if kind else None, ts=ATS, tdis=ATDIS, nrep=R, nbase=R, seed=SEED,
                               start="states", target=np.eye(AN + 1)[m]).reshape(len(AKS)) for m in range(AN + 1)])
    for iK, K in enumerate(AKS):
        assert anchor_check(got[:, iK], anchor_exact(kind)[K][0], f"kind {kind} K {K}") >= 6


# ---------------------------------------------------------------------------
# 6. the drop-ins: -R / -C at 26 patches, compiled and Python, -g 1 and -g 3
# ---------------------------------------------------------------------------
ROW26 = scnsim_ref.synthetic_row(26, 2, seed=4)
CLI_GRID = {"dieoff": ["-s", "5"], "loss": ["-s", "5", "-v", "3"]}
CLI_FLAGS = ["-a", "2", "-b", "3", "-e", "0.4", "-c", "0.5", "-p", "0.3", "-R", "1000", "-C", "10000", "-r", "5"]


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


@pytest.mark.parametrize("kind", ["dieoff", "loss"])
def test_dropins_same_bytes(tmp_path, kind):
    inp = tmp_path / "row26.txt"
    inp.write_text(" ".join(str(int(v)) for v in ROW26) + "\n")
    exe = str(_lib.DIEOFF_CLI_PATH if kind == "dieoff" else _lib.LOSS_CLI_PATH)
    files = {}
    for tag, cmd in {"c1": [exe, "-g", "1"], "c3": [exe, "-g", "3"],
                     "py1": [sys.executable, "-m", "midaspom_amd.scenario", kind, "-g", "1"],
                     "py3": [sys.executable, "-m", "midaspom_amd.scenario", kind, "-g", "3"]}.items():
        lh = tmp_path / f"{tag}.txt"
        r = subprocess.run([*cmd, *CLI_FLAGS, *CLI_GRID[kind], "-i", str(inp), "-o", str(lh)],
                           capture_output=True, text=True, timeout=180, env=_env(), cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        at = lines.index("Starting likelihood computation")
        assert lines[at + 1] == "Chain likelihood: 1000 replicates per class, 10000 baseline replicates, seed 5"
        files[tag] = lh.read_bytes()
    assert files["c1"] == files["c3"] == files["py1"] == files["py3"]
    k = kind == "loss"
    K = mdp.kgrid(5, 0.1, 100.0)
    dv = mdp.dgrid(3, 200.0, 4000.0) if k else None
    with mdp.ScenarioChain(ROW26, kind, p=0.3) as ch:
        L = ch.lik(0.4, 0.5, K, dv, ts=3, tdis=2, nrep=1000, nbase=10000, seed=5)[0, 0].reshape(5, -1)
    # (die-off at K = 0.1: e/K > 1, everything dies in the scenario years and the row's count is out of reach)
    assert (L >= 0).all() and (L[1:] > 0).all()
    want = "".join("".join(f"{v:.20f}\t" for v in Lrow) + ("\n" if k else "") for Lrow in L)
    assert files["c1"].decode() == want
