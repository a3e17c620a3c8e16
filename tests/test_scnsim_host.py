"""The scenario simulator (mdp_scenario_sim, k_scnsim<NM>), the parts that
need no GPU.

1. The numpy restatement of its replicate model (tests/scnsim_ref.py), the
   checker of the GPU tests, held to the reference-pinned oracle: on a
   complete row rho, oracle.dieoff_lik / oracle.loss_lik give exactly
   2^n P(final = rho) under a uniform initial state, so every count of the
   restatement is a binomial with a known p.  Bound per cell with R p >= 100:
   |count - R p| <= 5 sqrt(R p (1 - p)); p comes from the oracle alone.  About
   60 comparisons at 5 sigma: a false alarm near 3e-5 for the committed seed.
2. Exact identities of the restatement.
3. The host planner's stand-alone driver (_build/scnsim_plan_check) against a
   numpy restatement of its digest, and every refusal of the C ABI, which all
   come before the first device call.
"""
from __future__ import annotations

import ctypes
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle
import scnsim_ref as ref
from midaspom_amd import _lib
from midaspom_amd.scenario import _states

ROOT = Path(__file__).resolve().parents[1]
PLAN_CHECK = ROOT / "midaspom_amd" / "_build" / "scnsim_plan_check"

# the anchor of the issue: one committed seed
SEED = 20261020
R = 200_000
E, C, TS, TDIS, M_, D_ = 0.4, 0.5, 3, 2, 400.0, 200.0
KS = (0.3, 1.0, 5.0)
DSRC = (200.0, 1000.0)
ROW4 = (0, 1, 1, 0)
ROW6 = (1, -1, 0, 1, -1, 0)
P6 = 0.3


def anchor_tables(kind):
    """The restatement's tables of the anchor (shared with the GPU test)."""
    return ref.tables_cached(ROW4, kind, (E,), (C,), KS, DSRC if kind else (0.0,), TS, TDIS, R, SEED)


def oracle_lik(row, kind, p=0.5):
    """L[iK, id] of a row from the oracle."""
    if kind == 0:
        return oracle.dieoff_lik(row, KS, E, C, TS, TDIS, M_, p, D_).reshape(len(KS), 1)
    return oracle.loss_lik(row, KS, DSRC, E, C, TS, TDIS, M_, p, D_)


def within(count, p, what):
    exp, sd = R * p, math.sqrt(R * p * (1.0 - p))
    print(f"{what}: count {count} expected {exp:.2f} sd {sd:.2f} z {(count - exp) / sd if sd else 0.0:+.2f}")
    assert abs(count - exp) <= 5.0 * sd + 1e-6, what  # 1e-6: p = 1 up to rounding of the oracle's sum


@pytest.mark.parametrize("kind", [0, 1])
def test_restatement_against_oracle(kind):
    rows = [[(s >> (3 - j)) & 1 for j in range(4)] for s in range(16)]
    L = np.array([oracle_lik(r, kind) for r in rows])  # [16, nK, nd]
    # the premise: the 16 complete rows partition the final states
    assert np.abs(L.sum(axis=0) - 16.0).max() < 1e-12
    hist, match = anchor_tables(kind)
    pop = np.array([bin(s).count("1") for s in range(16)])
    for iK, idd in np.ndindex(L.shape[1], L.shape[2]):
        tested = 0
        for m in range(5):
            p = float(L[pop == m, iK, idd].sum() / 16.0)
            if R * p >= 100:
                within(int(hist[0, 0, iK, idd, m]), p, f"kind {kind} K {KS[iK]} d {idd} hist[{m}]")
                tested += 1
        if kind == 0 and E / KS[iK] > 1:
            # e/K > 1: every patch dies in the first scenario year and nothing
            # recolonises -- the oracle's distribution is one cell
            assert abs(L[0, iK, idd] - 16.0) < 1e-12 and tested == 1
        else:
            assert tested >= 4, "power: at least 4 hist cells per point"
        p = float(L[0b0110, iK, idd] / 16.0)
        if R * p >= 100:
            within(int(match[0, 0, iK, idd, 0]), p, f"kind {kind} K {KS[iK]} d {idd} match 0110")


@pytest.mark.parametrize("kind", [0, 1])
def test_match_with_missing_data(kind):
    hist, match = ref.tables_cached(ROW6, kind, (E,), (C,), KS, DSRC if kind else (0.0,), TS, TDIS, R, SEED)
    tested = 0
    for j in range(4):
        L = oracle_lik(ref.completion(ROW6, j), kind)
        for iK, idd in np.ndindex(L.shape):
            p = float(L[iK, idd] / 64.0)
            if R * p >= 100:
                within(int(match[0, 0, iK, idd, j]), p, f"kind {kind} K {KS[iK]} d {idd} match[{j}]")
                tested += 1
    assert tested >= 4
    # lik: the library's host formula on these counts, the restatement's, and
    # the formula spelled out
    want = ref.lik(ROW6, P6, match, R)
    pr = _states(np.array(ROW6), P6)[1]
    assert np.array_equal(ref.priors(2, P6), pr)
    spelled = np.zeros(match.shape[:-1])
    for idx in np.ndindex(spelled.shape):
        s = 0.0
        for j in range(4):
            s += float(pr[j]) * float(match[idx + (j,)])
        spelled[idx] = s * 64.0 / R
    assert np.array_equal(want, spelled)
    with mdp.ScenarioSim(ROW6, "loss" if kind else "dieoff", p=P6) as sim:
        assert np.array_equal(sim.lik(match, R), want)
    # and it estimates the oracle's likelihood of the row with missing data
    Lrow = oracle_lik(np.array(ROW6, dtype=np.int32), kind, P6)
    assert np.allclose(want[0, 0], Lrow, rtol=0.1)


# ---------------------------------------------------------------------------
# exact identities of the restatement
# ---------------------------------------------------------------------------
ROW9 = (1, 0, -1, 1, 0, 1, -1, 0, 1)


def test_hist_rows_sum_to_nrep():
    for kind in (0, 1):
        hist, _ = anchor_tables(kind)
        assert (hist.sum(axis=-1) == R).all()


def test_dieoff_at_K1_is_loss_at_K0():
    a = ref.tables(ROW9, 0, [0.3, 0.6], 0.4, [1.0], None, 3, 2, 500, seed=3)
    b = ref.tables(ROW9, 1, [0.3, 0.6], 0.4, [0.0], [200.0], 3, 2, 500, seed=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].sum() == 1000


def test_no_years_is_the_initial_state():
    n, nrep = 9, 700
    hist, match = ref.tables(ROW9, 0, 0.3, 0.4, [2.0], None, 0, 0, nrep, seed=5, rep0=11)
    occ = ref.initial_states(n, 5, np.arange(11, 11 + nrep, dtype=np.int64))
    assert np.array_equal(hist[0, 0, 0, 0], np.bincount(occ.sum(1), minlength=n + 1))
    # the initial bits straight from the generator's host restatement
    w = mdp.philox(5, [11 + 3, 0, 0xffffffff, 1])
    assert [bool((w[k >> 5] >> (k & 31)) & 1) for k in range(n)] == list(occ[3])
    row = np.array(ROW9)
    want = np.zeros(4, dtype=np.uint64)
    for o in occ:
        if all(o[k] == (row[k] == 1) for k in range(n) if row[k] != -1):
            want[2 * int(o[2]) + int(o[6])] += 1
    assert np.array_equal(match[0, 0, 0, 0], want) and want.sum() > 0


def test_split_accumulates_and_crosses_2_32():
    rep0 = (1 << 32) - 150
    args = (ROW9, 1, 0.3, 0.4, [0.5, 3.0], [300.0], 2, 2)
    whole = ref.tables(*args, nrep=400, seed=9, rep0=rep0)
    a = ref.tables(*args, nrep=150, seed=9, rep0=rep0)
    b = ref.tables(*args, nrep=250, seed=9, rep0=1 << 32)
    assert np.array_equal(whole[0], a[0] + b[0]) and np.array_equal(whole[1], a[1] + b[1])
    # the high counter word is in the stream: replicate 2^32 is not replicate 0
    lo = ref.initial_states(64, 9, np.arange(0, 64, dtype=np.int64))
    hi = ref.initial_states(64, 9, np.arange(1 << 32, (1 << 32) + 64, dtype=np.int64))
    assert not np.array_equal(lo, hi)
    w = mdp.philox(9, [0, 1, 0xffffffff, 1])
    assert [bool((w[k >> 5] >> (k & 31)) & 1) for k in range(64)] == list(hi[0])


def test_count_likelihood():
    hist = np.array([[[1, 3, 0], [0, 0, 0]]], dtype=np.uint64)
    got = mdp.count_likelihood(hist, 1)
    assert got.shape == (1, 2) and got[0, 0] == 0.75 and np.isnan(got[0, 1])


# ---------------------------------------------------------------------------
# the planner's driver against a numpy restatement of its digest
# ---------------------------------------------------------------------------
def fnv(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def row_text(row):
    return "".join("m" if v == -1 else str(int(v)) for v in row)


def _plan(row, kind=1, options="", nK=5, nrep=777, dsrc=300.0, p=0.3):
    return subprocess.run([str(PLAN_CHECK), row_text(row), "400", repr(p), "200", str(kind), options, str(nK),
                           str(nrep), repr(dsrc)], capture_output=True, text=True)


@pytest.mark.parametrize("n,nmiss", [(n, k) for n in (1, 8, 9, 26, 64) for k in (0, 1, 3, 10) if k <= n])
def test_plan_digest(n, nmiss):
    row = ref.synthetic_row(n, nmiss)
    nK, nrep, dsrc, p = 5, 777, 300.0, 0.3
    r = _plan(row, 1, "MDP_SIM_LAUNCH_PTS=2", nK, nrep, dsrc, p)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    nm = 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64
    assert lines[0] == f"kernel k_scnsim<{nm}>"
    fixed = sum(1 << k for k in range(n) if row[k] == 1)
    missing = sum(1 << k for k in range(n) if row[k] == -1)
    assert lines[1] == f"row n {n} nmiss {nmiss} live {(1 << n) - 1:x} fixed {fixed:x} missing {missing:x}"
    M = np.zeros((nm, nm))
    M[:n, :n] = ref.dispersal(n, 400.0, 200.0)
    src = np.zeros(nm)
    src[:n] = ref.source_row(n, 400.0, dsrc)
    miss = np.flatnonzero(row == -1).astype(np.uint32)
    pr = ref.priors(nmiss, p)
    assert lines[2] == (f"miss {fnv(miss.tobytes()):016x} M {fnv(M.tobytes()):016x} "
                        f"prior {fnv(pr.tobytes()):016x} src {fnv(src.tobytes()):016x}")
    tpp = (nrep + 255) // 256
    assert lines[3] == (f"call points {nK} tiles_per_point {tpp} hist {nK * (n + 1)} match {nK << nmiss} "
                        f"launches 3")
    assert lines[4:7] == [f"launch p0 {p0} npts {k} tiles {k * tpp} nwg {min(k * tpp, 4096)}"
                          for p0, k in ((0, 2), (2, 2), (4, 1))]
    s = 0.0
    for j in range(1 << nmiss):
        s += float(pr[j]) * 1.0
    assert lines[7].startswith("lik ") and float.fromhex(lines[7].split()[1]) == s * float(2 ** n) / nrep


def test_plan_launch_cut_and_options():
    row = ref.synthetic_row(26, 3)
    r = _plan(row, 0, "", 151, 10000)
    assert r.returncode == 0 and "launches 1" in r.stdout
    assert r.stdout.splitlines()[4] == f"launch p0 0 npts 151 tiles {151 * 40} nwg 4096"
    r = _plan(row, 0, "MDP_SIM_NM=64", 2, 1)
    assert r.returncode == 0 and r.stdout.startswith("kernel k_scnsim<64>\n")
    for bad in ("MDP_SIM_NM=16", "MDP_SIM_NM=12", "MDP_SIM_NM=", "MDP_SIM_LAUNCH_PTS=-1", "MDP_SIM_LAUNCH_PTS=x",
                "MDP_SIM_WIDE=1"):
        r = _plan(row, 0, bad)
        assert r.returncode == 1 and "scnsim_plan_check:" in r.stderr, bad
    r = _plan(ref.synthetic_row(26, 11), 0, "", 2, 10)  # hist alone: no lik line, no refusal
    assert r.returncode == 0 and "lik" not in r.stdout


# ---------------------------------------------------------------------------
# the C ABI: symbols, version, and every refusal without a device
# ---------------------------------------------------------------------------
def test_symbols_and_version():
    lib = _lib.lib()
    for name in ("create", "destroy", "kernel", "tables", "tables_device", "lik", "time_kernel"):
        assert hasattr(lib, "mdp_scenario_sim_" + name)
    assert lib.mdp_abi_version() == 9
    with mdp.ScenarioSim(np.ones(26, dtype=np.int32)) as sim:
        assert sim.kernel == "k_scnsim<32>"
    with mdp.ScenarioSim(np.ones(5, dtype=np.int32), options="MDP_SIM_NM=16") as sim:
        assert sim.kernel == "k_scnsim<16>"


def refused(code, fn, *a, **kw):
    with pytest.raises(mdp.MidaspomError, match=code):
        fn(*a, **kw)


def test_create_refusals():
    ok = np.ones(9, dtype=np.int32)
    refused("EINVAL", mdp.ScenarioSim, np.zeros(0, dtype=np.int32))
    refused("EINVAL", mdp.ScenarioSim, np.array([0, 2, 1], dtype=np.int32))
    refused("EINVAL", mdp.ScenarioSim, np.array([0, -2, 1], dtype=np.int32))
    refused("EUNSUPPORTED", mdp.ScenarioSim, np.ones(65, dtype=np.int32))
    for bad in ("MDP_SIM_NM=8", "MDP_SIM_NM=24", "MDP_SIM_NM=auto", "MDP_SIM_LAUNCH_PTS=1.5", "MDP_SCN_BIG=1", "X"):
        refused("EINVAL", mdp.ScenarioSim, ok, options=bad)


def _raw_tables(sim, e, c):
    """mdp_scenario_sim_tables on an (e, c) grid with one K and a one-cell
    hist: only for calls that are refused before the table is touched."""
    dp = lambda a: a.ctypes.data_as(_lib.c_dbl_p)
    one = np.ones(1)
    dummy = np.zeros(1, dtype=np.uint64)
    return _lib.lib().mdp_scenario_sim_tables(sim._h, 1, 1, dp(e), e.size, dp(c), c.size, dp(one), 1, dp(one), 1, 0, 0,
                                              1, dummy.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None)


def test_tables_refusals():
    """All of them on a host without a device: they come before the first device call."""
    u64 = np.uint64
    with mdp.ScenarioSim(ROW9, "loss") as sim:
        good = dict(e=0.3, c=0.4, K=[1.0], dsrc=[200.0], ts=2, tdis=2, nrep=10)
        refused("EINVAL", sim.tables, **good, hist=False, match=False)
        refused("EINVAL", sim.tables, **{**good, "ts": -1})
        refused("EINVAL", sim.tables, **{**good, "tdis": -1})
        for name in ("e", "c", "dsrc"):
            for bad in (-0.1, np.nan, np.inf):
                refused("EINVAL", sim.tables, **{**good, name: [bad]})
        for bad in (0.0, -1.0, np.nan, np.inf):
            refused("EINVAL", sim.tables, **{**good, "K": [1.0, bad]})
        refused("EUNSUPPORTED", sim.tables, **{**good, "ts": 12288, "tdis": 1})
        refused("EUNSUPPORTED", sim.tables, **{**good, "nrep": (1 << 31) + 1})
        # more than 2^20 points: 1025 x 1025 (e, c); refused before any table is touched
        rc = _raw_tables(sim, np.full(1025, 0.5), np.full(1025, 0.5))
        assert rc == -6 and b"points" in _lib.lib().mdp_last_error()
        refused("EINVAL", sim.lik, np.zeros((1, 4), dtype=u64), 0)
    with mdp.ScenarioSim(ref.synthetic_row(26, 11)) as sim:
        refused("EUNSUPPORTED", sim.tables, 0.3, 0.4, [1.0], nrep=10)  # match with 11 missing patches
        # 2^20 points x 27 hist cells: more than 2^24 cells
        rc = _raw_tables(sim, np.full(1024, 0.5), np.full(1024, 0.5))
        assert rc == -6 and b"cells" in _lib.lib().mdp_last_error()
        if mdp.device_count() == 0:  # hist alone passes every refusal and reaches the device
            refused("ENODEV", sim.tables, 0.3, 0.4, [1.0], nrep=10, match=False)
