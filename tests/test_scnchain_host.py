"""The scenario chain (mdp_scenario_chain, k_scnchain<NM>, k_chain_eval), the
parts that need no GPU.

1. A test-local exact enumerator of the one-year matrix over the 2^n states,
   written from the reference's year (independent extinctions, then
   independent colonisations of the patches empty after them), pinned to the
   oracle: the column sums of A^ts B^tdis are oracle.dieoff_lik / loss_lik.
2. The numpy restatement of the replicate model (tests/scnchain_ref.py), the
   checker of the GPU tests, held to the exact lumped matrices: every count is
   a binomial with a known p.  Bound per cell with R p >= 100:
   |count - R p| <= 5 sqrt(R p (1 - p)); cells with p = 0 are 0.
3. The exact-lumping anchor: with exchangeable patches (d = 0, source at
   distance 0) and start = C(n, k) the chain on the exact lumped doubles IS
   the sum of the oracle's likelihoods over the rows of a count, and the
   chain on the restatement's counts estimates it within 5 %.
4. The host evaluation and default target of the library against numpy, bit
   for bit; the planner's stand-alone driver against a numpy restatement of
   its digest; every refusal of the C ABI and of the drop-ins, which all come
   before the first device call.
"""
from __future__ import annotations

import ctypes
import functools
import itertools
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle
import scnchain_ref as ref
import scnsim_ref
from midaspom_amd import _lib
from test_scnsim_host import fnv, refused, row_text

ROOT = Path(__file__).resolve().parents[1]
BUILD = ROOT / "midaspom_amd" / "_build"
PLAN_CHECK = BUILD / "scnchain_plan_check"

# one committed seed
SEED = 20261021
R = 200_000
E, C, M_, D_ = 0.4, 0.5, 400.0, 200.0
KS = (0.3, 1.0, 5.0)
DSRC = 300.0
DURATIONS = ((1, 0), (0, 1), (1, 1), (3, 2))
EVAL_DURATIONS = ((0, 0), (3, 0), (0, 2), (3, 2), (20, 26))


# ---------------------------------------------------------------------------
# the exact enumerator: P[i, j] of one year over the 2^n states, bit k of a
# state number = patch k
# ---------------------------------------------------------------------------
def exact_year(n, M, E, c, mode, K=1.0, src=None):
    """mode 0 baseline, 1 die-off year, 2 loss year (scnsim_ref.one_year's)."""
    S = 1 << n
    P = np.zeros((S, S))
    for i in range(S):
        occupied = [k for k in range(n) if (i >> k) & 1]
        for keep in itertools.product((0, 1), repeat=len(occupied)):
            pe, s = 1.0, 0
            for k, b in zip(occupied, keep):
                pe *= (1.0 - E) if b else E
                s |= b << k
            if pe == 0.0:
                continue
            # colonisation of the patches empty after the extinctions
            dist = {s: pe}
            for k in range(n):
                if (s >> k) & 1:
                    continue
                s1 = 0.0
                for l in range(n):
                    if (s >> l) & 1:
                        s1 += M[l][k]
                if mode == 1:
                    pc = (c * s1) * K
                elif mode == 2:
                    pc = c * (s1 + src[k] * K)
                else:
                    pc = c * s1
                pc = min(1.0, pc)
                nxt = {}
                for st, pr in dist.items():
                    if pc < 1.0:
                        nxt[st] = nxt.get(st, 0.0) + pr * (1.0 - pc)
                    if pc > 0.0:
                        nxt[st | (1 << k)] = nxt.get(st | (1 << k), 0.0) + pr * pc
                dist = nxt
            for st, pr in dist.items():
                P[i, st] += pr
    return P


def year_matrices(n, kind, K, e=E, c=C, d=D_, dsrc=DSRC):
    """(A, B): the exact scenario and baseline years of one grid point."""
    M = scnsim_ref.dispersal(n, M_, d)
    src = scnsim_ref.source_row(n, M_, dsrc) if kind == 1 else None
    Es = min(1.0, e / K if kind == 0 else e)
    return exact_year(n, M, Es, c, 1 + kind, K, src), exact_year(n, M, min(1.0, e), c, 0)


def lump(P, n):
    """[k, l]: from a uniform state of class k to class l."""
    pop = np.array([bin(s).count("1") for s in range(1 << n)])
    out = np.zeros((n + 1, n + 1))
    for k in range(n + 1):
        rows = P[pop == k]
        for l in range(n + 1):
            out[k, l] = rows[:, pop == l].sum() / rows.shape[0]
    return out


def state_row(s, n):
    return [(s >> k) & 1 for k in range(n)]


def oracle_lik(row, kind, K, ts, tdis, e=E, c=C, d=D_, dsrc=DSRC):
    if kind == 0:
        return float(oracle.dieoff_lik(row, [K], e, c, ts, tdis, M_, 0.5, d)[0])
    return float(oracle.loss_lik(row, [K], [dsrc], e, c, ts, tdis, M_, 0.5, d)[0, 0])


@pytest.mark.parametrize("kind", [0, 1])
def test_exact_matrices_against_oracle(kind):
    n = 4
    worst = 0.0
    for K in KS:
        A, B = year_matrices(n, kind, K)
        assert np.abs(A.sum(axis=1) - 1.0).max() < 1e-14 and np.abs(B.sum(axis=1) - 1.0).max() < 1e-14
        for ts, tdis in DURATIONS:
            F = np.linalg.matrix_power(A, ts) @ np.linalg.matrix_power(B, tdis)
            for s in range(1 << n):
                want = oracle_lik(state_row(s, n), kind, K, ts, tdis)
                worst = max(worst, abs(F[:, s].sum() - want))
    print(f"kind {kind}: max |column sum - oracle| {worst:.3e}")
    assert worst <= 1e-12


def test_class_0_is_not_absorbing_under_loss():
    A, B = year_matrices(4, 1, 1.0)
    a0 = lump(A, 4)[0]
    print("loss, K = 1, class 0:", a0)
    assert a0[0] < 0.9 and a0[1] > 0.05
    assert lump(B, 4)[0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert lump(year_matrices(4, 0, 1.0)[0], 4)[0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]


# ---------------------------------------------------------------------------
# the restatement against the exact lumped matrices
# ---------------------------------------------------------------------------
def anchor_counts(kind, baseline):
    """The restatement's tables of the n = 4 anchor (shared with the GPU test)."""
    return ref.counts_cached(4, kind, (E,), (C,), None if baseline else KS, (DSRC,) if kind and not baseline else None,
                             R, SEED, 0, baseline)


def cells_within(cnt, exact, what):
    tested = 0
    for k, l in np.ndindex(exact.shape):
        p, got = float(exact[k, l]), int(cnt[k, l])
        if p == 0.0:
            assert got == 0, f"{what} [{k},{l}]: {got} replicates in an impossible cell"
        elif R * p >= 100:
            sd = math.sqrt(R * p * (1.0 - p))
            print(f"{what} [{k},{l}]: count {got} expected {R * p:.1f} sd {sd:.1f} z {(got - R * p) / sd if sd else 0:+.2f}")
            assert abs(got - R * p) <= 5.0 * sd + 1e-6, f"{what} [{k},{l}]"
            tested += 1
    return tested


@pytest.mark.parametrize("kind", [0, 1])
def test_restatement_against_exact_lumped(kind):
    scn, base = anchor_counts(kind, False), anchor_counts(kind, True)
    assert (scn.sum(axis=-1) == R).all() and (base.sum(axis=-1) == R).all()
    tested = 0
    for iK, K in enumerate(KS):
        A, B = year_matrices(4, kind, K)
        tested += cells_within(scn[0, 0, iK, 0], lump(A, 4), f"kind {kind} K {K} A")
    tested += cells_within(base[0, 0], lump(B, 4), f"kind {kind} B")
    print(f"kind {kind}: {tested} cells tested")
    assert tested >= 50


def test_start_states():
    n, nrep = 7, 20_000
    reps = np.arange(nrep, dtype=np.int64)
    for k in range(n + 1):
        occ = ref.start_states(n, k, SEED, reps)
        assert (occ.sum(axis=1) == k).all()
        code = (occ.astype(np.int64) << np.arange(n)).sum(axis=1)
        subsets = [sum(1 << j for j in s) for s in itertools.combinations(range(n), k)]
        seen = np.bincount(code, minlength=1 << n)
        assert seen[subsets].sum() == nrep
        p = 1.0 / len(subsets)
        sd = math.sqrt(nrep * p * (1.0 - p))
        z = (seen[subsets] - nrep * p) / sd if sd else np.zeros(1)
        print(f"k {k}: {len(subsets)} subsets, |z| max {np.abs(z).max():.2f}")
        assert np.abs(seen[subsets] - nrep * p).max() <= 5.0 * sd
    # the draws straight from the generator's host restatement
    need, want = 3, []
    for j in range(n):
        u = mdp.philox(SEED, [5, 0, 0xfffffffe, 16 * 3 + (j >> 2)])[j & 3]
        take = ((u * (n - j)) >> 32) < need
        need -= take
        want.append(bool(take))
    assert want == list(ref.start_states(n, 3, SEED, np.array([5], dtype=np.int64))[0]) and sum(want) == 3


# ---------------------------------------------------------------------------
# the exact-lumping anchor: exchangeable patches
# ---------------------------------------------------------------------------
AN, AE, AC, ATS, ATDIS = 6, 0.3, 0.1, 3, 2
AKS = (1.0, 5.0)


def anchor_oracle_sums(kind, K):
    """[m]: the sum of the oracle's likelihoods over the complete rows with m
    occupied patches (d = 0, source at distance 0)."""
    out = np.zeros(AN + 1)
    for s in range(1 << AN):
        out[bin(s).count("1")] += oracle_lik(state_row(s, AN), kind, K, ATS, ATDIS, AE, AC, 0.0, 0.0)
    return out


@functools.lru_cache(maxsize=None)
def anchor_exact(kind):
    """{K: (oracle sums[m], lumped A, lumped B)}, once per session."""
    out = {}
    for K in AKS:
        A, B = year_matrices(AN, kind, K, AE, AC, 0.0, 0.0)
        out[K] = (anchor_oracle_sums(kind, K), lump(A, AN), lump(B, AN))
    return out


def anchor_check(got, want, what):
    """got[m], want[m] over the targets m: 5 % at every m whose exact value is
    >= 0.1 of the largest; returns how many were held."""
    held = 0
    for m in range(AN + 1):
        if want[m] >= 0.1 * want.max():
            print(f"{what} m {m}: chain {got[m]:.6g} exact {want[m]:.6g} rel {got[m] / want[m] - 1:+.4f}")
            assert abs(got[m] - want[m]) <= 0.05 * want[m], f"{what} m {m}"
            held += 1
    return held


@pytest.mark.parametrize("kind", [0, 1])
def test_exact_lumping_anchor(kind):
    start = ref.states_start(AN)
    scn = ref.counts_cached(AN, kind, (AE,), (AC,), AKS, (0.0,) if kind else None, R, SEED, 0, False, M_, 0.0)
    base = ref.counts_cached(AN, kind, (AE,), (AC,), None, None, R, SEED, 0, True, M_, 0.0)
    for iK, K in enumerate(AKS):
        sums, A, B = anchor_exact(kind)[K]
        for m in range(AN + 1):
            target = np.eye(AN + 1)[m]
            exact, _ = ref.evaluate(A[None, None], B[None, None], ATS, ATDIS, start, target)
            assert abs(exact[0, 0] - sums[m]) <= 1e-12 * sums[m], (kind, K, m, exact[0, 0], sums[m])
        got = np.array([ref.evaluate_counts(scn[:, :, iK, 0], R, base, R, ATS, ATDIS, start, np.eye(AN + 1)[m])[0][0, 0]
                        for m in range(AN + 1)])
        assert anchor_check(got, sums, f"kind {kind} K {K}") >= 6  # power: six or seven targets carry the bound


# ---------------------------------------------------------------------------
# the library's host evaluation and default target
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_host_eval_equals_numpy(kind):
    scn, base = anchor_counts(kind, False), anchor_counts(kind, True)
    cs = scn[:, :, :, 0] if kind == 0 else scn  # die-off grids have no distance axis
    rows = {0: [0, 1, 1, 0], 2: [1, -1, 0, -1]}
    with mdp.ScenarioChain(rows[0], "loss" if kind else "dieoff") as ch, \
            mdp.ScenarioChain(rows[2], "loss" if kind else "dieoff", p=0.3) as ch2:
        for r, c_ in ((rows[0], ch), (rows[2], ch2)):
            want_t = ref.default_target(r, 0.5 if c_ is ch else 0.3)
            assert np.array_equal(c_.target(), want_t) and abs(want_t.sum() - 1.0) < 1e-7
        assert ch.target().tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]
        p = float(np.float32(0.3))
        assert ch2.target().tolist() == [0.0, (1.0 * 1.0) * math.pow(1 - p, 2.0), (2.0 * p) * (1 - p), (1.0 * (p * p)) * 1.0,
                                         0.0]
        for ts, tdis in EVAL_DURATIONS:
            for chain, row, pp in ((ch, rows[0], 0.5), (ch2, rows[2], 0.3)):
                for start in ("uniform", "states"):
                    w = None if start == "uniform" else ref.states_start(4)
                    want, want_by = ref.evaluate_counts(scn, R, base, R, ts, tdis, w, ref.default_target(row, pp))
                    if kind == 0:
                        want, want_by = want[:, :, :, 0], want_by[:, :, :, 0]
                    got, by = chain.eval(cs, R, base, R, ts=ts, tdis=tdis, start=start, by_class=True)
                    assert np.array_equal(got, want) and np.array_equal(by, want_by), (ts, tdis, start)
        # explicit weights
        t = np.array([0.1, 0.0, 2.0, 0.5, 0.25])
        want, _ = ref.evaluate_counts(scn, R, base, 2 * R, 3, 2, t[::-1], t)
        got = ch.eval(cs, R, base, 2 * R, ts=3, tdis=2, start=t[::-1], target=t)
        assert np.array_equal(got.reshape(want.shape), want)


# ---------------------------------------------------------------------------
# the planner's driver against a numpy restatement of its digest
# ---------------------------------------------------------------------------
def _plan(row, kind=1, options="", nK=5, nrep=777, dsrc=300.0, p=0.3):
    return subprocess.run([str(PLAN_CHECK), row_text(row), "400", repr(p), "200", str(kind), options, str(nK),
                           str(nrep), repr(dsrc)], capture_output=True, text=True)


def want_launches(G, tpp, launch_pts, parts, cells_per_point):
    per = min(G, launch_pts if launch_pts else max(1, (256 << 20) // (cells_per_point * 4)))
    out = []
    for p0 in range(0, G, per):
        npts = min(per, G - p0)
        pr = max(1, min(parts if parts else -(-2048 // npts), tpp))
        out.append(f"launch p0 {p0} npts {npts} parts {pr} units {npts * pr} nwg {min(npts * pr, 4096)}")
    return out


@pytest.mark.parametrize("n,nmiss", [(n, k) for n in (1, 8, 9, 26, 64) for k in (0, 1, 3, 10) if k <= n])
def test_plan_digest(n, nmiss):
    row = scnsim_ref.synthetic_row(n, nmiss)
    nK, nrep, dsrc, p = 5, 777, 300.0, 0.3
    r = _plan(row, 1, "MDP_CHAIN_LAUNCH_PTS=2", nK, nrep, dsrc, p)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    nm = 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64
    assert lines[0] == f"kernel k_scnchain<{nm}>"
    assert lines[1] == f"row n {n} nmiss {nmiss} n1 {int((row == 1).sum())}"
    M = np.zeros((nm, nm))
    M[:n, :n] = scnsim_ref.dispersal(n, 400.0, 200.0)
    src = np.zeros(nm)
    src[:n] = scnsim_ref.source_row(n, 400.0, dsrc)
    target = ref.default_target(row, p)
    assert lines[2] == f"M {fnv(M.tobytes()):016x} target {fnv(target.tobytes()):016x} src {fnv(src.tobytes()):016x}"
    tpc, ncl = (nrep + 255) // 256, n + 1
    assert lines[3] == (f"call points {nK} tiles_per_class {tpc} tiles_per_point {tpc * ncl} cells {nK * ncl * ncl} "
                        f"launches 3")
    assert lines[4:7] == want_launches(nK, tpc * ncl, 2, 0, ncl * ncl)
    assert lines[7] == f"base points 1 tiles_per_class {tpc} tiles_per_point {tpc * ncl} cells {ncl * ncl} launches 1"
    assert lines[8] == want_launches(1, tpc * ncl, 2, 0, ncl * ncl)[0]
    k, l = np.indices((ncl, ncl))
    a, b = ((7 * k + 3 * l) % 5 + 1).astype(np.uint64), ((k + 2 * l) % 3 + 1).astype(np.uint64)
    want, by = ref.evaluate_counts(a[None, None, None, None], 10, b[None, None], 10, 2, 1, None, target)
    word = lines[9].split()
    assert word[0] == "eval" and float.fromhex(word[1]) == float(want[0, 0, 0, 0])
    assert word[2:] == ["by_class", f"{fnv(by.tobytes()):016x}"]


def test_plan_cut_and_options():
    row = scnsim_ref.synthetic_row(26, 3)
    # the reference-shaped job: one workgroup per point for thousands of points, many for the one baseline point
    r = _plan(row, 0, "", 1000, 1000)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[4] == "launch p0 0 npts 1000 parts 3 units 3000 nwg 3000"
    r = _plan(row, 0, "", 46000, 1000)
    assert r.stdout.splitlines()[4] == "launch p0 0 npts 46000 parts 1 units 46000 nwg 4096"
    r = _plan(row, 0, "", 1, 100000)
    assert r.stdout.splitlines()[6] == "launch p0 0 npts 1 parts 2048 units 2048 nwg 2048"
    # the planner's cut: a 64-patch row holds floor(2^28 / (65*65*4)) = 15883 points in 256 MiB
    r = _plan(scnsim_ref.synthetic_row(64, 0), 0, "", 20000, 10)
    lines = r.stdout.splitlines()
    assert "launches 2" in lines[3] and lines[4].startswith("launch p0 0 npts 15883 ")
    assert lines[5].startswith("launch p0 15883 npts 4117 ")
    r = _plan(row, 0, "MDP_CHAIN_PARTS=3;MDP_CHAIN_NM=64", 4, 1000)
    assert r.stdout.startswith("kernel k_scnchain<64>\n") and "npts 4 parts 3 units 12 nwg 12" in r.stdout
    r = _plan(row, 0, "MDP_CHAIN_PARTS=1000000", 1, 10)  # never more runs than tiles
    assert "npts 1 parts 27 units 27" in r.stdout
    for bad in ("MDP_CHAIN_NM=16", "MDP_CHAIN_NM=12", "MDP_CHAIN_NM=", "MDP_CHAIN_LAUNCH_PTS=-1", "MDP_CHAIN_PARTS=x",
                "MDP_SIM_NM=32", "MDP_CHAIN_WIDE=1"):
        r = _plan(row, 0, bad)
        assert r.returncode == 1 and "scnchain_plan_check:" in r.stderr, bad


def test_plan_check_under_the_host_sanitizers(tmp_path):
    """The stand-alone driver built with -fsanitize=address,undefined runs clean."""
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "midaspom_amd" / "csrc"), "scnchain_plan_check_san",
                        f"OUT={tmp_path}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exe = tmp_path / "san" / "scnchain_plan_check"
    for row, opts, nK in ((scnsim_ref.synthetic_row(64, 10), "MDP_CHAIN_LAUNCH_PTS=3", 7),
                          (scnsim_ref.synthetic_row(1, 1), "", 1), (scnsim_ref.synthetic_row(26, 3), "MDP_CHAIN_PARTS=5", 9)):
        args = [row_text(row), "400", "0.3", "200", "1", opts, str(nK), "777", "300.0"]
        a = subprocess.run([str(exe), *args], capture_output=True, text=True)
        b = subprocess.run([str(PLAN_CHECK), *args], capture_output=True, text=True)
        assert a.returncode == 0 and a.stderr == "", a.stderr[-2000:]
        assert a.stdout == b.stdout


# ---------------------------------------------------------------------------
# the C ABI: symbols, version, and every refusal without a device
# ---------------------------------------------------------------------------
def test_symbols_version_and_option_names():
    lib = _lib.lib()
    for name in ("create", "destroy", "kernel", "target", "counts", "eval", "lik", "lik_device", "time_kernels"):
        assert hasattr(lib, "mdp_scenario_chain_" + name)
    assert lib.mdp_abi_version() == 9
    assert _lib.SCENARIO_SIM_OPTION_NAMES == ("MDP_SIM_NM", "MDP_SIM_LAUNCH_PTS", "MDP_SIM_WAVE", "MDP_SIM_NP")
    assert _lib.SCENARIO_CHAIN_OPTION_NAMES == ("MDP_CHAIN_NM", "MDP_CHAIN_LAUNCH_PTS", "MDP_CHAIN_PARTS")
    with mdp.ScenarioChain(np.ones(26, dtype=np.int32)) as ch:
        assert ch.kernel == "k_scnchain<32>"
    with mdp.ScenarioChain(np.ones(5, dtype=np.int32), options="MDP_CHAIN_NM=16") as ch:
        assert ch.kernel == "k_scnchain<16>"


def test_create_refusals():
    ok = np.ones(9, dtype=np.int32)
    refused("EINVAL", mdp.ScenarioChain, np.zeros(0, dtype=np.int32))
    refused("EINVAL", mdp.ScenarioChain, np.array([0, 2, 1], dtype=np.int32))
    refused("EINVAL", mdp.ScenarioChain, np.array([0, -2, 1], dtype=np.int32))
    refused("EINVAL", mdp.ScenarioChain, ok, m=0.0)
    refused("EUNSUPPORTED", mdp.ScenarioChain, np.ones(65, dtype=np.int32))
    for bad in ("MDP_CHAIN_NM=8", "MDP_CHAIN_NM=24", "MDP_CHAIN_NM=auto", "MDP_CHAIN_LAUNCH_PTS=1.5", "MDP_CHAIN_PARTS=-2",
                "MDP_SIM_WAVE=1", "X"):
        refused("EINVAL", mdp.ScenarioChain, ok, options=bad)


ROW9 = (1, 0, -1, 1, 0, 1, -1, 0, 1)


def _raw_counts(ch, e, c):
    """mdp_scenario_chain_counts on an (e, c) grid with one K and a one-cell
    table: only for calls that are refused before the table is touched."""
    dp = lambda a: a.ctypes.data_as(_lib.c_dbl_p)
    one = np.ones(1)
    dummy = np.zeros(1, dtype=np.uint64)
    return _lib.lib().mdp_scenario_chain_counts(ch._h, 0, dp(e), e.size, dp(c), c.size, dp(one), 1, dp(one), 1, 0, 0, 1,
                                                dummy.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))


def test_call_refusals():
    """All of them on a host without a device: they come before the first device call."""
    with mdp.ScenarioChain(ROW9, "loss") as ch:
        good = dict(e=0.3, c=0.4, K=[1.0], dsrc=[200.0], nrep=10)
        for name in ("e", "c", "dsrc"):
            for bad in (-0.1, np.nan, np.inf):
                refused("EINVAL", ch.counts, **{**good, name: [bad]})
                refused("EINVAL", ch.lik, **{**good, name: [bad]})
        for bad in (0.0, -1.0, np.nan, np.inf):
            refused("EINVAL", ch.counts, **{**good, "K": [1.0, bad]})
        refused("EINVAL", ch.counts, e=[-1.0], c=0.4, baseline=True)
        refused("EUNSUPPORTED", ch.counts, **{**good, "nrep": (1 << 31) + 1})
        rc = _raw_counts(ch, np.full(1025, 0.5), np.full(1025, 0.5))
        assert rc == -6 and b"points" in _lib.lib().mdp_last_error()
        rc = _raw_counts(ch, np.full(512, 0.5), np.full(512, 0.5))  # 2^18 points x 100 cells
        assert rc == -6 and b"cells" in _lib.lib().mdp_last_error()
        # the evaluation's, through lik (before any device call) and through eval (which makes none)
        cs, cb = np.zeros((1, 1, 1, 1, 10, 10), dtype=np.uint64), np.zeros((1, 1, 10, 10), dtype=np.uint64)
        for call, base in ((ch.lik, {**good, "nbase": 10}), (ch.eval, dict(cnt_scn=cs, nrep=10, cnt_base=cb, nbase=10))):
            refused("EINVAL", call, **{**base, "ts": -1})
            refused("EINVAL", call, **{**base, "tdis": -1})
            refused("EINVAL", call, **{**base, "nrep": 0})
            refused("EINVAL", call, **{**base, "nbase": 0})
            refused("EUNSUPPORTED", call, **{**base, "ts": 12288, "tdis": 1})
            refused("EUNSUPPORTED", call, **{**base, "nrep": (1 << 31) + 1})
            refused("EUNSUPPORTED", call, **{**base, "nbase": (1 << 31) + 1})
            for bad in (-1.0, np.nan, np.inf):
                w = np.ones(10)
                w[3] = bad
                refused("EINVAL", call, **{**base, "start": w})
                refused("EINVAL", call, **{**base, "target": w})
        assert ch.eval(cs, 10, cb, 10, ts=12288, tdis=0).shape == (1, 1, 1, 1)
        if mdp.device_count() == 0:  # a good call passes every refusal and reaches the device
            refused("ENODEV", ch.counts, **good)
            refused("ENODEV", ch.lik, **good)


# ---------------------------------------------------------------------------
# the drop-ins' refusals: exit 1 with a message before any device call
# ---------------------------------------------------------------------------
def _run(cmd, *flags):
    import os
    env = dict(os.environ)
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([*cmd, "-a", "2", "-b", "3", "-e", "0.4", "-c", "0.5", "-s", "3", *flags],
                          capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)


@pytest.mark.parametrize("kind", ["dieoff", "loss"])
def test_dropin_refusals(tmp_path, kind):
    ok, wide = tmp_path / "row26.txt", tmp_path / "row65.txt"
    ok.write_text(" ".join("1" for _ in range(26)) + "\n")
    wide.write_text(" ".join("1" for _ in range(65)) + "\n")
    exe = _lib.DIEOFF_CLI_PATH if kind == "dieoff" else _lib.LOSS_CLI_PATH
    out = str(tmp_path / "no.txt")
    for cmd in ([str(exe)], [sys.executable, "-m", "midaspom_amd.scenario", kind]):
        r = _run(cmd, "-i", str(ok), "-o", out, "-C", "1000")
        assert r.returncode == 1 and "-C" in r.stderr and "needs -R" in r.stderr, r.stderr
        r = _run(cmd, "-i", str(ok), "-o", out, "-C", "1000", "-R", "100", "-H", str(tmp_path / "no.hist"))
        assert r.returncode == 1 and "-H is not available with -C" in r.stderr, r.stderr
        r = _run(cmd, "-i", str(wide), "-o", out, "-C", "1000", "-R", "100")
        assert r.returncode == 1 and "65 patches in the first row: -C takes at most 64" in r.stderr, r.stderr
        assert "Chain likelihood" not in r.stdout
    assert not (tmp_path / "no.txt").exists()
