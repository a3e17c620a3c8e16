"""The future engine's summaries (mdp_future_summary), the parts that need no
GPU.

`summary_checker()` restates the loop of test_future_wide_host.checker so that
it records the state after every year: hist[t][m] (replicates with exactly m
occupied patches after year t + 1) and occ[t][k] (replicates with patch k
occupied).  It is pinned here to checker() -- counts, final states, and the
tables of checker(tfut=t) for every t -- and to oracle.future_counts
(hist[:, 0]) on that file's five oracle problems; the GPU tests
(test_gpu_future_summary.py) import it.

Also here: the two numpy helpers, the rpost reader of the -H / -O files, the
new symbols, and the window planner (future_plan_check's TFUT mode) against a
Python restatement, with the 2^21-cell cap's boundary.
"""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle
from midaspom_amd import rpost
from test_future_wide_host import (PLAN_CHECK, RAND_MAX, checker, layout, make_row, matrix, philox_pairs,
                                   posterior21)


def summary_checker(row, post, nrep, tfut, seed=0, rep0=0, m=400.0, d=200.0, KD=1.0, KS=0.0, dS=200.0):
    """(hist[tfut, n+1], occ[tfut, n], states[nrep, n]) of replicates
    [rep0, rep0 + nrep): checker()'s loop, every year recorded."""
    row = np.asarray(row, dtype=np.int64)
    n = row.size
    post = np.asarray(post, dtype=np.float64)
    s = post.shape[0] if post.size else 0
    M = matrix(n, m, d, dS)
    pcum = []
    acc = 0.0
    for ie in range(s):
        for ic in range(s):
            w = 1.0
            if ie in (0, s - 1):
                w *= 0.5
            if ic in (0, s - 1):
                w *= 0.5
            acc += w * float(post[ie, ic])
            pcum.append(acc)
    pscale = float((s - 1) * (s - 1))

    def scan(rep):
        r = int(philox_pairs(seed, rep, 0xffffffff, [0])[0, 0]) >> 1
        pec = pscale * float(r) / RAND_MAX
        for i, v in enumerate(pcum):
            if pec < v:
                return (i // s) * 0.01, (i % s) * 0.01
        return None

    missing = np.flatnonzero(row == -1)
    nmiss = missing.size
    pairs = np.arange((n + 1) // 2)
    k = np.arange(n)
    hist = np.zeros((tfut, n + 1), dtype=np.uint64)
    occt = np.zeros((tfut, n), dtype=np.uint64)
    states = np.zeros((nrep, n), dtype=bool)
    ec = (0.0, 0.0)
    q = rep0
    while q > 0:
        q -= 1
        found = scan(q)
        if found:
            ec = found
            break
    for i in range(nrep):
        rep = rep0 + i
        found = scan(rep)
        if found:
            ec = found
        e, c = ec
        init = (int(philox_pairs(seed, rep, 0xffffffff, [0])[1, 0]) >> 1) % (1 << nmiss)
        occ = row == 1
        for qi, col in enumerate(missing):
            occ[col] = (init >> (nmiss - 1 - qi)) & 1
        with np.errstate(divide="ignore", invalid="ignore"):
            E = np.float64(e) / np.float64(KD)
        if E > 1:
            E = 1.0
        for t in range(tfut):
            w = philox_pairs(seed, rep, t, pairs)
            ext = (w[2 * (k & 1), k >> 1] >> np.uint64(1)).astype(np.float64) / RAND_MAX
            col = (w[2 * (k & 1) + 1, k >> 1] >> np.uint64(1)).astype(np.float64) / RAND_MAX
            surv = occ & (ext > E)
            s1 = np.zeros(n)
            for l in np.flatnonzero(surv):
                s1 += M[l] * KD
            s1 += M[n] * KS
            pc = np.minimum(c * s1, 1.0)
            occ = surv | (~surv & (col < pc))
            hist[t, int(occ.sum())] += np.uint64(1)
            occt[t] += occ.astype(np.uint64)
        states[i] = occ
    return hist, occt, states


def identities(hist, occ, nrep):
    """The identities the tables hold by construction."""
    n = occ.shape[1]
    assert hist.shape == (occ.shape[0], n + 1)
    assert np.array_equal(hist.sum(axis=1), np.full(hist.shape[0], nrep, dtype=np.uint64))
    assert np.array_equal((hist * np.arange(n + 1, dtype=np.uint64)).sum(axis=1), occ.sum(axis=1))


# ---------------------------------------------------------------------------
# 1. the per-year checker against checker() and the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,KD,KS", [(1, 1.0, 0.0), (9, 0.3, 2.0), (17, 0.0, 1.0), (33, 1.0, 0.2), (64, 4.0, 0.7)])
def test_summary_checker_equals_checker_and_oracle(n, KD, KS):
    row = make_row(n, min(3, n), 0.5, seed=n)
    post = posterior21() * 0.5
    kw = dict(m=400.0, d=100.0, KD=KD, KS=KS, dS=150.0)
    ref = oracle.future_counts(row, post, tfut=9, nrep=300, seed=77, rep0=1234, **kw)
    hist, occ, states = summary_checker(row, post, 300, 9, seed=77, rep0=1234, **kw)
    counts, last = checker(row, post, 300, 9, seed=77, rep0=1234, **kw)
    assert np.array_equal(hist[:, 0], ref)
    assert np.array_equal(hist[:, 0], counts)
    assert np.array_equal(states, last)
    identities(hist, occ, 300)


def test_summary_checker_equals_checker_year_by_year():
    """checker(tfut=t) for t = 1..T gives the same tables (n = 65, missing data)."""
    row = make_row(65, 4, 0.3, seed=5)
    post = posterior21() * 0.7
    kw = dict(m=400.0, d=100.0, KD=0.5, KS=0.2, dS=150.0)
    nrep, T = 20, 5
    hist, occ, _ = summary_checker(row, post, nrep, T, seed=3, rep0=17, **kw)
    for t in range(1, T + 1):
        _, st = checker(row, post, nrep, t, seed=3, rep0=17, **kw)
        assert np.array_equal(occ[t - 1], st.sum(axis=0).astype(np.uint64))
        assert np.array_equal(hist[t - 1], np.bincount(st.sum(axis=1), minlength=66).astype(np.uint64))
    identities(hist, occ, nrep)
    assert len(np.flatnonzero(hist[-1])) > 3  # a spread of occupied counts


# ---------------------------------------------------------------------------
# 2. helpers and file formats
# ---------------------------------------------------------------------------
def test_helpers():
    hist = np.array([[0, 1, 2, 1], [3, 1, 0, 0], [0, 0, 0, 4]], dtype=np.uint64)
    assert np.array_equal(mdp.quasi_extinction(hist, 0), hist[:, 0])
    assert np.array_equal(mdp.quasi_extinction(hist, 1), [1, 4, 0])
    assert np.array_equal(mdp.quasi_extinction(hist, 3), [4, 4, 4])
    assert np.array_equal(mdp.quasi_extinction(hist, 7), [4, 4, 4])
    assert mdp.quasi_extinction(hist, 1).dtype == np.uint64
    assert np.array_equal(mdp.mean_occupied(hist), [(1 + 4 + 3) / 4, 1 / 4, 3.0])
    assert np.isnan(mdp.mean_occupied(np.zeros((1, 3), dtype=np.uint64))[0])


def test_rpost_reads_the_summary_files(tmp_path):
    h = tmp_path / "hist.txt"
    o = tmp_path / "occ.txt"
    h.write_text("1\t2\t0\t\n0\t0\t3\t\n")
    o.write_text("2\t0\t\n3\t3\t\n")
    hist, occ = rpost.read_future_summary(h, o, n=2, tfut=2)
    assert hist.dtype == np.uint64 and occ.dtype == np.uint64
    assert np.array_equal(hist, [[1, 2, 0], [0, 0, 3]])
    assert np.array_equal(occ, [[2, 0], [3, 3]])
    assert np.array_equal(rpost.read_future_table(h, 3), hist)
    big = tmp_path / "big.txt"
    big.write_text(f"{2**63 + 5}\t0\t\n")
    assert int(rpost.read_future_table(big, 2)[0, 0]) == 2**63 + 5  # no pass through float
    with pytest.raises(ValueError, match="cells"):
        rpost.read_future_table(h, 2)                      # n + 1 = 3 cells per line
    with pytest.raises(ValueError, match="lines"):
        rpost.read_future_summary(h, o, n=2, tfut=3)
    bad = tmp_path / "bad.txt"
    bad.write_text("1\t-2\t\n")
    with pytest.raises(ValueError):
        rpost.read_future_table(bad, 2)
    o.write_text("2\t0\t\n3\t2\t\n")                        # sum_k occ != sum_m m hist in year 1
    with pytest.raises(ValueError, match="year 1"):
        rpost.read_future_summary(h, o, n=2, tfut=2)


# ---------------------------------------------------------------------------
# 3. ABI
# ---------------------------------------------------------------------------
def test_summary_symbols_without_an_abi_bump():
    lib = mdp._lib.lib()
    assert lib.mdp_abi_version() == 9
    for name in ("mdp_future_summary", "mdp_future_summary_device", "mdp_future_time_summary"):
        assert hasattr(lib, name)


# ---------------------------------------------------------------------------
# 4. the window planner (future_plan_check ROW ... OPTIONS TFUT)
# ---------------------------------------------------------------------------
def window_plan(n, wide, tfut, cap=0):
    """The line future_plan_check prints, from DESIGN.md §12's arithmetic: a
    window's table takes at most 16 KB of LDS in 32-bit cells, and the grid
    is capped at the workgroups 256 CUs hold at the kernel's register count."""
    NP = (1 if n <= 128 else 2 if n <= 256 else 4 if n <= 512 else 8) if wide else 0
    cells = n + 1 + 128 * NP if wide else 2 * n + 1
    years = min(16384 // (4 * cells), tfut)
    if cap:
        years = min(years, cap)
    windows = -(-tfut // years)
    fixed = 2 * ((n + 128 * NP + 1) & ~1) * 8 if wide else (16384 if n <= 8 else 0)
    reps = 1 << 31 if windows == 1 else (1 << 16 if wide else 1 << 20)
    grid = {1: 2048, 2: 2048, 4: 1280, 8: 768}[NP] if wide else 2048 if n <= 8 else 1024 if n <= 16 else 512
    return (f"summary cells {cells} years {years} windows {windows} lds {fixed + years * cells * 4} "
            f"grid {grid} reps {reps}\n")


def _plan(row, options, tfut=None):
    assert PLAN_CHECK.exists(), "future_plan_check is built by `make -C midaspom_amd/csrc`"
    text = "".join("m" if v == -1 else str(int(v)) for v in row)
    args = [str(PLAN_CHECK), text, "400.0", "100.0", "0.7", "0.3", "150.0", options]
    return subprocess.run(args + ([str(tfut)] if tfut is not None else []), capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("n,tfut,cap", [(1, 50, 0), (7, 50, 0), (8, 12288, 0), (9, 50, 3), (17, 50, 0), (64, 50, 0),
                                        (64, 12288, 0), (64, 8, 1), (65, 8, 3), (128, 50, 0), (129, 50, 0),
                                        (257, 50, 0), (513, 50, 0), (1024, 50, 0), (1024, 1023, 0), (1024, 8, 1)])
def test_window_plan(n, tfut, cap):
    row = make_row(n, min(5, n), 0.4, seed=1000 + n)
    opts = "MDP_FUT_WIDE=auto" + (f";MDP_FUT_SUM_YEARS={cap}" if cap else "")
    r = _plan(row, opts, tfut)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines(keepends=True)
    assert lines[-1] == window_plan(n, n > 64, tfut, cap)
    # everything before the new line is the program's output without TFUT
    assert "".join(lines[:-1]) == _plan(row, opts).stdout
    if n <= 64:  # the same problem on the patch-parallel kernel
        r = _plan(row, "MDP_FUT_WIDE=1", tfut)
        assert r.returncode == 0, r.stderr
        assert r.stdout == layout(list(row), 400.0, 100.0, 0.7, 0.3, 150.0) + window_plan(n, True, tfut)
    years = int(lines[-1].split()[4])
    assert years >= 1 and years * int(lines[-1].split()[2]) * 4 <= 16384


def test_window_plan_cap_boundary():
    """tfut * (2n+1) <= 2^21 cells: 1023 years at 1024 patches pass, 1024 do
    not; the largest lane case, 12288 x 129, passes; 12289 years never do."""
    row = make_row(1024, 5, 0.4, seed=1)
    assert 1023 * 2049 <= 1 << 21 < 1024 * 2049
    assert _plan(row, "MDP_FUT_WIDE=auto", 1023).returncode == 0
    r = _plan(row, "MDP_FUT_WIDE=auto", 1024)
    assert r.returncode == 1 and "at most 2097152 cells" in r.stderr
    assert "check ok" in r.stdout  # the layout check itself still ran
    row = make_row(64, 5, 0.4, seed=1)
    assert _plan(row, "", 12288).returncode == 0
    for tfut in (0, 12289):
        r = _plan(row, "", tfut)
        assert r.returncode == 1 and "outside 1..12288 years" in r.stderr
    # 2n+1 is odd, so no run has exactly 2^21 cells; a second size where one
    # more year passes the cap
    row = make_row(341, 0, 0.4, seed=2)
    assert 3070 * 683 <= 1 << 21 < 3071 * 683
    assert _plan(row, "MDP_FUT_WIDE=auto", 3070).returncode == 0
    assert _plan(row, "MDP_FUT_WIDE=auto", 3071).returncode == 1


@pytest.mark.parametrize("options", ["MDP_FUT_SUM_YEARS=", "MDP_FUT_SUM_YEARS=-1", "MDP_FUT_SUM_YEARS=x",
                                     "MDP_FUT_SUM_YEARS=12289", "MDP_FUT_SUM_YEARS=3.5", "MDP_FUT_SUM_YEAR=3"])
def test_unknown_sum_years_value(options):
    r = _plan(make_row(9, 2, 0.4, seed=1), options, 8)
    assert r.returncode == 1 and ("MDP_FUT_SUM_YEARS=" in r.stderr or "unknown future option" in r.stderr)
    with pytest.raises(mdp.MidaspomError, match="EINVAL"):  # refused before any device call
        mdp.Future(np.ones(9, dtype=np.int32), posterior21(), options=options)
    r = _plan(make_row(9, 2, 0.4, seed=1), "MDP_FUT_SUM_YEARS=0;MDP_FUT_WIDE=auto", 8)
    assert r.returncode == 0 and r.stdout.splitlines()[-1].startswith("summary cells 19 years 8 windows 1 ")
