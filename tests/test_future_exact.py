"""The exact references of the future engine (fut_exact.py) on the CPU:
binom_p against scipy and brute force, the three references against each
other to 1e-12, the oracle's counts at 4e5 replicates against the chain, the
sensitivity of the GPU cases (five mutants of the chain, each rejected by a
named case from the oracle's counts), and the non-vacuity of every case that
test_gpu_future_exact.py runs, from the references alone.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import fut_exact as fx
import oracle


# ---------------------------------------------------------------------------
# 1. binom_p
# ---------------------------------------------------------------------------
def test_binom_p_matches_scipy():
    stats = pytest.importorskip("scipy.stats")
    cases = []
    for N, p in [(10 ** 6, 1e-5), (10 ** 6, 0.5), (10 ** 6, 1 - 1e-4), (400000, 0.0706), (100000, 0.93), (1000, 0.1),
                 (7, 0.3)]:
        sd = math.sqrt(N * p * (1 - p))
        for zz in (-9, -6, -5, -3, -1, -0.2, 0, 0.2, 1, 3, 5, 6, 9):
            k = int(round(N * p + zz * sd))
            if 0 <= k <= N:
                cases.append((k, N, p))
        cases += [(0, N, p), (N, N, p), (int(N * p), N, p), (int(N * p) + 1, N, p)]
    worst = 0.0
    for k, N, p in cases:
        want = min(1.0, 2.0 * min(stats.binom.cdf(k, N, p), stats.binom.sf(k - 1, N, p)))
        got = fx.binom_p(k, N, p)
        if want > 1e-290:
            worst = max(worst, abs(got / want - 1.0))
            assert got == pytest.approx(want, rel=1e-7), (k, N, p)
        else:
            assert got < 1e-280, (k, N, p)
    print("largest relative difference from scipy", worst)
    # at N p near 100 the 5-sigma normal tail is wrong by more than a factor of 10
    N, p = 10 ** 6, 1e-4
    k = int(N * p - 5 * math.sqrt(N * p))
    ratio = math.erfc(5 / math.sqrt(2)) / fx.binom_p(k, N, p)
    print("normal / exact at 5 sigma below N p = 100:", ratio)
    assert max(ratio, 1 / ratio) > 10


def test_binom_p_matches_brute_force_sums():
    for N in (1, 2, 13, 50):
        for p in (0.0, 1e-3, 0.2, 0.5, 0.77, 1.0):
            pmf = [math.comb(N, j) * p ** j * (1 - p) ** (N - j) for j in range(N + 1)]
            for k in range(N + 1):
                want = min(1.0, 2.0 * min(math.fsum(pmf[:k + 1]), math.fsum(pmf[k:])))
                assert fx.binom_p(k, N, p) == pytest.approx(want, rel=1e-12, abs=1e-300), (k, N, p)


def test_check_rule():
    N = 10000
    fx.check([5000, 0, N], N, [0.5, 0.0, 1.0])
    for counts in ([5000, 1, N], [5000, 0, N - 1], [5300, 0, N]):   # p = 0 counts 0, p = 1 counts N, 6 sigma
        with pytest.raises(AssertionError):
            fx.check(counts, N, [0.5, 0.0, 1.0])
    # Bonferroni: a p-value of 2.7e-6 fails alone (below 1e-5) and passes among ten cells (above 1e-6)
    k = next(k for k in range(5000, 5400) if fx.binom_p(k, N, 0.5) < 3e-6)
    assert 1e-6 < fx.binom_p(k, N, 0.5)
    with pytest.raises(AssertionError):
        fx.check([k], N, [0.5])
    fx.check([k] + [5000] * 9, N, [0.5] * 10)


# ---------------------------------------------------------------------------
# 2. the three references against each other
# ---------------------------------------------------------------------------
def test_year1_equals_the_chain():
    """n = 10, three missing patches, a cell with e/K_D > 1, the clamp out of reach."""
    row = np.array([1, 0, -1, 1, 0, 0, -1, 1, -1, 0], dtype=np.int32)
    post = fx.posterior(21, {(3, 5): 1.0, (8, 2): 2.0, (20, 9): 1.0, (0, 7): 0.5, (12, 0): 0.5})
    kw = dict(m=400.0, d=100.0, KD=0.1, KS=1.5, dS=60.0)
    assert max(e / kw["KD"] for e, _, _ in fx.cells(post)) > 1
    _, _, occ = fx.chain(row, post, 1, **kw)
    got = fx.year1(row, post, **kw)
    print("largest difference", np.abs(got - occ[0]).max())
    assert np.abs(got - occ[0]).max() < 1e-12
    with pytest.raises(ValueError, match="clamp"):
        fx.year1(row, post, **dict(kw, KS=20.0))


def test_isolated_equals_the_chain():
    row = np.array([1, -1, 0, 1, -1, 0], dtype=np.int32)
    post = fx.posterior(21, {(3, 5): 1.0, (8, 20): 2.0, (20, 9): 1.0, (12, 0): 0.5})
    kw = dict(m=2.0, d=200.0, KD=0.1, KS=3.0, dS=0.7)
    want = fx.chain(row, post, 7, **kw)
    got = fx.isolated(row, post, 7, **kw)
    for a, b in zip(got, want):
        assert np.abs(a - b).max() < 1e-12
    with pytest.raises(AssertionError):
        fx.isolated(row, post, 7, **dict(kw, d=150.0))


@pytest.mark.parametrize("name", sorted(fx.CHAIN_CASES))
def test_chain_tables_are_distributions(name):
    """Rows sum to 1, hist[:, 0] is P(all empty), and `identities` holds in
    expectation: sum_j j hist[t][j] = sum_k occ[t][k]."""
    c = fx.CHAIN_CASES[name]
    pext, hist, occ = chain_of(name)
    n = c["row"].size
    assert np.abs(hist.sum(axis=1) - 1.0).max() < 1e-12
    assert np.abs(hist[:, 0] - pext).max() < 1e-12
    assert np.abs(hist @ np.arange(n + 1) - occ.sum(axis=1)).max() < 1e-12
    assert hist.min() >= 0 and occ.min() >= 0 and occ.max() <= 1


def test_partial_mass_is_refused():
    with pytest.raises(ValueError, match="mass"):
        fx.cells(fx.posterior(11, {(2, 3): 1.0}) * 0.99)
    assert sum(w for _, _, w in fx.cells(fx.posterior(11, {(0, 0): 1.0, (10, 4): 2.0, (3, 3): 1.0}))) == pytest.approx(1)


# ---------------------------------------------------------------------------
# 3. the oracle against the chain
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_of(name, mutant=None):
    c = fx.CHAIN_CASES[name]
    return fx.chain(c["row"], c["post"], c["tfut"], mutant=mutant, **c["kw"])


@functools.lru_cache(maxsize=None)
def oracle_counts(name):
    c = fx.CHAIN_CASES[name]
    return oracle.future_counts(c["row"], c["post"], tfut=c["tfut"], nrep=c["N"], seed=c["seed"], rep0=c["rep0"],
                                **c["kw"])


@pytest.mark.parametrize("name", sorted(fx.CHAIN_CASES))
def test_oracle_against_the_chain(name):
    c = fx.CHAIN_CASES[name]
    assert c["N"] == 400000 and (c["row"] == -1).any()
    fx.check(oracle_counts(name), c["N"], chain_of(name)[0], label=f"oracle {name}")


@pytest.mark.parametrize("name", sorted(fx.CHAIN_CASES))
def test_oracle_against_the_chain_without_missing_patches(name):
    c = fx.CHAIN_CASES[name]
    row = np.where(c["row"] == -1, 1, c["row"]).astype(np.int32)
    N = 400000
    pext, _, _ = fx.chain(row, c["post"], c["tfut"], **c["kw"])
    counts = oracle.future_counts(row, c["post"], tfut=c["tfut"], nrep=N, seed=c["seed"] + 100, rep0=c["rep0"],
                                  **c["kw"])
    assert fx.informative(N, pext).sum() >= c["tfut"] / 2
    fx.check(counts, N, pext, label=f"oracle {name}, no missing patch")


def test_the_cases_cover_what_the_issue_lists():
    C = fx.CHAIN_CASES
    assert sorted(c["row"].size for c in C.values()) == [1, 2, 8, 9, 10]
    assert {c["kw"]["KS"] == 0 for c in C.values()} == {True, False}          # absorbing and not
    s = C["n9"]["post"].shape[0]
    assert C["n9"]["post"][[0, s - 1], :].sum() > 0 and C["n9"]["post"][:, [0, s - 1]].sum() > 0   # border mass
    assert max(e / C["n9"]["kw"]["KD"] for e, _, _ in fx.cells(C["n9"]["post"])) > 1               # e/K_D > 1
    # n10: c s1 > 1 for some survivor sets (and not for all of them)
    c = C["n10"]
    n = c["row"].size
    M = fx.matrix(n, c["kw"]["m"], c["kw"]["d"], c["kw"]["dS"])
    bits = (np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1
    s1 = bits @ (M[:n] * c["kw"]["KD"]) + M[n] * c["kw"]["KS"]
    cmax = max(cc for _, cc, _ in fx.cells(c["post"]))
    binds = ((cmax * s1 > 1) & (bits == 0)).any(axis=1)
    print("n10: the clamp binds for", int(binds.sum()), "of", 1 << n, "survivor sets")
    assert 50 < binds.sum() < (1 << n) - 50
    assert any("SUM_YEARS=3" in c["options"] for c in C.values())
    assert any(c["rep0"] < fx.TWO32 < c["rep0"] + c["N"] for c in C.values())


# ---------------------------------------------------------------------------
# 4. sensitivity: every mutant of the chain is rejected by a GPU case at its N
# ---------------------------------------------------------------------------
REJECTED_BY = {"pre": "n10", "src0": "n8", "noclamp": "n9", "sameword": "n8", "noborder": "n9"}


@pytest.mark.parametrize("mutant", fx.MUTANTS)
def test_each_mutant_is_rejected_by_a_gpu_case(mutant):
    """The oracle's counts of the named case (bit for bit the lane kernel's,
    test_gpu_future.py) pass the true chain and fail the mutated one under
    check()'s rule."""
    name = REJECTED_BY[mutant]
    c = fx.CHAIN_CASES[name]
    counts = oracle_counts(name)
    assert fx.rejects(counts, c["N"], chain_of(name)[0]) is None
    p = fx.rejects(counts, c["N"], chain_of(name, mutant)[0])
    print(f"mutant {mutant}: case {name}, N {c['N']}, smallest p-value {p}")
    assert p is not None
    with pytest.raises(AssertionError):
        fx.check(counts, c["N"], chain_of(name, mutant)[0], label=f"{name} against mutant {mutant}")


def test_mutant_table():
    """For the log: which case rejects which mutant."""
    for name in sorted(fx.CHAIN_CASES):
        c = fx.CHAIN_CASES[name]
        for mutant in fx.MUTANTS:
            if mutant == "sameword" and c["row"].size > 8:
                continue
            p = fx.rejects(oracle_counts(name), c["N"], chain_of(name, mutant)[0])
            print(f"{name:4s} {mutant:9s} {'passes' if p is None else f'rejected, smallest p-value {p:.3g}'}")
            assert p is not None or REJECTED_BY[mutant] != name


# ---------------------------------------------------------------------------
# 5. non-vacuity of the GPU cases, from the references alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fx.CHAIN_CASES))
def test_chain_cases_are_informative(name):
    """At least half of the years have N p (1-p) >= 100 for the all-empty
    count, and five cells of the last year's histogram (all of them where
    n + 1 < 5)."""
    c = fx.CHAIN_CASES[name]
    pext, hist, _ = chain_of(name)
    assert fx.informative(c["N"], pext).sum() >= c["tfut"] / 2
    assert fx.informative(c["N"], hist[-1]).sum() >= min(5, c["row"].size + 1)


@pytest.mark.parametrize("n", fx.LANE_SIZES + fx.WIDE_SIZES)
def test_year1_cases_are_informative(n):
    c = fx.year1_case(n)
    assert (c["row"] == -1).sum() == min(12, n // 5) and (c["row"] == 1).any() and (c["row"] == 0).any()
    p = fx.year1(c["row"], c["post"], **c["kw"])
    assert fx.informative(c["N"], p).all(), (p.min(), p.max())


@pytest.mark.parametrize("n", fx.LANE_SIZES + fx.WIDE_SIZES)
def test_isolated_cases_are_informative(n):
    c = fx.isolated_case(n)
    assert c["kw"]["KS"] > 0 and c["tfut"] == 6
    src = fx.matrix(n, c["kw"]["m"], c["kw"]["d"], c["kw"]["dS"])[n]
    assert src.max() > 0.85 and src.min() < 0.15          # the source row spans (e^-2, 1) over the patches
    _, _, occ = fx.isolated(c["row"], c["post"], c["tfut"], **c["kw"])
    assert fx.informative(c["N"], occ).all(), (occ.min(), occ.max())


def test_absorbing_isolated_case_is_informative():
    """K_S = 0 at n = 129: every patch informative in every year, and whole
    replicates extinct from the first year on, more of them every year."""
    c = fx.isolated_case(129, absorbing=True)
    assert c["kw"]["KS"] == 0 and not (c["row"] == 0).any()
    pext, _, occ = fx.isolated(c["row"], c["post"], c["tfut"], **c["kw"])
    assert fx.informative(c["N"], occ).all()
    assert fx.informative(c["N"], pext).all() and np.all(np.diff(pext) >= 0) and pext[-1] > pext[0] + 0.05
