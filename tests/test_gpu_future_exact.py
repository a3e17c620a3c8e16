"""The future engine's sixteen kernels against exact probabilities
(fut_exact.py): the counts, histograms and patch occupancies of 4 x 10^5
replicates are binomial variates of probabilities that come from a Markov
chain (n <= 10, every year), a closed form of the first year (any n, the real
dispersal coupling) and decoupled patches (any n, every year) -- no random
stream in the reference, and so no error that a replay of the simulation loop
could share with the kernels.  One check() per test: exact two-sided binomial
p-values, Bonferroni over the test's cells at alpha = 1e-5.  The cases and
their non-vacuity are pinned on the CPU (test_future_exact.py).

The lane kernels k_future<NM> / k_future_tab<NM> run under MDP_FUT_WIDE=auto
up to 64 patches, the patch-parallel k_future_wide<NP> / k_future_wide_tab<NP>
under MDP_FUT_WIDE=1 (n <= 64) and auto (beyond); simulate() runs the former
of each pair, summary() the latter.
"""
from __future__ import annotations

import time

import numpy as np
import pytest

import fut_exact as fx
import midaspom_amd as mdp
from test_future_summary_host import identities

pytestmark = pytest.mark.gpu

AUTO = "MDP_FUT_WIDE=auto"
WIDE = "MDP_FUT_WIDE=1"


def tab_kernel(kernel):
    """The summary kernel that an engine running `kernel` launches."""
    return kernel.replace("k_future<", "k_future_tab<").replace("k_future_wide<", "k_future_wide_tab<")


def run(c, options, tfut, kernel, tab):
    """(counts, hist, occ) of case c on an engine that must run `kernel`
    (simulate) and `tab` (summary)."""
    t0 = time.perf_counter()
    with mdp.Future(c["row"], c["post"], options=options, **c["kw"]) as f:
        assert f.kernel == kernel
        assert tab_kernel(f.kernel) == tab
        counts = f.simulate(c["N"], tfut, seed=c["seed"], rep0=c["rep0"])
        hist, occ = f.summary(c["N"], tfut, seed=c["seed"], rep0=c["rep0"])
    print(f"{kernel} and {tab}: n {c['row'].size}, N {c['N']}, {tfut} years, {time.perf_counter() - t0:.2f} s")
    identities(hist, occ, c["N"])
    assert np.array_equal(counts, hist[:, 0])
    return counts, hist, occ


# ---------------------------------------------------------------------------
# 1. the chain: every year, n <= 10, both paths
# ---------------------------------------------------------------------------
CHAIN_KERNELS = {"n1": "k_future<8>", "n2": "k_future<8>", "n8": "k_future<8>", "n9": "k_future<16>",
                 "n10": "k_future<16>"}
CHAIN_TABS = {"n1": "k_future_tab<8>", "n2": "k_future_tab<8>", "n8": "k_future_tab<8>", "n9": "k_future_tab<16>",
              "n10": "k_future_tab<16>"}


@pytest.mark.parametrize("name", sorted(fx.CHAIN_CASES))
def test_chain_every_year(name):
    """hist (its column 0 is simulate()'s counts) and occ of both paths
    against the 2^n-state chain.  n1 runs replicates across 2^32, n8 in
    windows of three years (a replicate rests in its record between them)."""
    c = fx.CHAIN_CASES[name]
    pext, phist, pocc = fx.chain(c["row"], c["post"], c["tfut"], **c["kw"])
    assert np.abs(phist[:, 0] - pext).max() < 1e-12
    _, hist, occ = run(c, AUTO + c["options"], c["tfut"], CHAIN_KERNELS[name], CHAIN_TABS[name])
    _, whist, wocc = run(c, WIDE + c["options"], c["tfut"], "k_future_wide<1>", "k_future_wide_tab<1>")
    assert np.array_equal(hist, whist) and np.array_equal(occ, wocc)
    fx.check(np.concatenate([hist.ravel(), occ.ravel()]), c["N"], np.concatenate([phist.ravel(), pocc.ravel()]),
             label=f"chain {name}, {CHAIN_KERNELS[name]} = k_future_wide<1>")


# ---------------------------------------------------------------------------
# 2. the first year at every size: the colonisation sums of every patch
# ---------------------------------------------------------------------------
KERNELS = {17: "k_future<32>", 32: "k_future<32>", 33: "k_future<64>", 64: "k_future<64>",
           65: "k_future_wide<1>", 128: "k_future_wide<1>", 129: "k_future_wide<2>", 256: "k_future_wide<2>",
           257: "k_future_wide<4>", 512: "k_future_wide<4>", 513: "k_future_wide<8>", 1024: "k_future_wide<8>"}
TABS = {17: "k_future_tab<32>", 32: "k_future_tab<32>", 33: "k_future_tab<64>", 64: "k_future_tab<64>",
        65: "k_future_wide_tab<1>", 128: "k_future_wide_tab<1>", 129: "k_future_wide_tab<2>",
        256: "k_future_wide_tab<2>", 257: "k_future_wide_tab<4>", 512: "k_future_wide_tab<4>",
        513: "k_future_wide_tab<8>", 1024: "k_future_wide_tab<8>"}


@pytest.mark.parametrize("n", fx.LANE_SIZES + fx.WIDE_SIZES)
def test_first_year_occupancy(n):
    """occ[0] over all n patches against sigma_k + (1 - sigma_k) c sbar_k; hist[0]
    through its mean and its sum (identities, exact)."""
    c = fx.year1_case(n)
    p = fx.year1(c["row"], c["post"], **c["kw"])
    assert fx.informative(c["N"], p).all()
    _, hist, occ = run(c, AUTO, 1, KERNELS[n], TABS[n])
    fx.check(occ[0], c["N"], p, label=f"year1 n {n}, {TABS[n]}")


# ---------------------------------------------------------------------------
# 3. decoupled patches at every size: six years of every patch's two draws,
#    the live mask, the histogram and the all-extinct count
# ---------------------------------------------------------------------------
def isolated_test(c, n, label):
    pext, phist, pocc = fx.isolated(c["row"], c["post"], c["tfut"], **c["kw"])
    assert fx.informative(c["N"], pocc).all()
    assert np.abs(phist[:, 0] - pext).max() < 1e-15
    counts, hist, occ = run(c, AUTO, c["tfut"], KERNELS[n], TABS[n])
    fx.check(np.concatenate([hist.ravel(), occ.ravel()]), c["N"], np.concatenate([phist.ravel(), pocc.ravel()]),
             label=f"{label} n {n}, {KERNELS[n]} and {TABS[n]}")
    return counts, pext


@pytest.mark.parametrize("n", fx.LANE_SIZES + fx.WIDE_SIZES)
def test_isolated_patches(n):
    c = fx.isolated_case(n)
    assert c["kw"]["KS"] > 0 and c["tfut"] == 6
    isolated_test(c, n, "isolated")


def test_isolated_patches_without_a_source():
    """K_S = 0 at n = 129: a patch, once empty, stays empty, and the wide
    kernels fill an extinct replicate's later years by their shortcut; a
    quarter of the replicates are extinct after the first year."""
    c = fx.isolated_case(129, absorbing=True)
    assert c["kw"]["KS"] == 0
    counts, pext = isolated_test(c, 129, "isolated, K_S = 0,")
    assert fx.informative(c["N"], pext).all() and 0 < counts[0] < counts[-1] < c["N"]
