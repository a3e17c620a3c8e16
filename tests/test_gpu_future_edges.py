"""The forward-simulation engine (k_future<NM>) at its launch and range
edges, per-year counts against the CPU oracle EXACTLY (integer work): the
second trip of the grid-stride loop, replicate indices at and past 2^32 (the
Philox counter's second word, the look-back across the boundary), the horizon
limit tfut = 12288 (64 KB of LDS at n <= 8), 16 and 18 missing patches in the
last row, and the refusals."""
from __future__ import annotations

import functools
import tempfile
from pathlib import Path

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"

M, D = 400.0, 100.0
ROW8 = np.array([1, 0, 0, 0, 0, -1, 0, 0], dtype=np.int32)  # sparse: extinct replicates in every year
ROW9 = np.append(ROW8, 0).astype(np.int32)
TWO32 = 1 << 32


@functools.lru_cache(maxsize=None)
def posterior(scale=1.0):
    """The 21-step posterior of the example input (trapezoid mass ~ 20^2, so
    at scale 0.5 about half the draws fall past it and look back)."""
    with tempfile.TemporaryDirectory() as tmp:
        oracle.run(GOLDEN / "occupancies.txt", Path(tmp) / "post.txt", m=M, d=D, s=21)
        post = oracle.read_posterior(Path(tmp) / "post.txt")
    assert post.shape == (21, 21) and np.isfinite(post).all() and (post >= 0).all()
    return post * scale


def engine_counts(row, post, nrep, tfut, seed=0, rep0=0, **kw):
    with mdp.Future(row, post, m=M, d=D, **kw) as f:
        return f.simulate(nrep, tfut, seed=seed, rep0=rep0)


def oracle_counts(row, post, nrep, tfut, seed=0, rep0=0, **kw):
    return oracle.future_counts(row, post, tfut=tfut, nrep=nrep, seed=seed, rep0=rep0, m=M, d=D, **kw)


# ---- a. grid-stride: 4096 x 256 lanes, then 777 more replicates -----------
NREP_STRIDE = 4096 * 256 + 777


@functools.lru_cache(maxsize=None)
def stride_reference(n):
    ref = oracle_counts(ROW8 if n == 8 else ROW9, posterior(), NREP_STRIDE, 12, seed=31)
    assert (ref > 0).all() and (ref < NREP_STRIDE).all(), ref  # equality below is not vacuous
    return ref


@pytest.mark.parametrize("n", [8, 9])
def test_grid_stride_second_trip(n):
    """The second trip holds 12 full waves and one of 9 lanes, whose ballot
    leader is elected among the lanes left: k_future<8> (table in LDS) and
    k_future<16>."""
    assert NREP_STRIDE - 4096 * 256 == 12 * 64 + 9
    got = engine_counts(ROW8 if n == 8 else ROW9, posterior(), NREP_STRIDE, 12, seed=31)
    assert np.array_equal(got, stride_reference(n))


# ---- b. replicate indices across 2^32 --------------------------------------
SEED_HI = (1 << 35) + 8


def looks_back(seed, rep, post):
    """Does replicate `rep`'s posterior draw fall past the posterior mass?"""
    s = post.shape[0]
    w = np.ones(s)
    w[0] = w[-1] = 0.5
    mass = float((np.outer(w, w) * post).sum())
    r = oracle.philox(seed, [rep & 0xffffffff, rep >> 32, 0xffffffff, 0])[0] >> 1
    return (s - 1) ** 2 * r / 2147483647.0 > mass * (1 + 1e-9)


@functools.lru_cache(maxsize=None)
def boundary_reference(scale):
    ref = oracle_counts(ROW8, posterior(scale), 4000, 12, seed=SEED_HI, rep0=TWO32 - 2000)
    assert (ref > 0).all() and (ref < 4000).all(), ref
    return ref


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_replicates_across_2_to_32(scale):
    """rep0 = 2^32 - 2000, 4000 replicates, a seed past 2^35: the whole run
    equals the oracle and the sum of the two runs split at 2^32.  At half the
    posterior mass about half the draws look back, replicate 2^32 among them
    (to 2^32 - 1: a borrow into the counter's second word)."""
    post = posterior(scale)
    if scale == 0.5:
        assert looks_back(SEED_HI, TWO32, post) and not looks_back(SEED_HI, TWO32 - 1, post)
    ref = boundary_reference(scale)
    with mdp.Future(ROW8, post, m=M, d=D) as f:
        whole = f.simulate(4000, 12, seed=SEED_HI, rep0=TWO32 - 2000)
        below = f.simulate(2000, 12, seed=SEED_HI, rep0=TWO32 - 2000)
        above = f.simulate(2000, 12, seed=SEED_HI, rep0=TWO32)
    assert np.array_equal(whole, ref)
    assert np.array_equal(below + above, ref)
    assert above.sum() > 0 and below.sum() > 0


# ---- c. the horizon limit ---------------------------------------------------
@pytest.mark.parametrize("n", [8, 9])
def test_longest_horizon(n):
    """tfut = 12288: with the n <= 8 survivor table exactly 64 KB of dynamic LDS."""
    row = ROW8 if n == 8 else ROW9
    got = engine_counts(row, posterior(), 2000, 12288, seed=5)
    ref = oracle_counts(row, posterior(), 2000, 12288, seed=5)
    assert np.array_equal(got, ref)
    assert 0 < ref[0] < 2000


@pytest.mark.parametrize("tfut", [12289, 0])
def test_horizon_outside_the_range_is_refused(tfut):
    with mdp.Future(ROW8, posterior(), m=M, d=D) as f:
        with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
            f.simulate(100, tfut)


# ---- d. more than 12 missing patches ---------------------------------------
@pytest.mark.parametrize("n,nmiss", [(17, 16), (21, 18)])
def test_many_missing_patches(n, nmiss):
    """The initial state is drawn among 2^16 and 2^18 completions."""
    row = np.full(n, -1, dtype=np.int32)
    row[np.linspace(1, n - 2, n - nmiss).astype(int)] = [1, 0, 1][: n - nmiss]
    assert (row == -1).sum() == nmiss
    got = engine_counts(row, posterior(), 20000, 25, seed=n, KD=0.4)
    ref = oracle_counts(row, posterior(), 20000, 25, seed=n, KD=0.4)
    assert np.array_equal(got, ref)
    assert ref[-1] > 0 and ref[0] < 20000


def test_31_missing_patches_are_refused():
    row = np.full(32, -1, dtype=np.int32)
    row[7] = 1
    with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
        mdp.Future(row, posterior(), m=M, d=D)


# ---- e. refusals ------------------------------------------------------------
def test_65_patches_are_refused():
    with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
        mdp.Future(np.ones(65, dtype=np.int32), posterior(), m=M, d=D)


@pytest.mark.parametrize("cell", [(0, 0), (7, 11), (20, 20)])
def test_negative_posterior_cell_is_refused(cell):
    post = posterior().copy()
    post[cell] = -1e-3
    with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
        mdp.Future(ROW8, post, m=M, d=D)


@pytest.mark.parametrize("kw", [{"KD": -0.5}, {"KS": -1.0}, {"KD": float("nan")}, {"KS": float("nan")}])
def test_negative_or_nan_capacity_is_refused(kw):
    with pytest.raises(mdp.MidaspomError, match="EINVAL"):
        mdp.Future(ROW8, posterior(), m=M, d=D, **kw)
