"""numpy restatement of the scenario simulator's replicate model, the checker
of k_scnsim<NM> (tests/test_gpu_scnsim.py) -- TEST INFRASTRUCTURE ONLY.

Written from the reference's year (main_MIDASPOM_dieoff.c:51-83,
main_MIDASPOM_loss.c:52-105, :365) and the stream definition of
include/midaspom.h, not from the kernel: the literal n x n matrix M, an
explicit ascending loop over the surviving patches for the colonisation sums
(one add per survivor; a numpy reduction would sum pairwise), u = r / RAND_MAX
compared as the reference compares rand() / RAND_MAX.  Vectorised over
replicates only.  The Philox words come from `philox_pairs` of
test_future_wide_host.py, which that file pins to the oracle's generator.

tests/test_scnsim_host.py holds this restatement to the reference-pinned
oracle (oracle.dieoff_lik / oracle.loss_lik) by a 5-sigma test per cell.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from midaspom_amd.scenario import _states
from test_future_wide_host import philox_pairs

RAND_MAX = 2147483647.0
CHUNK = 1 << 16  # replicates per pass (memory)


def dispersal(n, m, d):
    """M[l][k] = exp(-(1/m)|l-k|d), 0 on the diagonal (dieoff.c:238-248)."""
    a = 1.0 / m
    M = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            M[i, j] = M[j, i] = math.exp(-a * float(j - i) * d)
    return M


def source_row(n, m, dsrc):
    """M[n][k] = exp(-(1/m)(k+1)dsrc) (loss.c:365)."""
    return np.array([math.exp(-(1.0 / m) * (k + 1) * dsrc) for k in range(n)])


def initial_states(n, seed, reps):
    """bool[R, n]: patch k from bit k & 31 of word k >> 5 of counter (rep, 0xffffffff, 1)."""
    one = np.broadcast_to(np.array([1], dtype=np.uint64), (reps.size, 1))
    w = philox_pairs(seed, reps[:, None], 0xffffffff, one)[:, :, 0]  # [4, R]
    k = np.arange(n)
    return ((w[k >> 5, :].T >> (k & 31).astype(np.uint64)) & np.uint64(1)).astype(bool)


def year_draws(n, seed, reps, t):
    """(u_ext, u_col)[R, n] of year t: pair k >> 1, words 2(k&1) and 2(k&1)+1."""
    pairs = np.broadcast_to(np.arange((n + 1) // 2, dtype=np.uint64), (reps.size, (n + 1) // 2))
    w = philox_pairs(seed, reps[:, None], t, pairs)  # [4, R, P]
    k = np.arange(n)
    ext = (w[2 * (k & 1), :, k >> 1].T >> np.uint64(1)).astype(np.float64) / RAND_MAX
    col = (w[2 * (k & 1) + 1, :, k >> 1].T >> np.uint64(1)).astype(np.float64) / RAND_MAX
    return ext, col


def one_year(occ, ext, col, M, E, c, mode, K, src):
    """simpij of dieoff.c / loss.c: extinction, then colonisation of the
    patches empty after it.  mode 0 baseline, 1 die-off year, 2 loss year."""
    surv = occ & (ext > E)
    s1 = np.zeros(occ.shape)
    for l in range(occ.shape[1]):  # ascending l, one add per survivor
        s1 += np.where(surv[:, l, None], M[l][None, :], 0.0)
    if mode == 1:
        pc = (c * s1) * K  # dieoff.c:78
    elif mode == 2:
        pc = c * (s1 + (src * K)[None, :])  # loss.c:95-98: the product rounded before the add
    else:
        pc = c * s1
    pc = np.where(pc > 1, 1.0, pc)
    return surv | (~surv & (col < pc))


def final_states(n, kind, e, c, K, dsrc, ts, tdis, M, m, occ0, draws):
    """bool[R, n] after ts scenario years and tdis baseline years of one grid point."""
    e, c, K = np.float64(e), np.float64(c), np.float64(K)
    with np.errstate(divide="ignore", invalid="ignore"):
        Es = e / K if kind == 0 else e  # dieoff.c:56-57, loss.c:57
    Es = 1.0 if Es > 1 else Es
    Eb = 1.0 if e > 1 else e
    src = source_row(n, m, dsrc) if kind == 1 else None
    occ = occ0
    for t in range(ts + tdis):
        ext, col = draws[t]
        if t < ts:
            occ = one_year(occ, ext, col, M, Es, c, 1 + kind, K, src)
        else:
            occ = one_year(occ, ext, col, M, Eb, c, 0, K, src)
    return occ


def tables(row, kind, e, c, K, dsrc=None, ts=3, tdis=2, nrep=300, seed=0, rep0=0, m=400.0, d=200.0):
    """(hist, match) of replicates [rep0, rep0 + nrep): uint64 arrays of shape
    (ne, nc, nK, nd, n + 1) and (ne, nc, nK, nd, 2**nmiss), nd = 1 for the
    die-off kind (0); kind 1 is habitat loss."""
    row = np.asarray(row, dtype=np.int64)
    n = row.size
    e, c, K = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (e, c, K))
    dsrc = np.atleast_1d(np.asarray(dsrc, dtype=np.float64)) if kind == 1 else np.zeros(1)
    missing = np.flatnonzero(row == -1)
    nmiss = missing.size
    known = np.flatnonzero(row != -1)
    M = dispersal(n, m, d)
    hist = np.zeros((e.size, c.size, K.size, dsrc.size, n + 1), dtype=np.uint64)
    match = np.zeros((e.size, c.size, K.size, dsrc.size, 1 << nmiss), dtype=np.uint64)
    for r0 in range(0, nrep, CHUNK):
        reps = np.arange(rep0 + r0, rep0 + min(nrep, r0 + CHUNK), dtype=np.int64)
        occ0 = initial_states(n, seed, reps)
        draws = [year_draws(n, seed, reps, t) for t in range(ts + tdis)]
        for ie, ic, iK, idd in np.ndindex(e.size, c.size, K.size, dsrc.size):
            occ = final_states(n, kind, e[ie], c[ic], K[iK], dsrc[idd], ts, tdis, M, m, occ0, draws)
            hist[ie, ic, iK, idd] += np.bincount(occ.sum(axis=1), minlength=n + 1).astype(np.uint64)
            ok = (occ[:, known] == (row[known] == 1)).all(axis=1)
            j = np.zeros(reps.size, dtype=np.int64)
            for q, col in enumerate(missing):  # the first missing patch is the most significant bit
                j |= occ[:, col].astype(np.int64) << (nmiss - 1 - q)
            match[ie, ic, iK, idd] += np.bincount(j[ok], minlength=1 << nmiss).astype(np.uint64)
    return hist, match


@functools.lru_cache(maxsize=None)
def tables_cached(row, kind, e, c, K, dsrc, ts, tdis, nrep, seed, rep0=0, m=400.0, d=200.0):
    """tables() on hashable arguments (tuples), computed once per session and
    shared read-only between the tests."""
    h, mt = tables(row, kind, e, c, K, dsrc if kind == 1 else None, ts, tdis, nrep, seed, rep0, m, d)
    h.setflags(write=False)
    mt.setflags(write=False)
    return h, mt


def priors(nmiss, p):
    """float32 priors of the 2**nmiss completions (dieoff.c:230): the products
    of scenario._states, without its state numbers (which need n < 63)."""
    p = np.float32(p)
    pr = np.ones(1 << nmiss, dtype=np.float32)
    for q in range(nmiss):
        for k in range(1 << nmiss):
            b = (k >> (nmiss - 1 - q)) & 1
            pr[k] = np.float32(pr[k] * np.float32(np.float32(b) * p + np.float32(1 - b) * np.float32(1 - p)))
    return pr


def lik(row, p, match, nrep):
    """(sum_j (double)prior_j * (double)match[..., j], j ascending) * 2^n / nrep."""
    row = np.asarray(row, dtype=np.int64)
    pr = priors(int((row == -1).sum()), p)
    out = np.zeros(match.shape[:-1])
    for j in range(match.shape[-1]):
        out = out + np.float64(pr[j]) * match[..., j].astype(np.float64)
    return out * float(2 ** row.size) / float(nrep)


def completion(row, j):
    """The complete row that completion j of `row` stands for."""
    row = np.array(row, dtype=np.int32)
    missing = np.flatnonzero(row == -1)
    for q, col in enumerate(missing):
        row[col] = (j >> (missing.size - 1 - q)) & 1
    return row


def synthetic_row(n, nmiss, seed=1):
    """A row of n patches with `nmiss` missing ones, the rest 0 / 1."""
    rng = np.random.default_rng(seed * 1000 + n * 17 + nmiss)
    row = rng.integers(0, 2, size=n).astype(np.int32)
    row[rng.choice(n, size=nmiss, replace=False)] = -1
    return row
