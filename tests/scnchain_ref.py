"""numpy restatement of the scenario chain's replicate model and evaluation,
the checker of k_scnchain<NM> and k_chain_eval (tests/test_gpu_scnchain.py)
-- TEST INFRASTRUCTURE ONLY.

Written from the model's text in include/midaspom.h, not from the kernels:
the start state by selection sampling from the addressed Philox stream, the
year of tests/scnsim_ref.py (`year_draws` with the class as the year word,
`one_year`), the literal tally, and the evaluation as explicit ascending
sums with each product rounded before its add.  Vectorised over replicates
and classes only.

tests/test_scnchain_host.py holds this restatement to the reference-pinned
oracle through exact one-year matrices.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import scnsim_ref as sim
from test_future_wide_host import philox_pairs

CHUNK = 1 << 16  # replicates per pass (memory)


def start_states(n, k, seed, reps):
    """bool[R, n]: exactly k patches by selection sampling; u_j = word j & 3 of
    counter (rep, 0xfffffffe, 16 k + (j >> 2))."""
    nq = (n + 3) // 4
    ctr = np.broadcast_to(np.uint64(16 * k) + np.arange(nq, dtype=np.uint64), (reps.size, nq))
    w = philox_pairs(seed, reps[:, None], 0xfffffffe, ctr)  # [4, R, nq]
    occ = np.zeros((reps.size, n), dtype=bool)
    need = np.full(reps.size, k, dtype=np.uint64)
    for j in range(n):
        u = w[j & 3, :, j >> 2]
        take = ((u * np.uint64(n - j)) >> np.uint64(32)) < need
        occ[:, j] = take
        need = need - take.astype(np.uint64)
    return occ


def _rates(kind, baseline, e, c, K):
    """(E, mode) of one_year: mode 0 baseline, 1 die-off year, 2 loss year."""
    e, c, K = np.float64(e), np.float64(c), np.float64(K)
    if baseline:
        return (1.0 if e > 1 else e), 0
    Es = e / K if kind == 0 else e
    return (1.0 if Es > 1 else Es), 1 + kind


def counts(n, kind, e, c, K=None, dsrc=None, nrep=300, seed=0, rep0=0, baseline=False, m=400.0, d=200.0):
    """uint64 transition counts of replicates [rep0, rep0 + nrep) per class:
    (ne, nc, nK, nd, n+1, n+1) for the scenario table (nd = 1 for die-off),
    (ne, nc, n+1, n+1) for the baseline table."""
    e, c = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (e, c))
    K = np.ones(1) if baseline else np.atleast_1d(np.asarray(K, dtype=np.float64))
    dsrc = np.atleast_1d(np.asarray(dsrc, dtype=np.float64)) if kind == 1 and not baseline else np.zeros(1)
    M = sim.dispersal(n, m, d)
    cnt = np.zeros((e.size, c.size, K.size, dsrc.size, n + 1, n + 1), dtype=np.uint64)
    for r0 in range(0, nrep, CHUNK):
        reps = np.arange(rep0 + r0, rep0 + min(nrep, r0 + CHUNK), dtype=np.int64)
        for k in range(n + 1):
            occ0 = start_states(n, k, seed, reps)
            ext, col = sim.year_draws(n, seed, reps, k)
            for ie, ic, iK, idd in np.ndindex(e.size, c.size, K.size, dsrc.size):
                E, mode = _rates(kind, baseline, e[ie], c[ic], K[iK])
                src = sim.source_row(n, m, dsrc[idd]) if mode == 2 else None
                occ = sim.one_year(occ0, ext, col, M, E, c[ic], mode, K[iK], src)
                cnt[ie, ic, iK, idd, k] += np.bincount(occ.sum(axis=1), minlength=n + 1).astype(np.uint64)
    return cnt[:, :, 0, 0] if baseline else cnt


@functools.lru_cache(maxsize=None)
def counts_cached(n, kind, e, c, K, dsrc, nrep, seed, rep0=0, baseline=False, m=400.0, d=200.0):
    """counts() on hashable arguments, computed once per session and shared
    read-only between the tests."""
    out = counts(n, kind, e, c, K, dsrc, nrep, seed, rep0, baseline, m, d)
    out.setflags(write=False)
    return out


def default_target(row, p):
    """target[n1 + j] = (C(nmiss, j) p^j) (1 - p)^(nmiss - j), p = (double)(float)p."""
    row = np.asarray(row)
    n1, nmiss = int((row == 1).sum()), int((row == -1).sum())
    p = float(np.float32(p))
    t = np.zeros(row.size + 1)
    for j in range(nmiss + 1):
        t[n1 + j] = (float(math.comb(nmiss, j)) * math.pow(p, float(j))) * math.pow(1.0 - p, float(nmiss - j))
    return t


def matvec(mat, v):
    """v'[..., k] = sum_l mat[..., k, l] v[..., l], l ascending from 0.0, each
    product rounded before its add."""
    s = np.zeros(mat.shape[:-1])
    for l in range(mat.shape[-1]):
        s = s + mat[..., :, l] * v[..., l, None]
    return s


def evaluate(a, b, ts, tdis, start, target):
    """(out, by_class) of matrices a[ne, nc, ..., n+1, n+1] (scenario) and
    b[ne, nc, n+1, n+1] (baseline): doubles, whatever they came from."""
    ncl = a.shape[-1]
    grid = a.shape[:-2]
    v = np.broadcast_to(np.asarray(target, dtype=np.float64), b.shape[:-1]).copy()
    for _ in range(tdis):
        v = matvec(b, v)
    v = np.broadcast_to(v.reshape(v.shape[:2] + (1,) * (len(grid) - 2) + (ncl,)), grid + (ncl,)).copy()
    for _ in range(ts):
        v = matvec(a, v)
    out = np.zeros(grid)
    for k in range(ncl):
        out = out + np.float64(start[k]) * v[..., k]
    return out, v


def evaluate_counts(cnt_scn, nrep, cnt_base, nbase, ts, tdis, start=None, target=None):
    """The evaluation of count tables: a = (double)cnt / (double)nrep."""
    ncl = cnt_scn.shape[-1]
    a = cnt_scn.astype(np.float64) / np.float64(nrep)
    b = cnt_base.astype(np.float64) / np.float64(nbase)
    if start is None:
        start = np.full(ncl, 1.0 / float(ncl))
    return evaluate(a, b, ts, tdis, start, target)


def states_start(n):
    """start[k] = C(n, k): every one of the 2^n start states once."""
    return np.array([float(math.comb(n, k)) for k in range(n + 1)])
