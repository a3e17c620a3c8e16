"""numpy restatement of the scenario simulator's replicate model for rows of
any length, the checker of k_scnsim_wave<NP> (tests/test_gpu_scnsim_wave.py)
-- TEST INFRASTRUCTURE ONLY.

The year is the reference's (main_MIDASPOM_dieoff.c:51-83,
main_MIDASPOM_loss.c:52-105, :365) as tests/scnsim_ref.py restates it --
`dispersal`, `source_row`, `year_draws`, `one_year` and `final_states` are
that file's, unchanged -- and the initial state is the stream definition of
include/midaspom.h past 64 patches:

    patch k is occupied iff bit k & 31 of word (k >> 5) & 3 of
    philox(seed; rg_lo, rg_hi, 0xffffffff, 1 + (k >> 7)) is set.

For k < 64 that is scnsim_ref.initial_states (tests/test_scnsim_wave_host.py
holds the two equal).  Nothing here is written from the kernel: no lanes, no
ballots, no distance image.
"""
from __future__ import annotations

import functools

import numpy as np

from scnsim_ref import CHUNK, dispersal, final_states, year_draws
from test_future_wide_host import philox_pairs


def initial_states(n, seed, reps):
    """bool[R, n]: patch k from bit k & 31 of word (k >> 5) & 3 of counter
    (rep, 0xffffffff, 1 + (k >> 7))."""
    reps = np.asarray(reps, dtype=np.int64)
    blocks = (n + 127) >> 7
    ctr = np.broadcast_to(1 + np.arange(blocks, dtype=np.uint64), (reps.size, blocks))
    w = philox_pairs(seed, reps[:, None], 0xffffffff, ctr)  # [4, R, blocks]
    k = np.arange(n)
    words = w[(k >> 5) & 3, :, k >> 7].T  # [R, n]
    return ((words >> (k & 31).astype(np.uint64)) & np.uint64(1)).astype(bool)


def tables(row, kind, e, c, K, dsrc=None, ts=3, tdis=2, nrep=300, seed=0, rep0=0, m=400.0, d=200.0):
    """(hist, match) of replicates [rep0, rep0 + nrep), as scnsim_ref.tables
    gives them, for a row of any length: uint64 arrays of shape
    (ne, nc, nK, nd, n + 1) and (ne, nc, nK, nd, 2**nmiss)."""
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
