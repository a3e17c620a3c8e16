"""Long-double reference of the scenario likelihood, and the a-priori error
bound the scenario tests assert (a helper module: nothing here is collected).

The likelihood (main_MIDASPOM_dieoff.c:304-351, main_MIDASPOM_loss.c:341-386)

    L = 1' PK^ts P^tdis w,        P = Pe Pc,  PK = Pe(E_K) Pc(p_K)

is evaluated straight from the model definition: the dense 2^n x 2^n
colonisation matrix Pc[j][b] = prod_k (j_k ? b_k : (b_k ? p_jk : 1 - p_jk)),
a dense matrix-vector product per year, and the per-patch extinction passes
y[s | m] = E y[s] + (1 - E) y[s | m], ascending patch.  None of the kernels'
factorisations (hi/lo tables, tree contraction) and none of the oracle's code
is used.

Inputs in double, as the engine (mdp_scenario_create_opts,
mdp_scenario_set_grid) and the reference form them -- the dispersal M, the
sums S[j][k] over ascending l, the source terms, p_jk = min(1, (c S) K)
(die-off) or min(1, c (S + src K)) (loss), E = min(1, e / K) or min(1, e), the
float32 prior products.  (The kernels form p and E themselves: a correctly
rounded division, products that cannot fuse, and the loss pressure kept
unfused by loss_pc in spom_scenario.hip, so theirs are the same doubles.)
Everything after them in np.longdouble (64-bit
mantissa on x86): 1 - p and 1 - E are then exact to 2^-64, so the result is
the value of the polynomial in (p, E, w) that the kernels evaluate, and
nothing is amplified where p is close to 1.


The bound
---------
bound(n, ts, tdis) = ((ts + tdis) (2^n + 4 n + 1) + 2^n) 2^-53, relative.

Past the double inputs every operation is a sum or product of non-negative
numbers, so nothing cancels: the relative error of L is at most the largest
number of roundings (each <= u = 2^-53, to first order) on any path from an
input to the output.  Per year, follow the contribution of y[b] through the
colonisation row j (b a superset of j, f = the patches free in j) and the
extinction passes into y'[s] (s a superset of j), patch by patch:

  * a patch free in j gives one factor, p (an input, exact) or 1 - p (one
    rounding), one multiplication that joins it to the product, and in its
    extinction pass the branch E y[s] of y[s | m] = E y[s] + (1 - E) y[s | m]
    (a multiplication and an addition, or nothing when s lacks the patch):
    at most 4 roundings;
  * a patch occupied in j gives no factor and the branch (1 - E) y[s | m]:
    the rounding of 1 - E, a multiplication, an addition: 3 roundings;
  * the sum over the 2^f supersets adds at most 2^f <= 2^n roundings to a
    term, and one more is left for a final combination (k_scn's pair_sum).

That is 2^n + 4 n + 1 per year; the final sum over the 2^n states adds at most
2^n.  Checked against the three kernels (spom_scenario.hip), whose fused
multiply-adds only remove roundings from this count:

  k_scn<NL, NH>  row (jh, jl) with fh, fl free hi / lo patches: the lo product
      A has fl factors and fl - 1 multiplications (it starts from 1.0), the hi
      product B fh and fh - 1; the inner FMA chain over the lo supersets has
      depth 2^fl, the outer one over the hi supersets of one half-wave
      max(1, 2^(fh-1)) (with fh = 0 the factor is 1.0 and the other half adds
      an exact zero), pair_sum 1, the passes 3 per occupied and <= 2 per free
      patch: 2^fl + 2^(fh-1) + 3 n + fl + fh - 1 <= 2^n + 4 n - 1.  Final sum:
      2^NH - 1 over hi, then 2^NL over lo.
  k_scn_big, k_scn_row  the tree contraction passes each free patch's level
      once, either parked (1 - p and a multiplication) or fused (one FMA): 2 f,
      with no separate sum; passes as above: <= 4 n.  Final sum: 2^n - 1
      sequential (big); a strided partial and 256 sequential adds (row), which
      is <= 2^n for n >= 9 and, below, adds exact zeros past the 2^n states.

The two roundings a year that the kernels leave unused cover what first
order drops and this reference's own error (the same path count times 2^-64,
i.e. count / 2048 in units of u) for any n <= 11.

The CPU oracles are a different matter: the dense one multiplies matrix powers
(sums of depth 2^n per dgemm level) and both take Pe from pow(), so their own
worst case is larger -- oracle.scenario_vec: per year 2^f + 2 f - 1 for Pc
(dense row sum) and 2^n + n + 5 for Pe (two pow() of <= 1 ulp each, 1 - E to
a power, two multiplications, a dense sum), <= 2 2^n + 2 n + 4.  They are held
to the same bound() by measurement (tests/test_scenario_ld.py), not by this
derivation.  Where a kernel is compared with scenario_vec (n = 9..12) the sum
of the two bounds is what is asserted, and that sum does hold a priori:
4 n (k_scn_row) + 2 2^n + 2 n + 4 <= 2 (2^n + 4 n + 1) per year for n >= 1.
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
OK = np.finfo(LD).nmant >= 63
SKIP_REASON = f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa here: no better than double as a reference"


def bound(n: int, ts: int, tdis: int) -> float:
    """A-priori relative error of a scenario kernel against lik() (module docstring)."""
    return ((ts + tdis) * (2 ** n + 4 * n + 1) + 2 ** n) * 2.0 ** -53


def _bits(n):
    """bits[s][k] = patch k of state s (patch 0 is the top bit)."""
    s = np.arange(1 << n)
    return np.stack([(s >> (n - 1 - k)) & 1 for k in range(n)], axis=1)


def _inputs(row, m, p, d):
    """n, S[j][k] and the prior vector w, in double (float32 prior products)."""
    row = np.asarray(row, dtype=np.int64)
    n = row.size
    a = 1.0 / m
    M = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            M[i, j] = M[j, i] = math.exp(-a * float(j - i) * d)
    bits = _bits(n).astype(np.float64)
    S = np.zeros((1 << n, n))
    for k in range(n):
        for l in range(n):  # ascending l, one double addition each
            if l != k:
                S[:, k] = S[:, k] + M[l, k] * bits[:, l]
    miss = [j for j in range(n) if row[j] == -1]
    w = np.zeros(1 << n)
    pf = np.float32(p)
    for q in range(1 << len(miss)):
        st, pr = 0, np.float32(1.0)
        for j in range(n):
            if row[j] > -1:
                st |= int(row[j]) << (n - 1 - j)
            else:
                b = (q >> (len(miss) - 1 - miss.index(j))) & 1
                st |= b << (n - 1 - j)
                pr = np.float32(pr * (pf if b else np.float32(np.float32(1.0) - pf)))
        w[st] += float(pr)
    return n, S, w


def _pc(n, p):
    """Dense Pc[j][b] from the double pressures p[j][k], in long double."""
    bits = _bits(n)
    p = p.astype(LD)
    Pc = np.ones((1 << n, 1 << n), dtype=LD)
    for k in range(n):
        jk, bk = bits[:, k][:, None], bits[:, k][None, :]
        pk = p[:, k][:, None]
        Pc *= np.where(jk == 1, bk.astype(LD), np.where(bk == 1, pk, LD(1) - pk))
    return Pc


def _year(n, Pc, Y, E):
    """One year on the columns of Y[state][e]: colonisation, then the
    extinction passes over ascending patch."""
    Y = Pc @ Y
    s = np.arange(1 << n)
    for k in range(n):
        m = 1 << (n - 1 - k)
        hi = s[(s & m) != 0]
        Y[hi] = E * Y[hi ^ m] + (LD(1) - E) * Y[hi]
    return Y


def grid(row, kind, e, c, K, dsrc=None, ts=20, tdis=10, m=400.0, p=0.5, d=200.0):
    """L[ie][ic][iK] (die-off) or L[ie][ic][iK][id] (loss) in long double.
    One dense matrix per c (after the event) and per (c, K[, dsrc]) (before
    it); the e values run as the columns of the state array."""
    loss = kind == "loss"
    e = np.atleast_1d(np.asarray(e, dtype=np.float64))
    c = np.atleast_1d(np.asarray(c, dtype=np.float64))
    K = np.atleast_1d(np.asarray(K, dtype=np.float64))
    dsrc = np.atleast_1d(np.asarray(dsrc, dtype=np.float64)) if loss else np.zeros(1)
    n, S, w = _inputs(row, m, p, d)
    E0 = np.minimum(1.0, e).astype(LD)
    out = np.zeros((e.size, c.size, K.size, dsrc.size), dtype=LD)
    for ic, cv in enumerate(c):
        Pc0 = _pc(n, np.minimum(1.0, float(cv) * S))
        V = np.repeat(w.astype(LD)[:, None], e.size, axis=1)
        for _ in range(tdis):
            V = _year(n, Pc0, V, E0)
        for iK, Kv in enumerate(K):
            for idd, dv in enumerate(dsrc):
                if loss:
                    src = np.array([math.exp(-(1.0 / m) * (k + 1) * float(dv)) for k in range(n)])
                    pk = np.minimum(1.0, float(cv) * (S + src[None, :] * float(Kv)))
                    E = E0
                else:
                    pk = np.minimum(1.0, (float(cv) * S) * float(Kv))
                    E = np.minimum(1.0, e / float(Kv)).astype(LD)
                PcK = _pc(n, pk)
                Y = V.copy()
                for _ in range(ts):
                    Y = _year(n, PcK, Y, E)
                out[:, ic, iK, idd] = Y.sum(axis=0)
    return out if loss else out[..., 0]


def lik(row, kind, K, e, c, ts, tdis, m, p, d, dsrc=0.0):
    """One point: L(e, c, K[, dsrc]) as a long double."""
    g = grid(row, kind, [e], [c], [K], [dsrc] if kind == "loss" else None, ts=ts, tdis=tdis, m=m, p=p, d=d)
    return g.reshape(-1)[0]


def check(got, ref, tol, what=""):
    """got == 0 exactly where ref == 0, |got - ref| <= tol ref elsewhere (no
    absolute floor).  Returns the largest relative error as a fraction of tol."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    zero = ref == 0
    assert np.array_equal(got[zero], np.zeros(int(zero.sum()))), f"{what}: non-zero where the reference is 0"
    if zero.all():
        return 0.0
    rel = np.abs(got[~zero].astype(LD) - ref[~zero]) / ref[~zero]
    frac = float(rel.max() / LD(tol))
    assert frac <= 1.0, f"{what}: max relative error {float(rel.max()):.3e} = {frac:.3f} of the bound {tol:.3e}"
    return frac
