"""Long-double reference of the posterior engine's likelihood, and the
a-priori error bound the forward tests assert (a helper module: nothing here
is collected; modelled on tests/scn_ld.py).

The likelihood (main_MIDASPOM.c:341-392)

    L = prior0 1' P_(T-1) ... P_1 1,     P = Pe Pc   (Q3: ones over year 0's states)

is evaluated straight from the model definition: over all 2^nvar hidden
states, extinction as one pass per variable patch over the hidden-state
vector (V[j \\ b] += x V[j], V[j] = y V[j]), the dense colonisation matrix
Pc[j][B] = [j <= B] prod_{k not in j} (B_k ? p_jk : 1 - p_jk) (a product of
per-patch factors, 1 - p_jk for the always-zero patches) and a dense
vector-matrix product per year.  No Q table, no ratio form, no deferred
exponent, no butterfly radix, nothing from the engine's plan and none of the
oracle's code.

Inputs in double, formed as the reference forms them: the dispersal
M = exp(((-1/m) |i - j|) d), the sums S[j][k] over ascending occupied
variable patches, the pressures p = min(1, c S) (one double product), x =
min(e, 1), the float32 prior product, each year's observation-compatible
states.  Everything after them in np.longdouble (64-bit mantissa on x86):
y = 1 - x and 1 - p are then exact to 2^-64, so the result is the value of the
polynomial in (p, x, prior0) that every forward path evaluates.


The bound
---------
Past the double inputs every operation on every path is a sum or product of
non-negative numbers, a correctly rounded division (z = y / x or x / y) or a
binary-power chain: nothing cancels, so the relative error of L is at most
the largest number of roundings (each <= u = 2^-53, first order) on a path
from an input to L.  An input that is itself rounded by the kernel (y = 1 - x,
z) counts once for each time it multiplies into a term (its multiplicity).
With n patches, nv of them variable, np' states in the source year, np in the
target year, |A_k| occupied patches in source state k, per year:

  item   2 n + 4 + (n - nv) kappa / 2   every Pc[j][B]: per variable patch
         1 - p (one rounding; p itself is the reference's double) and one
         multiplication (the factor tree is no deeper than a chain); per
         always-zero patch fma(-c, S, 1) and one multiplication, the four Z
         chains joined as (za zb)(zc zd), Z times the tree.  The fma rounds
         1 - c S once, where the reference rounds p = c S first: against the
         reference's 1 - p the kernel's factor is off by p u / 2 absolute,
         p / (1 - p) u / 2 relative, on top of its own rounding.  kappa = the
         largest p / (1 - p) over the grid's c, the hidden states and the
         always-zero patches with p < 1 (0 without such patches): computed
         from the inputs, and the reason the cases keep c S away from 1 on
         always-zero patches (the clamp itself on such a patch is
         tests/test_gpu_forward_ld.py::test_clamp_on_an_always_zero_patch).
  qsum   7 + 2 max(0, nv - 3)   a Q entry sums <= 2^nv items in the canonical
         order of k_qrows, k_wq and the fused kernel: groups of 8 left to
         right, then the group sums through a binary counter (<= nv - 3
         levels) folded from its lowest level up (<= nv - 3 more).
  then the longest of
  ratio  (mdp_fwd_jit fused / reading / LDS-state / chunked, k_qrows'
         coefficients)  Horner 2 nv (nX FMAs, each counted as a product and a
         sum); y and z, multiplicity <= nv each: 2 nv; g^d from its power
         table and its product: nv; the source pre-scale B^(|A| - min): nv;
         a flush or the final power, power_expr's binary chain for
         E <= 191 + 2 nv < 256: 16 multiplications and its product: 17; the
         sequential sum over the sources with the product v P: np' + 1.
         6 nv + 18 + np'.
  gemm   (k_fwd_mmt, k_fwd_mma, k_fwd_wide)  the x^r and y^r tables nv each,
         y's multiplicity nv, W = v x^r y^m 2; the sum over K = sum_k
         (|A_k| + 1) entries, each k-step of an FP64 MFMA (and each FMA of
         k_fwd_wide's sequential sums) one rounding; at most 16 slice sums.
         3 nv + 18 + K.
  generic (k_coefs, k_forward; its own Q sum instead of qsum: parts of 16
         subsets summed in order, then the parts in order, 16 + 2^(nv-4))
         R[r] = sum_m Q[m] C(.,.) <= 2 (nv + 1); the weight tables and y's
         multiplicity 3 nv + 2; the dot product nv + 1; the sum over the
         sources np' + 1.   2^max(0, nv-4) + 6 nv + 22 + np'.
  hs     (k_fwd_hs)  one butterfly FMA per patch: nv; the y^|j| table, y's
         multiplicity and its product 2 nv + 1; U Pc over the j <= B in W
         (padded K entries add exact zeros): H = max_l 2^|B_l & W| k-steps,
         16 slice sums.   3 nv + 17 + H   (and no qsum; the kernel takes at
         most 10 variable patches, so this enters for nv <= 10 only).
  zser   (every path but the generic one: k_zrows, k_qrows, the fused kernel)
         For the grid's bound cmax (its largest c, or mdp_engine_set_cbound's
         if larger) z_split (csrc/spom_plan.cpp) takes the always-zero columns
         of a row with cmax S <= 2^-55 out of the product ("dropped") and
         replaces those with 2^-55 < cmax S <= 2^-7 ("small", ns of them) by
         exp(-A~), A = sum_i=1..8 c^i P_i / i, P_i = sum_small S^i.  Against
         the reference's prod (1 - fl(c S)), in units of u:
           A (ns + 16)   the argument: a coefficient P_i / i is ns additions,
                         at most 7 multiplications and a division of
                         non-negative terms (ns + 8), Horner's 7 FMAs and the
                         product with c (8); a relative error r of the
                         argument is A r in exp(-A);
           sum_small p / (1 - p) / 2   the reference's own p = fl(c S), against
                         the series of the exact c S (as for the fma, `item`);
           sum_small (c S)^9 / (9 (1 - c S)) / u   the truncated tail of
                         -log(1 - x) = sum x^i / i;
           2 + 1         the device library's exp, 1 ulp = 2 u in double (the
                         HIP programming guide's "HIP math API" table of
                         double-precision functions; the toolchain installs no
                         copy of it), and the product of Z with it;
           nd / 4        nd dropped columns with S > 0, each factor within
                         2^-55 = u / 4 of 1 (S = 0: the factor is exactly 1).
         The largest such sum over the grid's c and the reachable rows (the
         subsets of A & B of a transition), once per year on top of `item`,
         whose count of explicit columns stays at all n: over-counted.  0
         where no row has a small or a dropped column with S > 0 (every case
         from before this term, asserted in tests/test_forward_ld.py).
After the years the final sum, the prior and the final power: np_last + 18.
Fused multiply-adds only remove roundings from these counts.  The reference's
own error is the same count times 2^-64 (count / 2048 in units of u), and
what underflows in double is covered by one more rounding per 2^19
operations (check(), below).  bound() = that total times 2^-53; the tests
require it to be <= 2e-12 for every case.

The CPU oracle sums each year's dense dgemm over all 2^nv hidden states and
takes Pe from pow(): it is held to the same bound() by measurement
(tests/test_forward_ld.py), not by this derivation.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
OK = np.finfo(LD).nmant >= 63
SKIP_REASON = f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa here: no better than double as a reference"

U = 2.0 ** -53
LOG_DBL_MIN = float(np.log(np.finfo(np.float64).tiny))
L_NORMAL = LD(2.0) ** -950   # ref_L from here up: every term below DBL_MIN is below 2^-72 of L
K_LOG_FAST = 3.5             # mdp_log: 2 ulp of the library's (test_engine_log_accuracy) + its 1 + rounding log L
K_LOG_LIB = 1.5              # MDP_FAST_LOG=0: the library's 1 ulp + rounding log L


@dataclass(frozen=True)
class Inputs:
    """The double inputs of one problem (obs, m, p, d), formed here."""
    n: int
    nvar: int
    var_cols: tuple
    M: np.ndarray          # [n][n]
    S: np.ndarray          # [2^nvar][n]
    prior0: float          # float32 product, widened
    years: tuple           # per year: the hidden-state ids of its observation-compatible states
    bits: np.ndarray       # [2^nvar][nvar]: bit b (variable column b) of state j


def _key(obs):
    a = np.ascontiguousarray(obs, dtype=np.int64)
    return a.shape, a.tobytes()


def inputs(obs, m=400.0, p=0.5, d=100.0) -> Inputs:
    return _inputs(*_key(obs), float(m), float(p), float(d))


@functools.lru_cache(maxsize=None)
def _inputs(shape, raw, m, p, d):
    obs = np.frombuffer(raw, dtype=np.int64).reshape(shape)
    T, n = obs.shape
    var = [j for j in range(n) if (obs[:, j] != 0).any()]
    nvar = len(var)
    w = {col: 1 << (nvar - 1 - b) for b, col in enumerate(var)}
    a = 1.0 / m
    M = np.array([[0.0 if i == j else math.exp(-a * abs(j - i) * d) for j in range(n)] for i in range(n)])
    j = np.arange(1 << nvar)
    bits = np.stack([(j >> (nvar - 1 - b)) & 1 for b in range(nvar)], axis=1) if nvar else np.zeros((1, 0), int)
    S = np.zeros((1 << nvar, n))
    for b, col in enumerate(var):  # ascending l, one double addition each (M[k][k] = 0)
        S = S + M[col][None, :] * bits[:, b][:, None].astype(np.float64)
    years = []
    for t in range(T):
        miss = [c for c in range(n) if obs[t, c] == -1]
        base = sum(w[c] for c in range(n) if obs[t, c] == 1)
        ids = []
        for k in range(1 << len(miss)):
            ids.append(base + sum(w[c] for q, c in enumerate(miss) if (k >> (len(miss) - 1 - q)) & 1))
        years.append(tuple(ids))
    pf, pr = np.float32(p), np.float32(1.0)
    for _ in range(sum(1 for c in range(n) if obs[0, c] == -1)):  # state k = 0: every unvisited patch empty
        pr = np.float32(pr * np.float32(np.float32(1.0) - pf))
    S.setflags(write=False)
    return Inputs(n, nvar, tuple(var), M, S, float(pr), tuple(years), bits)


def _pc(inp: Inputs, c: float, cols, z=None):
    """Dense Pc[j][B] for the target states `cols`, every hidden state j, in
    long double from the double pressures.  `z` (tests/test_forward_ld.py's
    mutated series alone): z(c) -> [2^nvar] stands in for the product over the
    always-zero patches."""
    p = np.minimum(1.0, c * inp.S).astype(LD)
    nj = 1 << inp.nvar
    Pc = np.ones((nj, len(cols)), dtype=LD)
    var = set(inp.var_cols)
    if z is not None:
        Pc *= np.asarray(z(c), dtype=LD)[:, None]
    for k in range(inp.n):
        if k not in var and z is None:
            Pc *= (LD(1) - p[:, k])[:, None]
    cols = np.asarray(cols, dtype=np.int64)
    for b, k in enumerate(inp.var_cols):
        jb = inp.bits[:, b][:, None]
        Bb = ((cols >> (inp.nvar - 1 - b)) & 1)[None, :]
        pk = p[:, k][:, None]
        Pc *= np.where(jb == 1, Bb.astype(LD), np.where(Bb == 1, pk, LD(1) - pk))
    return Pc


def grid(inp: Inputs, e, c, z=None) -> np.ndarray:
    """L[ie][ic] in long double (`z`: _pc)."""
    e = np.atleast_1d(np.asarray(e, dtype=np.float64))
    c = np.atleast_1d(np.asarray(c, dtype=np.float64))
    x = np.minimum(e, 1.0).astype(LD)
    y = LD(1) - x
    nj = 1 << inp.nvar
    j = np.arange(nj)
    out = np.zeros((e.size, c.size), dtype=LD)
    for ic, cv in enumerate(c):
        V = np.zeros((nj, e.size), dtype=LD)
        V[list(inp.years[0])] = LD(1)
        for t in range(1, len(inp.years)):
            for b in range(inp.nvar):  # extinction, one pass per variable patch
                m = 1 << (inp.nvar - 1 - b)
                hi = j[(j & m) != 0]
                V[hi ^ m] += x * V[hi]
                V[hi] = y * V[hi]
            cols = list(inp.years[t])
            live = np.flatnonzero((V != 0).any(axis=1))  # (the other rows are exact zeros)
            new = _pc(inp, float(cv), cols, z)[live].T @ V[live] if live.size else np.zeros((len(cols), e.size), LD)
            V = np.zeros((nj, e.size), dtype=LD)
            V[cols] = new
        out[:, ic] = V.sum(axis=0) * LD(inp.prior0)
    return out


def lik(inp: Inputs, e: float, c: float):
    """One point: L(e, c) as a long double."""
    return grid(inp, [e], [c])[0, 0]


@functools.lru_cache(maxsize=None)
def _reference(shape, raw, m, p, d, eraw, craw):
    g = grid(_inputs(shape, raw, m, p, d), np.frombuffer(eraw), np.frombuffer(craw))
    g.setflags(write=False)
    return g


def reference(obs, m, p, d, e, c) -> np.ndarray:
    """grid() computed once per (problem, grid) and shared, read-only."""
    e = np.ascontiguousarray(e, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    return _reference(*_key(obs), float(m), float(p), float(d), e.tobytes(), c.tobytes())


def kappa(inp: Inputs, c) -> float:
    """The largest p / (1 - p) over the grid's c values, the hidden states and
    the always-zero patches with p < 1 (module docstring, `item`)."""
    nonvar = [k for k in range(inp.n) if k not in inp.var_cols]
    if not nonvar:
        return 0.0
    worst = 0.0
    for cv in np.atleast_1d(c):
        p = np.minimum(1.0, float(cv) * inp.S[:, nonvar])
        p = p[p < 1.0]
        if p.size:
            worst = max(worst, float((p / (1.0 - p)).max()))
    return worst


Z_TAU = 2.0 ** -7     # z_split: cmax S above this stays an explicit factor
Z_DROP = 2.0 ** -55   # z_split: cmax S up to this is dropped
Z_TERMS = 8


@functools.lru_cache(maxsize=None)
def _reachable(years, nvar):
    rows = set()
    for t in range(1, len(years)):
        for x in {a & b for a in years[t - 1] for b in years[t]}:
            j = x
            while True:  # every subset of x
                rows.add(j)
                if j == 0:
                    break
                j = (j - 1) & x
    return tuple(sorted(rows))


def reachable_rows(inp: Inputs) -> tuple:
    """The hidden states j with a Pc[j][B] some transition reads: the subsets
    of A & B (the engine's Z rows)."""
    return _reachable(inp.years, inp.nvar)


def nonvar_cols(inp: Inputs) -> list:
    return [k for k in range(inp.n) if k not in inp.var_cols]


def z_classes(inp: Inputs, cmax: float):
    """z_split's classes restated: (rows, cols, x, small, large) with x =
    fl(cmax S)[rows][cols] in double over the reachable rows and the
    always-zero columns; dropped = neither small nor large."""
    rows, cols = list(reachable_rows(inp)), nonvar_cols(inp)
    x = float(cmax) * inp.S[np.ix_(rows, cols)] if rows and cols else np.zeros((len(rows), len(cols)))
    small = (x > Z_DROP) & (x <= Z_TAU)
    large = ~(x <= Z_DROP) & ~small
    return rows, cols, x, small, large


def zseries_term(inp: Inputs, c=(), cbound=0.0) -> float:
    """`zser` of the module docstring, in units of u: the largest over the
    grid's c values and the reachable rows."""
    c = np.atleast_1d(np.asarray(c, dtype=np.float64))
    if not c.size or not nonvar_cols(inp):
        return 0.0
    cmax = max(float(c.max()), float(cbound))
    rows, cols, _, small, large = z_classes(inp, cmax)
    S = inp.S[np.ix_(rows, cols)].astype(LD)
    nd = ((S > 0) & ~small & ~large).sum(axis=1)
    ns = small.sum(axis=1)
    if not ns.any() and not nd.any():
        return 0.0
    worst = 0.0
    for cv in c:
        p = np.where(small, LD(float(cv)) * S, LD(0))   # < 2^-7 (1 + u)
        A = sum((p ** i).sum(axis=1) / i for i in range(1, Z_TERMS + 1))
        own = (p / (1 - p)).sum(axis=1) / 2
        tail = (p ** (Z_TERMS + 1) / ((Z_TERMS + 1) * (1 - p))).sum(axis=1) / LD(U)
        term = A * (ns + 16) + own + tail + np.where(ns > 0, 3, 0) + nd / LD(4)
        worst = max(worst, float(term.max()))
    return worst * (1 + 2.0 ** -40)   # (rounded up: the sums above are long double)


def roundings(inp: Inputs, c=(), cbound=0.0) -> float:
    """The count of the module docstring, in units of u."""
    n, nv = inp.n, inp.nvar
    pc = [bin(s).count("1") for s in range(1 << nv)]
    item = 2 * n + 4 + (n - nv) * kappa(inp, c) / 2 + zseries_term(inp, c, cbound)
    qsum = 7 + 2 * max(0, nv - 3)
    total, ops = 0.0, 0
    for t in range(1, len(inp.years)):
        src, dst = inp.years[t - 1], inp.years[t]
        W = 0
        for a in src:
            W |= a
        K = sum(pc[a] + 1 for a in src)
        H = max(1 << pc[b & W] for b in dst)
        ratio = 6 * nv + 18 + len(src)
        gemm = 3 * nv + 18 + K
        generic = 2 ** max(0, nv - 4) + 6 * nv + 22 + len(src)
        hs = 3 * nv + 17 + H if nv <= 10 else 0
        total += item + max(qsum + max(ratio, gemm), generic, hs)
        ops += 2 * len(src) * len(dst) * (nv + 1)
    total += len(inp.years[-1]) + 18
    return total * (1 + 1 / 2048) + math.ceil(ops / 2 ** 19)


def bound(inp: Inputs, c=(), cbound=0.0) -> float:
    """A-priori relative error of L on any forward path against grid()
    (module docstring); `c` = the grid's c values (they enter through kappa
    and zser), `cbound` = the engine's mdp_engine_set_cbound value if any: the
    Z rows' classes are split at max(the grid's largest c, cbound)."""
    return roundings(inp, c, cbound) * U


def check(got_loglik, ref_L, bnd, what="", k_log=K_LOG_FAST) -> float:
    """Cell by cell: -inf exactly where ref_L == 0 (a structural zero, exact
    on every path); |got - log ref_L| <= bnd + k_log ulp(log ref_L) where
    ref_L >= 2^-950 (any term that underflows in double is then below 2^-72
    of L, one rounding per 2^19 of them: counted in bound()); below that,
    tests/test_gpu_parity.py::assert_loglik_close's rule as it stands: where
    either side is below log DBL_MIN both are below log DBL_MIN + 1e-9 (or
    -inf), and a cell still normal on both sides (DBL_MIN <= L < 2^-950,
    where partial underflow may cost more than the bound) keeps to 1e-9.
    NaN nowhere (the reference has none).  Returns the largest error of the
    cells with ref_L >= 2^-950 as a fraction of their tolerance."""
    got = np.asarray(got_loglik, dtype=np.float64)
    ref = np.asarray(ref_L)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert not np.isnan(got).any(), f"{what}: NaN at {np.argwhere(np.isnan(got))[:4].tolist()}"
    zero = ref == 0
    assert np.isneginf(got[zero]).all(), \
        f"{what}: finite log L at {np.argwhere(zero & ~np.isneginf(got))[:4].tolist()} where the reference is exactly 0"
    low = ~zero & (ref < L_NORMAL)
    if low.any():
        lref = np.log(ref[low]).astype(np.float64)
        sub = (lref < LOG_DBL_MIN) | (got[low] < LOG_DBL_MIN)
        assert (got[low][sub] < LOG_DBL_MIN + 1e-9).all() and (lref[sub] < LOG_DBL_MIN + 1e-9).all(), \
            f"{what}: a normal likelihood faces a subnormal / zero one"
        assert (np.abs(got[low][~sub] - lref[~sub]) <= 1e-9).all(), f"{what}: |dlogL| > 1e-9 below 2^-950"
    nrm = ~zero & ~low
    if not nrm.any():
        return 0.0
    lref = np.log(ref[nrm])
    tol = LD(bnd) + LD(k_log) * np.spacing(np.abs(lref.astype(np.float64))).astype(LD)
    assert np.isfinite(got[nrm]).all(), f"{what}: -inf / inf where the reference is normal"
    err = np.abs(got[nrm].astype(LD) - lref)
    frac = err / tol
    worst = float(frac.max())
    if worst > 1.0:
        q = int(frac.argmax())
        raise AssertionError(f"{what}: |dlogL| = {float(err[q]):.3e} at cell {np.argwhere(nrm)[q].tolist()} is "
                             f"{worst:.3f} of the tolerance {float(tol[q]):.3e} (bound {bnd:.3e})")
    return worst


def normal_fraction(ref_L) -> float:
    """Share of the cells under the ref_L >= 2^-950 rule."""
    ref = np.asarray(ref_L)
    return float((ref >= L_NORMAL).sum()) / ref.size


# ---------------------------------------------------------------------------
# the border grid and the cases (tests/test_forward_ld.py holds the oracle to
# them on the CPU, tests/test_gpu_forward_ld.py every forward path)
# ---------------------------------------------------------------------------
E12 = np.array([0.0, 1e-300, 1e-17, 0.2, np.nextafter(0.5, 0.0), 0.5, np.nextafter(0.5, 1.0), 0.9,
                1.0 - 2.0 ** -52, 1.0 - 2.0 ** -53, 1.0, 1.3])
# 66 points: both ratio forms in one 64-lane wave, and a second wave partly
# filled at 1, 2 and 4 points per lane
E66 = np.sort(np.concatenate([E12, np.linspace(0.03, 0.97, 54)]))


def clamp_c(inp: Inputs, variable=True):
    """(c, j, k): the double nearest 1 / S[j][k] for the largest S[j][k] over
    the reachable hidden states j (A & B of a transition, or that less one patch) and the
    variable (or the always-zero) patches k outside j."""
    best = None
    cols = inp.var_cols if variable else tuple(k for k in range(inp.n) if k not in inp.var_cols)
    for t in range(1, len(inp.years)):
        for a in inp.years[t - 1]:
            for b in inp.years[t]:
                x = a & b
                for j in [x] + [x & ~(1 << q) for q in range(inp.nvar) if (x >> q) & 1]:
                    for k in cols:
                        if k in inp.var_cols and inp.bits[j, inp.var_cols.index(k)]:
                            continue
                        s = float(inp.S[j, k])
                        if s > 0 and (best is None or s > best[0]):
                            best = (s, j, k)
    if best is None:  # a one-year series has no transition: any S
        j, k = np.unravel_index(int(inp.S.argmax()), inp.S.shape)
        best = (float(inp.S[j, k]), int(j), int(k))
    s, j, k = best
    return 1.0 / s, j, k


def border_c(inp: Inputs, reduced=False):
    """0, 1e-300, 0.3, the clamp c of a variable patch with its two
    neighbouring doubles, and one c above every clamp; reduced: 0.3, the
    clamp c, its upper neighbour and the c above every clamp."""
    c1, _, _ = clamp_c(inp)
    pos = inp.S[inp.S > 0]
    top = 1.5 / float(pos.min())
    if reduced:
        return np.array([0.3, c1, np.nextafter(c1, np.inf), top])
    return np.array([0.0, 1e-300, 0.3, np.nextafter(c1, 0.0), c1, np.nextafter(c1, np.inf), top])


@dataclass(frozen=True, eq=False)
class Case:
    name: str
    obs: np.ndarray
    e: np.ndarray
    c: np.ndarray
    m: float = 400.0
    p: float = 0.5
    d: float = 100.0
    # None: no always-zero column is in the Z rows' series; a double: the case
    # is built so that fl(cmax S) of one reachable (row, always-zero column)
    # equals it (2^-7: the last small column; around 2^-55: the last dropped)
    zedge: float | None = None
    zprops: object = None   # (x, small, large) -> None: asserts the case's class mix (z_classes at cmax)

    @property
    def inp(self) -> Inputs:
        return inputs(self.obs, self.m, self.p, self.d)

    @property
    def bound(self) -> float:
        return bound(self.inp, self.c)

    def ref(self) -> np.ndarray:
        """The long-double grid, once per case; at least half of its cells
        under the ref_L >= 2^-950 rule, and bound() within 2e-12."""
        r = reference(self.obs, self.m, self.p, self.d, self.e, self.c)
        assert 2 * (r >= L_NORMAL).sum() >= r.size, f"{self.name}: only {normal_fraction(r):.2f} of the cells are normal"
        assert self.bound <= 2e-12, f"{self.name}: bound {self.bound:.3e}"
        if self.zedge is None:
            # no always-zero patch in the Z rows' exp series (2^-55 < cmax S <= 2^-7)
            assert float(self.c.max()) * math.exp(-(self.inp.n - 1) * self.d / self.m) > 2.0 ** -7
        else:
            _, _, x, small, large = z_classes(self.inp, float(self.c.max()))
            assert (x == self.zedge).any(), f"{self.name}: no reachable column with fl(cmax S) = {self.zedge!r}"
            self.zprops(x, small, large)
        return r


def make_case(name, obs, m=400.0, p=0.5, d=100.0, e=None, reduced=False) -> Case:
    obs = np.ascontiguousarray(obs, dtype=np.int32)
    inp = inputs(obs, m, p, d)
    e = (E12 if reduced else E66) if e is None else np.asarray(e, dtype=np.float64)
    return Case(name, obs, e, border_c(inp, reduced), m, p, d)


def _obs_a1():
    """12 patches, the 8 variable ones in the middle of the row (columns
    2-9), 6 years, up to 4 unvisited patches a year (16 states)."""
    rng = np.random.default_rng(2101)
    obs = np.zeros((6, 12), dtype=np.int32)
    obs[:, 2:10] = rng.random((6, 8)) < 0.6
    for yr, k in {0: 2, 1: 4, 3: 3, 4: 3, 5: 1}.items():
        obs[yr, 2 + rng.choice(8, size=k, replace=False)] = -1
    return obs


def _obs_a2():
    """9 patches, all variable, 5 years, up to 3 unvisited patches a year."""
    rng = np.random.default_rng(2102)
    obs = (rng.random((5, 9)) < 0.55).astype(np.int32)
    obs[0, 0] = obs[1, 8] = 1
    for yr, k in {1: 3, 2: 1, 4: 2}.items():
        obs[yr, rng.choice(9, size=k, replace=False)] = -1
    return obs


def _series(occ, n):
    """One fully observed year per entry of `occ`: the set of empty patches."""
    obs = np.ones((len(occ), n), dtype=np.int32)
    for t, empty in enumerate(occ):
        obs[t, list(empty)] = 0
    return obs


def edge_c(inp: Inputs, value: float, order):
    """(c, j, k): the largest double c with fl(c S[j][k]) == value exactly
    (so the next double above c puts the product above value), for the first
    reachable row j and always-zero column k in the order of the key
    `order(S[j][k])` that has one (a nextafter search around value / S: the
    products of neighbouring c values are S ulp(c) apart, which can step
    over the one double `value`)."""
    rows, cols = reachable_rows(inp), nonvar_cols(inp)
    cand = sorted(((float(inp.S[j, k]), j, k) for j in rows for k in cols if inp.S[j, k] > 0), key=lambda t: order(t[0]))
    for s, j, k in cand:
        c = value / s
        for _ in range(4):
            c = float(np.nextafter(c, np.inf))
        for _ in range(9):
            if c * s == value:
                return c, j, k
            c = float(np.nextafter(c, 0.0))
    raise AssertionError(f"no c with fl(c S) = {value!r}")


def _obs_z(n, var, T, seed, missing, stay=0.8, col=0.15):
    """T years x n patches, always zero outside the columns `var`; there a
    patch stays occupied with probability `stay` and is colonised with `col`
    (few colonisations: L stays far above 2^-950 at the small c of the flat
    cases); `missing` = {year: unvisited variable patches}."""
    rng = np.random.default_rng(seed)
    obs = np.zeros((T, n), dtype=np.int32)
    cur = rng.random(len(var)) < 0.7
    cur[0] = True
    for t in range(T):
        obs[t, var] = cur
        cur = np.where(cur, rng.random(len(var)) < stay, rng.random(len(var)) < col)
    for yr, k in missing.items():
        obs[yr, rng.choice(var, size=k, replace=False)] = -1
    return obs


def z_case(name, obs, m, d, value, order, zprops) -> Case:
    """A case whose largest c puts one reachable (row, always-zero column)
    at fl(cmax S) == value: c = cmax / 4, cmax / 2, the double below cmax and
    cmax, on E12."""
    obs = np.ascontiguousarray(obs, dtype=np.int32)
    cmax, _, _ = edge_c(inputs(obs, m, 0.5, d), value, order)
    c = np.array([cmax / 4, cmax / 2, np.nextafter(cmax, 0.0), cmax])
    return Case(name, obs, E12, c, m, 0.5, d, zedge=value, zprops=zprops)


def _z_steep(x, small, large):
    # all three classes in one row, at most 8 explicit columns a row (kmax 8)
    assert (small.any(axis=1) & large.any(axis=1) & (~small & ~large & (x > 0)).any(axis=1)).any()
    assert large.sum(axis=1).max() <= 8 and small.sum(axis=1).max() >= 30


def _z_all_small(x, small, large):
    # every column of every occupied row small; the full row within 10 % of the threshold
    assert not large.any() and (small == (x > 0)).all()
    full = x[np.argmax(x.sum(axis=1))]
    assert (full > 0.9 * Z_TAU).all() and (full <= Z_TAU).all()


def _z_just_small(x, small, large):
    # every column just above the drop threshold: small, within the rows' spread (<= 6 patches) of it
    assert not large.any() and (small == (x > 0)).all() and small.any() and (x[small] <= 8 * Z_DROP).all()


def _z_all_dropped(x, small, large):
    assert not large.any() and not small.any() and (x > 0).any()


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    from test_gpu_parity import _wide_obs
    out = {}
    out["a1"] = make_case("a1", _obs_a1())
    out["a2"] = make_case("a2", _obs_a2(), m=250.0, p=0.3)
    # (b) the LDS-state kernel: 12 patches x 5 years, 5 and 6 unvisited patches
    for k in (5, 6):
        out[f"b{k}"] = make_case(f"b{k}", _wide_obs(np.random.default_rng(2200 + k), 12, 5, {2: k}), reduced=True)
    # (c) wide years: 10 patches, 4 years, 7-10 unvisited patches in year 1
    for k in (7, 8, 9, 10):
        obs = _wide_obs(np.random.default_rng(2300 + k), 10, 4, {1: min(k, 9)})
        if k == 10:
            obs[1, :] = -1
        out[f"c{1 << k}"] = make_case(f"c{1 << k}", obs, reduced=True)
    # (d) flush boundaries: fully observed series of 6 (7) patches, small
    # enough for the fused kernel, whose pending exponent (the sum of the
    # source years' occupied patches) reaches 191, 192, 193 at year 32, and one
    # that flushes on its last transition
    ed = np.array([1e-17, 0.05, 0.2, 0.45, np.nextafter(0.5, 0.0), 0.5, np.nextafter(0.5, 1.0), 0.6, 0.9,
                   1.0 - 2.0 ** -53])
    out["d191"] = make_case("d191", _series([{2}] + [()] * 34, 6), e=ed)
    out["d192"] = make_case("d192", _series([()] * 35, 6), e=ed)
    out["d193"] = make_case("d193", _series([()] + [{6}] * 34, 7), e=ed)
    out["dlast"] = make_case("dlast", _series([()] * 33, 6), e=ed)
    # (e) one year: L = the state count times the prior
    out["e1"] = make_case("e1", np.array([[1, -1, -1, 1, -1, 0, 1]]), p=0.3, reduced=True)
    # (f) two e blocks: a1 on 600 x 3
    a1 = out["a1"]
    e600 = np.sort(np.concatenate([E12, np.linspace(0.011, 0.989, 588)]))
    out["f600"] = Case("f600", a1.obs, e600, a1.c[[2, 4, 5]], a1.m, a1.p, a1.d)
    # (z) the Z rows' series (module docstring, `zser`): 6 years each, up to
    # 4 unvisited variable patches a year
    miss = {0: 2, 1: 4, 3: 3, 4: 3, 5: 1}
    # steep: 68 patches, the 8 variable ones in columns 20-27, S falls by e a
    # column: up to 8 explicit columns a row (4 on either side), the small
    # ones, and from 38 columns away (e^-38 cmax < 2^-55: a row of 48 patches
    # would have none) dropped ones, in one row; cmax near 0.73, kappa < 1
    steep = _obs_z(68, list(range(20, 28)), 6, 2401, miss, stay=0.75, col=0.3)
    out["z-steep"] = z_case("z-steep", steep, 100.0, 100.0, Z_TAU, lambda s: abs(Z_TAU / s - 0.73), _z_steep)
    # flat: 6 variable patches at one end, S within 10 % along the row; cmax =
    # 2^-7 / max S: every column small and near the threshold (A = 0.26 at 34
    # columns, 0.85 at 114)
    flat = _obs_z(40, list(range(6)), 6, 2402, miss)
    out["z-flat"] = z_case("z-flat", flat, 4000.0, 10.0, Z_TAU, lambda s: -s, _z_all_small)
    wide = _obs_z(120, list(range(6)), 6, 2403, miss)
    out["z-flat-wide"] = z_case("z-flat-wide", wide, 12000.0, 10.0, Z_TAU, lambda s: -s, _z_all_small)
    # drop: the flat shape with the smallest S one double above 2^-55 (all
    # small, A of the order of ns 2^-55), and with the largest at 2^-55 (all dropped)
    out["z-drop"] = z_case("z-drop", flat, 4000.0, 10.0, float(np.nextafter(Z_DROP, 1.0)), lambda s: s, _z_just_small)
    out["z-drop0"] = z_case("z-drop0", flat, 4000.0, 10.0, Z_DROP, lambda s: -s, _z_all_dropped)
    return out
