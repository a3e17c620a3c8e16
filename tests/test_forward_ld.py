"""The long-double reference of the forward likelihood (tests/fwd_ld.py) on
the CPU: against exact rational arithmetic, its inputs against the host's
(which tests/test_host.py pins to the oracle bit for bit), the CPU oracle
against it on every case of tests/test_gpu_forward_ld.py, the bound's
monotonicity, and the Z rows' small-column series: the bound's term for it is
0 on every earlier case, the expression restated in host doubles keeps within
that term on the series cases, and z-flat's likelihood leaves bound() when
term 3, 4, 5 or 6 of the series is taken out (6.9 times the tolerance for
term 6, the weakest).

Measured on x86-64 (80-bit long double): the reference agrees with the exact
rational value to 2^-62.5 relative at worst (asserted: 2^-60); the oracle's
largest error over the cases is 0.151 of the tolerance (bound() + 1.5 ulp of
log L; case a1 and z-drop0, 0.012 on the 1 024-state year; 0.063-0.141 on the
other series cases), with every case's bound() between 2.9e-15 and 7.3e-13.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle
import fwd_ld

pytestmark = pytest.mark.skipif(not fwd_ld.OK, reason=fwd_ld.SKIP_REASON)

SMALL = [
    np.array([[1, 0, -1, 1], [0, 1, 1, -1], [1, -1, 0, 1]]),
    np.array([[0, 1, 0], [-1, 1, 0], [1, 0, 0]]),          # an always-zero patch
    np.array([[-1, -1], [1, -1]]),
    np.array([[1, 1, 0, 1], [1, 0, 0, 1], [1, 0, 1, -1]]),
]


def _exact(inp, e, c):
    """L(e, c) as a Fraction, from SURVEY.md Appendix A's per-point steps 1-6
    on the double inputs: Pe and Pc entry by entry, P = Pe Pc, v <- v P."""
    x = Fraction(min(e, 1.0))
    y = 1 - x
    nj = 1 << inp.nvar
    pcnt = lambda s: bin(s).count("1")
    p = [[Fraction(min(1.0, c * float(inp.S[j, k]))) for k in range(inp.n)] for j in range(nj)]

    def pc(j, B):
        if j & ~B:
            return Fraction(0)
        f = Fraction(1)
        for k in range(inp.n):
            if k in inp.var_cols:
                bit = 1 << (inp.nvar - 1 - inp.var_cols.index(k))
                if j & bit:
                    continue
                f *= p[j][k] if B & bit else 1 - p[j][k]
            else:
                f *= 1 - p[j][k]
        return f

    v = {a: Fraction(1) for a in inp.years[0]}
    for t in range(1, len(inp.years)):
        nv = {}
        for B in inp.years[t]:
            acc = Fraction(0)
            for A, va in v.items():
                P = sum((x ** (pcnt(A) - pcnt(j)) * y ** pcnt(j) * pc(j, B) for j in range(nj) if not j & ~A), Fraction(0))
                acc += va * P
            nv[B] = acc
        v = nv
    return Fraction(inp.prior0) * sum(v.values())


@pytest.mark.parametrize("i", range(len(SMALL)))
def test_reference_against_exact_arithmetic(i):
    inp = fwd_ld.inputs(SMALL[i], 400.0, 0.3, 100.0)
    c1, _, _ = fwd_ld.clamp_c(inp)
    pts = [(0.0, 0.3), (1e-300, 0.3), (1e-17, 0.7), (0.2, 0.0), (float(np.nextafter(0.5, 0.0)), c1), (0.5, 1e-300),
           (float(np.nextafter(0.5, 1.0)), float(np.nextafter(c1, 0.0))), (0.9, float(np.nextafter(c1, np.inf))),
           (1.0 - 2.0 ** -53, 0.3), (1.0 - 2.0 ** -52, 2.5), (1.0, 0.4), (1.3, 0.9), (0.37, 50.0)]
    worst = 0.0
    for e, c in pts:
        exact, got = _exact(inp, e, c), fwd_ld.lik(inp, e, c)
        if exact == 0:
            assert got == 0, (e, c)
            continue
        # the long double as an exact rational: its mantissa in two double halves
        mant, ex = np.frexp(got)
        hi = float(mant)
        gf = (Fraction(hi) + Fraction(float(mant - np.longdouble(hi)))) * Fraction(2) ** int(ex)
        rel = abs(gf - exact) / exact
        assert rel <= Fraction(1, 2 ** 60), (e, c, float(rel))
        worst = max(worst, float(rel))
    print(f"problem {i}: worst relative error {worst:.3e} = 2^{np.log2(worst) if worst else -np.inf:.1f}")


@pytest.mark.parametrize("name", ["a1", "a2", "b6", "c128", "d193", "e1"])
def test_inputs_match_the_host(name):
    """M, each year's states and the prior formed here equal the host's."""
    cs = fwd_ld.cases()[name]
    inp = cs.inp
    pm = mdp.Model.from_obs(cs.obs, m=cs.m, p=cs.p, d=cs.d)
    assert (pm.n, pm.nvar) == (inp.n, inp.nvar) and tuple(int(v) for v in pm.var_cols) == inp.var_cols
    assert np.array_equal(pm.M, inp.M)
    ss = pm.short_state
    assert [tuple(int(ss[a]) for a in ids) for ids in pm.year_ids] == list(inp.years)
    assert float(pm.prior[0]) == inp.prior0


@pytest.mark.parametrize("name", sorted(fwd_ld.cases()) if fwd_ld.OK else [])
def test_oracle_against_long_double(name):
    """oracle.OracleModel.loglik_grid held to bound() + 1.5 ulp of log L (the
    host libm's log) on every case of the GPU file.  By measurement: the
    oracle's dense dgemm sums all 2^nvar hidden states a year, which bound()
    does not count."""
    cs = fwd_ld.cases()[name]
    ref = cs.ref()
    got = oracle.OracleModel.from_obs(cs.obs, cs.m, cs.p, cs.d).loglik_grid(cs.e, cs.c, threads=16)
    bnd = cs.bound
    frac = fwd_ld.check(got, ref, bnd, f"oracle on {name}", k_log=fwd_ld.K_LOG_LIB)
    print(f"{name}: oracle {frac:.3f} of the tolerance, bound {cs.bound:.3e}, {fwd_ld.normal_fraction(ref):.2f} normal")


ZCASES = ["z-steep", "z-flat", "z-flat-wide", "z-drop", "z-drop0"]


def test_earlier_cases_keep_their_bounds():
    """The Z-series term is exactly 0 for every case from before it (no
    reachable row has a small column, or a dropped one with S > 0), so their
    bound() is the earlier count to the bit; the series cases have it."""
    for name, cs in fwd_ld.cases().items():
        inp, term = cs.inp, fwd_ld.zseries_term(cs.inp, cs.c)
        if name in ZCASES:
            assert cs.zedge is not None and term > 0, name
            continue
        assert cs.zedge is None and term == 0.0, (name, term)
        # roundings() as it stood, restated
        n, nv = inp.n, inp.nvar
        pc = [bin(s).count("1") for s in range(1 << nv)]
        item = 2 * n + 4 + (n - nv) * fwd_ld.kappa(inp, cs.c) / 2
        total, ops = 0.0, 0
        for t in range(1, len(inp.years)):
            src, dst = inp.years[t - 1], inp.years[t]
            W = 0
            for a in src:
                W |= a
            K = sum(pc[a] + 1 for a in src)
            H = max(1 << pc[b & W] for b in dst)
            hs = 3 * nv + 17 + H if nv <= 10 else 0
            total += item + max(7 + 2 * max(0, nv - 3) + max(6 * nv + 18 + len(src), 3 * nv + 18 + K),
                                2 ** max(0, nv - 4) + 6 * nv + 22 + len(src), hs)
            ops += 2 * len(src) * len(dst) * (nv + 1)
        total += len(inp.years[-1]) + 18
        assert cs.bound == (total * (1 + 1 / 2048) + np.ceil(ops / 2 ** 19)) * fwd_ld.U, name


# ---------------------------------------------------------------------------
# the Z rows' series: the expression in doubles, whole and with a term taken out
# ---------------------------------------------------------------------------
def _fma(a, b, c):
    """fl(a b + c): one rounding, as the device's fma."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _z_emulated(inp, cmax, without=None):
    """z_split and zseries restated in doubles (the expression alone: nothing
    of the engine's): c -> Z[hidden state] over the reachable rows (1 for the
    others, which meet exact zeros only), `without` = the term k of the series
    left out (its coefficient P_k / k set to 0).  Also returns, per c, the
    series factor and the long-double product it stands for."""
    rows, cols, x, small, large = fwd_ld.z_classes(inp, cmax)
    coef = np.zeros((len(rows), 8))
    for r, j in enumerate(rows):
        pw = [0.0] * 8
        for q, k in enumerate(cols):   # ascending columns, t = S^(i+1) by repeated products
            if small[r, q]:
                t = sv = float(inp.S[j, k])
                for i in range(8):
                    pw[i] += t
                    t *= sv
        coef[r] = [pw[i] / (i + 1) for i in range(8)]
    if without is not None:
        coef[:, without - 1] = 0.0
    parts = {}

    def z(c):
        out = np.ones(1 << inp.nvar)
        ser, ref = np.ones(len(rows)), np.ones(len(rows), dtype=fwd_ld.LD)
        for r, j in enumerate(rows):
            q = coef[r, 7]
            for i in range(6, -1, -1):
                q = _fma(q, c, coef[r, i])
            ser[r] = np.exp(-(q * c))
            zz = 1.0
            for qk, k in enumerate(cols):
                p = fwd_ld.LD(c * float(inp.S[j, k]))
                if large[r, qk]:
                    zz *= max(0.0, _fma(-c, float(inp.S[j, k]), 1.0))
                else:
                    ref[r] *= 1 - p
            out[j] = zz * ser[r]
        parts[c] = (ser, ref)
        return out
    return z, parts


@pytest.mark.parametrize("name", ["z-steep", "z-flat", "z-flat-wide"])
def test_series_expression_within_its_term(name):
    """The series as the kernels write it, in host doubles, against the
    long-double product over the small and the dropped columns: within
    zseries_term() u (measured: 9.0e-17, 1.0e-16 and 3.8e-16 relative, the
    terms 6.8e-16, 1.8e-15 and 1.3e-14)."""
    cs = fwd_ld.cases()[name]
    z, parts = _z_emulated(cs.inp, float(cs.c.max()))
    term = fwd_ld.zseries_term(cs.inp, cs.c) * fwd_ld.U
    worst = 0.0
    for c in cs.c:
        z(float(c))
        ser, ref = parts[float(c)]
        worst = max(worst, float(np.abs(ser.astype(fwd_ld.LD) / ref - 1).max()))
    print(f"\n{name}: series against the product {worst:.3e} relative, its term {term:.3e}")
    assert worst <= term


@pytest.mark.parametrize("without", [None, 3, 4, 5, 6])
def test_flat_case_sees_a_missing_term(without):
    """z-flat's likelihood with Z from the emulated series: whole, it passes
    check() under the case's bound; with term 3, 4, 5 or 6 of the series left
    out it does not.  A condition on the case (34 columns at the threshold, 5
    transitions), not a measurement of the engine: terms 7 and 8 move log L
    by less than the tolerance and are held on the host table
    (tests/test_zsplit_host.py)."""
    cs = fwd_ld.cases()["z-flat"]
    ref = cs.ref()
    z, _ = _z_emulated(cs.inp, float(cs.c.max()), without)
    with np.errstate(divide="ignore"):
        got = np.log(fwd_ld.grid(cs.inp, cs.e, cs.c, z)).astype(np.float64)
    if without is None:
        frac = fwd_ld.check(got, ref, cs.bound, "z-flat emulated")
        print(f"\nz-flat with the emulated series: {frac:.3f} of the tolerance")
        return
    with pytest.raises(AssertionError, match="of the tolerance") as ei:
        fwd_ld.check(got, ref, cs.bound, f"z-flat without term {without}")
    print(f"\n{ei.value}")


def test_bound_monotone():
    """bound() does not decrease when patches, years or states are added."""
    base = np.array([[1, 0, 1, 1, 0, 1], [1, 1, 0, 1, 0, 1], [0, 1, 1, 1, 0, 0]])
    b0 = fwd_ld.bound(fwd_ld.inputs(base))
    wider = np.hstack([base, [[1], [0], [1]]])
    zero = np.hstack([base, [[0], [0], [0]]])
    longer = np.vstack([base, [[1, 0, 0, 1, 0, 1]]])
    prev = b0
    for k in range(1, 5):  # more and more unvisited patches in year 1
        more = base.copy()
        more[1, :k] = -1
        b = fwd_ld.bound(fwd_ld.inputs(more))
        assert b >= prev
        prev = b
    for obs in (wider, zero, longer):
        assert fwd_ld.bound(fwd_ld.inputs(obs)) >= b0
    assert fwd_ld.bound(fwd_ld.inputs(zero), [0.3]) >= fwd_ld.bound(fwd_ld.inputs(zero))  # kappa adds
    assert max(cs.bound for cs in fwd_ld.cases().values()) <= 2e-12
