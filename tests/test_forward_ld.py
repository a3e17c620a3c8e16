"""The long-double reference of the forward likelihood (tests/fwd_ld.py) on
the CPU: against exact rational arithmetic, its inputs against the host's
(which tests/test_host.py pins to the oracle bit for bit), the CPU oracle
against it on every case of tests/test_gpu_forward_ld.py, and the bound's
monotonicity.

Measured on x86-64 (80-bit long double): the reference agrees with the exact
rational value to 2^-62.5 relative at worst (asserted: 2^-60); the oracle's
largest error over the cases is 0.151 of the tolerance (bound() + 1.5 ulp of
log L; case a1, 0.012 on the 1 024-state year), with every case's bound()
between 2.9e-15 and 7.3e-13.
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
