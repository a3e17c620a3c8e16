"""Both CPU oracles of the scenario likelihood (the reference's dense
matrix-power form, oracle.dieoff_lik / loss_lik, and the vector-propagation
form, oracle.scenario_vec) against the long-double evaluation of the model
(tests/scn_ld.py), so that the GPU parity tests stand on something measured:
exactly 0 where the long-double value is 0, within scn_ld.bound(n, ts, tdis)
relative everywhere else.

The bound is derived for the kernels' summation orders; the oracles' own
worst case is larger (scn_ld's docstring), so for them it is a measured
statement.  Measured on x86-64 (80-bit long double), worst case over every
case below: the dense oracle 0.161 of the bound, the vector oracle 0.119.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import scn_ld

pytestmark = pytest.mark.skipif(not scn_ld.OK, reason=scn_ld.SKIP_REASON)

ROW = np.array([1, -1, 0, 1, 0, -1, 1, 1], dtype=np.int32)  # n = its first n entries
M, P, D = 400.0, 0.5, 100.0

# (e, c, K, dsrc): e = 0, e = 1, e > 1, e / K > 1, c = 0, c S K > 1 (S reaches
# 0.78 next to one occupied neighbour at d / m = 0.25), K on both sides of 1
POINTS = [
    (0.0, 0.3, 0.5, 300.0),
    (0.2, 0.0, 2.0, 900.0),
    (0.35, 0.9, 2.5, 250.0),
    (0.6, 0.4, 0.8, 1500.0),
    (0.9, 0.5, 0.8, 400.0),
    (1.0, 0.3, 1.7, 600.0),
    (1.3, 0.6, 3.0, 200.0),
    (0.05, 1.5, 1.0, 2000.0),
    (0.5, 0.25, 4.0, 350.0),
    (0.15, 0.7, 0.3, 800.0),
]


@pytest.mark.parametrize("tt", [(3, 2), (20, 10), (0, 4), (5, 0)], ids=lambda t: f"ts{t[0]}_tdis{t[1]}")
@pytest.mark.parametrize("kind", ["dieoff", "loss"])
@pytest.mark.parametrize("n", range(1, 9))
def test_oracles_against_long_double(n, kind, tt):
    ts, tdis = tt
    row = ROW[:n]
    pts = POINTS
    tol = scn_ld.bound(n, ts, tdis)
    ref = np.array([scn_ld.lik(row, kind, K, e, c, ts, tdis, M, P, D, ds) for e, c, K, ds in pts])
    assert 2 * int((ref > 0).sum()) >= ref.size, f"only {int((ref > 0).sum())} of {ref.size} points are non-zero"
    dense, vec = np.empty(len(pts)), np.empty(len(pts))
    for i, (e, c, K, ds) in enumerate(pts):
        if kind == "dieoff":
            dense[i] = oracle.dieoff_lik(row, np.array([K]), e, c, ts=ts, tdis=tdis, m=M, p=P, d=D)[0]
        else:
            dense[i] = oracle.loss_lik(row, np.array([K]), np.array([ds]), e, c, ts=ts, tdis=tdis, m=M, p=P, d=D)[0, 0]
        vec[i] = oracle.scenario_vec(row, kind, K, e, c, ts=ts, tdis=tdis, m=M, p=P, d=D, dsrc=ds)
    fd = scn_ld.check(dense, ref, tol, "dense oracle")
    fv = scn_ld.check(vec, ref, tol, "vector oracle")
    print(f"n={n} {kind} ts={ts} tdis={tdis}: dense {fd:.3f} vector {fv:.3f} of the bound, "
          f"{int((ref > 0).sum())}/{ref.size} non-zero")


@pytest.mark.parametrize("kind", ["dieoff", "loss"])
@pytest.mark.parametrize("n", [9, 10])
def test_vector_oracle_past_8_patches(n, kind):
    """The vector oracle is the GPU tests' reference for n = 9..12: where the
    dense long-double matrix still fits, it keeps to the same bound."""
    row = np.array([1, -1, 0, 1, 0, -1, 1, 1, 0, 1], dtype=np.int32)[:n]
    pts = [POINTS[i] for i in (0, 2, 3, 9)]
    ref = np.array([scn_ld.lik(row, kind, K, e, c, 3, 2, M, P, D, ds) for e, c, K, ds in pts])
    assert (ref > 0).sum() >= 3
    vec = np.array([oracle.scenario_vec(row, kind, K, e, c, ts=3, tdis=2, m=M, p=P, d=D, dsrc=ds)
                    for e, c, K, ds in pts])
    print(f"n={n} {kind}: vector {scn_ld.check(vec, ref, scn_ld.bound(n, 3, 2), 'vector oracle'):.3f} of the bound")


def test_bound_formula():
    assert scn_ld.bound(8, 3, 2) == (5 * (256 + 33) + 256) * 2.0 ** -53
    assert scn_ld.bound(1, 0, 0) == 2 * 2.0 ** -53
