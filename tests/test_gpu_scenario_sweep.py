"""Every dispatch and launch boundary of the scenario engine against the
long-double evaluation of the model (tests/scn_ld.py): all eight k_scn<NL, NH>
instantiations, k_scn_row and k_scn_big at every n <= 8 and k_scn_row at
n = 9..12, each over a whole (e, c, K[, d]) grid -- every e lane of both
32-value chunks -- and the multi-launch paths of k_scn_big and k_scn_row
(p0 > 0, a short last launch, the scratch reused across launches).  One
engine over three grids pins the grid buffers it keeps between set_grid calls.

What is asserted: exactly 0 where the reference is 0, and a relative error of
at most scn_ld.bound(n, ts, tdis) everywhere else, however small L is -- the
bound is derived in scn_ld's docstring from the roundings on a path, not from
what the kernels deliver.

Measured on an MI355X, the largest error of test_every_dispatch over n = 1..8
and both kinds as a fraction of that bound: k_scn 0.134, k_scn_row 0.134,
k_scn_big 0.134 (all three at n = 1, loss; the fraction falls with n, to
0.012, 0.013 and 0.013 at n = 8).  k_scn_row at n = 9..12 against the vector
oracle: at most 0.020 of the two bounds.
"""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle
import scn_ld

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not scn_ld.OK, reason=scn_ld.SKIP_REASON)]

# the first n entries are the row for n patches: a missing patch from n = 2 on,
# observed-occupied and observed-empty patches around it
ROW = np.array([1, -1, 0, 1, 0, -1, 1, 1, 0, 1, -1, 0], dtype=np.int32)
M, P, D = 400.0, 0.5, 100.0
TS, TDIS = 3, 2
KERNELS = {"lds": {"MDP_SCN_BIG": 0, "MDP_SCN_ROW": 0}, "row": {"MDP_SCN_ROW": 1}, "big": {"MDP_SCN_BIG": 1}}

# 33 e values: a full 32-lane chunk and one live lane in the second.  e = 0,
# e = 1, e > 1, and e / K > 1 from 0.9 on at K = 0.8 and at 2.6 for every K;
# c = 0 and a c whose pressure c S K passes 1 next to occupied neighbours
# (S reaches 0.78 per neighbour at d / m = 0.25); K on both sides of 1
E33 = np.concatenate([[0.0], np.linspace(0.02, 0.7, 28), [0.9, 1.0, 1.3, 2.6]])
C2 = np.array([0.0, 0.9])
K3 = np.array([0.8, 1.0, 2.5])
D2 = np.array([250.0, 1500.0])


def run(row, kind, opts, e, c, K, d, ts=TS, tdis=TDIS):
    with mdp.Scenario(row, kind, m=M, p=P, d=D, options=opts) as sc:
        return sc.lik(e, c, K, d if kind == "loss" else None, ts=ts, tdis=tdis)


def reference(row, kind, e, c, K, d, ts=TS, tdis=TDIS):
    ref = scn_ld.grid(row, kind, e, c, K, d if kind == "loss" else None, ts=ts, tdis=tdis, m=M, p=P, d=D)
    assert 2 * int((ref > 0).sum()) >= ref.size, f"only {int((ref > 0).sum())} of {ref.size} points are non-zero"
    return ref


@functools.lru_cache(maxsize=None)
def sweep_reference(n, kind):
    """One long-double grid per (n, kind), shared by the three kernels."""
    return reference(ROW[:n], kind, E33, C2, K3, D2)


@pytest.mark.parametrize("kernel", ["lds", "row", "big"])
@pytest.mark.parametrize("kind", ["dieoff", "loss"])
@pytest.mark.parametrize("n", range(1, 9))
def test_every_dispatch(n, kind, kernel):
    """n = 1..8 on the LDS kernel (k_scn<1,0> .. k_scn<3,5>), k_scn_row and
    k_scn_big: the whole 33 x 2 x 3 (x 2) grid, every lane."""
    ref = sweep_reference(n, kind)
    got = run(ROW[:n], kind, KERNELS[kernel], E33, C2, K3, D2)
    frac = scn_ld.check(got, ref, scn_ld.bound(n, TS, TDIS), f"{kernel} n={n} {kind}")
    print(f"sweep {kernel} n={n} {kind}: {frac:.4f} of the bound")


E5 = np.array([0.0, 0.2, 0.55, 1.0, 1.3])
K2 = np.array([0.8, 2.5])


@functools.lru_cache(maxsize=None)
def vec_reference(n, kind):
    """oracle.scenario_vec over the 5 x 2 x 2 (x 2) grid (the dense
    long-double matrix is out of reach at these n)."""
    row = ROW[:n]
    nd = 2 if kind == "loss" else 1
    pts = [(ie, ic, iK, idd) for ie in range(5) for ic in range(2) for iK in range(2) for idd in range(nd)]

    def one(pt):
        ie, ic, iK, idd = pt
        return oracle.scenario_vec(row, kind, K2[iK], E5[ie], C2[ic], ts=TS, tdis=TDIS, m=M, p=P, d=D,
                                   dsrc=float(D2[idd]))
    with ThreadPoolExecutor(max_workers=8) as ex:  # the C oracle releases the GIL
        ref = np.array(list(ex.map(one, pts))).reshape(5, 2, 2, nd)
    assert 2 * int((ref > 0).sum()) >= ref.size
    return ref if kind == "loss" else ref[..., 0]


@pytest.mark.parametrize("kind", ["dieoff", "loss"])
@pytest.mark.parametrize("n", [9, 10, 11, 12])
def test_row_kernel_default_range(n, kind):
    """n = 9..12, k_scn_row by default, against the vector oracle: the
    kernel's bound plus the oracle's own (scn_ld's docstring: the sum holds
    a priori for this pair)."""
    ref = vec_reference(n, kind)
    got = run(ROW[:n], kind, {}, E5, C2, K2, D2)
    frac = scn_ld.check(got, ref, 2 * scn_ld.bound(n, TS, TDIS), f"row n={n} {kind}")
    print(f"sweep row n={n} {kind}: {frac:.4f} of the two bounds")


# ---------------------------------------------------------------------------
# launch boundaries: MDP_SCN_LAUNCH_PTS=256 on 600-point grids whose first
# pass (v per (c, e), 300 points) crosses a boundary too
# ---------------------------------------------------------------------------
def boundary_grid(kind):
    if kind == "dieoff":  # 30 x 10 x 2
        return np.linspace(0.0, 1.16, 30), np.linspace(0.0, 1.35, 10), np.array([0.8, 2.5]), None
    # 25 x 12 x 1 x 2
    return np.linspace(0.0, 1.2, 25), np.linspace(0.0, 1.32, 12), np.array([1.7]), D2


@functools.lru_cache(maxsize=None)
def boundary_reference(n, kind):
    e, c, K, d = boundary_grid(kind)
    assert e.size * c.size * K.size * (2 if kind == "loss" else 1) == 600 and e.size * c.size == 300
    return reference(ROW[:n], kind, e, c, K, d)


@pytest.mark.parametrize("kernel", ["row", "big"])
@pytest.mark.parametrize("kind", ["dieoff", "loss"])
@pytest.mark.parametrize("n", [3, 6])
def test_launch_boundaries(n, kind, kernel):
    """600 points in launches of 256, 256 and 88 (k_scn_big: the last with
    dead lanes): bit-identical to the uncapped run -- a point's arithmetic
    does not depend on its launch -- and the whole grid within the bound."""
    e, c, K, d = boundary_grid(kind)
    ref = boundary_reference(n, kind)
    whole = run(ROW[:n], kind, KERNELS[kernel], e, c, K, d)
    capped = run(ROW[:n], kind, {**KERNELS[kernel], "MDP_SCN_LAUNCH_PTS": 256}, e, c, K, d)
    assert np.array_equal(capped, whole)
    scn_ld.check(capped, ref, scn_ld.bound(n, TS, TDIS), f"{kernel} n={n} {kind} capped")


@pytest.mark.parametrize("kind", ["dieoff", "loss"])
def test_one_point_launches(kind):
    """k_scn_row with one point per launch on a 7-point grid (both passes)."""
    n = 6
    e, c, K, d = np.linspace(0.0, 0.9, 7), np.array([0.6]), np.array([1.7]), np.array([400.0])
    ref = reference(ROW[:n], kind, e, c, K, d)
    whole = run(ROW[:n], kind, KERNELS["row"], e, c, K, d)
    capped = run(ROW[:n], kind, {**KERNELS["row"], "MDP_SCN_LAUNCH_PTS": 1}, e, c, K, d)
    assert np.array_equal(capped, whole)
    scn_ld.check(capped, ref, scn_ld.bound(n, TS, TDIS), f"row n={n} {kind} one point per launch")


REUSE = {"lds": (4, KERNELS["lds"]), "row": (3, KERNELS["row"]),
         "big": (3, {**KERNELS["big"], "MDP_SCN_LAUNCH_PTS": 256})}


@pytest.mark.parametrize("kernel", ["lds", "row", "big"])
@pytest.mark.parametrize("kind", ["dieoff", "loss"])
def test_grid_buffers_reused(kind, kernel):
    """One engine over three grids: the device buffers of a grid are kept and
    grown, so the smaller second grid leaves the first one's values in their
    tails (the axes, the source rows, v and k_scn_big's state scratch).  Every
    result is bit-identical to a fresh engine's."""
    n, opts = REUSE[kernel]
    A = (E33, C2, K3, D2, 3, 2)
    B = (E33[::8], C2[1:], K3[:2], D2[:1], 1, 4)  # 5 x 1 x 2 (x 1)
    assert B[0].size == 5
    with mdp.Scenario(ROW[:n], kind, m=M, p=P, d=D, options=opts) as sc:
        for e, c, K, d, ts, tdis in (A, B, A):
            got = sc.lik(e, c, K, d if kind == "loss" else None, ts=ts, tdis=tdis)
            fresh = run(ROW[:n], kind, opts, e, c, K, d, ts=ts, tdis=tdis)
            assert 2 * int((fresh > 0).sum()) >= fresh.size
            assert np.array_equal(got, fresh)


def real_size_grid():
    e = np.linspace(1.05, 0.03, 64)  # descending: the launch boundary falls among the small e
    c = np.array([0.0, 0.2, 0.45, 0.9, 1.4])
    return e, c, mdp.kgrid(41, 0.2, 5.0), mdp.dgrid(20)


def real_size_points():
    """Flat indices either side of the launch boundary, the last point, and
    eight more."""
    rng = np.random.default_rng(262144)
    return [262143, 262144, 262399] + [int(i) for i in rng.integers(0, 262400, 8)]


def real_size_reference():
    e, c, K, d = real_size_grid()
    shape = (e.size, c.size, K.size, d.size)
    pts = real_size_points()
    ref = np.array([scn_ld.lik(ROW[:8], "loss", K[iK], e[ie], c[ic], 2, 1, M, P, D, d[idd])
                    for ie, ic, iK, idd in (np.unravel_index(q, shape) for q in pts)])
    assert 2 * int((ref > 0).sum()) >= ref.size
    return pts, ref


def test_launch_boundary_at_the_real_size():
    """n = 8 on k_scn_big with no cap: 262 400 points against the 262 144 that
    fit one launch's 1 GiB scratch, so the second launch starts at
    p0 = 262 144 with 256 live lanes.  The whole test, both engines and the
    eleven reference points included, took 0.12 s on an MI355X."""
    n, ts, tdis = 8, 2, 1
    e, c, K, d = real_size_grid()
    per_launch = (1 << 30) // (2 * (1 << n) * 8)  # scratch / (two state vectors of 2^n doubles)
    npts = e.size * c.size * K.size * d.size
    assert per_launch == 262144 and per_launch < npts == 262400 < 2 * per_launch
    pts, ref = real_size_reference()
    big = run(ROW[:n], "loss", KERNELS["big"], e, c, K, d, ts=ts, tdis=tdis)
    lds = run(ROW[:n], "loss", KERNELS["lds"], e, c, K, d, ts=ts, tdis=tdis)
    assert 2 * int((lds > 0).sum()) >= lds.size
    scn_ld.check(big, lds, 2 * scn_ld.bound(n, ts, tdis), "big against lds, whole grid")
    scn_ld.check(big.reshape(-1)[pts], ref, scn_ld.bound(n, ts, tdis), "big at the launch boundary")
