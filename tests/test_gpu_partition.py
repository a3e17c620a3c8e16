"""Grid-partition invariance of the posterior engine, bit for bit.

A slab of the (e, c) grid computed alone has the bits of the same cells of a
one-rank run (midaspom_amd/dist.py, mdp_engine_set_cbound in
include/midaspom.h, README): the multi-GPU drop-ins rest on it.  The grid
planner (mdp_plan_grid, csrc/spom_plan.cpp; tests/test_grid_plan_host.py
holds it to its table on the CPU) picks a grid's kernels from the slab's own
shape, so the slabs here are cut where those choices change:

  * fused (one e block a column) <-> k_qrows + the reading kernel;
  * the reading kernel's tall variant (kb512: an even number of e blocks and a
    workgroup for every CU) <-> the plain one;
  * k_qrows at 4, 2 and 1 c values per workgroup (nc >= 1024, >= 512, less);
  * the wide paths' c chunks (MDP_WIDE_CB seams);
  * the point list of kernels with several points per lane: the s-form run and
    the t-form run, each padded with duplicates that compute and do not store,
    and a list that is not the identity (e not ascending) -- a duplicate names
    the last row of its own run, so its value is that row's and a store would
    only repeat it; what changes bits (by 1 ulp) is a run left unpadded, whose
    last lane then computes a row in the other form;
  * the XCD-aware block order of k_qrows, mdp_fwd_jit, k_fwd_mmt and k_fwd_hs
    (full = gridDim.x & ~7) at workgroup counts around the multiples of 8.

Every comparison between two GPU runs is whole-array bit equality (_same):
a cell wrong at a seam, or written to a neighbouring cell, can pass a 1e-9
check at sampled points but not this.  Bit equality of two runs proves
nothing if both are wrong the same way, so every full grid is also held to
the oracle at 16 points, corners included, at test_gpu_parity's tolerance
(_anchor).  The runs write into a buffer filled with a value no log
likelihood takes (_run), so a cell no workgroup wrote is seen as well.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle
from midaspom_amd.dist import row_slab

from test_gpu_layout import CASES, KNOBS
from test_gpu_parity import assert_loglik_close

pytestmark = pytest.mark.gpu

SENTINEL = 7.0  # log L <= 0 (L is a probability): a cell that keeps 7.0 was not written
TALL = "mdp_fwd_jit<reading,kb512>"


def _engine(model, options=None, devices=(0,)):
    """An engine with exactly these options (a dict): the MDP_* variables of
    the environment are not forwarded."""
    options = dict(options or {})
    assert set(options) <= set(_lib_names()), options
    return mdp.Engine(model, devices=list(devices), options=options)


def _lib_names():
    from midaspom_amd import _lib
    return _lib.ENGINE_OPTION_NAMES


def _run(eng, e, c, cbound=None):
    """The device-resident run of the grid into a padded buffer of SENTINEL:
    the [ne][nc] result, every cell written, the padding untouched."""
    import torch

    e = np.ascontiguousarray(e, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    if cbound is not None:
        eng.set_cbound(cbound)
    eng.set_layout("ec")
    eng.set_grid(e, c)
    ld = c.size + 3
    buf = torch.full((e.size + 1, ld), SENTINEL, dtype=torch.float64, device="cuda")
    eng.run(buf.data_ptr(), ld)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:, c.size:] == SENTINEL).all() and (out[e.size:] == SENTINEL).all(), "stores past the grid"
    got = np.ascontiguousarray(out[:e.size, :c.size])
    assert not (got == SENTINEL).any(), f"{int((got == SENTINEL).sum())} cells not written"
    return got


def _same(got, ref, what):
    """Whole-array bit equality (NaN cells at the same places)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if np.array_equal(got, ref, equal_nan=True):
        return
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    fin = bad & np.isfinite(got) & np.isfinite(ref)
    ulp = int(np.abs(got[fin].view(np.int64) - ref[fin].view(np.int64)).max()) if fin.any() else -1
    first = tuple(int(i) for i in np.argwhere(bad)[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} cells differ (first at {first}: "
                         f"{got[first]!r} != {ref[first]!r}; max distance {ulp} ulp over the finite pairs)")


_ORACLE_REF = {}


def _anchor(key, om, e, c, got):
    """The grid against the oracle at 16 points (the corners, then points
    with a finite result where there are enough), at the suite's tolerance.
    `om` makes the oracle model; the reference of one (key, grid) is computed
    once and shared by the paths that run it."""
    e, c = np.asarray(e), np.asarray(c)
    k = (key, e.tobytes(), c.tobytes())
    if k not in _ORACLE_REF:
        rng = np.random.default_rng(16)
        cand = np.argwhere(np.isfinite(got))
        if len(cand) >= 12:
            pick = cand[rng.choice(len(cand), 12, replace=False)]
        else:
            pick = np.stack([rng.integers(0, e.size, 12), rng.integers(0, c.size, 12)], axis=1)
        ie = np.concatenate([[0, e.size - 1, 0, e.size - 1], pick[:, 0]])
        ic = np.concatenate([[0, 0, c.size - 1, c.size - 1], pick[:, 1]])
        _ORACLE_REF[k] = (ie, ic, om().loglik_points(e[ie], c[ic], threads=16))
    ie, ic, ref = _ORACLE_REF[k]
    assert_loglik_close(got[ie, ic], ref)


def _col_slabs(nc, world):
    return [row_slab(r, world, nc) for r in range(world)]


def _has(launched, pattern):
    return any(re.fullmatch(pattern, k) for k in launched)


# ---------------------------------------------------------------------------
# 1. column slabs under a c bound, where the kernel choice flips
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fname", ["config2_64x50.txt", "config3_256x200.txt"])
def test_column_slabs_cross_tall_and_qrows_width(golden, fname):
    """1 024 e rows are two e blocks (256 threads x 2 points), so the full
    grid is never fused and, with a workgroup for every CU, tall; its 1 024
    columns take k_qrows at 4 c values a workgroup.  The column slabs of 2, 3,
    4, 8 and (1024 // CUs + 1) ranks, each computed alone under the full
    grid's c bound, take k_qrows at 2 and at 1, and the narrow ones -- fewer
    columns than CUs -- the plain reading kernel.  c runs to 1.5, so the
    grid's max |c| lives only in the last slab: without the bound the other
    slabs would prune their Z tables for a smaller |c|."""
    import torch

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    model = mdp.Model.load(golden / fname)
    e, _ = mdp.grid(1024)
    c, _ = mdp.grid(1024, 0.0, 1.5)
    cmax = float(np.abs(c).max())
    assert np.abs(c[:512]).max() < 1.0 < cmax
    with _engine(model) as eng:
        full = _run(eng, e, c)
        launched = eng.launched()
    assert TALL in launched, f"the full grid did not take the tall reading kernel on {ncu} CUs: {launched}"
    assert _has(launched, r"k_qrows<8,[01],4>"), launched
    _anchor(fname, lambda: oracle.OracleModel.load(golden / fname), e, c, full)

    derived = min(1024 // ncu + 1, 64)  # its narrowest slabs have fewer columns than the device has CUs
    worlds = sorted({2, 3, 4, 8, derived}, reverse=True)
    plain = []
    with _engine(model) as eng:
        for world in worlds:  # the narrow slabs first: launched() only grows
            slabs = _col_slabs(c.size, world)
            if world == 3:
                assert slabs[0][1] - slabs[0][0] == slabs[1][1] - slabs[1][0] + 1  # the remainder on rank 0
            parts = [_run(eng, e, c[a:b], cbound=cmax) for a, b in slabs]
            _same(np.hstack(parts), full, f"{fname}: column slabs of {world} ranks")
            if TALL not in eng.launched():
                plain.append(world)
        launched = eng.launched()
    assert plain, (f"no rank count of {worlds} gave a slab the plain reading kernel on {ncu} CUs: the table no "
                   f"longer crosses the tall threshold (nc * gy / 2 >= CUs)")
    assert _has(launched, r"mdp_fwd_jit<reading,maxA\d+>"), launched
    assert _has(launched, r"k_qrows<8,[01],2>") and _has(launched, r"k_qrows<8,[01],1>"), launched
    assert not _has(launched, r"k_qrows<8,[01],4>"), launched


# widths of the column slabs of an 84-column grid: the fused kernel takes two
# columns a workgroup, k_qrows (below 512 columns) and the reading kernel one
BLOCK_ORDER = {
    "fused": ({}, (1, 13, 16, 17, 34, 3), 2, r"mdp_fwd_jit<fused,maxA\d+>", 1.0),
    "reading": ({"MDP_FUSED": "0"}, (1, 7, 8, 9, 17, 42), 1, r"mdp_fwd_jit<reading,maxA\d+>", 1.5),
}


@pytest.mark.parametrize("name", sorted(BLOCK_ORDER))
def test_column_slabs_cross_block_order(golden, name):
    """The XCD-aware block order maps block b < full = gridDim.x & ~7 to
    (b & 7) * (full / 8) + b / 8 and the tail to itself: slabs whose launches
    have 1, 7, 8, 9 and 17 workgroups (no permuted block, only a tail, no
    tail, one tail block, two rounds and a tail) against the 84-column grid,
    on k_qrows + the reading kernel and on the fused kernel."""
    options, widths, per_wg, kernel, chi = BLOCK_ORDER[name]
    assert sum(widths) == 84 and {1, 7, 8, 9, 17} <= {-(-w // per_wg) for w in widths}
    model = mdp.Model.load(golden / "config2_64x50.txt")
    e, _ = mdp.grid(101, 0.0, 1.1)
    c, _ = mdp.grid(84, 0.0, chi)  # the fused kernel holds the Z columns of |c| <= 1
    cmax = float(np.abs(c).max())
    with _engine(model, options) as eng:
        full = _run(eng, e, c)
        assert _has(eng.launched(), kernel), eng.launched()
    _anchor("config2", lambda: oracle.OracleModel.load(golden / "config2_64x50.txt"), e, c, full)
    with _engine(model, options) as eng:
        c0 = 0
        for w in widths:
            part = _run(eng, e, c[c0:c0 + w], cbound=cmax)
            _same(part, full[:, c0:c0 + w], f"{name}: columns [{c0}, {c0 + w})")
            c0 += w
        launched = eng.launched()
    assert _has(launched, kernel), launched
    assert (name == "fused") != _has(launched, r"k_qrows<8,[01],1>"), launched


# ---------------------------------------------------------------------------
# 2. row slabs where fused flips, through the multi-context engine as well
# ---------------------------------------------------------------------------
ROW_SLABS = [(0, 1), (1, 3), (3, 460), (460, 461), (461, 917), (917, 1100)]


def _sform(e):
    x = np.minimum(e, 1.0)
    return x < 1.0 - x


@pytest.fixture(scope="module")
def tall_narrow(golden):
    """Config 2 on 1 100 x 37 (three e blocks a column: k_qrows + the plain
    reading kernel), computed once by a single-context engine."""
    model = mdp.Model.load(golden / "config2_64x50.txt")
    e, _ = mdp.grid(1100, 0.0, 1.2)
    c, _ = mdp.grid(37)
    with _engine(model) as eng:
        full = _run(eng, e, c)
        host = eng.loglik_grid(e, c)
        launched = eng.launched()
    _same(host, full, "loglik_grid against the device-resident run")
    assert _has(launched, r"mdp_fwd_jit<reading,maxA\d+>") and _has(launched, r"k_qrows<8,[01],1>"), launched
    assert not any("mdp_fwd_jit<fused" in k for k in launched) and TALL not in launched, launched
    _anchor("config2", lambda: oracle.OracleModel.load(golden / "config2_64x50.txt"), e, c, full)
    full.setflags(write=False)
    return model, e, c, full


def test_row_slabs_cross_fused(tall_narrow):
    """Row slabs of at most 512 rows are one e block a column, so each takes
    the fused kernel where the full grid takes k_qrows + the reading kernel.
    The slabs hold only s-form rows (e < 0.5), only t-form rows, rows of
    e >= 1 alone, and both forms with an odd s-form count, whose padding
    duplicates then sit in the middle of the point list."""
    model, e, c, full = tall_narrow
    s = [_sform(e[a:b]) for a, b in ROW_SLABS]
    assert all(b - a <= 512 for a, b in ROW_SLABS) and ROW_SLABS[-1][1] == e.size
    assert s[0].all() and s[1].all() and not s[3].any() and not s[4].any()
    assert s[2].any() and not s[2].all() and s[2].sum() % 2 == 1
    assert (e[ROW_SLABS[5][0]:] >= 1.0).all()
    order = np.random.default_rng(6).permutation(len(ROW_SLABS))
    assert not np.array_equal(order, np.sort(order))
    with _engine(model) as eng:
        for i in order:
            a, b = ROW_SLABS[i]
            _same(_run(eng, e[a:b], c), full[a:b], f"rows [{a}, {b}) computed alone")
        launched = eng.launched()
    assert _has(launched, r"mdp_fwd_jit<fused,maxA\d+>"), launched
    assert not any("mdp_fwd_jit<reading" in k or k.startswith("k_qrows") for k in launched), launched


@pytest.mark.parametrize("contexts", [3, 7])
def test_multi_context_engine_equals_single(tall_narrow, contexts):
    """mdp_loglik_grid splits the e rows over the engine's contexts (the
    remainder to the first): on 3 and on 7 contexts of one device every slab
    of the 1 100 rows is fused, and the grid is the single-context engine's
    in both layouts."""
    model, e, c, full = tall_narrow
    with _engine(model, devices=[0] * contexts) as eng:
        ec = eng.loglik_grid(e, c, layout="ec")
        ce = eng.loglik_grid(e, c, layout="ce")
        launched = eng.launched()
    _same(ec, full, f"{contexts} contexts, layout ec")
    _same(ce, full, f"{contexts} contexts, layout ce")
    assert _has(launched, r"mdp_fwd_jit<fused,maxA\d+>"), launched
    assert not any("mdp_fwd_jit<reading" in k for k in launched), launched


# ---------------------------------------------------------------------------
# 3. permutation equivariance on every forward path
# ---------------------------------------------------------------------------
def _table_model(name):
    return CASES[name][0]()


# name -> (model, ne, nc, options, kernel): the layout table's rows at its
# grid sizes or smaller, the e count odd (direct paths) or one past a
# multiple of the matrix-core kernels' point tile (16 rt points a workgroup:
# a partial last tile), and two rows of this module's
EQUIV = {name: (make, ne, nc, env, kernel) for name, (make, ne, nc, env, kernel) in CASES.items()}
EQUIV_NE = {"fused": 95, "reading": 95, "chunked": 299, "generic": 69, "lds_states": 129, "wide": 129,
            "wide_mma5": 129, "wide_big": 65, "wide_big_mmt": 65, "wide_hs": 129, "wide_plain": 129,
            "gathered": 95, "qglobal": 95}
EQUIV["gathered"] = (CASES["fused"][0], 96, 80, {"MDP_JIT_GATHER": "1"}, "gather>")
EQUIV["qglobal"] = (CASES["fused"][0], 96, 80, {"MDP_QGLOBAL": "1"}, "k_wq")


def _points_per_workgroup(launched):
    """Points of a matrix-core forward workgroup, from the instantiation's name."""
    for k in launched:
        m = re.match(r"k_fwd_(hs|mmt)<(\d+),", k)
        if m:
            return 16 * int(m.group(2))
        m = re.match(r"k_fwd_mma<(\d+)>", k)
        if m:
            return 32 if int(m.group(1)) > 128 else 64
    return None


def test_equivariance_table_covers_the_layout_table():
    assert set(EQUIV) == set(CASES) | {"gathered", "qglobal"} and set(EQUIV_NE) == set(EQUIV)
    assert all(EQUIV_NE[n] <= EQUIV[n][1] and EQUIV_NE[n] % 2 == 1 for n in EQUIV)
    assert set(k for _, _, _, env, _ in EQUIV.values() for k in env) <= set(KNOBS)


@pytest.mark.parametrize("name", sorted(EQUIV))
def test_permuting_the_grid_permutes_the_result(name):
    """The ABI takes any e and c arrays.  The grid on e[pe] x c[pc] is the
    ascending grid's A[pe][:, pc], bit for bit; so are the grid on reversed
    e and the grid on an e array that holds each value twice.  With several
    points per lane an e array that is not ascending gives a point list that
    is not the identity (s-form rows first, padded runs), which no ascending
    grid runs."""
    make, _, nc, options, kernel = EQUIV[name]
    ne = EQUIV_NE[name]
    model = make()
    e, _ = mdp.grid(ne, 0.0, 1.1)
    c, _ = mdp.grid(nc)
    rng = np.random.default_rng(31)
    pe, pc = rng.permutation(ne), rng.permutation(nc)
    with _engine(model, options) as eng:
        perm = _run(eng, e[pe], c[pc])
        launched = eng.launched()
        assert any(kernel in k for k in launched), launched  # the permuted run took the path
        if name == "lds_states":  # years of 17-64 states: the specialised kernel with its states in LDS
            assert 16 < model.npstates.max() <= 64 and 10000 <= eng.info()["variant"] < 20000, eng.info()
        A = _run(eng, e, c)
        rev = _run(eng, e[::-1], c)
        half = e[: (ne + 1) // 2]
        twice = _run(eng, np.repeat(half, 2), c)
        assert eng.launched() == launched, (launched, eng.launched())
    pts = _points_per_workgroup(launched)
    if pts and "k_fwd_wide" not in kernel:
        assert ne % pts == 1 and ne > pts, (ne, pts)  # a partial last tile
    _same(perm, A[np.ix_(pe, pc)], f"{name}: permuted e and c")
    _same(rev, A[::-1], f"{name}: reversed e")
    _same(twice, np.repeat(A[: half.size], 2, axis=0), f"{name}: every e twice")
    assert np.isfinite(A).mean() > 0.5
    obs = model.obs
    _anchor(obs.tobytes(), lambda: oracle.OracleModel.from_obs(obs), e, c, A)


# ---------------------------------------------------------------------------
# 4. slabs and chunk seams on the wide paths
# ---------------------------------------------------------------------------
# (input of the layout table, options, kernel, points per workgroup)
WIDE = {
    "n12-mmt": ("wide", {"MDP_WIDE": "1", "MDP_WIDE_MMA": "2"}, "k_fwd_mmt<4,128,2buf>", 64),
    "n12-plain": ("wide", {"MDP_WIDE": "1", "MDP_WIDE_MMA": "0"}, "k_fwd_wide", 256),
    "n10-hs": ("wide_big", {}, "k_fwd_hs<1,10>", 16),
    "n10-mmt": ("wide_big", {"MDP_WIDE_MMA": "2"}, "k_fwd_mmt<2,512,1buf>", 32),
    "n10-plain": ("wide_big", {"MDP_WIDE": "1", "MDP_WIDE_MMA": "0"}, "k_fwd_wide", 256),
}
# column slabs of the 37 columns, three ways: with one tile of e rows the
# forward launches 7, 8, 9, 13 / 15, 16, 6 / 17, 20 workgroups
WIDE_WIDTHS = [(7, 8, 9, 13), (15, 16, 6), (17, 20)]


@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_slabs_and_chunk_seams(name):
    """The wide paths on 70 x 37: column slabs under the c bound on the rows
    of one point tile (so the matrix-core forward's XCD-aware order sees 7,
    8, 9, 15, 16 and 17 workgroups), row slabs of 1, 17 and the other 52
    rows, and the grid cut into c chunks of 1 and of 5 columns (MDP_WIDE_CB:
    k_witems + k_wq per chunk, k_fwd_hs and k_fwd_wide per chunk) all equal
    the grid computed whole."""
    table, options, kernel, pts = WIDE[name]
    model = _table_model(table)
    e, _ = mdp.grid(70, 0.0, 1.1)
    c, _ = mdp.grid(37, 0.0, 1.5)
    cmax = float(np.abs(c).max())
    with _engine(model, options) as eng:
        full = _run(eng, e, c)
        launched = eng.launched()
    assert kernel in launched, launched
    if kernel != "k_fwd_wide":
        assert _points_per_workgroup(launched) == pts
    obs = model.obs
    _anchor(obs.tobytes(), lambda: oracle.OracleModel.from_obs(obs), e, c, full)

    ne_tile = min(pts, 64) - 3  # one (partial) tile of e rows: a workgroup per column
    counts = set()
    with _engine(model, options) as eng:
        for widths in WIDE_WIDTHS:
            assert sum(widths) == c.size
            c0 = 0
            for w in widths:
                part = _run(eng, e[:ne_tile], c[c0:c0 + w], cbound=cmax)
                _same(part, full[:ne_tile, c0:c0 + w], f"{name}: rows [0, {ne_tile}) x columns [{c0}, {c0 + w})")
                counts.add(-(-ne_tile // pts) * w)
                c0 += w
        assert {7, 8, 9, 15, 16, 17} <= counts
        eng.set_cbound(0.0)
        for a, b in [(0, 1), (1, 18), (18, 70)]:
            _same(_run(eng, e[a:b], c), full[a:b], f"{name}: rows [{a}, {b})")
        assert kernel in eng.launched()
    for cb in ("1", "5"):
        with _engine(model, dict(options, MDP_WIDE_CB=cb)) as eng:
            _same(_run(eng, e, c), full, f"{name}: c chunks of {cb}")
            assert kernel in eng.launched()


# ---------------------------------------------------------------------------
# 5. state carried between grids
# ---------------------------------------------------------------------------
def test_state_carried_between_grids(golden):
    """One engine through a shuffled sequence of (e, c, c bound) that moves
    the grid's max |c| up and down, the bound from a value to 0 and back, the
    forward between fused, reading and tall, and the point list between the
    identity and a list: every result is a fresh engine's for that triple
    alone (the Z tables cached for the last bound, the point list, the
    loaded variant and the k_qrows width are all state of the context)."""
    import torch

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    model = mdp.Model.load(golden / "config2_64x50.txt")
    rng = np.random.default_rng(51)
    e_fused, _ = mdp.grid(101, 0.0, 1.1)   # one e block a column
    e_read, _ = mdp.grid(1100, 0.0, 1.2)   # three: never tall
    e_tall, _ = mdp.grid(1024)             # two, tall with a workgroup for every CU
    c_low, _ = mdp.grid(37, 0.0, 0.6)
    c_high, _ = mdp.grid(37, 0.0, 1.5)
    c_many, _ = mdp.grid(ncu + 8, 0.0, 1.0)
    triples = [
        (e_fused, c_low, 0.0),
        (e_read, c_high, 0.0),
        (e_fused, c_low, 1.5),
        (e_tall, c_many, 0.0),
        (e_fused[rng.permutation(e_fused.size)], c_low, 0.0),
        (e_read[rng.permutation(e_read.size)], c_low, 2.0),
        (e_fused, c_high, 0.7),
        (e_tall, c_many, 1.5),
        (e_read, c_low, 0.0),
    ]
    order = rng.permutation(len(triples))
    with _engine(model) as eng:
        got = {int(i): _run(eng, *triples[i][:2], cbound=triples[i][2]) for i in order}
        launched = eng.launched()
    assert _has(launched, r"mdp_fwd_jit<fused,maxA\d+>") and _has(launched, r"mdp_fwd_jit<reading,maxA\d+>"), launched
    assert TALL in launched, launched
    for i, (e, c, cbound) in enumerate(triples):
        with _engine(model) as fresh:
            _same(got[i], _run(fresh, e, c, cbound=cbound), f"triple {i} (position {list(order).index(i)} of the sequence)")


def test_set_cbound_api(golden):
    """mdp_engine_set_cbound refuses a negative value, NaN and infinity and
    leaves the engine as it was; a bound below the grid's own max |c| changes
    nothing."""
    model = mdp.Model.load(golden / "config2_64x50.txt")
    e, _ = mdp.grid(41, 0.0, 1.1)
    c, _ = mdp.grid(23, 0.0, 1.5)
    with _engine(model) as eng:
        ref = _run(eng, e, c)
        for bad in (-0.5, float("nan"), float("inf"), float("-inf")):
            with pytest.raises(mdp.MidaspomError):
                eng.set_cbound(bad)
            _same(_run(eng, e, c), ref, f"after the refused bound {bad}")
        _same(_run(eng, e, c, cbound=0.3), ref, "a bound below the grid's max |c|")
        _same(_run(eng, e, c, cbound=float(np.abs(c).max())), ref, "a bound equal to the grid's max |c|")
    _anchor("config2", lambda: oracle.OracleModel.load(golden / "config2_64x50.txt"), e, c, ref)
