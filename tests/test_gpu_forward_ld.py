"""Every forward path of the posterior engine against the long-double
evaluation of the model (tests/fwd_ld.py), on a grid of border points: e = 0,
1e-300, 1e-17, the last doubles around 0.5 (where the two ratio forms switch
per lane), 0.9, the two doubles below 1, 1 and 1.3, padded with interior
values to 66 points (both forms in one wave, a second wave partly filled at
1, 2 and 4 points per lane); c = 0, 1e-300, 0.3, the c at which the pressure
c S of one reachable (hidden state, variable patch) reaches the clamp at 1,
with its two neighbouring doubles, and one c above every clamp.

What is asserted (fwd_ld.check): -inf exactly where the reference is 0; where
the reference is at least 2^-950, |log L - log ref| <= fwd_ld.bound() + k_log
ulp(log ref), with bound() counted from the roundings on a path (fwd_ld's
docstring; at most 2e-12 for every case, against the 1e-9 of
tests/test_gpu_parity.py) and k_log = 3.5 (mdp_log's 2 ulp of the library log,
the library's 1, half an ulp for rounding log L) or 1.5 with MDP_FAST_LOG=0;
below 2^-950 test_gpu_parity's rule for subnormal L.  Each test prints its
largest error as a fraction of that tolerance.

Measured on an MI355X, the largest error of each path as a fraction of the
tolerance (every path of one case lands on the same worst cell, where the
rounding of log L itself dominates): case a1 0.091 and a2 0.069 on each of
the nine engine paths (mdp_fwd_jit fused and reading after k_qrows, k_coefs +
k_forward_lds, k_fwd_mmt<4,128,2buf>, k_fwd_wide, k_fwd_hs<2,8> and <2,9>,
whole and one c per launch); the clamp on an always-zero patch 0.070; the
LDS-state kernel 0.055 (32 states) and 0.052 (64), MDP_VSPLIT 1 and 4 alike;
the wide forwards 0.054 / 0.045 / 0.015 / 0.011 at 128 / 256 / 512 / 1 024
states on k_fwd_hs<1,10>, k_fwd_mmt's four shapes, k_fwd_mma<128|256> and
k_fwd_wide (0.043 at 256); the flush series 0.058-0.063, fused, reading,
chunked with gather and with Q rows from HBM alike; the one-year series
0.014; a1 with the library log 0.151 of its smaller tolerance; two e blocks
and 1, 2, 4 points per lane 0.091.  The bounds run from 2.9e-15 (one year) to
7.3e-13 (the 1 024-state year).

The Z rows' small-column series (section (z); fwd_ld's `zser` term in the
bound), same device: z-steep 0.049 on every path, z-flat 0.063 on the eight
paths with the series and 0.076 on the generic one (k_zpv multiplies the 34
factors out: the control), Q rows from HBM and a chunked forward alike;
z-flat-wide (114 small columns, argument 0.85) 0.057, z-drop 0.087 and z-drop0
0.094 on the fused kernel, k_qrows + reading and k_zrows alike; z-steep under
the six |c| bounds (kmax 8, 16, 16, 32, 40, 64) 0.049-0.050; z-flat on 512 /
1 024 c values (k_qrows<8,0,2> / <8,0,4>) 0.074 / 0.070; k_zrows' block edges
(130, 193 c values) 0.056, 0.057.  Bounds 9.9e-14 to 2.6e-13.  On these cells
the 3.5 ulp of log L are about a tenth of the tolerance: the arithmetic's own
error is far inside bound().  What the section can and cannot see: a series
term k <= 6 gone or exchanged on any one implementation leaves the bound on
z-flat (term 6, the weakest: 6.9 times the tolerance, tests/test_forward_ld.py);
an error of less than about a seventh of P6 / 6 alone, and anything in terms
7 and 8 (<= 3e-14 and 2e-16 of L), is below it -- the host table is held by
tests/test_zsplit_host.py, and an exchange among coefficients 7 and 8 in one
kernel shows only in test_series_fused_and_qrows_identical.
"""
from __future__ import annotations

import numpy as np
import pytest

import midaspom_amd as mdp
import fwd_ld
from test_gpu_parity import engine_path, _wide_engine_run, launched_forward  # noqa: F401 (engine_path: a fixture)
from test_zsplit_host import STEEP_BOUNDS, steep_bound

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not fwd_ld.OK, reason=fwd_ld.SKIP_REASON)]

KNOBS = ("MDP_JIT", "MDP_JIT_SLOTS", "MDP_JIT_XCD", "MDP_FUSED", "MDP_WIDE", "MDP_WIDE_CB", "MDP_WIDE_MMA", "MDP_VSPLIT",
         "MDP_JIT_CHUNK", "MDP_JIT_GATHER", "MDP_QGLOBAL", "MDP_FAST_LOG", "MDP_EPL")


def case(name):
    cs = fwd_ld.cases()[name]
    return cs, cs.ref()  # (asserts the case's normal cells and its bound)


def model_of(cs):
    return mdp.Model.from_obs(cs.obs, m=cs.m, p=cs.p, d=cs.d)


def run(cs, monkeypatch, env=None):
    """(log L, launched kernels, info) with exactly `env` of the knobs set
    (None: the environment as the engine_path fixture left it)."""
    if env is not None:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    with mdp.Engine(model_of(cs)) as eng:
        got = eng.loglik_grid(cs.e, cs.c)
        return got, eng.launched(), eng.info()


def held(got, ref, cs, what, k_log=fwd_ld.K_LOG_FAST, bnd=None):
    bnd = cs.bound if bnd is None else bnd
    frac = fwd_ld.check(got, ref, bnd, what, k_log)
    print(f"\n{what}: frac {frac:.3f} of the tolerance (bound {bnd:.3e}, {fwd_ld.normal_fraction(ref):.2f} normal)")
    return frac


# ---------------------------------------------------------------------------
# (a) every engine path, two small problems, the whole border grid
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a1", "a2"])
def test_every_engine_path(name, engine_path, monkeypatch):
    """a1: 12 patches with the 8 variable ones in the middle of the row (four
    always-zero patches: Z rows), 6 years of up to 16 states; a2: 9 patches,
    all variable, 5 years, p = 0.3, m = 250."""
    cs, ref = case(name)
    got, launched, info = run(cs, monkeypatch)
    ran_on(engine_path, model_of(cs), launched, info)
    held(got, ref, cs, f"{name} {engine_path} {sorted(launched)}")


def ran_on(engine_path, model, launched, info):
    """The kernels of the engine_path fixture's value ran."""
    if engine_path.startswith("wide"):
        assert info["variant"] >= 20000, info
        path = {"wide-plain": "wide-plain", "wide-hs": "wide-hs", "wide-hs-chunked": "wide-hs"}.get(engine_path, "wide")
        assert launched_forward(model, path) in launched, launched
    elif engine_path == "generic":
        assert info["variant"] < 10000 and any(k.startswith("k_forward") for k in launched), (info, launched)
    else:
        assert 10000 <= info["variant"] < 20000, info
        assert any(k.startswith("mdp_fwd_jit<") for k in launched), launched
        if engine_path == "direct-qrows":
            assert any(k.startswith("k_qrows<") for k in launched) and "mdp_fwd_jit<fused" not in " ".join(launched), launched


def test_clamp_on_an_always_zero_patch(monkeypatch):
    """a1 at the c where c S reaches 1 on an always-zero patch of a reachable
    hidden state, and its two neighbouring doubles: the reference's factor is
    1 - min(1, fl(c S)).  Held to the bound without its kappa term (fwd_ld's
    docstring, `item`), i.e. to the reference's own semantics at the clamp."""
    a1 = fwd_ld.cases()["a1"]
    c1, j, k = fwd_ld.clamp_c(a1.inp, variable=False)
    c = np.array([np.nextafter(c1, 0.0), c1, np.nextafter(c1, np.inf)])
    cs = fwd_ld.Case("a1-zclamp", a1.obs, fwd_ld.E12, c, a1.m, a1.p, a1.d)
    ref = fwd_ld.reference(cs.obs, cs.m, cs.p, cs.d, cs.e, cs.c)
    assert 2 * (ref >= fwd_ld.L_NORMAL).sum() >= ref.size
    bnd = fwd_ld.bound(cs.inp)
    assert bnd <= 2e-12
    for env in ({}, {"MDP_FUSED": "0"}, {"MDP_WIDE": "1"}):
        got, launched, _ = run(cs, monkeypatch, env)
        frac = fwd_ld.check(got, ref, bnd, f"zclamp {env}")
        print(f"\nzclamp {env} {sorted(launched)}: frac {frac:.3f} (hidden state {j}, patch {k}, c = {c1!r})")


# ---------------------------------------------------------------------------
# (b) the LDS-state kernel: years of 32 and 64 states
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("vsplit", ["1", "4"])
@pytest.mark.parametrize("name", ["b5", "b6"])
def test_lds_state_kernel(name, vsplit, monkeypatch):
    cs, ref = case(name)
    model = model_of(cs)
    assert model.npstates.max() == {"b5": 32, "b6": 64}[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MDP_VSPLIT", vsplit)
    got = _wide_engine_run(model, cs.e, cs.c, "default", monkeypatch)  # asserts mdp_fwd_jit<reading ran
    held(got, ref, cs, f"{name} vsplit {vsplit}")


# ---------------------------------------------------------------------------
# (c) the wide forwards: years of 128 to 1 024 states
# ---------------------------------------------------------------------------
WIDE = [(s, p) for s in (128, 256, 512, 1024) for p in ("default", "wide-mmt", "wide-mma5", "wide-plain")
        if p != "wide-mma5" or s <= 256]  # (k_fwd_mma holds years of up to 256 states)


@pytest.mark.parametrize("states,path", WIDE, ids=[f"{s}-{p}" for s, p in WIDE])
def test_wide_forwards(states, path, monkeypatch):
    """10 patches (all variable), 4 years, year 1 with 7-10 unvisited
    patches: k_fwd_hs<1,10> by default -- with case (a)'s <2,8> and <2,9>
    every k_fwd_hs instantiation -- k_fwd_mmt's four shapes, k_fwd_mma<128>
    and <256>, and k_fwd_wide (_wide_engine_run asserts which one ran)."""
    cs, ref = case(f"c{states}")
    model = model_of(cs)
    assert model.npstates.max() == states
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    got = _wide_engine_run(model, cs.e, cs.c, path, monkeypatch)
    held(got, ref, cs, f"c{states} {path} {launched_forward(model, path)}")


# ---------------------------------------------------------------------------
# (d) flush boundaries of the deferred exponent
# ---------------------------------------------------------------------------
def _powcost(x):
    return 0 if x <= 1 else x.bit_length() - 1 + bin(x).count("1") - 1


def _schedule(inp):
    """schedule() of csrc/spom_jit.cpp restated: (the pending exponent after
    each year before any flush, {year: flushed exponent}, the final one)."""
    E, seen, flush = 0, [], {}
    for t in range(1, len(inp.years)):
        E += min(bin(a).count("1") for a in inp.years[t - 1])
        seen.append(E)
        if E >= 192:
            flush[t] = E
            E = 0
    return seen, flush, E


def _ratio_work(inp, flush, final):
    """mdp_jit_ratio_work's per-point counts for these flushes (the formula
    of test_gpu_parity's work-fact test): what the generator's plan reports
    through mdp_engine_work_fact, so a flush at another year or exponent
    shows."""
    groups, gd, yr = set(), set(), 0.0
    for t in range(1, len(inp.years)):
        src, dst = inp.years[t - 1], inp.years[t]
        a_src = [bin(a).count("1") for a in src]
        for b in dst:
            for a in src:
                nX, nA = bin(a & b).count("1"), bin(a).count("1")
                if (a & b, b) not in groups:
                    groups.add((a & b, b))
                    yr += 2 * nX
                if nA > nX:
                    gd.add((a & b, b, nA - nX))
        yr += len(dst) * (2 * len(src) - 1) + sum(1 for a in a_src if a > min(a_src))
        if t in flush:
            yr += len(dst) + _powcost(flush[t])
    final_r = len(inp.years[-1]) + 1 + (_powcost(final) + 1 if final else 0)
    return yr + 0.5 * len(gd), final_r


FLUSH = {"d191": (191, {33: 197}, 6), "d192": (192, {32: 192}, 12), "d193": (193, {32: 193}, 12),
         "dlast": (192, {32: 192}, 0)}
VARIANTS = {"fused": {"MDP_FUSED": "1"}, "reading": {"MDP_FUSED": "0"},
            "chunks-gather": {"MDP_JIT_CHUNK": "12", "MDP_JIT_GATHER": "1"}, "qglobal": {"MDP_QGLOBAL": "1"}}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(FLUSH))
def test_flush_boundaries(name, variant, monkeypatch):
    """Fully observed series of 6 (7) patches whose pending exponent is 191,
    192, 193 after year 32 -- flushed in year 33 as 197, in year 32 as 192 and
    193 -- and a 33-year series that flushes 192 on its last transition (final
    exponent 0); e on both sides of 0.5, at 1e-17 and just below 1.  The
    exponents are asserted on the restated schedule and, through
    mdp_engine_work_fact, on the generator's own."""
    cs, ref = case(name)
    inp = cs.inp
    seen, flush, final = _schedule(inp)
    at32, want_flush, want_final = FLUSH[name]
    assert (seen[31], flush, final) == (at32, want_flush, want_final)
    env = VARIANTS[variant]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g8, _ = mdp.grid(8)  # rows 0-3 s-form, 4-7 t-form
    with mdp.Engine(model_of(cs)) as eng:
        eng.set_grid(g8, g8)
        w = eng.work_fact(8, 8)
        got = eng.loglik_grid(cs.e, cs.c)
        launched = eng.launched()
    use, fin = _ratio_work(inp, flush, final)
    assert (w["use_pt_ratio"], w["final_pt_ratio"]) == (pytest.approx(use), fin)
    names = " ".join(sorted(launched))
    if variant == "fused":
        assert "mdp_fwd_jit<fused" in names, launched
    elif variant == "reading":
        assert "mdp_fwd_jit<reading" in names and "k_qrows<" in names, launched
    elif variant == "chunks-gather":
        assert "chunks" in names and "gather" in names, launched
    else:
        assert {"k_zrows", "k_wq"} <= launched and "k_qrows<" not in names, launched
    held(got, ref, cs, f"{name} {variant}")


# ---------------------------------------------------------------------------
# (e) the log alone
# ---------------------------------------------------------------------------
def test_one_year_is_the_log_alone(monkeypatch):
    """One year of 8 states: L = 8 prior0 on every point, so only the log's
    error is left (no transition: the runtime-shape kernels, and the wide
    path when forced)."""
    cs, ref = case("e1")
    assert (ref == np.longdouble(8 * cs.inp.prior0)).all()
    for env in ({}, {"MDP_WIDE": "1"}):
        got, launched, _ = run(cs, monkeypatch, env)
        held(got, ref, cs, f"e1 {env} {sorted(launched)}")


def test_library_log(monkeypatch):
    """a1 with MDP_FAST_LOG=0: k_log drops to the library's 1.5, which leaves
    the arithmetic ahead of the log."""
    cs, ref = case("a1")
    got, launched, _ = run(cs, monkeypatch, {"MDP_FAST_LOG": "0"})
    held(got, ref, cs, f"a1 library log {sorted(launched)}", k_log=fwd_ld.K_LOG_LIB)


# ---------------------------------------------------------------------------
# (f) grid shapes that change the variant
# ---------------------------------------------------------------------------
def test_two_e_blocks_fused(monkeypatch):
    """a1 on 600 e values x 3 c values: two e blocks, the fused kernel forms
    its column's Q in both."""
    cs, ref = case("f600")
    got, launched, _ = run(cs, monkeypatch, {"MDP_FUSED": "1"})
    assert any(k.startswith("mdp_fwd_jit<fused") for k in launched), launched
    held(got, ref, cs, f"f600 {sorted(launched)}")


@pytest.mark.parametrize("epl", ["1", "2", "4"])
def test_points_per_lane(epl, monkeypatch):
    cs, ref = case("a1")
    got, launched, _ = run(cs, monkeypatch, {"MDP_EPL": epl})
    assert any(k.startswith("mdp_fwd_jit<") for k in launched), launched
    held(got, ref, cs, f"a1 epl {epl} {sorted(launched)}")


# ---------------------------------------------------------------------------
# (z) the Z rows' small-column series (fwd_ld's docstring, `zser`): every
# implementation -- zseries in k_zrows, k_qrows' quad gather at 1, 2 and 4 c
# values a workgroup, the fused kernel's Horner -- on cases whose columns sit
# in the series, under the bound extended by its term
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["z-steep", "z-flat"])
def test_series_on_every_engine_path(name, engine_path, monkeypatch):
    """z-steep (68 patches: explicit, small and dropped columns in one row, a
    column at fl(cmax S) = 2^-7) and z-flat (34 small columns within 10 % of
    the threshold) on the nine paths: the fused kernel, the reading kernel
    behind k_qrows, k_zrows behind k_witems for the mmt, plain and hs
    forwards; the generic path (k_zpv: no series) is the control."""
    cs, ref = case(name)
    got, launched, info = run(cs, monkeypatch)
    ran_on(engine_path, model_of(cs), launched, info)
    if engine_path.startswith("wide"):
        assert "k_zrows" in launched, launched
    if engine_path == "direct":
        assert any(k.startswith("mdp_fwd_jit<fused") for k in launched), launched
    held(got, ref, cs, f"{name} {engine_path} {sorted(launched)}")


@pytest.mark.parametrize("variant", ["qglobal", "chunks"])
@pytest.mark.parametrize("name", ["z-steep", "z-flat"])
def test_series_qglobal_and_chunked(name, variant, monkeypatch):
    """Q rows built in HBM (k_zrows + k_witems + k_wq ahead of the reading
    kernel) and a chunked forward behind k_qrows."""
    cs, ref = case(name)
    got, launched, _ = run(cs, monkeypatch, {"qglobal": {"MDP_QGLOBAL": "1"}, "chunks": {"MDP_JIT_CHUNK": "40"}}[variant])
    names = " ".join(sorted(launched))
    if variant == "qglobal":
        assert {"k_zrows", "k_wq"} <= launched and "k_qrows<" not in names, launched
    else:
        assert "chunks" in names and "k_qrows<" in names, launched
    held(got, ref, cs, f"{name} {variant} {sorted(launched)}")


SERIES_ENV = {"fused": {"MDP_FUSED": "1"}, "reading": {"MDP_FUSED": "0"}, "wide": {"MDP_WIDE": "1"}}


def _series_ran(variant, launched):
    names = " ".join(sorted(launched))
    if variant == "fused":
        assert "mdp_fwd_jit<fused" in names, launched
    elif variant == "reading":
        assert "mdp_fwd_jit<reading" in names and "k_qrows<" in names, launched
    else:
        assert "k_zrows" in launched, launched


@pytest.mark.parametrize("variant", list(SERIES_ENV))
@pytest.mark.parametrize("name", ["z-flat-wide", "z-drop", "z-drop0"])
def test_series_large_and_tiny_arguments(name, variant, monkeypatch):
    """z-flat-wide: 114 small columns, a series argument of 0.85; z-drop:
    every column one notch above 2^-55 (an argument of the order of 2^-50);
    z-drop0: every column dropped (all coefficients zero: exp(0))."""
    cs, ref = case(name)
    got, launched, _ = run(cs, monkeypatch, SERIES_ENV[variant])
    _series_ran(variant, launched)
    held(got, ref, cs, f"{name} {variant} {sorted(launched)}")


@pytest.mark.parametrize("which", list(STEEP_BOUNDS))
def test_class_boundary_moves(which, monkeypatch):
    """z-steep behind k_qrows under mdp_engine_set_cbound = cmax, the next
    double (the threshold column turns explicit), 2 cmax, 2^14, 2^20 and a
    bound that makes every column explicit: kmax 8, 16, 16, 32, 40, 64
    (asserted on the host planner for these very bounds by tests/
    test_zsplit_host.py::test_steep_kmax_under_a_bound; the engine reports no
    kmax), so k_qrows' long-row loop (chain pairs past the first three) does
    not run, runs without its trailing pair (32), with it (40) and twice
    (64).  Each run within the bound of its own split."""
    cs, ref = case("z-steep")
    b = steep_bound(which)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MDP_FUSED", "0")
    with mdp.Engine(model_of(cs)) as eng:
        eng.set_cbound(b)
        got = eng.loglik_grid(cs.e, cs.c)
        launched = eng.launched()
    _series_ran("reading", launched)
    held(got, ref, cs, f"z-steep cbound {which} = {b!r} (kmax {STEEP_BOUNDS[which]})", bnd=fwd_ld.bound(cs.inp, cs.c, b))


def _columns(nc, must, groups, seed):
    """Sorted column indices: `must`, and `groups` whole groups of four
    consecutive columns drawn with `seed`."""
    rng = np.random.default_rng(seed)
    g = rng.choice(np.arange(1, nc // 4 - 1), size=groups, replace=False)
    return np.unique(np.concatenate([np.asarray(must), (4 * g[:, None] + np.arange(4)).ravel()]))


@pytest.mark.parametrize("nc,cb", [(512, 2), (1024, 4)])
def test_qrows_two_and_four_c_per_workgroup(nc, cb, monkeypatch):
    """z-flat on 12 e values x 512 and 1 024 c values up to the case's cmax,
    MDP_FUSED=0: k_qrows<8,0,2> and <8,0,4> (mdp_plan_grid's choice, asserted
    on what ran), whose lanes gather the eight coefficients across a quad and
    pick c per lane (cq at 4 c values).  The reference on 64 columns: the
    first and the last group of four and 14 groups between, so every
    position of a group."""
    cs, _ = case("z-flat")
    cmax = float(cs.c.max())
    c = np.linspace(cmax / 4, cmax, nc)
    assert c[-1] == cmax
    idx = _columns(nc, [0, 1, 2, 3, nc - 4, nc - 3, nc - 2, nc - 1], 14, 2500 + cb)
    assert idx.size == 64 and {int(i) % 4 for i in idx} == {0, 1, 2, 3}
    ref = fwd_ld.reference(cs.obs, cs.m, cs.p, cs.d, cs.e, c[idx])
    assert 2 * (ref >= fwd_ld.L_NORMAL).sum() >= ref.size
    bnd = fwd_ld.bound(cs.inp, c[idx])   # (idx holds the last column, cmax: the engine's split)
    assert bnd <= 2e-12
    big = fwd_ld.Case(f"z-flat-{nc}", cs.obs, cs.e, c, cs.m, cs.p, cs.d)
    got, launched, _ = run(big, monkeypatch, {"MDP_FUSED": "0"})
    assert f"k_qrows<8,0,{cb}>" in launched, launched
    held(got[:, idx], ref, big, f"z-flat {nc} c values {sorted(launched)}", bnd=bnd)


@pytest.mark.parametrize("nc", [130, 193])
def test_zrows_block_edges(nc, monkeypatch):
    """z-steep under MDP_WIDE=1 on 130 and 193 c values: k_zrows takes 128 a
    block (two per lane), so a second block in x with two live lanes in its
    first slot, and with one live lane in its second.  The reference on the
    columns at every edge."""
    cs, _ = case("z-steep")
    cmax = float(cs.c.max())
    c = np.linspace(cmax / 4, cmax, nc)
    assert c[-1] == cmax
    idx = np.unique([0, 1, 62, 63, 64, 65, 126, 127, 128, 129, nc - 2, nc - 1] + ([190, 191, 192] if nc > 192 else []))
    ref = fwd_ld.reference(cs.obs, cs.m, cs.p, cs.d, cs.e, c[idx])
    assert 2 * (ref >= fwd_ld.L_NORMAL).sum() >= ref.size
    bnd = fwd_ld.bound(cs.inp, c[idx])
    assert bnd <= 2e-12
    big = fwd_ld.Case(f"z-steep-{nc}", cs.obs, cs.e, c, cs.m, cs.p, cs.d)
    got, launched, _ = run(big, monkeypatch, {"MDP_WIDE": "1"})
    assert "k_zrows" in launched, launched
    held(got[:, idx], ref, big, f"z-steep {nc} c values {sorted(launched)}", bnd=bnd)


@pytest.mark.parametrize("name", ["z-steep", "z-flat"])
def test_series_fused_and_qrows_identical(name, monkeypatch):
    """The fused kernel's Horner and k_qrows' gathered one give the same
    bits (the claim of test_gpu_parity's test_fused_and_qrows_identical, here
    where the series carries Z).  The only test that can see an exchange
    among coefficients 7 and 8 on one side: their terms move L by less than
    any bound on it."""
    cs, _ = case(name)
    fused, lf, _ = run(cs, monkeypatch, SERIES_ENV["fused"])
    reading, lr, _ = run(cs, monkeypatch, SERIES_ENV["reading"])
    _series_ran("fused", lf)
    _series_ran("reading", lr)
    assert np.array_equal(fused, reading, equal_nan=True), np.argwhere(fused != reading)[:4].tolist()
