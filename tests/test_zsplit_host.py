"""z_split's Z-row tables (csrc/spom_plan.cpp) read back through `plan_check
--grid ... --ztables` and held to their definition on the inputs of
tests/fwd_ld.py -- not to a digest:

* the partition: every always-zero column of every row is exactly one of
  dropped (cmax S <= 2^-55), small (2^-55 < cmax S <= 2^-7) or large, on
  fl(cmax S) in double; the large ones stored with the row's largest S first,
  zero padding, kmax = the longest row rounded up to 8, k_qrows' chain-major
  copy the same slots;
* both thresholds to the last bit: at a cmax with fl(cmax S) == 2^-7 for one
  reachable (row, column) that column is small, at the next double above it is
  large; at 2^-55 dropped, then small;
* the eight series coefficients P_i / i against a long-double sum.  Their
  tolerance is counted from z_split's code: pw[i] += t is one addition per
  small column (ns), t = S^(i+1) took i multiplications, and the division by
  i + 1: ns + i + 1 roundings of at most u = 2^-53 each on non-negative terms,
  so |coef - exact| <= gamma(ns + i + 1) exact, gamma(k) = k u / (1 - k u)
  (plus k 2^-64 for the long-double sum itself).  This is what holds P7 / 7
  and P8 / 8, whose terms sit below the rounding floor of any comparison of L;
* kmax of the z-steep case under the |c| bounds tests/test_gpu_forward_ld.py
  ::test_class_boundary_moves runs it with (the engine reports no kmax).

One dump also goes through the program built with the address and
undefined-behaviour sanitizers."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import fwd_ld
from fwd_ld import LD, U, Z_DROP, Z_TAU
from test_plan_host import PLAN_CHECK, sanitized  # noqa: F401  (sanitized: a fixture)

pytestmark = pytest.mark.skipif(not fwd_ld.OK, reason=fwd_ld.SKIP_REASON)


def dump(exe, tmp_path, cs, cmax, options="", cbound=None):
    """plan_check --ztables of the case's problem on a one-column grid c =
    (cmax): (kmax, {hidden state: (columns, zs, zsq, coef)}, the process)."""
    path = tmp_path / f"{cs.name}.txt"
    if not path.exists():
        np.savetxt(path, cs.obs, fmt="%d")
    args = [str(exe), "--grid", "2", "1", "256", "--c", "0", float(cmax).hex()]
    if cbound is not None:
        args += ["--cbound", float(cbound).hex()]
    r = subprocess.run([*args, "--ztables", str(path), repr(cs.m), repr(cs.d), options], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.strip().split("\n")
    assert lines[0].startswith("path ") and lines[1].startswith("grid "), r.stdout
    head = lines[2].split()
    assert (head[0], head[1], head[3], head[5]) == ("ztables", "nj", "kmax", "cmax"), lines[2]
    nj, kmax = int(head[2]), int(head[4])
    assert float.fromhex(head[6]) == max(float(cmax), float(cbound or 0.0))
    rows = {}
    assert len(lines) == 3 + nj, r.stdout
    for i, ln in enumerate(lines[3:]):
        zs, zsq, zc = ln.split(" | ")
        f = zs.split()
        assert f[0] == "zrow" and int(f[1]) == i and f[2] == "bits" and f[4] == "nl" and f[6] == "zs", ln
        slots = [s.split(":") for s in f[7:]]
        assert len(slots) == kmax and int(f[5]) == sum(1 for k, _ in slots if k != "-"), ln
        cols = [None if k == "-" else int(k) for k, _ in slots]
        q, c = zsq.split(), zc.split()
        assert q[0] == "zsq" and len(q) == 1 + kmax and c[0] == "zc" and len(c) == 9, ln
        assert int(f[3]) not in rows
        rows[int(f[3])] = (cols, [float.fromhex(v) for _, v in slots], [float.fromhex(v) for v in q[1:]],
                           [float.fromhex(v) for v in c[1:]])
    return kmax, rows, r


def classes(inp, j, cmax):
    """(dropped, small, large) always-zero columns of row j by the documented
    thresholds on fl(cmax S) in double."""
    out = ([], [], [])
    for k in fwd_ld.nonvar_cols(inp):
        x = float(cmax) * float(inp.S[j, k])
        out[0 if x <= Z_DROP else 1 if x <= Z_TAU else 2].append(k)
    return out


def verify(inp, kmax, rows, cmax):
    """The whole dump against the definition; returns the largest coefficient
    error as a fraction of its tolerance."""
    assert tuple(sorted(rows)) == fwd_ld.reachable_rows(inp)
    longest, worst = 0, 0.0
    for j, (cols, zs, zsq, coef) in rows.items():
        dropped, small, large = classes(inp, j, cmax)
        assert sorted(dropped + small + large) == fwd_ld.nonvar_cols(inp)
        # the large columns in ascending order, the first exchanged with the row's (first) largest S
        want = list(large)
        if want:
            i = max(range(len(want)), key=lambda i: (float(inp.S[j, want[i]]), -i))
            want[0], want[i] = want[i], want[0]
            assert float(inp.S[j, want[0]]) == max(float(inp.S[j, k]) for k in large)
        nl = len(want)
        assert cols[:nl] == want and cols[nl:] == [None] * (kmax - nl), (j, cols, want)
        assert zs[:nl] == [float(inp.S[j, k]) for k in want], j
        assert all(v == 0.0 and not np.signbit(v) for v in zs[nl:]), (j, zs)
        assert kmax % 8 == 0 and all(zsq[(k % 4) * (kmax // 4) + k // 4] == zs[k] for k in range(kmax)), j
        longest = max(longest, nl)
        ns = len(small)
        if not ns:
            assert coef == [0.0] * 8, (j, coef)
            continue
        s = inp.S[j, small].astype(LD)
        for i in range(8):
            exact = (s ** (i + 1)).sum() / LD(i + 1)
            k = ns + i + 1   # ns additions, i multiplications, one division (module docstring)
            tol = (LD(k) * LD(U) / (1 - LD(k) * LD(U)) + LD(k) * LD(2.0) ** -64) * exact
            err = abs(LD(coef[i]) - exact)
            assert err <= tol, f"row {j} coef[{i}] = {coef[i]!r}: off by {float(err / exact):.3e} relative, tolerance {float(tol / exact):.3e}"
            worst = max(worst, float(err / tol))
    assert kmax == (longest + 7) // 8 * 8
    return worst


def _case(name):
    return fwd_ld.cases()[name]


@pytest.mark.parametrize("name,options", [("z-steep", ""), ("z-steep", "MDP_FUSED=0"), ("z-steep", "MDP_WIDE=1"),
                                          ("z-flat", ""), ("z-flat-wide", ""), ("z-drop", ""), ("z-drop0", ""), ("a1", "")])
def test_tables_at_the_cases_bound(name, options, tmp_path):
    """The tables of each series case at its own cmax, on the fused-capable,
    the reading and the wide plan (one z_split behind all three); a1's rows
    have no small column: all eight coefficients are zero."""
    cs = _case(name)
    cmax = float(cs.c.max())
    kmax, rows, _ = dump(PLAN_CHECK, tmp_path, cs, cmax, options)
    frac = verify(cs.inp, kmax, rows, cmax)
    nsmall = max(len(classes(cs.inp, j, cmax)[1]) for j in rows)
    print(f"\n{name} {options}: kmax {kmax}, {len(rows)} rows, up to {nsmall} small columns, coefficients {frac:.3f} of the tolerance")
    if name == "a1":
        assert nsmall == 0 and all(r[3] == [0.0] * 8 for r in rows.values()) and kmax == 8
    if name == "z-drop0":
        assert kmax == 0 and nsmall == 0
    if name == "z-steep":
        assert kmax == 8 and nsmall >= 30


@pytest.mark.parametrize("name,value", [("z-steep", Z_TAU), ("z-flat", Z_TAU), ("z-drop0", Z_DROP)])
def test_thresholds_to_the_last_bit(name, value, tmp_path):
    """fl(cmax S[j][k]) == the threshold: the column is in the lower class
    (small at 2^-7, dropped at 2^-55); at the next double above cmax the
    product is above the threshold and the column in the upper class (large,
    small).  cmax is the largest double with that product (fwd_ld.edge_c)."""
    cs = _case(name)
    inp = cs.inp
    cmax, j, k = fwd_ld.edge_c(inp, value, (lambda s: abs(Z_TAU / s - 0.73)) if name == "z-steep" else (lambda s: -s))
    assert cmax == float(cs.c.max()) and cmax * float(inp.S[j, k]) == value
    up = float(np.nextafter(cmax, np.inf))
    assert up * float(inp.S[j, k]) > value
    at = {}
    for c in (cmax, up):
        kmax, rows, _ = dump(PLAN_CHECK, tmp_path, cs, c)
        verify(inp, kmax, rows, c)
        at[c] = rows[j]
    if value == Z_TAU:
        assert k not in at[cmax][0] and k in at[up][0]
        # the column's S leaves P1 as it becomes explicit
        assert at[cmax][3][0] - at[up][3][0] == pytest.approx(float(inp.S[j, k]), rel=1e-12)
    else:
        assert at[cmax][3] == [0.0] * 8 and k not in at[cmax][0]
        assert at[up][3][0] >= float(inp.S[j, k]) and k not in at[up][0]


def test_cmax_zero(tmp_path):
    """cmax = 0: everything dropped, no explicit column, no coefficient."""
    cs = _case("z-steep")
    kmax, rows, _ = dump(PLAN_CHECK, tmp_path, cs, 0.0)
    assert kmax == 0 and verify(cs.inp, kmax, rows, 0.0) == 0.0
    assert all(r[3] == [0.0] * 8 and r[1] == [] for r in rows.values())


# the |c| bounds of tests/test_gpu_forward_ld.py::test_class_boundary_moves on z-steep and the kmax of each
STEEP_BOUNDS = {"cmax": 8, "next": 16, "double": 16, "kmax32": 32, "kmax40": 40, "explicit": 64}


def steep_bound(which):
    cs = _case("z-steep")
    cmax = float(cs.c.max())
    pos = cs.inp.S[list(fwd_ld.reachable_rows(cs.inp))][:, fwd_ld.nonvar_cols(cs.inp)]
    return {"cmax": cmax, "next": float(np.nextafter(cmax, np.inf)), "double": 2 * cmax, "kmax32": 2.0 ** 14, "kmax40": 2.0 ** 20,
            "explicit": 2.0 * Z_TAU / float(pos[pos > 0].min())}[which]


@pytest.mark.parametrize("which", list(STEEP_BOUNDS))
def test_steep_kmax_under_a_bound(which, tmp_path):
    """z-steep's tables under mdp_engine_set_cbound's value (--cbound): the
    split follows the bound, and kmax is the figure the GPU test relies on
    (32: k_qrows' long-row loop runs once without its trailing pair, 40: with
    it, 64: every column explicit)."""
    cs = _case("z-steep")
    b = steep_bound(which)
    kmax, rows, _ = dump(PLAN_CHECK, tmp_path, cs, float(cs.c.max()), "MDP_FUSED=0", cbound=b)
    verify(cs.inp, kmax, rows, b)
    assert kmax == STEEP_BOUNDS[which]
    if which == "explicit":
        assert all(r[3] == [0.0] * 8 for r in rows.values())
        assert all(len(classes(cs.inp, j, b)[2]) == (60 if j else 0) for j in rows)


@pytest.mark.parametrize("nc,cb", [(511, 1), (512, 2), (1024, 4)])
def test_flat_qrows_cb(nc, cb, tmp_path):
    """mdp_plan_grid's c values per k_qrows workgroup on z-flat's 12 x nc
    grids (tests/test_gpu_forward_ld.py::test_qrows_two_and_four_c_per_workgroup
    asserts the instantiation that ran)."""
    cs = _case("z-flat")
    path = tmp_path / "z-flat.txt"
    np.savetxt(path, cs.obs, fmt="%d")
    r = subprocess.run([str(PLAN_CHECK), "--grid", "12", str(nc), "256", "--c", "0", float(cs.c.max()).hex(), str(path),
                        repr(cs.m), repr(cs.d), "MDP_FUSED=0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"| qrows_cb {cb} " in r.stdout and f"k_qrows<8,0,{cb}>" in r.stdout, (r.stdout, r.stderr)


def test_dump_sanitized(sanitized, tmp_path):   # noqa: F811
    """The same dump through the sanitized program: the same text, nothing on stderr."""
    cs = _case("z-steep")
    cmax = float(cs.c.max())
    _, _, plain = dump(PLAN_CHECK, tmp_path, cs, cmax)
    kmax, rows, r = dump(sanitized, tmp_path, cs, cmax)
    verify(cs.inp, kmax, rows, cmax)
    assert r.stdout == plain.stdout and r.stderr == ""


def test_lines_without_the_flag_unchanged(tmp_path):
    """--ztables only adds lines after the existing ones."""
    cs = _case("z-flat")
    _, _, r = dump(PLAN_CHECK, tmp_path, cs, float(cs.c.max()))
    args = [a for a in r.args if a != "--ztables"]
    bare = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert bare.returncode == 0 and r.stdout.startswith(bare.stdout) and len(bare.stdout.strip().split("\n")) == 2
