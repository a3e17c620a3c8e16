"""The posterior engine's grid planner (mdp_plan_grid, csrc/spom_plan.cpp) on
its own: `plan_check --grid NE NC NCU` plans one grid as mdp_engine_set_grid
would on a device of NCU compute units, without a device, and prints what it
decided -- the forward variant, the point list, k_qrows' c values per
workgroup, the wide paths' c chunks, every buffer size, the launch shape and
the kernel instantiations a run would note.  One table: each row asserts the
decision it is there for (never a digest), and goes through the program built
with the address and undefined-behaviour sanitizers as well.  The rows are
the seams tests/test_gpu_partition.py cuts its slabs at; tests/
test_gpu_grid_plan.py ties some of them to what a device then runs."""
from __future__ import annotations

import re
import subprocess

import pytest

from test_plan_host import INPUTS, PLAN_CHECK, inputs, sanitized  # noqa: F401  (inputs, sanitized: fixtures)

# 512 e values from 0 to 1.004: 255 on the s-form (254 * 1.004 / 511 < 0.5 <= 255 * 1.004 / 511), 257 on the t-form,
# so both runs of the point list are padded (2 points per lane)
ODD = ["--e", "0", "1.004"]
C8 = 8   # columns of the fused / reading rows (the variant does not depend on them)


# (id, input, options, grid arguments, {field: expected value or predicate})
ROWS = [
    # fused against reading: config 2's reading shape is 256 threads x 2 points, 512 e rows a block
    ("fused-512", "config2", "", ["512", C8, "256"],
     dict(variant="fused", gy=1, nlist=512, identity=1, ne_sform=256, kernels={"mdp_fwd_jit<fused,maxA7>"})),
    ("reading-513", "config2", "", ["513", C8, "256"], dict(variant="reading", gy=2, identity=0)),
    ("reading-514-list", "config2", "", ["512", C8, "256", *ODD],
     dict(variant="reading", gy=2, nlist=514, ne_sform=255, identity=0, listed=1)),
    ("fused-forced", "config2", "MDP_FUSED=1", ["512", C8, "256", *ODD], dict(variant="fused", nlist=514, gy=2)),
    ("fused-off", "config2", "MDP_FUSED=0", ["512", C8, "256"], dict(variant="reading", gy=1, identity=1)),
    # tall: an even number of e blocks and a workgroup for every CU
    ("tall-1024x1024", "config3", "", ["1024", "1024", "256"],
     dict(variant="tall", gy=2, block=512, kernels=lambda k: "mdp_fwd_jit<reading,kb512>" in k)),
    ("tall-1024x256", "config3", "", ["1024", "256", "256"], dict(variant="tall")),
    ("plain-1024x255", "config3", "", ["1024", "255", "256"], dict(variant="reading", block=256)),
    ("plain-1536x1024", "config3", "", ["1536", "1024", "256"], dict(variant="reading", gy=3)),
    ("tall-1024x128-128cu", "config3", "", ["1024", "128", "128"], dict(variant="tall")),
    ("never-tall-epl", "config3", "MDP_EPL=2", ["1024", "1024", "256"], dict(variant="reading")),
    ("never-tall-epl1", "config3", "MDP_EPL=1", ["1024", "1024", "256"], dict(variant="reading")),
    ("never-tall-kblock", "config3", "MDP_JIT_KBLOCK=256", ["1024", "1024", "256"], dict(variant="reading")),
    # k_qrows' c values per workgroup
    ("qrows-cb4", "config3", "", ["64", "1024", "256"], dict(qrows_cb=4, kernels=lambda k: "k_qrows<8,1,4>" in k)),
    ("qrows-cb2", "config3", "", ["64", "512", "256"], dict(qrows_cb=2, kernels=lambda k: "k_qrows<8,1,2>" in k)),
    ("qrows-cb1", "config3", "", ["64", "511", "256"], dict(qrows_cb=1, kernels=lambda k: "k_qrows<8,1,1>" in k)),
    ("qrows-nvar12", "highvar12", "", ["64", "1024", "256"], dict(qrows_cb=lambda v: v <= 2)),
    ("qrows-nvar16", "highvar16", "", ["64", "1024", "256"], dict(qrows_cb=lambda v: v <= 2)),
    ("qrows-nvar16-512", "highvar16", "", ["1024", "512", "256"],   # (two e blocks: not fused, so k_qrows runs)
     dict(qrows_cb=lambda v: v <= 2, kernels=lambda k: any(re.fullmatch(r"k_qrows<16,0,[12]>", x) for x in k))),
    ("qrows-nvar20", "highvar20", "", ["1024", "1024", "256"],
     dict(qrows_cb=1, kernels=lambda k: "k_qrows<24,0,1>" in k)),
    # the wide paths
    ("wide-hs", "s128", "", ["64", "64", "256"],
     dict(variant="-", pg_zero=1, kernels=lambda k: "k_fwd_hs<2,8>" in k and "k_zrows" in k)),
    ("wide-plain", "s128", "MDP_WIDE_MMA=0", ["64", "64", "256"],
     dict(pg_zero=0, v=lambda v: v == 2 * 128 * 64 * 256, kernels=lambda k: "k_fwd_wide" in k and "k_wq" in k)),
    ("wide-mmt", "s128", "MDP_WIDE_MMA=2", ["64", "64", "256"],
     dict(v=0, kernels=lambda k: "k_fwd_mmt<4,128,2buf>" in k)),
    ("wide-cb3", "s128", "MDP_WIDE_MMA=0;MDP_WIDE_CB=3", ["64", "7", "256"], dict(wide_cb_items=3, wide_cb_fwd=3)),
    ("wide-hs-cb3", "s128", "MDP_WIDE_CB=3", ["64", "7", "256"], dict(wide_cb_items=3, pg=lambda v: v % 3 == 0 and v > 0)),
    # Q rows built in HBM, and the generic path's buffers
    ("qglobal", "config2", "MDP_QGLOBAL=1", ["64", "7", "256"],
     dict(variant="reading", zg=7 * 80 + 1, kernels=lambda k: {"k_zrows", "k_wq", "k_witems<8>"} <= k)),
    ("generic", "manual", "MDP_JIT=0", ["8", "8", "256"],
     dict(variant="-", zpv=lambda v: v > 0, r=lambda v: v > 0, qrow=0, kernels=lambda k: "k_zpv" in k)),
]
# the point list itself: (id, input, grid arguments, number of s-form rows, points per lane)
LISTS = [
    ("ascending", "config2", ["37", "3", "256"], 18, 2),
    ("descending", "config2", ["37", "3", "256", "--e", "1", "0"], 18, 2),
    ("all-t-form", "config2", ["37", "3", "256", "--e", "0.5", "2"], 0, 2),
    ("odd-runs", "config2", ["512", "3", "256", *ODD], 255, 2),
    ("epl4", "config2", ["37", "3", "256"], 18, 4),
]

GRID = re.compile(
    r"^grid (?P<variant>\S+) \| gy (?P<gy>\d+) nlist (?P<nlist>\d+) epl (?P<epl>\d+) identity (?P<identity>[01]) "
    r"ne_sform (?P<ne_sform>\d+) \| qrows_cb (?P<qrows_cb>\d+) wide_cb_items (?P<wide_cb_items>\d+) "
    r"wide_cb_fwd (?P<wide_cb_fwd>\d+) \| kmax (?P<kmax>\d+) ct_len (?P<ct_len>\d+) zrows_lds (?P<zrows_lds>\d+) \| "
    r"launch nblk (?P<nblk>\d+) threads (?P<threads>\d+) pro (?P<pro>\d+) block (?P<block>\d+) lds (?P<lds>\d+) "
    r"nlist (?P<fwd_nlist>\d+) listed (?P<listed>[01]) \| buf qrow (?P<qrow>\d+) zg (?P<zg>\d+) pg (?P<pg>\d+) "
    r"pg_zero (?P<pg_zero>[01]) v (?P<v>\d+) vscr (?P<vscr>\d+) ldv (?P<ldv>\d+) zpv (?P<zpv>\d+) r (?P<r>\d+) "
    r"gpart (?P<gpart>\d+) stamps (?P<stamps>\d+,\d+,\d+) \| kernels (?P<kernels>\S+) \| fnv plist (?P<f_plist>[0-9a-f]{16}) "
    r"elist (?P<f_elist>[0-9a-f]{16}) zs (?P<f_zs>[0-9a-f]{16}) zsq (?P<f_zsq>[0-9a-f]{16}) zc (?P<f_zc>[0-9a-f]{16}) "
    r"coltab (?P<f_coltab>[0-9a-f]{16})$")
TEXT = ("variant", "stamps", "kernels", "f_plist", "f_elist", "f_zs", "f_zsq", "f_zc", "f_coltab")


def plan_grid(exe, paths, name, options, grid, extra=()):
    """plan_check --grid over one input: the completed process."""
    _, m, d = INPUTS[name]
    return subprocess.run([str(exe), "--grid", *map(str, grid), *extra, str(paths[name]), str(m), str(d), options],
                          capture_output=True, text=True, timeout=120)


def parse(r):
    """The fields of the grid line (numbers as int, kernels as a set) and the point list, if printed."""
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.strip().split("\n")
    assert lines[0].startswith("path "), r.stdout
    m = GRID.match(lines[1])
    assert m, lines[1]
    f = {k: v if k in TEXT else int(v) for k, v in m.groupdict().items()}
    f["kernels"] = set() if f["kernels"] == "-" else set(f["kernels"].split(";"))
    plist = [int(v) for v in lines[2].split()[1:]] if len(lines) > 2 and lines[2].startswith("plist") else None
    return f, plist


def _check(r, want):
    f, _ = parse(r)
    for k, w in want.items():
        assert w(f[k]) if callable(w) else f[k] == w, (k, f[k], r.stdout)
    return f


IDS = [row[0] for row in ROWS]


@pytest.mark.parametrize("rid,name,options,grid,want", ROWS, ids=IDS)
def test_grid_decisions(inputs, rid, name, options, grid, want):   # noqa: F811
    f = _check(plan_grid(PLAN_CHECK, inputs, name, options, grid), want)
    if f["variant"] != "-":   # the launch covers the list: whole lanes, whole blocks
        assert f["nlist"] % f["epl"] == 0
        assert f["threads"] * f["pro"] % f["block"] == 0 and f["nblk"] > 0


@pytest.mark.parametrize("rid,name,options,grid,want", ROWS, ids=IDS)
def test_grid_decisions_sanitized(inputs, sanitized, rid, name, options, grid, want):   # noqa: F811
    """The same row through the sanitized program: exit 0, the same decision, nothing on stderr."""
    r = plan_grid(sanitized, inputs, name, options, grid, ["--list"])
    _check(r, want)
    assert r.stderr == "", r.stderr


def _sform(grid):
    """s-form rows of the grid's e axis, by the kernels' test (x = min(e, 1), x < 1 - x) on mdp_grid's values."""
    ne = int(grid[0])
    lo, hi = (float(grid[grid.index("--e") + 1]), float(grid[grid.index("--e") + 2])) if "--e" in grid else (0.0, 1.0)
    win = (hi - lo) / (ne - 1)
    e = [i * win + lo for i in range(ne - 1)] + [hi]
    return [i for i, v in enumerate(e) if min(v, 1.0) < 1.0 - min(v, 1.0)]


@pytest.mark.parametrize("rid,name,grid,ns,epl", LISTS, ids=[row[0] for row in LISTS])
def test_point_list(inputs, rid, name, grid, ns, epl):   # noqa: F811
    """The listed rows without bit 31 are every row once, all s-form rows then all t-form rows, each in grid order;
    each run is padded to whole lanes with bit-31 duplicates of its own last row."""
    ne = int(grid[0])
    f, plist = parse(plan_grid(PLAN_CHECK, inputs, name, f"MDP_EPL={epl}" if epl != 2 else "", grid, ["--list"]))
    s_rows = _sform(grid)
    t_rows = [i for i in range(ne) if i not in set(s_rows)]
    assert len(s_rows) == ns and f["ne_sform"] == ns and f["epl"] == epl
    want = []
    for rows in (s_rows, t_rows):
        want += rows + [rows[-1] | 1 << 31 for _ in range(-len(rows) % epl)]
    assert plist == want
    assert f["nlist"] == len(plist) and len(plist) % epl == 0
    assert sorted(v for v in plist if not v >> 31) == list(range(ne))
    assert f["identity"] == int(plist == list(range(len(plist))))
    if rid == "odd-runs":   # two duplicates, each naming the last row of its own run
        assert [v & 0x7fffffff for v in plist if v >> 31] == [254, 511] and f["nlist"] == 514


def test_empty_grid_lists_one_lane(inputs):   # noqa: F811
    f, plist = parse(plan_grid(PLAN_CHECK, inputs, "config2", "", ["0", "3", "256"], ["--list"]))
    assert plist == [1 << 31] * f["epl"] and f["epl"] == 2 and f["kernels"] == set()


@pytest.mark.parametrize("hi,shown", [("-1", "-1"), ("nan", "nan"), ("inf", "inf")])
def test_refused_c(inputs, hi, shown):   # noqa: F811
    """One column at c = hi: refused as mdp_engine_set_grid refuses it."""
    r = plan_grid(PLAN_CHECK, inputs, "config2", "", ["4", "1", "256", "--c", "0", hi])
    assert r.returncode == 1 and "\ngrid " not in r.stdout
    assert r.stderr.strip() == f"plan_check: colonisation rate c[0] = {shown} (the engine takes finite c >= 0)"


def test_c_tables_follow_the_bound(inputs):   # noqa: F811
    """The c tables depend on the |c| bound alone: a column slab under the full grid's bound has the full grid's
    tables, and config 3's Z rows keep more explicit columns under a larger bound."""
    def tables(grid):
        f, _ = parse(plan_grid(PLAN_CHECK, inputs, "config3", "", grid))
        return {k: f[k] for k in ("kmax", "ct_len", "f_zs", "f_zsq", "f_zc", "f_coltab")}
    full = tables(["64", "64", "256"])
    slab = tables(["64", "16", "256", "--c", "0", "0.25", "--cbound", "1"])
    assert slab == full
    assert tables(["64", "16", "256", "--c", "0", "0.25"])["f_zs"] != full["f_zs"]
    assert tables(["64", "64", "256", "--cbound", "4"])["f_zs"] != full["f_zs"]
