"""The exact scenario engine's host planner (csrc/spom_scenario_plan.cpp) on
its own: _build/scenario_plan_check plans one survey row and one grid without
a device or the HIP runtime.

1. Its digest restated in numpy for every kernel the row length and the
   options select: the colonisation sums S, the prior vector w, the hi factor
   offsets, the longest-processing-time-first wave schedule, the row order and
   both LDS formulas.  The dispersal table, the source row and the float
   priors are those of tests/scnsim_ref.py, which the scenario simulator's
   digests (test_scnsim_host.py) pin too: the two engines share one copy.
2. The launch lists of both passes on each path.
3. Every refusal that needs no device, through the driver and -- where the
   ABI reaches it before the device check -- through mdp.Scenario.
4. Three of the digest cases again through the driver built with the address
   and undefined-behaviour sanitizers.
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

import midaspom_amd as mdp
import scnsim_ref as ref

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "midaspom_amd" / "csrc"
PLAN_CHECK = ROOT / "midaspom_amd" / "_build" / "scenario_plan_check"

# the 12-entry ROW of test_gpu_scenario_sweep.py, extended to 16
ROW = np.array([1, -1, 0, 1, 0, -1, 1, 1, 0, 1, -1, 0, 1, 0, -1, 1], dtype=np.int32)
M, P, D = 400.0, 0.5, 100.0
WAVES, E_PER_WG, ROW_BLOCK = 16, 32, 256

# (n, options, the kernel the planner must name)
CASES = [
    (1, "", "k_scn<1,0>"), (2, "", "k_scn<2,0>"), (3, "", "k_scn<3,0>"), (4, "", "k_scn<3,1>"),
    (8, "", "k_scn<3,5>"), (9, "", "k_scn_row"), (12, "", "k_scn_row"), (13, "", "k_scn_big"),
    (16, "", "k_scn_big"),
    (3, "MDP_SCN_ROW=1", "k_scn_row"), (8, "MDP_SCN_ROW", "k_scn_row"),
    (3, "MDP_SCN_BIG=1", "k_scn_big"), (8, "MDP_SCN_BIG", "k_scn_big"),
    (3, "MDP_SCN_BIG=0;MDP_SCN_ROW=0", "k_scn<3,0>"), (8, "MDP_SCN_BIG=0, MDP_SCN_ROW=0", "k_scn<3,5>"),
    (8, "MDP_SCN_BIG=1;MDP_SCN_ROW=1", "k_scn_big"),
    (13, "MDP_SCN_ROW=1", "k_scn_big"),  # the row kernel holds n <= 12: falls through
]
SAN_CASES = [CASES[4], CASES[6], CASES[8]]  # one per path: n = 8 lds, n = 12 row, n = 16 big


def fnv(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def row_text(row):
    return "".join("m" if v == -1 else "-" if v == -2 else str(int(v)) for v in row)


def plan(row, kind=1, options="", grid=(5, 2, 3, 2), years=(), exe=PLAN_CHECK):
    return subprocess.run([str(exe), row_text(row), repr(M), repr(P), repr(D), str(kind), options,
                           *(str(g) for g in grid), *(str(y) for y in years)], capture_output=True, text=True,
                          timeout=120)


def popcount(x):
    return bin(x).count("1")


def tables(row, p):
    """(S, w) of a row: S[j][k] the sum over l != k, ascending and with the
    zero terms added, of M[l][k] * (bit n-1-l of j); w[state] the float prior
    of the completion with that state, as a double."""
    n = len(row)
    ns = 1 << n
    Mx = ref.dispersal(n, M, D)
    bits = ((np.arange(ns)[:, None] >> (n - 1 - np.arange(n))[None, :]) & 1).astype(np.float64)  # [j, l]
    S = np.zeros((ns, n))
    for k in range(n):
        s1 = np.zeros(ns)
        for l in range(n):  # one add per l: numpy's own reductions sum pairwise
            if l != k:
                s1 = s1 + Mx[l, k] * bits[:, l]
        S[:, k] = s1
    pr = ref.priors(int((row == -1).sum()), p)
    w = np.zeros(ns)
    for k in range(pr.size):
        comp = ref.completion(row, k)
        w[sum(int(comp[j]) << (n - 1 - j) for j in range(n))] += float(pr[k])
    return S, w


def lds_tables(n):
    """(boff, btot, jsched, nsched, LDS bytes) of k_scn<NL, NH>."""
    nl = min(3, n)
    nh = n - nl
    boff, off = [], 0
    for jh in range(1 << nh):
        boff.append(off)
        off += (1 << (nh - popcount(jh))) << nl

    def cost(jh):
        f = nh - popcount(jh)
        return (1 << (f - 1) if f else 1) + 1
    rows = sorted(range(1 << nh), key=lambda jh: -cost(jh))  # stable
    waves, load = [[] for _ in range(WAVES)], [0] * WAVES
    for jh in rows:
        g = load.index(min(load))  # the first least-loaded wave
        waves[g].append(jh)
        load[g] += cost(jh)
    nsched = max(len(v) for v in waves)
    jsched = np.full((WAVES, nsched), 0xffffffff, dtype=np.uint32)
    for g, v in enumerate(waves):
        jsched[g, :len(v)] = v
    na = ((3 ** nl + 1) & ~1) << nh
    lds = (2 * ((1 << n) * E_PER_WG + (2 << nl)) + na + off + (1 << nl)) * 8
    return np.array(boff, dtype=np.uint32), off, jsched, nsched, lds


def expected_head(row, kind, kernel, p=P):
    """The first three lines of the driver."""
    n = len(row)
    ns = 1 << n
    S, w = tables(row, p)
    empty = np.zeros(0, dtype=np.uint32)
    boff, btot, jsched, nsched, lds, jord = empty, 0, empty, 0, 0, empty
    if kernel == "k_scn_row":
        jord = np.array(sorted(range(ns), key=popcount), dtype=np.uint32)  # stable: ascending j within a count
        lds = (2 * ns + 3 * n * ROW_BLOCK) * 8
    elif kernel != "k_scn_big":
        boff, btot, jsched, nsched, lds = lds_tables(n)
    return [f"kernel {kernel}",
            f"plan n {n} ns {ns} nsched {nsched} btot {btot} lds {lds}",
            f"S {fnv(S.tobytes()):016x} w {fnv(w.tobytes()):016x} boff {fnv(boff.tobytes()):016x} "
            f"jsched {fnv(jsched.tobytes()):016x} jord {fnv(jord.tobytes()):016x}"]


def expected_src(n, kind, nd):
    src = np.zeros((nd, n))
    if kind == 1:
        for i in range(nd):
            src[i] = ref.source_row(n, M, 250.0 * (i + 1))
    return fnv(src.tobytes())


IDS = [f"n{n}-{o or 'default'}" for n, o, _ in CASES]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n,options,kernel", CASES, ids=IDS)
def test_plan_digest(n, options, kernel, kind):
    row = ROW[:n]
    r = plan(row, kind, options)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[:3] == expected_head(row, kind, kernel)
    if n == 8 and kernel == "k_scn<3,5>":
        assert " lds 154112" in lines[1]
    nd = 2 if kind else 1
    assert lines[3].startswith(f"grid ne 5 nc 2 nK 3 nd {nd} src {expected_src(n, kind, nd):016x} nV {2 * (1 << n) * 5} ")


def test_priors_follow_p():
    """p != 1/2, so that the order of a prior's float factors shows."""
    row = ROW[:8]
    r = subprocess.run([str(PLAN_CHECK), row_text(row), repr(M), "0.3", repr(D), "0", "", "5", "2", "3", "1"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[:3] == expected_head(row, 0, "k_scn<3,5>", p=0.3)


def launches(r):
    """{mode: [(p0, points, workgroups)]} and the grid line's fields."""
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    g = lines[3].split()
    grid = {g[i]: g[i + 1] for i in range(1, len(g), 2)}
    out = {0: [], 1: []}
    for ln in lines[4:]:
        f = ln.split()
        assert f[0] == "launch" and f[1] == "mode" and f[3] == "p0" and f[5] == "points" and f[7] == "workgroups"
        out[int(f[2])].append((int(f[4]), int(f[6]), int(f[8])))
    return out, grid


@pytest.mark.parametrize("kind,grid", [(0, (33, 2, 3, 7)), (1, (33, 2, 3, 2)), (1, (64, 5, 41, 20))])
def test_launches_lds(kind, grid):
    ne, nc, nK, nd = grid
    nd = nd if kind else 1  # a die-off grid has no distance axis
    got, g = launches(plan(ROW[:4], kind, "", grid))
    chunks = (ne + 31) // 32
    assert got == {0: [(0, ne * nc, chunks * nc)], 1: [(0, ne * nc * nK * nd, chunks * nc * nK * nd)]}
    assert int(g["nd"]) == nd and int(g["nV"]) == nc * 16 * ne and int(g["nY"]) == 0 and int(g["big_pts"]) == 0


def test_launches_row():
    # 600 points (30 x 10 x 2), a 300-point first pass, at most 256 points per launch
    got, _ = launches(plan(ROW[:3], 0, "MDP_SCN_ROW=1;MDP_SCN_LAUNCH_PTS=256", (30, 10, 2, 1)))
    assert got == {0: [(0, 256, 256), (256, 44, 44)], 1: [(0, 256, 256), (256, 256, 256), (512, 88, 88)]}
    got, _ = launches(plan(ROW[:6], 1, "MDP_SCN_ROW=1;MDP_SCN_LAUNCH_PTS=1", (7, 1, 1, 1)))
    assert got == {m: [(i, 1, 1) for i in range(7)] for m in (0, 1)}
    got, _ = launches(plan(ROW[:9], 1, "", (25, 12, 1, 2)))  # no cap: 2^22 points per launch
    assert got == {0: [(0, 300, 300)], 1: [(0, 600, 600)]}
    got, _ = launches(plan(ROW[:3], 0, "MDP_SCN_ROW=1;MDP_SCN_LAUNCH_PTS=0", (30, 10, 2, 1)))  # 0: no cap
    assert got == {0: [(0, 300, 300)], 1: [(0, 600, 600)]}
    got, _ = launches(plan(ROW[:3], 0, "MDP_SCN_ROW=1", ((1 << 22) + 5, 1, 1, 1)))
    assert got[1] == [(0, 1 << 22, 1 << 22), (1 << 22, 5, 5)]


def test_launches_big():
    # the cap is rounded up to whole blocks of 256 lanes: 200 -> 256, 257 -> 512
    got, g = launches(plan(ROW[:3], 0, "MDP_SCN_BIG=1;MDP_SCN_LAUNCH_PTS=200", (30, 10, 2, 1)))
    assert got == {0: [(0, 256, 1), (256, 44, 1)], 1: [(0, 256, 1), (256, 256, 1), (512, 88, 1)]}
    assert int(g["big_pts"]) == 256 and int(g["nY"]) == 2 * 8 * 256
    got, g = launches(plan(ROW[:3], 0, "MDP_SCN_BIG=1;MDP_SCN_LAUNCH_PTS=257", (30, 10, 2, 1)))
    assert got == {0: [(0, 300, 2)], 1: [(0, 512, 2), (512, 88, 2)]} and int(g["big_pts"]) == 512
    # no cap, a small grid: one launch of the points rounded up to whole blocks
    got, g = launches(plan(ROW[:3], 0, "MDP_SCN_BIG=1", (30, 10, 2, 1)))
    assert got == {0: [(0, 300, 3)], 1: [(0, 600, 3)]} and int(g["big_pts"]) == 768
    # no cap at the real size: 1 GiB of scratch holds 262 144 points of two 2^8-state vectors
    got, g = launches(plan(ROW[:8], 1, "MDP_SCN_BIG=1", (64, 5, 41, 20)))
    assert int(g["big_pts"]) == 262144 and int(g["nY"]) == 2 * 256 * 262144
    assert got == {0: [(0, 320, 1024)], 1: [(0, 262144, 1024), (262144, 256, 1024)]}
    # n = 16: 1024 points per launch
    got, g = launches(plan(ROW[:16], 0, "", (64, 5, 41, 1)))
    assert int(g["big_pts"]) == 1024 and got[1][-1] == (12288, 64 * 5 * 41 - 12288, 4) and len(got[1]) == 13


def test_empty_grid():
    got, g = launches(plan(ROW[:4], 1, "", (5, 0, 3, 2)))
    assert got == {0: [], 1: []} and [g[k] for k in ("ne", "nc", "nK", "nd")] == ["0"] * 4


# ---------------------------------------------------------------------------
# refusals without a device
# ---------------------------------------------------------------------------
def refused_by_driver(text, *a, **kw):
    r = plan(*a, **kw)
    assert r.returncode == 1 and r.stderr.startswith("scenario_plan_check: ") and text in r.stderr, (r.stdout, r.stderr)
    return r


def test_driver_refusals():
    row = ROW[:5]
    refused_by_driver("null argument", row[:0])
    refused_by_driver("observation 2 not in {-1,0,1}", np.array([0, 2, 1]))
    refused_by_driver("observation -2 not in {-1,0,1}", np.array([0, -2, 1]))
    refused_by_driver("17 patches: the scenario engine takes n <= 16 (2^n states)", np.ones(17, dtype=int))
    refused_by_driver("unknown scenario option 'MDP_SCN_WIDE'", row, options="MDP_SCN_WIDE=1")
    refused_by_driver("unknown scenario option 'MDP_SIM_NM'", row, options="MDP_SCN_BIG=1;MDP_SIM_NM=8")
    # today's order: the options before the row's length and values
    refused_by_driver("unknown scenario option 'X'", np.ones(17, dtype=int), options="X")
    refused_by_driver("17 patches", np.full(17, 2), options="MDP_SCN_BIG")
    refused_by_driver("negative number of years", row, years=(-1, 2))
    refused_by_driver("negative number of years", row, years=(3, -1))
    for i in range(3):
        grid = ["5", "2", "3", "2"]
        grid[i] += "!"
        refused_by_driver("null argument", row, grid=grid)
    refused_by_driver("null source distances", row, kind=1, grid=("5", "2", "3", "2!"))
    assert plan(row, 0, "", ("5", "2", "3", "2!")).returncode == 0  # die-off reads no distances
    assert plan(row, 1, "", ("0!", "2", "3", "2")).returncode == 0  # an empty axis may be null


def test_grid_too_large_is_not_wrapped():
    row = ROW[:5]
    # the workgroups of the second pass, ceil(ne/32) nc nK nd, must stay below 2^31
    assert plan(row, 1, "", (32, 1 << 15, 1 << 15, 1)).returncode == 0  # 2^30
    refused_by_driver("grid of 68719476736 points too large", row, grid=(32, 1 << 16, 1 << 15, 1))  # 2^31
    # 2^26 2^31 2^31 2^20 = 2^108 and, die-off, 2^26 2^31 2^31 = 2^88: both 0 modulo 2^64
    r = refused_by_driver("points too large", row, kind=1, grid=(1 << 31, 1 << 31, 1 << 31, 1 << 20))
    assert f"grid of {2 ** 113} points" in r.stderr
    r = refused_by_driver("points too large", row, kind=0, grid=(1 << 31, 1 << 31, 1 << 31, 1 << 31))
    assert f"grid of {2 ** 93} points" in r.stderr


def test_abi_refusals():
    """What mdp_scenario_create_opts refuses before it asks for a device."""
    def refused(code, text, row, **kw):
        with pytest.raises(mdp.MidaspomError, match=code) as ei:
            mdp.Scenario(np.asarray(row, dtype=np.int32), **kw)
        assert text in str(ei.value)
    refused("EINVAL", "null argument", [])
    refused("EINVAL", "observation 2 not in", [0, 2, 1])
    refused("EINVAL", "observation -2 not in", [0, -2, 1], kind="loss")
    refused("EUNSUPPORTED", "17 patches", np.ones(17))
    refused("EINVAL", "unknown scenario option 'MDP_SIM_NM'", ROW[:5], options="MDP_SIM_NM=8")
    refused("EINVAL", "unknown scenario option 'X'", np.ones(17), options={"MDP_SCN_BIG": 0, "X": 1})
    if mdp.device_count() == 0:  # a row that passes every refusal reaches the device check
        refused("ENODEV", "no HIP device", ROW[:5], options={"MDP_SCN_BIG": 0, "MDP_SCN_ROW": 0})


# ---------------------------------------------------------------------------
# the same driver under the host sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """scenario_plan_check built with -fsanitize=address,undefined (make scenario_plan_check_san)."""
    tmp = tmp_path_factory.mktemp("scenario_plan_san")
    probe = tmp / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["cc", "-fsanitize=address", str(probe), "-o", str(tmp / "probe")], capture_output=True,
                       text=True)
    if r.returncode != 0:
        pytest.skip("the compiler cannot link -fsanitize=address: " + r.stderr.strip()[-200:])
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "scenario_plan_check_san", f"OUT={tmp}"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return tmp / "san" / "scenario_plan_check"


@pytest.mark.parametrize("n,options,kernel", SAN_CASES, ids=[f"n{n}" for n, _, _ in SAN_CASES])
def test_plan_digest_sanitized(sanitized, n, options, kernel):
    """Exit 0, the same output as the plain driver and nothing on stderr; a
    capped multi-launch grid on the two paths that take the cap."""
    opts = options if kernel.startswith("k_scn<") else "MDP_SCN_LAUNCH_PTS=256"
    r = plan(ROW[:n], 1, opts, (30, 10, 1, 2), exe=sanitized)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.splitlines()[:3] == expected_head(ROW[:n], 1, kernel)
    assert r.stdout == plan(ROW[:n], 1, opts, (30, 10, 1, 2)).stdout
