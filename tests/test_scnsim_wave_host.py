"""The scenario simulator's patch-parallel kernel family (k_scnsim_wave<NP>,
MDP_SIM_WAVE), the parts that need no GPU.

1. The initial state past 64 patches (tests/scnsim_wave_ref.py) against the
   restatement of the lane kernel's (tests/scnsim_ref.py) for n <= 64 and
   against the generator's host restatement mdp.philox beyond.
2. The option strings the library accepts and refuses, the kernel each
   selects, and every refusal of the library and of the drop-ins, all on a
   host without a device.
3. The wave digest of the planner's stand-alone driver
   (_build/scnsim_plan_check) against a numpy restatement: the two copies of
   the distance image bit for bit, the per-lane words, the (lane, bit) list,
   the source row and the launch cut.  The driver itself checks every slot
   the kernel can address; its line is asserted.
4. The likelihood estimate at 1024 patches: 0 for an empty table, finite for
   one count (2^1024 is not a double).
5. The same driver built with -fsanitize=address,undefined (make
   scnsim_plan_check_san), on the same sizes and on the refusals.
"""
from __future__ import annotations

import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import midaspom_amd as mdp
import scnsim_ref as ref
import scnsim_wave_ref as wref
from midaspom_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "midaspom_amd" / "csrc"
PLAN_CHECK = ROOT / "midaspom_amd" / "_build" / "scnsim_plan_check"

SIZES = (1, 64, 65, 128, 129, 257, 513, 1024)
NMISS = (0, 3, 10)
DIGEST_CASES = [(n, k) for n in SIZES for k in NMISS if k <= n]


def need_np(n):
    return 1 if n <= 128 else 2 if n <= 256 else 4 if n <= 512 else 8


# ---------------------------------------------------------------------------
# 1. the initial state
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9, 33, 64])
def test_initial_states_is_the_lane_definition_up_to_64(n):
    for seed, rep0 in ((5, 0), (9, (1 << 32) - 7)):
        reps = np.arange(rep0, rep0 + 40, dtype=np.int64)
        assert np.array_equal(wref.initial_states(n, seed, reps), ref.initial_states(n, seed, reps))


def test_initial_states_against_philox():
    seed, n = 20261020, 1024
    reps = np.array([0, 3, (1 << 32) + 11], dtype=np.int64)
    occ = wref.initial_states(n, seed, reps)
    assert occ.shape == (3, n)
    for i, rg in enumerate(int(r) for r in reps):
        for k in (0, 31, 32, 63, 64, 127, 128, 511, 512, 1023):
            w = mdp.philox(seed, [rg & 0xffffffff, rg >> 32, 0xffffffff, 1 + (k >> 7)])
            assert bool((w[(k >> 5) & 3] >> (k & 31)) & 1) == bool(occ[i, k]), (rg, k)
    # a prefix of a longer row is the shorter row's state; fair bits
    assert np.array_equal(occ[:, :130], wref.initial_states(130, seed, reps))
    big = wref.initial_states(n, seed, np.arange(200, dtype=np.int64))
    assert abs(big.mean() - 0.5) < 5 * 0.5 / math.sqrt(big.size)
    # the blocks of 128 patches do not repeat each other
    assert not np.array_equal(big[:, :128], big[:, 128:256])


# ---------------------------------------------------------------------------
# 2. options, kernel selection and refusals, without a device
# ---------------------------------------------------------------------------
def refused(code, fn, *a, **kw):
    with pytest.raises(mdp.MidaspomError, match=code):
        fn(*a, **kw)


def kernel_of(n, options):
    with mdp.ScenarioSim(np.ones(n, dtype=np.int32), options=options) as sim:
        return sim.kernel


def test_option_names():
    assert {"MDP_SIM_WAVE", "MDP_SIM_NP", "MDP_SIM_NM", "MDP_SIM_LAUNCH_PTS"} == set(_lib.SCENARIO_SIM_OPTION_NAMES)
    assert _lib.lib().mdp_abi_version() == 9


def test_kernel_selection():
    for n in (1, 9, 64):
        assert kernel_of(n, None) == kernel_of(n, "MDP_SIM_WAVE=0") == kernel_of(n, "MDP_SIM_WAVE=auto")
        assert kernel_of(n, "MDP_SIM_WAVE=auto").startswith("k_scnsim<")
        assert kernel_of(n, "MDP_SIM_WAVE=1") == "k_scnsim_wave<1>"
        for np_ in (1, 2, 4, 8):
            assert kernel_of(n, f"MDP_SIM_WAVE=1;MDP_SIM_NP={np_}") == f"k_scnsim_wave<{np_}>"
    assert kernel_of(26, "MDP_SIM_WAVE=auto MDP_SIM_NM=64") == "k_scnsim<64>"
    for n in (65, 128, 129, 256, 257, 512, 513, 1024):
        for mode in ("auto", "1"):
            assert kernel_of(n, f"MDP_SIM_WAVE={mode}") == f"k_scnsim_wave<{need_np(n)}>"
            for np_ in (1, 2, 4, 8):
                opts = {"MDP_SIM_WAVE": mode, "MDP_SIM_NP": np_, "MDP_SIM_LAUNCH_PTS": 3}
                if np_ >= need_np(n):
                    assert kernel_of(n, opts) == f"k_scnsim_wave<{np_}>"
                else:
                    refused("EINVAL", mdp.ScenarioSim, np.ones(n, dtype=np.int32), options=opts)


def test_create_refusals():
    ones = lambda n: np.ones(n, dtype=np.int32)
    # the default is today's: 65 patches are not held
    for opts in (None, "", "MDP_SIM_WAVE=0", "MDP_SIM_LAUNCH_PTS=2"):
        refused("EUNSUPPORTED", mdp.ScenarioSim, ones(65), options=opts)
    # more than 1024 patches: under every setting
    for opts in (None, "MDP_SIM_WAVE=0", "MDP_SIM_WAVE=auto", "MDP_SIM_WAVE=1", "MDP_SIM_WAVE=1;MDP_SIM_NP=8"):
        refused("EUNSUPPORTED", mdp.ScenarioSim, ones(1025), options=opts)
    # MDP_SIM_NP with a lane kernel selected
    for n, opts in ((9, "MDP_SIM_NP=1"), (9, "MDP_SIM_WAVE=0;MDP_SIM_NP=2"), (64, "MDP_SIM_WAVE=auto;MDP_SIM_NP=8")):
        refused("EINVAL", mdp.ScenarioSim, ones(n), options=opts)
    # MDP_SIM_NM with a wave kernel selected
    for n, opts in ((9, "MDP_SIM_WAVE=1;MDP_SIM_NM=64"), (65, "MDP_SIM_WAVE=auto;MDP_SIM_NM=64"),
                    (9, "MDP_SIM_NM=16,MDP_SIM_WAVE=1")):
        refused("EINVAL", mdp.ScenarioSim, ones(n), options=opts)
    # any other name or value
    for bad in ("MDP_SIM_WAVE=2", "MDP_SIM_WAVE=", "MDP_SIM_WAVE", "MDP_SIM_WAVE=on", "MDP_SIM_WAVE=AUTO",
                "MDP_SIM_WIDE=1", "MDP_SIM_WIDE=auto", "MDP_FUT_WIDE=auto", "MDP_SIM_WAVE=1;MDP_SIM_NP=3",
                "MDP_SIM_WAVE=1;MDP_SIM_NP=16", "MDP_SIM_WAVE=1;MDP_SIM_NP=", "MDP_SIM_WAVE=1;MDP_SIM_NP=auto"):
        refused("EINVAL", mdp.ScenarioSim, ones(9), options=bad)
    # the row is still checked
    refused("EINVAL", mdp.ScenarioSim, np.zeros(0, dtype=np.int32), options="MDP_SIM_WAVE=1")
    bad_row = ones(130)
    bad_row[129] = 2
    refused("EINVAL", mdp.ScenarioSim, bad_row, options="MDP_SIM_WAVE=auto")


def test_tables_refusals_with_a_wave_plan():
    """As test_scnsim_host.test_tables_refusals: before the first device call."""
    row = ref.synthetic_row(130, 3)
    with mdp.ScenarioSim(row, "loss", options="MDP_SIM_WAVE=auto") as sim:
        good = dict(e=0.3, c=0.4, K=[1.0], dsrc=[200.0], ts=2, tdis=2, nrep=10)
        refused("EINVAL", sim.tables, **good, hist=False, match=False)
        refused("EINVAL", sim.tables, **{**good, "ts": -1})
        refused("EINVAL", sim.tables, **{**good, "K": [0.0]})
        refused("EINVAL", sim.tables, **{**good, "dsrc": [np.nan]})
        refused("EUNSUPPORTED", sim.tables, **{**good, "ts": 12288, "tdis": 1})
        refused("EUNSUPPORTED", sim.tables, **{**good, "nrep": (1 << 31) + 1})
        # 2^24 cells: 130000 points x 131 hist cells
        refused("EUNSUPPORTED", sim.tables, **{**good, "K": np.full(130000, 1.0)}, match=False)
    with mdp.ScenarioSim(ref.synthetic_row(130, 11), options="MDP_SIM_WAVE=auto") as sim:
        refused("EUNSUPPORTED", sim.tables, 0.3, 0.4, [1.0], nrep=10)  # match with 11 missing patches
        if mdp.device_count() == 0:  # hist alone passes every refusal and reaches the device
            refused("ENODEV", sim.tables, 0.3, 0.4, [1.0], nrep=10, match=False)


@pytest.mark.parametrize("kind", ["dieoff", "loss"])
def test_dropins_refuse_more_than_1024_patches(tmp_path, kind):
    inp = tmp_path / "row1025.txt"
    inp.write_text(" ".join("1" for _ in range(1025)) + "\n")
    flags = ["-a", "1", "-b", "1", "-e", "0.4", "-c", "0.5", "-s", "2", "-R", "10", "-i", str(inp),
             "-o", str(tmp_path / "no.txt")]
    exe = str(_lib.DIEOFF_CLI_PATH if kind == "dieoff" else _lib.LOSS_CLI_PATH)
    for cmd in ([exe], [sys.executable, "-m", "midaspom_amd.scenario", kind]):
        r = subprocess.run([*cmd, *flags], capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 1 and "1025 patches in the first row: -R takes at most 1024" in r.stderr, r.stderr[-500:]
        assert "Migration matrix" not in r.stdout and not (tmp_path / "no.txt").exists()


# ---------------------------------------------------------------------------
# 3. the wave digest of the planner's driver, restated
# ---------------------------------------------------------------------------
def fnv(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def row_text(row):
    return "".join("m" if v == -1 else str(int(v)) for v in row)


def _plan(exe, row, kind=1, options="", nK=5, nrep=777, dsrc=300.0, p=0.3):
    return subprocess.run([str(exe), row_text(row), "400", repr(p), "200", str(kind), options, str(nK), str(nrep),
                           repr(dsrc)], capture_output=True, text=True)


def slot0(n, length, l):
    """First 16-byte slot of survivor l's row (the copy whose alignment fits)."""
    base = n - 1 - l
    return (length + base - 1) >> 1 if base & 1 else base >> 1


def want_digest(row, np_, nK, nrep, dsrc, p):
    """The lines scnsim_plan_check prints in wave mode under MDP_SIM_LAUNCH_PTS=2."""
    n = row.size
    nmiss = int((row == -1).sum())
    length = (n + 128 * np_ + 1) & ~1
    a = 1.0 / 400.0
    G = np.zeros(length + 1)
    for dist in range(1, n):
        G[n - 1 - dist] = G[n - 1 + dist] = math.exp(-a * float(dist) * 200.0)
    image = np.concatenate([G[:length], G[1:length + 1]])
    # the image is the literal matrix: survivor l, pair m reads slot m + slot0(l)
    M = ref.dispersal(n, 400.0, 200.0) if n <= 129 else None
    if M is not None:
        pairs = image.reshape(-1, 2)
        for l in range(n):
            got = pairs[slot0(n, length, l):slot0(n, length, l) + 64 * np_].ravel()[:n]
            assert got.tobytes() == M[l].tobytes()
    fixed, missing, miss = [0] * 64, [0] * 64, []
    for k in range(n):
        lane, bit = (k >> 1) & 63, 2 * (k >> 7) + (k & 1)
        if row[k] == 1:
            fixed[lane] |= 1 << bit
        elif row[k] == -1:
            missing[lane] |= 1 << bit
            miss.append((lane << 8) | bit)
    src = np.zeros(128 * np_)
    src[:n] = ref.source_row(n, 400.0, dsrc)
    pr = ref.priors(nmiss, p)
    tpp = (nrep + 3) // 4
    s = 0.0
    for j in range(1 << nmiss):
        s += float(pr[j]) * 1.0
    lik = s * float(2 ** n) / nrep if n <= 64 else math.ldexp(s / nrep, n)
    lines = [f"kernel k_scnsim_wave<{np_}>",
             f"row n {n} nmiss {nmiss} len {length}",
             "fixed" + "".join(f" {v:x}" for v in fixed),
             "missing" + "".join(f" {v:x}" for v in missing),
             "miss" + "".join(f" {v:x}" for v in miss),
             f"image {fnv(image.tobytes()):016x} prior {fnv(pr.tobytes()):016x} src {fnv(src.tobytes()):016x}",
             f"slots {n} x {64 * np_} inside the image",
             f"call points {nK} tiles_per_point {tpp} hist {nK * (n + 1)} match {nK << nmiss} launches 3"]
    lines += [f"launch p0 {p0} npts {k} tiles {k * tpp} nwg {min(k * tpp, 4096)}" for p0, k in ((0, 2), (2, 2), (4, 1))]
    return lines, lik


def check_digest(exe, n, nmiss, np_=None):
    row = ref.synthetic_row(n, nmiss)
    nK, nrep, dsrc, p = 5, 777, 300.0, 0.3
    opts = "MDP_SIM_WAVE=1;MDP_SIM_LAUNCH_PTS=2" + (f";MDP_SIM_NP={np_}" if np_ else "")
    r = _plan(exe, row, 1, opts, nK, nrep, dsrc, p)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    got = r.stdout.splitlines()
    want, lik = want_digest(row, np_ or need_np(n), nK, nrep, dsrc, p)
    assert got[:len(want)] == want
    assert len(got) == len(want) + 1 and got[-1].startswith("lik ")
    assert math.isfinite(lik) and float.fromhex(got[-1].split()[1]) == lik


@pytest.mark.parametrize("n,nmiss", DIGEST_CASES)
def test_wave_plan_digest(n, nmiss):
    check_digest(PLAN_CHECK, n, nmiss)


@pytest.mark.parametrize("n,np_", [(1, 8), (65, 2), (65, 8), (129, 4), (257, 8)])
def test_wave_plan_digest_larger_np(n, np_):
    check_digest(PLAN_CHECK, n, 3 if n >= 3 else 0, np_)


def test_wave_plan_launch_cut_and_mode_0_lines():
    row = ref.synthetic_row(130, 3)
    r = _plan(PLAN_CHECK, row, 0, "MDP_SIM_WAVE=auto", 151, 10000)
    assert r.returncode == 0 and "launches 1" in r.stdout
    assert f"launch p0 0 npts 151 tiles {151 * 2500} nwg 4096" in r.stdout.splitlines()
    r = _plan(PLAN_CHECK, row, 0, "MDP_SIM_WAVE=auto", 3, 5)  # 3 points x ceil(5/4) tiles
    assert "call points 3 tiles_per_point 2 " in r.stdout and "launch p0 0 npts 3 tiles 6 nwg 6" in r.stdout
    # auto and 0 on a short row: the lane digest, byte for byte the default's
    row26 = ref.synthetic_row(26, 3)
    plain = _plan(PLAN_CHECK, row26, 1, "MDP_SIM_LAUNCH_PTS=2")
    assert plain.returncode == 0 and plain.stdout.startswith("kernel k_scnsim<32>\n")
    for opts in ("MDP_SIM_WAVE=0;MDP_SIM_LAUNCH_PTS=2", "MDP_SIM_WAVE=auto;MDP_SIM_LAUNCH_PTS=2"):
        assert _plan(PLAN_CHECK, row26, 1, opts).stdout == plain.stdout
    for bad, n in (("", 65), ("MDP_SIM_WAVE=0", 65), ("MDP_SIM_WAVE=auto", 1025), ("MDP_SIM_WAVE=1;MDP_SIM_NM=8", 5),
                   ("MDP_SIM_NP=1", 5), ("MDP_SIM_WAVE=1;MDP_SIM_NP=1", 129), ("MDP_SIM_WAVE=x", 5)):
        r = _plan(PLAN_CHECK, ref.synthetic_row(n, 0), 0, bad)
        assert r.returncode == 1 and "scnsim_plan_check:" in r.stderr, (bad, n)


# ---------------------------------------------------------------------------
# 4. the likelihood estimate past 64 patches
# ---------------------------------------------------------------------------
def test_lik_at_1024_patches():
    row = np.ones(1024, dtype=np.int32)
    row[[5, 700]] = -1
    with mdp.ScenarioSim(row, "loss", p=0.3, options="MDP_SIM_WAVE=auto") as sim:
        zero = np.zeros((3, 4), dtype=np.uint64)
        assert np.array_equal(sim.lik(zero, 1000), np.zeros(3))  # not NaN: inf * 0
        one = zero.copy()
        one[1, 2] = 1
        got = sim.lik(one, 1000)
        assert np.isfinite(got).all() and got[0] == 0.0 and got[2] == 0.0
        assert got[1] == math.ldexp(float(ref.priors(2, 0.3)[2]) * 1.0 / 1000.0, 1024) and got[1] > 1e300
    # wherever (sum 2^n) / nrep is finite the two forms agree; n <= 64 keeps its bits
    for n in (64, 65, 130):
        r = ref.synthetic_row(n, 2)
        match = np.array([[3, 0, 7, 1]], dtype=np.uint64)
        with mdp.ScenarioSim(r, p=0.3, options="MDP_SIM_WAVE=1") as sim:
            assert np.array_equal(sim.lik(match, 300), ref.lik(r, 0.3, match, 300))


# ---------------------------------------------------------------------------
# 5. the driver under the host sanitizers: a stand-alone program, no Python
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """scnsim_plan_check built with -fsanitize=address,undefined (make scnsim_plan_check_san)."""
    tmp = tmp_path_factory.mktemp("scnsim_wave_san")
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "scnsim_plan_check_san", f"OUT={tmp}"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return tmp / "san" / "scnsim_plan_check"


def test_wave_plan_sanitized(sanitized):
    """Exit 0, the plain driver's lines and nothing on stderr, on every size
    of the digest test; the refusals exit 1 with the library's message alone."""
    for n, nmiss in DIGEST_CASES:
        check_digest(sanitized, n, nmiss)
    check_digest(sanitized, 65, 3, 8)
    for bad, n in (("", 65), ("MDP_SIM_WAVE=auto", 1025), ("MDP_SIM_WAVE=1;MDP_SIM_NM=8", 5), ("MDP_SIM_NP=1", 5),
                   ("MDP_SIM_WAVE=1;MDP_SIM_NP=1", 129), ("MDP_SIM_WAVE=x", 5), ("MDP_SIM_WIDE=1", 5)):
        r = _plan(sanitized, ref.synthetic_row(n, 0), 0, bad)
        assert r.returncode == 1 and r.stderr.startswith("scnsim_plan_check:") and r.stderr.count("\n") == 1, (bad, n)
