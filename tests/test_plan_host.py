"""The engine's host planner (csrc/spom_plan.cpp) on its own: _build/plan_check
loads a problem, plans it with gfx950's 160 KiB of LDS and generates the
forward sources, without a device, the HIP runtime or hipRTC.  One table of
cases walks every planner (generic, direct, chunks, gathered Q, vlds and the
four wide forwards with each of their shapes); the first test asserts the path
each row takes, the second runs the same table through the program built with
the address and undefined-behaviour sanitizers, so the tables the wide kernels
index unchecked are at least filled within bounds."""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from midaspom_amd import synth

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "midaspom_amd" / "csrc"
PLAN_CHECK = ROOT / "midaspom_amd" / "_build" / "plan_check"
GOLDEN = ROOT / "tests" / "golden"

LATER = [[1, 1, 0, 1, 0, 1, 1, 0], [1, 0, 0, 1, 1, 1, 0, 1]]   # test_wide_years_plan_offline's later rows


def _wide_obs(rng, n, T, missing):   # as tests/test_gpu_layout.py
    obs = rng.integers(0, 2, size=(T, n))
    for y, k in missing.items():
        obs[y, rng.choice(n, size=k, replace=False)] = -1
    return obs


def _full_year(n, year):
    """4 years x n patches, every patch unvisited in `year` (2^n states)."""
    obs = np.random.default_rng(10 * n + year).integers(0, 2, size=(4, n))
    obs[year, :] = -1
    return obs


def _long_occupied(n, T, year, k):
    """T years x n patches, all occupied, k patches unvisited in `year` (2^k states): min |A| is n in nearly every
    year, so the forward's deferred exponent passes its flush threshold (192) within the series."""
    obs = np.ones((T, n), dtype=int)
    obs[year, :k] = -1
    return obs


def _highvar(nvar):   # as tests/test_gpu_highvar.py
    n, T, nv, dense, sparse, nmiss, seed = {12: (16, 8, 12, 11, 4, 2, 1), 16: (20, 8, 16, 15, 4, 2, 2),
                                            20: (22, 7, 20, 19, 3, 2, 3)}[nvar]
    return synth.alternating_obs(np.random.default_rng(seed), n, T, nv, dense, sparse, nmiss)


# name -> (golden file | callable returning the observations | synth config, m, d)
INPUTS = {
    "manual": ("manual_p3_obs.txt", 400, 200),
    "occupancies": ("occupancies.txt", 400, 100),
    "config2": ("config2_64x50.txt", 400, 100),
    "config3": ("config3_256x200.txt", 400, 100),
    "long200": (synth.LONG200, 400, 100),   # tests/test_gpu_longseries.py: 3 086 uses
    "s64": (lambda: np.array([[1, -1, -1, -1, -1, -1, -1, 1]] + LATER), 400, 100),
    "s128": (lambda: np.array([[-1] * 7 + [1]] + LATER), 400, 100),
    "s32flush": (lambda: _long_occupied(8, 30, 27, 5), 400, 100),
    **{f"s512@{y}": ((lambda y=y: _full_year(9, y)), 400, 100) for y in (0, 2, 3)},
    **{f"s1024@{y}": ((lambda y=y: _full_year(10, y)), 400, 100) for y in (0, 1, 3)},
    "nvar12w": (lambda: _wide_obs(np.random.default_rng(3), 12, 5, {1: 6}), 400, 100),
    **{f"highvar{v}": ((lambda v=v: _highvar(v)), 400, 100) for v in (12, 16, 20)},
}

# (case, input, options, the path plan_check must name: a regular expression, matched whole)
CASES = [
    ("a", "manual", "", "direct fused-capable"),
    ("a", "manual", "MDP_JIT=0", "generic"),
    ("a", "manual", "MDP_WIDE=1", "wide-mmt<4,128,2buf>"),
    ("b", "occupancies", "", "direct fused-capable"),
    ("c", "config2", "", "direct fused-capable"),
    ("d", "config3", "", "direct"),
    # tests/test_gpu_longseries.py: its long survey without knobs, and its knob sets on config 2 (40 uses a chunk)
    ("e", "long200", "", r"direct chunked<\d+>"),
    ("e", "config2", "MDP_JIT_CHUNK=40", r"direct chunked<\d+>"),
    ("e", "config2", "MDP_JIT_CHUNK=40;MDP_JIT_GATHER=1", r"direct chunked<\d+,gathered>"),
    ("e", "config2", "MDP_JIT_GATHER=1", r"direct chunked<\d+,gathered>"),
    ("e", "config2", "MDP_QGLOBAL=1", "direct qglobal"),
    ("e", "config2", "MDP_QGLOBAL=1;MDP_JIT_CHUNK=40", r"direct chunked<\d+> qglobal"),
    ("f", "s64", "", "vlds"),
    ("f", "s32flush", "", "vlds"),   # a vlds year that applies the deferred exponent
    ("f'", "s64", "MDP_WIDE=1", "wide-mmt<4,128,2buf>"),
    ("g", "s128", "", "wide-hs<2,8,8>"),
    ("g", "s128", "MDP_WIDE_MMA=0", "wide-plain"),
    ("g", "s128", "MDP_WIDE_MMA=1", "wide-mma<128>"),
    ("g", "s128", "MDP_WIDE_MMA=2", "wide-mmt<4,128,2buf>"),
    ("g", "s128", "MDP_WIDE_MMA=3", "wide-hs<2,8,8>"),
    *[("h", f"s512@{y}", o, p) for y in (0, 2, 3)
      for o, p in (("", "wide-hs<2,9,16>"), ("MDP_WIDE_MMA=2", "wide-mmt<2,512,1buf>"))],
    *[("h", f"s1024@{y}", o, p) for y in (0, 1, 3)
      for o, p in (("", "wide-hs<1,10,16>"), ("MDP_WIDE_MMA=2", "wide-mmt<1,1024,1buf>"))],
    ("i", "nvar12w", "MDP_WIDE=1;MDP_WIDE_MMA=3", "wide-mmt<4,128,2buf>"),   # nvar > 10: not k_fwd_hs
    *[("j", f"highvar{v}", o, p) for v in (12, 16, 20)
      for o, p in (("", "direct( fused-capable)?"), ("MDP_JIT=0", "generic"), ("MDP_WIDE=1", "wide-mmt<4,128,2buf>"))],
    # the knobs that shape the generated forward source (csrc/spom_jit.cpp), one form of its text each
    *[("k", "config2", o, "direct fused-capable") for o in (
        "MDP_EPL=1", "MDP_EPL=4", "MDP_JIT_KBLOCK=512", "MDP_FUSED_COLS=1", "MDP_FUSED_COLS=4",
        "MDP_JIT_ROT=0;MDP_JIT_SPLIT=0;MDP_JIT_XCD=0;MDP_JIT_EFAST=0;MDP_FAST_LOG=0",
        "MDP_JIT_SLOTS=0;MDP_JIT_WINDOW=4", "MDP_JIT_SLOTS=2;MDP_JIT_WINDOW=16",
        "MDP_DIAG=1", "MDP_JIT_HACK=1", "MDP_JIT_HACK=2;MDP_JIT_WPE=2")],   # the last three: plan_check --diag
    *[("k", "s64", o, "vlds") for o in ("MDP_VSPLIT=1", "MDP_VSPLIT=2", "MDP_VLDS_EPL=2")],
    ("k", "s64", "MDP_JIT_CHUNK=40", r"vlds chunked<\d+>"),
]
DIAG_OPTIONS = ("MDP_DIAG", "MDP_JIT_HACK", "MDP_JIT_WPE")   # measurement-only names: accepted with --diag alone

LINE = re.compile(r"^path (?P<path>.+) \| nj (\d+) nitems (?P<nitems>\d+) ldQ (\d+) nqi (\d+) qmaxlen (\d+) kzmax (\d+) "
                  r"slots (?P<slots>\d+) conflicts (?P<gather>\d+) \+ (?P<store>\d+) \| digest [0-9a-f]{16}$")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Every input of the table as an observation file."""
    tmp = tmp_path_factory.mktemp("plan_inputs")
    paths = {}
    for name, (src, m, d) in INPUTS.items():
        if isinstance(src, str):
            paths[name] = GOLDEN / src
        elif isinstance(src, dict):
            paths[name] = Path(synth.write(tmp / f"{name}.txt", **src))
        else:
            paths[name] = tmp / f"{name}.txt"
            np.savetxt(paths[name], src(), fmt="%d")
    return paths


def _run(exe, inputs, name, options):
    _, m, d = INPUTS[name]
    flags = ["--diag"] if any(k in options for k in DIAG_OPTIONS) else []
    return subprocess.run([str(exe), *flags, str(inputs[name]), str(m), str(d), options], capture_output=True,
                          text=True, timeout=120)


def _check(r, case, name, options, path):
    assert r.returncode == 0, (case, name, options, r.stdout, r.stderr)
    m = LINE.match(r.stdout.strip())
    assert m, (case, name, options, r.stdout)
    assert re.fullmatch(path, m["path"]), (case, name, options, m["path"], path)
    if case == "d":   # config 3's slot colouring (tests/test_jit_offline.py asserts the same bounds)
        nitems, slots, gather, store = (int(m[k]) for k in ("nitems", "slots", "gather", "store"))
        assert nitems == 1881
        assert slots <= nitems + 16 + 64
        assert gather <= 32 and store <= 96


IDS = [f"{c}-{n}-{o or 'default'}" for c, n, o, _ in CASES]


@pytest.mark.parametrize("case,name,options,path", CASES, ids=IDS)
def test_planner_paths(inputs, case, name, options, path):
    _check(_run(PLAN_CHECK, inputs, name, options), case, name, options, path)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """plan_check built with -fsanitize=address,undefined (make plan_check_san)."""
    tmp = tmp_path_factory.mktemp("plan_san")
    probe = tmp / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["cc", "-fsanitize=address", str(probe), "-o", str(tmp / "probe")], capture_output=True,
                       text=True)
    if r.returncode != 0:
        pytest.skip("the compiler cannot link -fsanitize=address: " + r.stderr.strip()[-200:])
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "plan_check_san", f"OUT={tmp}"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return tmp / "san" / "plan_check"


@pytest.mark.parametrize("case,name,options,path", CASES, ids=IDS)
def test_planner_sanitized(inputs, sanitized, case, name, options, path):
    """The same row through the sanitized program: exit 0, the same path and
    nothing on stderr."""
    r = _run(sanitized, inputs, name, options)
    _check(r, case, name, options, path)
    assert r.stderr == "", (case, name, options, r.stderr)
