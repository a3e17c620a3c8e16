#!/usr/bin/env python3
"""Listing of every forward source the host planner generates over the table of
tests/test_plan_host.py (its CASES rows that take a JIT path, plus the default
rows of its other inputs): `plan_check --sources` per row, one `src` line per
source -- bytes, FNV-1a and flops_pt.  Two generators emit the same text
exactly when their listings are equal, so a change that must not alter the
kernels is checked on a host:

    scripts/jit_sources.py --rev HEAD~1 profiles/rNN/x/sources_parent.txt
    scripts/jit_sources.py profiles/rNN/x/sources_branch.txt
    cmp profiles/rNN/x/sources_parent.txt profiles/rNN/x/sources_branch.txt

With --full the listing is the planner's whole decision instead: for every row
of CASES the complete output of `plan_check --sources` (the path line with its
digest, then the src lines), and for every row of tests/test_grid_plan_host.py
(ROWS and LISTS) that of `plan_check --grid ... --list` (path, grid with its
kernels and buffer sizes, plist).  Two planners that decide alike print the
same bytes.

Without --rev the tree's own plan_check (midaspom_amd/_build, `make`) runs.
With it csrc/ and include/ of that revision are unpacked to a temporary
directory, this tree's plan_check.cpp is put in their place (its --sources
flag; it compiles against older planners) and plan_check is built there.
"""
from __future__ import annotations

import argparse
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import test_plan_host as T  # noqa: E402
import test_grid_plan_host as G  # noqa: E402


def rows():
    seen = set()
    for _, name, options, path in T.CASES:
        if path.startswith(("generic", "wide")):
            continue
        seen.add((name, options))
        yield name, options
    for name in ("manual", "occupancies", "config3", "long200", "highvar12", "highvar16", "highvar20", "s64"):
        if (name, "") not in seen:
            yield name, ""


def full_rows():
    """(heading, plan_check flags, input, options) of the --full listing."""
    for _, name, options, _ in T.CASES:
        yield f"{name} {options or 'default'}", ["--sources"], name, options
    for rid, name, options, grid, _ in G.ROWS:
        yield f"grid {rid}", ["--grid", *map(str, grid), "--list"], name, options
    for rid, name, grid, _, epl in G.LISTS:
        yield f"list {rid}", ["--grid", *map(str, grid), "--list"], name, f"MDP_EPL={epl}" if epl != 2 else ""


def inputs(tmp: Path):
    paths = {}
    for name, (src, _, _) in T.INPUTS.items():
        if isinstance(src, str):
            paths[name] = T.GOLDEN / src
        elif isinstance(src, dict):
            paths[name] = Path(T.synth.write(tmp / f"{name}.txt", **src))
        else:
            paths[name] = tmp / f"{name}.txt"
            T.np.savetxt(paths[name], src(), fmt="%d")
    return paths


def build_rev(rev: str, tmp: Path) -> Path:
    tar = subprocess.run(["git", "-C", str(ROOT), "archive", rev, "midaspom_amd/csrc", "include"], check=True,
                         capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", str(tmp)], input=tar, check=True)
    csrc = tmp / "midaspom_amd" / "csrc"
    (csrc / "plan_check.cpp").write_bytes((T.CSRC / "plan_check.cpp").read_bytes())
    subprocess.run(["make", "-s", "-j8", "-C", str(csrc), "../_build/plan_check"], check=True)
    return tmp / "midaspom_amd" / "_build" / "plan_check"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rev", help="generate with the planner and generator of this git revision")
    ap.add_argument("--exe", type=Path, help="another build of plan_check (a --coverage one, say)")
    ap.add_argument("--full", action="store_true", help="every line of every row, the grid table's rows included")
    ap.add_argument("out", type=Path)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t:
        tmp = Path(t)
        exe = build_rev(a.rev, tmp) if a.rev else a.exe or T.PLAN_CHECK
        paths = inputs(tmp)
        lines = []
        todo = full_rows() if a.full else ((f"{n} {o or 'default'}", ["--sources"], n, o) for n, o in rows())
        for heading, mode, name, options in todo:
            _, m, d = T.INPUTS[name]
            flags = ["--diag"] if any(k in options for k in T.DIAG_OPTIONS) else []
            r = subprocess.run([str(exe), *mode, *flags, str(paths[name]), str(m), str(d), options],
                               capture_output=True, text=True, check=True)
            lines.append(f"# {heading}\n")
            lines += [ln + "\n" for ln in r.stdout.splitlines() if a.full or ln.startswith("src ")]
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
