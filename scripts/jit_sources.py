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
    ap.add_argument("out", type=Path)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t:
        tmp = Path(t)
        exe = build_rev(a.rev, tmp) if a.rev else a.exe or T.PLAN_CHECK
        paths = inputs(tmp)
        lines = []
        for name, options in rows():
            _, m, d = T.INPUTS[name]
            flags = ["--diag"] if any(k in options for k in T.DIAG_OPTIONS) else []
            r = subprocess.run([str(exe), "--sources", *flags, str(paths[name]), str(m), str(d), options],
                               capture_output=True, text=True, check=True)
            lines.append(f"# {name} {options or 'default'}\n")
            lines += [ln + "\n" for ln in r.stdout.splitlines() if ln.startswith("src ")]
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
