#!/usr/bin/env python3
"""Two device listings of one unit compared per symbol: a change that must not
alter the kernels is checked on a host, without a device.

    hipcc $(HIPFLAGS) -S --cuda-device-only spom_engine.hip -o parent.s   (at the parent)
    hipcc $(HIPFLAGS) -S --cuda-device-only spom_engine.hip -o branch.s   (here)
    scripts/isa_symbols.py parent.s branch.s

A symbol is a label that is neither a basic block nor local; its text is every
line up to the next symbol, without comments, .file / .loc / .ident lines and
the per-build __hip_cuid_* symbol.  Prints the counts and every symbol that
differs, appears or disappears; exit 1 if there is one."""
import re
import sys


def symbols(path):
    syms, cur, kernels = {}, None, 0
    for ln in open(path, errors="replace"):
        ln = ln.split(";")[0].rstrip()
        t = ln.strip()
        if not t or t.startswith((".file", ".loc", ".ident")) or "__hip_cuid_" in t:
            continue
        kernels += t.startswith(".amdhsa_kernel ")
        m = re.match(r"^([A-Za-z_.$][\w.$]*):$", ln)
        if m and not m.group(1).startswith((".L", "BB")):
            cur = m.group(1)
            syms[cur] = []
        elif cur:
            syms[cur].append(t)
    return syms, kernels


def main():
    (a, ka), (b, kb) = symbols(sys.argv[1]), symbols(sys.argv[2])
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(f"{len(a)} / {len(b)} symbols, {ka} / {kb} kernels; {len(diff)} differ")
    for k in diff:
        print("  ", k, "only in the first" if k not in b else "only in the second" if k not in a else "differs")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
