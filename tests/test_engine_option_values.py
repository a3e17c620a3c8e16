"""What each engine option's value means, pinned on the host through plan_check.

The parser (parse_engine_opts, csrc/spom_plan.cpp) refuses names, never a
value: text that is no number counts as 0, numbers out of range are clamped or
fall back to the default, a name without '=' has the value "1" and a repeated
name takes its last value.  Each row runs plan_check twice over one input,
with options A and with options B, and asserts that the two runs are
identical (exit code, stdout with its source digest, stderr) or that their
stdout differs.  Nothing is recorded here, so a change of the generated
sources does not touch this file; a change of a conversion does.

mode "src": `plan_check --sources` (the path, the plan's counts, every
generated source's digest); mode "grid": `plan_check --grid 64 64 256 --list`
(what a 64 x 64 grid runs on 256 compute units).  MDP_FWD and the generic
path's MDP_EPL are not visible to plan_check: tests/test_gpu_options.py pins
them on the device."""
from __future__ import annotations

import subprocess

import pytest

from test_plan_host import INPUTS, PLAN_CHECK, inputs  # noqa: F401  (inputs: a fixture)

EQ, NE = True, False

# (input, options A, options B, mode, equal?)
ROWS = [
    ("config2", "MDP_JIT=00", "", "src", EQ),
    ("config2", "MDP_JIT", "", "src", EQ),
    ("config2", "MDP_FUSED_COLS=9", "MDP_FUSED_COLS=4", "src", EQ),
    ("config2", "MDP_FUSED_COLS=0", "MDP_FUSED_COLS=1", "src", EQ),
    ("config2", "MDP_FUSED_COLS=banana", "MDP_FUSED_COLS=1", "src", EQ),
    ("config2", "MDP_JIT_KBLOCK=300", "MDP_JIT_KBLOCK=256", "src", EQ),
    ("config2", "MDP_EPL=banana", "MDP_EPL=0", "src", EQ),
    ("config2", "MDP_EPL=1;MDP_EPL=4", "MDP_EPL=4", "src", EQ),
    ("config2", "MDP_JIT_GATHER=0", "", "src", EQ),
    ("config2", "MDP_JIT_GATHER=2", "MDP_JIT_GATHER=1", "src", EQ),
    ("config2", "MDP_QGLOBAL=0", "", "src", EQ),
    ("config2", "MDP_QGLOBAL=5", "MDP_QGLOBAL=1", "src", EQ),
    ("config2", "MDP_JIT_XCD=2", "MDP_JIT_XCD=1", "src", EQ),
    ("config2", "MDP_JIT_SPLIT=2", "MDP_JIT_SPLIT=1", "src", EQ),
    ("config2", "MDP_JIT_SLOTS=banana", "MDP_JIT_SLOTS=0", "src", EQ),
    ("config2", "MDP_JIT_WINDOW=banana", "MDP_JIT_WINDOW=0", "src", EQ),
    ("config2", "MDP_JIT_THREADS=3;MDP_JIT_VERBOSE;MDP_JIT_CHECK=1;MDP_QROWS_XCD=0;MDP_FWD=scalar", "", "src", EQ),
    ("config2", "MDP_FUSED=7", "MDP_FUSED=1", "grid", EQ),
    ("config2", "MDP_QGLOBAL=1;MDP_WIDE_CB=0", "MDP_QGLOBAL=1;MDP_WIDE_CB=1", "grid", EQ),
    ("config2", "MDP_WIDE_CB=3", "", "grid", EQ),   # honoured on the q-global paths only
    ("config2", "MDP_JIT=0", "", "src", NE),
    ("config2", "MDP_FUSED_COLS=1", "MDP_FUSED_COLS=4", "src", NE),
    ("config2", "MDP_JIT_KBLOCK=512", "MDP_JIT_KBLOCK=256", "src", NE),
    ("config2", "MDP_JIT_KBLOCK=256", "", "src", NE),   # given: one shape for both variants
    ("config2", "MDP_EPL=2", "", "src", NE),            # the same
    ("config2", "MDP_EPL=1", "MDP_EPL=4", "src", NE),
    ("config2", "MDP_JIT_XCD=0", "", "src", NE),
    ("config2", "MDP_JIT_ROT=0", "", "src", NE),
    ("config2", "MDP_FAST_LOG=0", "", "src", NE),
    ("config2", "MDP_JIT_EFAST=0", "", "src", NE),
    ("config2", "MDP_FUSED=0", "", "grid", NE),
    ("config2", "MDP_QGLOBAL=1;MDP_WIDE_CB=1", "MDP_QGLOBAL=1", "grid", NE),
    ("manual", "MDP_JIT_CHUNK=0", "MDP_JIT_CHUNK=1", "src", EQ),
    ("manual", "MDP_JIT_CHUNK=1", "", "src", NE),
    ("manual", "MDP_WIDE=2", "MDP_WIDE=1", "src", EQ),
    ("manual", "MDP_WIDE=0", "", "src", EQ),
    ("manual", "MDP_WIDE=banana", "", "src", EQ),
    # vlds
    ("s64", "MDP_VSPLIT=3", "MDP_VSPLIT=4", "src", EQ),
    ("s64", "MDP_VSPLIT=4", "", "src", EQ),
    ("s64", "MDP_VSPLIT=1", "MDP_VSPLIT=2", "src", NE),
    ("s64", "MDP_VLDS_EPL=3", "", "src", EQ),
    ("s64", "MDP_VLDS_EPL=2", "", "src", NE),
    ("s64", "MDP_VLDS_MAXUSES=-5", "MDP_VLDS_MAXUSES=0", "src", EQ),
    ("s64", "MDP_VLDS_MAXUSES=0", "", "src", NE),
    ("s64", "MDP_JIT_KBLOCK=512", "", "src", EQ),   # wholly ignored under vlds
    # k_fwd_hs, 8 cube bits
    ("s128", "MDP_HS_RADIX=99", "", "src", EQ),
    ("s128", "MDP_HS_RADIX=0", "MDP_HS_RADIX=1", "src", EQ),
    ("s128", "MDP_HS_RADIX=1", "", "src", NE),
    ("s128", "MDP_HS_WAVES=banana", "MDP_HS_WAVES=16", "src", EQ),
    ("s128", "MDP_HS_WAVES=8", "", "src", EQ),
    ("s128", "MDP_HS_WAVES=16", "", "src", NE),
    ("s128", "MDP_WIDE_MMA=banana", "MDP_WIDE_MMA=0", "src", EQ),
    ("s128", "MDP_WIDE_MMA=7", "MDP_WIDE_MMA=0", "src", EQ),
    ("s128", "MDP_WIDE_MMA=-1", "MDP_WIDE_MMA=0", "src", EQ),
    # 9 cube bits: 16 waves whatever is asked
    ("s512@0", "MDP_HS_WAVES=8", "", "src", EQ),
]

_runs = {}


def _run(paths, name, options, mode):
    """One plan_check run (shared among the rows that name it)."""
    key = (name, options, mode)
    if key not in _runs:
        _, m, d = INPUTS[name]
        flags = ["--sources"] if mode == "src" else ["--grid", "64", "64", "256", "--list"]
        r = subprocess.run([str(PLAN_CHECK), *flags, str(paths[name]), str(m), str(d), options], capture_output=True,
                           text=True, timeout=120)
        _runs[key] = (r.returncode, r.stdout, r.stderr)
    return _runs[key]


@pytest.mark.parametrize("name,a,b,mode,equal", ROWS,
                         ids=[f"{n}-{a}-{'eq' if e else 'ne'}-{b or 'none'}-{m}" for n, a, b, m, e in ROWS])
def test_option_value(inputs, name, a, b, mode, equal):  # noqa: F811
    ra, rb = _run(inputs, name, a, mode), _run(inputs, name, b, mode)
    assert ra[0] == 0 and rb[0] == 0 and ra[1] and rb[1], (ra, rb)
    if equal:
        assert ra == rb
    else:
        assert ra[1] != rb[1]
