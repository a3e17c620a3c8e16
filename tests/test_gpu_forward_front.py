"""The front and the tail of mdp_fwd_jit (csrc/spom_jit.cpp): the loads and
kernel-argument reads ahead of the first barrier and after the last one, at
the smallest shapes where they can go wrong.

Every variant issues its staging loads first, reads e, c, the point list and
the chunk hand-over vectors through a clamped index with the value selected
afterwards, and takes the workgroup count of the XCD-aware block order as an
argument.  None of that may change a bit of the result, so each case is held
three ways:

  * to the bits the kernels gave before the front was reordered
    (tests/golden/forward_front_bits.json: per case the SHA-256 of the
    [ne][nc] float64 result's bytes and 16 sampled cells, as hex floats, for
    diagnosis);
  * fused against reading, whole-array bit equality, where both run the grid;
  * to the oracle at 16 points (test_gpu_partition._anchor), at the suite's
    tolerance.

The fixture pins the bits of one toolchain: the hipRTC compiler of the ROCm
release it was recorded with.  Another compiler may contract or order the
same expressions differently; if these cases then fail while the fused /
reading and oracle comparisons hold, re-record it on an MI355X with

    MDP_FORWARD_FRONT_RECORD=/some/path.json pytest tests/test_gpu_forward_front.py

(at a commit whose results are trusted) and copy the file over the fixture.

The grids: e and c hold 0 and 1 exactly, so -inf cells appear; both layouts
run into buffers wider than the grid (ld_out > extent), filled with a value
no log likelihood takes.
"""
from __future__ import annotations

import hashlib
import json
import os
from pathlib import Path

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle

from test_gpu_parity import assert_loglik_close  # noqa: F401  (the tolerance _anchor applies)
from test_gpu_partition import SENTINEL, TALL, _anchor, _engine, _run, _same

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).parent / "golden" / "forward_front_bits.json"
RECORD = os.environ.get("MDP_FORWARD_FRONT_RECORD")
INPUT = "config2_64x50.txt"

# name -> (options, ne, nc, e descending, launched kernel)
CASES = {
    # 4 workgroups of 2 columns: the last one's second column is past nc; 33 of 512 points a column
    "fused_33x7": ({}, 33, 7, False, "mdp_fwd_jit<fused"),
    # two e blocks x 3 column groups: 6 workgroups, below the 8 of one XCD round
    "fused_forced_520x5": ({"MDP_FUSED": "1"}, 520, 5, False, "mdp_fwd_jit<fused"),
    # 3 e blocks x 9 columns: 27 workgroups, 24 permuted and a tail of 3
    "reading_1030x9": ({"MDP_FUSED": "0"}, 1030, 9, False, "mdp_fwd_jit<reading"),
    "tall_1024x256": ({}, 1024, 256, False, TALL),
    # e descending, an odd number of s-form rows: a point list that is not the identity
    "list_fused_95x7": ({}, 95, 7, True, "mdp_fwd_jit<fused"),
    "list_reading_95x7": ({"MDP_FUSED": "0"}, 95, 7, True, "mdp_fwd_jit<reading"),
    # chunks hand their state vectors over through vscr
    "chunked_70x3": ({"MDP_JIT_CHUNK": "64"}, 70, 3, False, "chunks"),
    "gathered_70x3": ({"MDP_JIT_CHUNK": "64", "MDP_JIT_GATHER": "1"}, 70, 3, False, "gather>"),
}

# grids both the fused and the reading kernel run: (ne, nc, e descending)
PAIRS = {"33x7": (33, 7, False), "520x5": (520, 5, False), "1030x9": (1030, 9, False),
         "1024x256": (1024, 256, False), "95x7_descending": (95, 7, True)}


def _axis(n, hi):
    """n ascending values from 0 to hi with the one nearest 1 set to 1."""
    a = np.linspace(0.0, hi, n)
    a[int(np.abs(a - 1.0).argmin())] = 1.0
    assert a[0] == 0.0 and (a == 1.0).any() and (np.diff(a) > 0).all()
    return a


def _grid(ne, nc, desc):
    # (the tall variant needs an even number of e blocks: 1 024 rows on [0, 1] are 512 s-form and 512
    # t-form rows, so the point list is not padded past two blocks; the other grids run past e = 1)
    e = _axis(ne, 1.0 if ne == 1024 else 1.1)
    c = _axis(nc, 1.0)  # the fused kernel holds the Z columns of |c| <= 1
    return (e[::-1].copy() if desc else e), c


def _run_ce(eng, e, c):
    """_run in the CE layout: the [nc][ne] result out of a padded buffer."""
    import torch

    eng.set_layout("ce")
    eng.set_grid(e, c)
    ld = e.size + 5
    buf = torch.full((c.size + 1, ld), SENTINEL, dtype=torch.float64, device="cuda")
    eng.run(buf.data_ptr(), ld)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:, e.size:] == SENTINEL).all() and (out[c.size:] == SENTINEL).all(), "stores past the grid"
    return np.ascontiguousarray(out[:c.size, :e.size])


_RESULTS = {}


def _result(golden, options, ne, nc, desc):
    """(e, c, [ne][nc] result, launched) of one engine and grid, computed once:
    the EC run, and the CE run held to its transpose."""
    key = (tuple(sorted(options.items())), ne, nc, desc)
    if key not in _RESULTS:
        e, c = _grid(ne, nc, desc)
        with _engine(mdp.Model.load(golden / INPUT), options) as eng:
            got = _run(eng, e, c)
            ce = _run_ce(eng, e, c)
            launched = eng.launched()
        _same(ce, got.T, f"{options} {ne} x {nc}: CE layout against EC transposed")
        got.setflags(write=False)
        _RESULTS[key] = (e, c, got, launched)
    return _RESULTS[key]


def _cells(shape):
    rng = np.random.default_rng(20)
    return [(int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1]))) for _ in range(16)]


def _entry(got):
    return {"shape": list(got.shape), "sha256": hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest(),
            "cells": [[i, j, float(got[i, j]).hex()] for i, j in _cells(got.shape)]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_front_keeps_the_recorded_bits(golden, name):
    options, ne, nc, desc, kernel = CASES[name]
    e, c, got, launched = _result(golden, options, ne, nc, desc)
    assert any(kernel in k for k in launched), launched
    if name.startswith("list_"):
        x = np.minimum(e, 1.0)
        assert int((x < 1.0 - x).sum()) % 2 == 1 and not np.array_equal(e, np.sort(e))
    assert np.isneginf(got).any() and np.isfinite(got).mean() > 0.5
    ent = _entry(got)
    if RECORD:
        path = Path(RECORD)
        table = json.loads(path.read_text()) if path.exists() else {}
        table[name] = ent
        path.write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
    else:
        ref = json.loads(FIXTURE.read_text())[name]
        assert ent["shape"] == ref["shape"]
        if ent["sha256"] != ref["sha256"]:
            diff = [(a, b) for a, b in zip(ent["cells"], ref["cells"]) if a != b]
            raise AssertionError(f"{name}: result bytes differ from the recorded ones; of the 16 sampled cells "
                                 f"{len(diff)} differ (got, recorded): {diff}")
    _anchor("config2-front", lambda: oracle.OracleModel.load(golden / INPUT), e, c, got)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_fused_equals_reading(golden, name):
    ne, nc, desc = PAIRS[name]
    _, _, fused, lf = _result(golden, {"MDP_FUSED": "1"}, ne, nc, desc)
    _, _, reading, lr = _result(golden, {"MDP_FUSED": "0"}, ne, nc, desc)
    assert any("mdp_fwd_jit<fused" in k for k in lf) and not any("mdp_fwd_jit<reading" in k for k in lf), lf
    assert any("mdp_fwd_jit<reading" in k for k in lr) and not any("mdp_fwd_jit<fused" in k for k in lr), lr
    _same(fused, reading, f"{name}: fused against reading")


def test_launched_is_noted_once(golden):
    """The instantiations an engine reports after 100 runs on one grid are
    those it reports after one."""
    import torch

    e, c = _grid(33, 7, False)
    with _engine(mdp.Model.load(golden / INPUT)) as eng:
        first = _run(eng, e, c)
        once = eng.launched()
        assert once
        buf = torch.full((e.size, c.size), SENTINEL, dtype=torch.float64, device="cuda")
        for _ in range(100):
            eng.run(buf.data_ptr(), c.size)
        torch.cuda.synchronize()
        assert eng.launched() == once
        _same(buf.cpu().numpy(), first, "the 100th run against the first")
