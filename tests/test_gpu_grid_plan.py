"""The host grid planner against the device: for some rows of tests/
test_grid_plan_host.py's table a fresh engine sets the grid and runs it once,
and the kernel instantiations it then reports (mdp_engine_launched) must be
the ones `plan_check --grid` names for the same grid on a device of as many
compute units -- the planner the CPU table tests is the one that picked what
ran here."""
from __future__ import annotations

import pytest

import midaspom_amd as mdp

from test_grid_plan_host import ODD, parse, plan_grid
from test_gpu_partition import _engine, _run
from test_plan_host import INPUTS, PLAN_CHECK, inputs  # noqa: F401  (inputs: a fixture)

pytestmark = pytest.mark.gpu


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# (id, input, options, ne, nc (a function of the device's CU count), e-axis arguments of plan_check)
ROWS = [
    ("config2-512", "config2", {}, 512, lambda cu: 8, []),
    ("config2-513", "config2", {}, 513, lambda cu: 8, []),
    ("config2-514-list", "config2", {}, 512, lambda cu: 8, ODD),
    ("config3-1024xCUs", "config3", {}, 1024, lambda cu: cu, []),
    ("config3-1024xCUs-1", "config3", {}, 1024, lambda cu: cu - 1, []),
    ("s128", "s128", {}, 64, lambda cu: 64, []),
    ("s128-mmt", "s128", {"MDP_WIDE_MMA": "2"}, 64, lambda cu: 64, []),
    ("highvar16-64x512", "highvar16", {}, 64, lambda cu: 512, []),
]


@pytest.mark.parametrize("rid,name,options,ne,nc_of,eargs", ROWS, ids=[r[0] for r in ROWS])
def test_device_runs_what_the_planner_names(inputs, rid, name, options, ne, nc_of, eargs):   # noqa: F811
    cu = _cus()
    nc = nc_of(cu)
    lo, hi = (float(eargs[1]), float(eargs[2])) if eargs else (0.0, 1.0)
    f, _ = parse(plan_grid(PLAN_CHECK, inputs, name, ";".join(f"{k}={v}" for k, v in options.items()),
                           [ne, nc, cu, *eargs]))
    assert f["kernels"], f
    _, m, d = INPUTS[name]
    model = mdp.Model.load(inputs[name], m=m, d=d)
    e, c = mdp.grid(ne, lo, hi)[0], mdp.grid(nc)[0]
    with _engine(model, options) as eng:
        _run(eng, e, c)   # (every cell written, none past the grid)
        assert eng.launched() == f["kernels"], (rid, f["variant"])
