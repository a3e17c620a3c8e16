"""mdp_engine_kernel_name over every path of the posterior engine: for one
small input per path a fresh engine sets an 8 x 8 grid and times its kernels
once (time_kernels keys its result by the slots' names and drops the unnamed
ones), and the names, with the instantiations the engine then reports
(mdp_engine_launched), must be the rows of a literal table -- recorded from the
library as it stood before the names became a lookup by the grid plan's steps,
and unchanged since.  One more row reads the three names of a fresh engine
before any grid is set."""
from __future__ import annotations

import pytest

import midaspom_amd as mdp

from test_gpu_partition import _engine
from test_plan_host import INPUTS, inputs  # noqa: F401  (inputs: a fixture)

pytestmark = pytest.mark.gpu

N = 8   # the grid: 8 x 8, one e block a column (a fused-capable plan runs fused)

# id -> (input, options, the keys of time_kernels, what launched() then holds)
TABLE = {
    "fused": ("manual", {},
        ["k_forward"],
        ["mdp_fwd_jit<fused,maxA4>"]),
    "reading": ("manual", {"MDP_FUSED": "0"},
        ["k_forward", "k_qrows"],
        ["k_qrows<8,0,1>", "mdp_fwd_jit<reading,maxA4>"]),
    "generic": ("manual", {"MDP_JIT": "0"},
        ["k_coefs", "k_forward", "k_zpv"],
        ["k_coefs<1,1,8>", "k_forward_lds<2,4,2>", "k_zpv"]),
    "qglobal": ("manual", {"MDP_QGLOBAL": "1"},
        ["k_forward", "k_witems+k_wq", "k_zrows"],
        ["k_witems<8>", "k_wq", "k_zrows", "mdp_fwd_jit<reading,maxA4>"]),
    "chunks": ("config2", {"MDP_JIT_CHUNK": "40"},
        ["k_forward", "k_qrows"],
        ["k_qrows<8,1,1>", "mdp_fwd_jit<reading,maxA7,chunks3>"]),
    "vlds": ("s64", {},
        ["k_forward", "k_qrows"],
        ["k_qrows<8,1,1>", "mdp_fwd_jit<reading,maxA8>"]),
    "wide-hs": ("s128", {},
        ["k_fwd_hs", "k_witems", "k_zrows"],
        ["k_fwd_hs<2,8>", "k_witems<8>", "k_zrows"]),
    "wide-plain": ("s128", {"MDP_WIDE_MMA": "0"},
        ["k_fwd_wide", "k_witems+k_wq", "k_zrows"],
        ["k_fwd_wide", "k_witems<8>", "k_wq", "k_zrows"]),
    "wide-mma": ("s128", {"MDP_WIDE_MMA": "1"},
        ["k_fwd_mma", "k_witems+k_wq", "k_zrows"],
        ["k_fwd_mma<128>", "k_witems<8>", "k_wq", "k_zrows"]),
    "wide-mmt": ("s128", {"MDP_WIDE_MMA": "2"},
        ["k_fwd_mmt", "k_witems+k_wq", "k_zrows"],
        ["k_fwd_mmt<4,128,2buf>", "k_witems<8>", "k_wq", "k_zrows"]),
    "wide-hs-cb3": ("s128", {"MDP_WIDE_CB": "3"},
        ["k_fwd_hs", "k_witems", "k_zrows"],
        ["k_fwd_hs<2,8>", "k_witems<8>", "k_zrows"]),   # k_fwd_hs takes its item factors per chunk of 3 columns
}
# a fresh engine over "manual", no grid set: mdp_engine_kernel_name(k), k = 0, 1, 2
NO_GRID = ["", "k_qrows", "k_forward"]


def _collect(paths, name, options):
    import torch

    _, m, d = INPUTS[name]
    model = mdp.Model.load(paths[name], m=m, d=d)
    g = mdp.grid(N)[0]
    with _engine(model, options) as eng:
        eng.set_grid(g, g)
        buf = torch.zeros((N, N), dtype=torch.float64, device="cuda")
        ms = eng.time_kernels(buf.data_ptr(), N, reps=1)
        torch.cuda.synchronize()
        return set(ms), eng.launched()


@pytest.mark.parametrize("rid", list(TABLE))
def test_names_and_launches(inputs, rid):   # noqa: F811
    name, options, keys, launched = TABLE[rid]
    got = _collect(inputs, name, options)
    print(f"{rid!r}: ({name!r}, {options!r},\n    {sorted(got[0])!r},\n    {sorted(got[1])!r}),")
    assert got[0] == set(keys), rid
    assert got[1] == set(launched), rid


def test_names_before_a_grid(inputs):   # noqa: F811
    from midaspom_amd._lib import lib

    _, m, d = INPUTS["manual"]
    with _engine(mdp.Model.load(inputs["manual"], m=m, d=d)) as eng:
        got = [lib().mdp_engine_kernel_name(eng._h, k).decode() for k in range(3)]
    print("NO_GRID =", got)
    assert got == NO_GRID
