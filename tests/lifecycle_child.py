"""The child process of tests/test_gpu_lifecycle.py, and the rows both sides
share.  Run as a program it walks every row in a fresh process -- no other
engine alive, nothing garbage-collected mid-row -- and prints one JSON record
per row and repeat ("REC " + json): mdp_dev_live_bytes() before the handle is
created, once its device side exists, and after close(), with what the handle
computed in between.  It asserts nothing; the parent does."""
from __future__ import annotations

import ctypes
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT / "tests"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)

REPEATS = 3
GOLDEN = ROOT / "tests" / "golden"

# ---------------------------------------------------------------------------
# posterior engine: (row id, input of test_plan_host.INPUTS, options, a kernel the row must have launched)
# ---------------------------------------------------------------------------
POSTERIOR = [
    ("manual-fused", "manual", "", "mdp_fwd_jit<fused"),
    ("manual-unfused", "manual", "MDP_FUSED=0", "k_qrows<"),
    ("manual-generic", "manual", "MDP_JIT=0", "k_coefs<"),
    ("config2-chunks-gather", "config2", "MDP_JIT_CHUNK=40;MDP_JIT_GATHER=1", ",gather>"),
    ("config2-qglobal", "config2", "MDP_QGLOBAL=1", "k_wq"),
    ("s64-vlds", "s64", "", "mdp_fwd_jit<reading"),
    ("s128-hs", "s128", "", "k_fwd_hs<"),
    ("s128-plain", "s128", "MDP_WIDE_MMA=0", "k_fwd_wide"),
    ("s128-mma", "s128", "MDP_WIDE_MMA=1", "k_fwd_mma<"),
    ("s128-mmt", "s128", "MDP_WIDE_MMA=2", "k_fwd_mmt<"),
]
# the grids of a row, in order: the second reallocates, the third keeps the
# allocation; all three under c in [0, 1], then under c in [0, 2] (the c
# tables are rebuilt and uploaded again)
GRIDS = [(3, 2), (70, 5), (3, 2)]
C_HI = [1.0, 2.0]
TWO_DEV_GRID = (5, 4)


def observations(name):
    """(golden file or None, observation matrix or None, m, d) of an input."""
    from test_plan_host import INPUTS
    src, m, d = INPUTS[name]
    return (GOLDEN / src, None, m, d) if isinstance(src, str) else (None, src(), m, d)


def axes(ne, nc, c_hi):
    """Interior points (the likelihood is 0 on the edges e = 0, e = 1 and c = 0); the largest c is c_hi."""
    return np.linspace(0.05, 0.95, ne), np.linspace(0.1 * c_hi, c_hi, nc)


# ---------------------------------------------------------------------------
# future engine: the smallest rows of test_gpu_future_wide.test_wide_kernel_equals_the_oracle
# (id, patches, options; None: mdp_future_create).  k_future<8> builds the
# colonisation table, k_future<16> does not.
# ---------------------------------------------------------------------------
FUTURE = [("lane-n1-table", 1, None), ("lane-n9", 9, None), ("wide-n1", 1, "MDP_FUT_WIDE=1")]
FUT_KW = dict(m=400.0, d=100.0, KD=1.0, KS=0.0, dS=200.0)
FUT_NREP, FUT_TFUT, FUT_SEED, FUT_REP0 = 3000, 10, (1 << 35) + 8, (1 << 32) - 1500
FUT_SMALL = 300   # replicates of the summary and of the states (the numpy checkers' size)


def future_case(n):
    from test_future_wide_host import make_row
    from test_gpu_future_wide import NMISS, harsh21
    return make_row(n, NMISS[n], 0.5 if n < 9 else 0.15, seed=40 + n), harsh21() * 0.5


# ---------------------------------------------------------------------------
# scenario engine (the manual's 5-patch row of test_gpu_scenario, on the grid
# of its test_examples_input_grid_vs_oracle) and scenario simulator
# (test_gpu_scnsim.test_sizes, n = 1): two grids, growing
# ---------------------------------------------------------------------------
KINDS = ("dieoff", "loss")
SCN_TS, SCN_TDIS = 7, 4


def scenario_grids():
    import midaspom_amd as mdp
    e, c = np.array([0.05, 0.3, 0.9, 1.4]), np.array([0.1, 0.6, 2.0])
    return [(e[:2], c[:2], mdp.kgrid(3), mdp.dgrid(2)), (e, c, mdp.kgrid(5), mdp.dgrid(3))]


def scenario_row():
    import midaspom_amd as mdp
    return mdp.first_row(GOLDEN / "manual_p3_obs.txt")


SIM_GRIDS = [([0.2], [0.3], [0.4, 1.0], [200.0]), ([0.2, 0.5], [0.3, 0.9], [0.4, 1.0, 3.0], [200.0, 900.0])]
SIM_KW = dict(ts=3, tdis=2, nrep=300, seed=8)


def sim_row():
    import scnsim_ref
    return scnsim_ref.synthetic_row(1, 1)


# ---------------------------------------------------------------------------
# the child
# ---------------------------------------------------------------------------
def main():
    import midaspom_amd as mdp
    from midaspom_amd import _lib

    fn = _lib.lib().mdp_dev_live_bytes   # internal (mdp_internal.h): not among _lib.SIGNATURES
    fn.restype, fn.argtypes = ctypes.c_ulonglong, []

    def live():
        return int(fn())

    def emit(**rec):
        print("REC " + json.dumps(rec), flush=True)

    def code_of(call):
        try:
            call()
        except mdp.MidaspomError as exc:
            return exc.code
        return 0

    def model_of(name):
        path, obs, m, d = observations(name)
        return mdp.Model.load(path, m=m, d=d) if path else mdp.Model.from_obs(obs, m=m, d=d)

    for rid, name, options, _ in POSTERIOR:
        model = model_of(name)
        for rep in range(REPEATS):
            before = live()
            eng = mdp.Engine(model, devices=[0], options=options)
            created = live()
            lik = [eng.loglik_grid(*axes(ne, nc, hi)).tolist() for hi in C_HI for ne, nc in GRIDS]
            launched = sorted(eng.launched())
            eng.close()
            emit(row="posterior-" + rid, rep=rep, before=before, created=created, after=live(), lik=lik,
                 launched=launched)

    model = model_of("manual")
    for rep in range(REPEATS):
        # a grid refused once the engine exists; then a valid one
        before = live()
        eng = mdp.Engine(model, devices=[0], options="")
        created = live()
        e, c = axes(3, 2, 1.0)
        refused = code_of(lambda: eng.set_grid(e, np.array([-0.5, 1.0])))
        lik = eng.loglik_grid(e, c).tolist()
        eng.close()
        emit(row="posterior-refused-grid", rep=rep, before=before, created=created, after=live(), code=refused, lik=lik)
        # a device refused after the engine was planned
        before = live()
        refused = code_of(lambda: mdp.Engine(model, devices=[99], options=""))
        emit(row="posterior-refused-device", rep=rep, before=before, after=live(), code=refused)
        if mdp.device_count() >= 2:
            before = live()
            eng = mdp.Engine(model, devices=[0, 1], options="")
            created = live()
            lik = eng.loglik_grid(*axes(*TWO_DEV_GRID, 1.0)).tolist()
            n_devices = eng.info()["n_devices"]
            eng.close()
            emit(row="posterior-two-devices", rep=rep, before=before, created=created, after=live(), lik=lik,
                 n_devices=n_devices)

    for rid, n, options in FUTURE:
        row, post = future_case(n)
        for rep in range(REPEATS):
            before = live()
            f = mdp.Future(row, post, options=options, **FUT_KW)
            created = live()
            kernel = f.kernel
            counts = f.simulate(FUT_NREP, FUT_TFUT, seed=FUT_SEED, rep0=FUT_REP0)
            hist, occ = f.summary(FUT_SMALL, FUT_TFUT, seed=FUT_SEED, rep0=FUT_REP0)
            states = f.states(FUT_SMALL, FUT_TFUT, seed=FUT_SEED, rep0=FUT_REP0) if options else None
            f.close()
            emit(row="future-" + rid, rep=rep, before=before, created=created, after=live(), kernel=kernel,
                 counts=counts.tolist(), hist=hist.tolist(), occ=occ.tolist(),
                 states=None if states is None else states.astype(int).tolist())

    for kind in KINDS:
        for rep in range(REPEATS):
            before = live()
            sc = mdp.Scenario(scenario_row(), kind, m=400, d=100)
            created = live()
            lik = [sc.lik(e, c, K, d, ts=SCN_TS, tdis=SCN_TDIS).tolist() for e, c, K, d in scenario_grids()]
            sc.close()
            emit(row="scenario-" + kind, rep=rep, before=before, created=created, after=live(), lik=lik)
    for kind in KINDS:
        for rep in range(REPEATS):
            before = live()
            sim = mdp.ScenarioSim(sim_row(), kind)   # (no device call yet: its first computing call sets the device up)
            out = []
            for e, c, K, d in SIM_GRIDS:
                hist, match = sim.tables(e, c, K, d if kind == "loss" else None, **SIM_KW)
                out.append(dict(hist=hist.tolist(), match=match.tolist(), lik=sim.lik(match, SIM_KW["nrep"]).tolist()))
            created = live()
            kernel = sim.kernel
            sim.close()
            emit(row="scnsim-" + kind, rep=rep, before=before, created=created, after=live(), kernel=kernel, grids=out)


if __name__ == "__main__":
    main()
