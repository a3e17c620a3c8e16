"""Device memory over the life of every handle: the four HIP units keep their
device allocations in owning buffers (DevBuf, csrc/spom_dev.h), which count
their live bytes (mdp_dev_live_bytes, internal).  One fresh child process
(tests/lifecycle_child.py) walks every row three times; per row and repeat the
count must be 0 before the handle exists, positive once its device side does,
and 0 again after close() -- exact, whatever other jobs do to the device's
free memory -- and what the handle computed in between must be the oracle's,
to the tolerance the parity tests hold the same input to:
  posterior engine   |dlogL| <= 1e-9 (test_gpu_parity.assert_loglik_close)
  future engine      counts, tables and states equal, integer for integer
  scenario engine    relative 1e-9 (test_gpu_scenario.close)
  scenario simulator tables equal cell for cell, lik the host formula's bits
"""
from __future__ import annotations

import functools
import json
import subprocess
import sys

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle
import scnsim_ref
import lifecycle_child as lc
from test_future_summary_host import identities, summary_checker
from test_future_wide_host import checker
from test_gpu_parity import assert_loglik_close
from test_gpu_scenario import close as scenario_close

pytestmark = pytest.mark.gpu

MDP_EINVAL, MDP_ENODEV = -1, -5


@pytest.fixture(scope="module")
def records():
    """{row id: its records in repeat order} of one child process."""
    r = subprocess.run([sys.executable, str(lc.ROOT / "tests" / "lifecycle_child.py")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("REC "):
            rec = json.loads(line[4:])
            out.setdefault(rec["row"], []).append(rec)
    return out


def lifecycle(recs, created=True):
    """Every repeat: 0 live bytes before, some while the handle lives, 0 after."""
    assert [r["rep"] for r in recs] == list(range(lc.REPEATS))
    for r in recs:
        print(r["row"], r["rep"], "live bytes before", r["before"], "created", r.get("created"), "after", r["after"])
        assert r["before"] == 0, r["before"]
        assert not created or r["created"] > 0
        assert r["after"] == 0, r["after"]


@functools.lru_cache(maxsize=None)
def posterior_reference(name, ne, nc, c_hi):
    path, obs, m, d = lc.observations(name)
    om = oracle.OracleModel.load(path, m, 0.5, d) if path else oracle.OracleModel.from_obs(obs, m, 0.5, d)
    return om.loglik_grid(*lc.axes(ne, nc, c_hi))


@pytest.mark.parametrize("rid,name,options,kernel", lc.POSTERIOR, ids=[r[0] for r in lc.POSTERIOR])
def test_posterior_engine(records, rid, name, options, kernel):
    recs = records["posterior-" + rid]
    lifecycle(recs)
    grids = [(ne, nc, hi) for hi in lc.C_HI for ne, nc in lc.GRIDS]
    for r in recs:
        assert any(kernel in k for k in r["launched"]), (kernel, r["launched"])   # real kernels, the row's path
        assert len(r["lik"]) == len(grids)
        for (ne, nc, hi), lik in zip(grids, r["lik"]):
            ref = posterior_reference(name, ne, nc, hi)
            assert np.isfinite(ref).any()
            assert_loglik_close(np.array(lik), ref)


def test_posterior_grid_refused_then_valid(records):
    """A negative c is refused (MDP_EINVAL) once the engine exists; the next
    valid grid runs correctly, and the close leaves nothing."""
    recs = records["posterior-refused-grid"]
    lifecycle(recs)
    for r in recs:
        assert r["code"] == MDP_EINVAL
        assert_loglik_close(np.array(r["lik"]), posterior_reference("manual", 3, 2, 1.0))


def test_posterior_device_refused_after_planning(records):
    recs = records["posterior-refused-device"]
    lifecycle(recs, created=False)
    assert [r["code"] for r in recs] == [MDP_ENODEV] * lc.REPEATS


def test_posterior_two_devices(records):
    if mdp.device_count() < 2:
        pytest.skip("one device visible")
    recs = records["posterior-two-devices"]
    lifecycle(recs)
    for r in recs:
        assert r["n_devices"] == 2
        assert_loglik_close(np.array(r["lik"]), posterior_reference("manual", *lc.TWO_DEV_GRID, 1.0))


@pytest.mark.parametrize("rid,n,options", lc.FUTURE, ids=[r[0] for r in lc.FUTURE])
def test_future_engine(records, rid, n, options):
    recs = records["future-" + rid]
    lifecycle(recs)
    row, post = lc.future_case(n)
    at = dict(seed=lc.FUT_SEED, rep0=lc.FUT_REP0, **lc.FUT_KW)
    counts = oracle.future_counts(row, post, tfut=lc.FUT_TFUT, nrep=lc.FUT_NREP, **at)
    assert counts.max() > 0 and counts.min() < lc.FUT_NREP   # the equality is not vacuous
    hist, occ, _ = summary_checker(row, post, lc.FUT_SMALL, lc.FUT_TFUT, **at)
    for r in recs:
        assert r["kernel"] == ("k_future_wide<1>" if options else f"k_future<{8 if n <= 8 else 16}>")
        assert np.array_equal(np.array(r["counts"], dtype=np.uint64), counts)
        got_hist, got_occ = np.array(r["hist"], dtype=np.uint64), np.array(r["occ"], dtype=np.uint64)
        identities(got_hist, got_occ, lc.FUT_SMALL)
        assert np.array_equal(got_hist, hist) and np.array_equal(got_occ, occ)
        if options:
            _, last = checker(row, post, lc.FUT_SMALL, lc.FUT_TFUT, **at)
            assert np.array_equal(np.array(r["states"], dtype=bool), last)


@functools.lru_cache(maxsize=None)
def scenario_reference(kind, grid):
    row = lc.scenario_row()
    e, c, K, d = lc.scenario_grids()[grid]
    kw = dict(ts=lc.SCN_TS, tdis=lc.SCN_TDIS, m=400, d=100)
    return np.array([[oracle.dieoff_lik(row, K, ev, cv, **kw) if kind == "dieoff" else oracle.loss_lik(row, K, d, ev, cv, **kw)
                      for cv in c] for ev in e])


@pytest.mark.parametrize("kind", lc.KINDS)
def test_scenario_engine(records, kind):
    recs = records["scenario-" + kind]
    lifecycle(recs)
    for r in recs:
        assert len(r["lik"]) == len(lc.scenario_grids())
        for grid, lik in enumerate(r["lik"]):
            ref = scenario_reference(kind, grid)
            assert (ref > 1e-14).any()
            scenario_close(np.array(lik), ref)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_scenario_simulator(records, kind):
    """(The simulator's create makes no device call: `created` is read after
    its first computing calls.)"""
    recs = records["scnsim-" + kind]
    lifecycle(recs)
    row = lc.sim_row()
    for r in recs:
        assert r["kernel"] == "k_scnsim<8>"
        assert len(r["grids"]) == len(lc.SIM_GRIDS)
        for (e, c, K, d), g in zip(lc.SIM_GRIDS, r["grids"]):
            hist, match = scnsim_ref.tables(row, lc.KINDS.index(kind), e, c, K, d, **lc.SIM_KW)
            if kind == "dieoff":
                hist, match = hist[:, :, :, 0, :], match[:, :, :, 0, :]
            assert (hist.sum(axis=-1) == lc.SIM_KW["nrep"]).all()
            assert np.array_equal(np.array(g["hist"], dtype=np.uint64), hist)
            assert np.array_equal(np.array(g["match"], dtype=np.uint64), match)
            assert np.array_equal(np.array(g["lik"]), scnsim_ref.lik(row, 0.5, match, lc.SIM_KW["nrep"]))
