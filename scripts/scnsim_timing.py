#!/usr/bin/env python
"""Timing of the scenario simulator k_scnsim<NM> beside the future engine's
lane kernel k_future<NM> of the same NM.

    python scripts/scnsim_timing.py [--nrep 10000] [--reps 3]
                                    [--out profiles/r11/scnsim/timing.jsonl]

mdp_scenario_sim_time_kernel on the reference programs' grid -- 151 K values
on [0.1, 100], 10^4 replicates per point, 20 scenario + 26 baseline years,
e = 0.03, c = 0.05 -- at n = 11, 26 and 64, die-off and loss (one source
distance; 20 distances at n = 26).  In the same process, for every n,
mdp_future_time_kernel of k_future<NM> over the same number of replicate-years
(151 x 10^4 replicates x 46 years, K_D = 1, no source, the posterior's mass at
e = 0.02..0.04, c = 0.03..0.08).  One JSON line per case: ms,
replicate-years/s, and for the simulator the ratio to k_future's rate
(yardstick: at least 0.5).

    python scripts/scnsim_timing.py --wave [--reps 3]
                                    [--out profiles/r13/scnsim_wave/timing.jsonl]

The patch-parallel k_scnsim_wave<NP> (MDP_SIM_WAVE=auto) at n = 128, 256 and
1024, die-off and loss, on the same 151 K values x 46 years, beside
k_future_wide<NP> (Future(options="MDP_FUT_WIDE=auto").time_kernel) in the
same process on the same n and the same replicate-years.  Replicates per
point, chosen so that each case runs well under a second: 1000 at n = 128,
400 at 256, 40 at 1024 (WAVE_NREP).  The yardstick is k_future_wide's rate,
not the code under test; the bar is the same half.  The simulator's record
also holds the mean final occupancy at the first and the last K, the future
engine's that after the first and the last year (the two run in different
occupancy regimes: a uniform start against the last survey row).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import midaspom_amd as mdp  # noqa: E402


def problem(n):
    rng = np.random.default_rng(n)
    row = (rng.random(n) < 0.5).astype(np.int32)
    row[rng.choice(n, size=min(4, n), replace=False)] = -1
    post = np.zeros((11, 11))
    post[2:5, 3:9] = 1.0
    w = np.ones(11)
    w[0] = w[-1] = 0.5
    return row, post * (100.0 / float((np.outer(w, w) * post).sum()))


WAVE_NREP = {128: 1000, 256: 400, 1024: 40}  # replicates per grid point


def wave_cases(reps):
    """One record per kernel and case of the --wave mode."""
    ts, tdis, nK = 20, 26, 151
    K = mdp.kgrid(nK, 0.1, 100.0)
    for n, nrep in WAVE_NREP.items():
        row, post = problem(n)
        years = nK * nrep * (ts + tdis)
        with mdp.Future(row, post, m=400.0, d=200.0, KD=1.0, KS=0.0, options="MDP_FUT_WIDE=auto") as f:
            ms = f.time_kernel(nK * nrep, ts + tdis, seed=1, reps=reps)
            fh, _ = f.summary(nK * nrep, ts + tdis, seed=1, occ=False)
            fut = {"n": n, "kernel": f.kernel, "nrep": nK * nrep, "tfut": ts + tdis, "reps": reps, "ms": ms,
                   "replicate_years_per_s": years / (ms * 1e-3),
                   "mean_occupied_first_last_year": [float(mdp.mean_occupied(fh)[i]) for i in (0, -1)]}
        yield fut
        for kind in ("dieoff", "loss"):
            dv = np.array([200.0])
            with mdp.ScenarioSim(row, kind, m=400.0, d=200.0, options="MDP_SIM_WAVE=auto") as sim:
                ms = sim.time_kernel(0.03, 0.05, K, dv, ts=ts, tdis=tdis, nrep=nrep, seed=1, reps=reps)
                hist, _ = sim.tables(0.03, 0.05, K, dv, ts=ts, tdis=tdis, nrep=nrep, seed=1, match=False)
                rate = years / (ms * 1e-3)
                yield {"n": n, "kernel": sim.kernel, "kind": kind, "points": nK, "nrep": nrep, "ts": ts, "tdis": tdis,
                       "reps": reps, "ms": ms, "replicate_years_per_s": rate,
                       "rate_over_k_future_wide": rate / fut["replicate_years_per_s"],
                       "mean_occupied_first_last_K": [float(mdp.mean_occupied(hist.reshape(-1, n + 1))[i])
                                                      for i in (0, -1)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nrep", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", action="store_true", help="time k_scnsim_wave<NP> beside k_future_wide<NP>")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sub = ("r13", "scnsim_wave") if a.wave else ("r11", "scnsim")
    out = Path(a.out or ROOT / "profiles" / sub[0] / sub[1] / "timing.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    if a.wave:
        lines = []
        for rec in wave_cases(a.reps):
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        out.write_text("".join(json.dumps(r) + "\n" for r in lines))
        return
    ts, tdis, nK = 20, 26, 151
    K = mdp.kgrid(nK, 0.1, 100.0)
    lines = []
    for n in (11, 26, 64):
        row, post = problem(n)
        years = nK * a.nrep * (ts + tdis)
        with mdp.Future(row, post, m=400.0, d=200.0, KD=1.0, KS=0.0) as f:
            ms = f.time_kernel(nK * a.nrep, ts + tdis, seed=1, reps=a.reps)
            fut = {"n": n, "kernel": f.kernel, "nrep": nK * a.nrep, "tfut": ts + tdis, "reps": a.reps, "ms": ms,
                   "replicate_years_per_s": years / (ms * 1e-3)}
        lines.append(fut)
        print(json.dumps(fut), flush=True)
        for kind, nd in [("dieoff", 1), ("loss", 1)] + ([("loss", 20)] if n == 26 else []):
            dv = mdp.dgrid(20, 200.0, 4000.0)[:nd] if nd > 1 else np.array([200.0])
            with mdp.ScenarioSim(row, kind, m=400.0, d=200.0) as sim:
                ms = sim.time_kernel(0.03, 0.05, K, dv, ts=ts, tdis=tdis, nrep=a.nrep, seed=1, reps=a.reps)
                hist, _ = sim.tables(0.03, 0.05, K, dv, ts=ts, tdis=tdis, nrep=a.nrep, seed=1, match=False)
                rate = years * nd / (ms * 1e-3)
                rec = {"n": n, "kernel": sim.kernel, "kind": kind, "points": nK * nd, "nrep": a.nrep, "ts": ts,
                       "tdis": tdis, "reps": a.reps, "ms": ms, "replicate_years_per_s": rate,
                       "rate_over_k_future": rate / fut["replicate_years_per_s"],
                       "mean_occupied_first_last_K": [float(mdp.mean_occupied(hist.reshape(-1, n + 1))[i])
                                                      for i in (0, -1)]}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    out.write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
