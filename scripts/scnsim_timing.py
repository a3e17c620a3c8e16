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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nrep", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r11" / "scnsim" / "timing.jsonl"))
    a = ap.parse_args()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
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
