#!/usr/bin/env python
"""Timing of the scenario chain (k_scnchain<NM>, k_chain_eval) beside the
trajectory path k_scnsim<NM> on the reference-shaped job.

    python scripts/chain_timing.py [--reps 3] [--out profiles/r16/scnchain/timing.jsonl]

A 26-patch first row, ts = 20, tdis = 26, e = 0.03, c = 0.05, 1000 K values
on [0.1, 100] (die-off) and 1000 K x 46 source distances (loss), 1000
replicates per class and grid point, 100 000 per class of the baseline year.
In one process, per kind:

* mdp_scenario_chain_time_kernels: the baseline counts, the scenario counts
  and the two evaluations (ms each), and their sum;
* mdp_scenario_sim_time_kernel of k_scnsim<32> on the same grid with 1000
  replicates per point: whole trajectories of 46 years, the histogram alone
  (the row has 11 missing patches, past what the match table holds).

One JSON line per kind with the three times, the ratio trajectory / chain and
the simulated replicate-years of each path.
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

N, TS, TDIS, NK, ND, NREP, NBASE = 26, 20, 26, 1000, 46, 1000, 100_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = Path(a.out or ROOT / "profiles" / "r16" / "scnchain" / "timing.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(N)
    row = (rng.random(N) < 0.5).astype(np.int32)
    row[rng.choice(N, size=11, replace=False)] = -1
    K = mdp.kgrid(NK, 0.1, 100.0)
    lines = []
    for kind, nd in (("dieoff", 1), ("loss", ND)):
        dv = mdp.dgrid(nd, 200.0, 4000.0) if nd > 1 else np.array([200.0])
        points = NK * nd
        with mdp.ScenarioChain(row, kind, m=400.0, d=200.0) as ch:
            ms = ch.time_kernels(0.03, 0.05, K, dv, ts=TS, tdis=TDIS, nrep=NREP, nbase=NBASE, seed=1, reps=a.reps)
            name = ch.kernel
        with mdp.ScenarioSim(row, kind, m=400.0, d=200.0) as sim:
            traj = sim.time_kernel(0.03, 0.05, K, dv, ts=TS, tdis=TDIS, nrep=NREP, seed=1, reps=a.reps)
            sim_name = sim.kernel
        total = sum(ms.values())
        chain_years = (points * NREP + NBASE) * (N + 1)
        rec = {"n": N, "kind": kind, "points": points, "ts": TS, "tdis": TDIS, "nrep": NREP, "nbase": NBASE,
               "reps": a.reps, "kernel": name, "ms_base_counts": ms["base_counts"], "ms_scn_counts": ms["scn_counts"],
               "ms_eval": ms["eval"], "ms_chain": total, "chain_replicate_years": chain_years,
               "chain_replicate_years_per_s": chain_years / ((ms["base_counts"] + ms["scn_counts"]) * 1e-3),
               "trajectory_kernel": sim_name, "ms_trajectory": traj,
               "trajectory_replicate_years": points * NREP * (TS + TDIS),
               "trajectory_replicate_years_per_s": points * NREP * (TS + TDIS) / (traj * 1e-3),
               "trajectory_over_chain": traj / total}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    out.write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
