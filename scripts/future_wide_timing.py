#!/usr/bin/env python
"""Timing of the future engine's two kernels and of their summary variants
(DESIGN.md §12).

    python scripts/future_wide_timing.py [--nrep 100000] [--tfut 50] [--reps 3]
                                         [--out profiles/r09/future_summary/timing.jsonl]

mdp_future_time_kernel over 10^5 replicates x 50 years on generated problems
(half the patches occupied, K_D = 1, the posterior's mass at e = 0.02..0.04,
c = 0.03..0.08: over 0.9 of the patches end up occupied, so the colonisation
sums see about 0.9 n survivors a year):
  * n = 64 under k_future<64> and under k_future_wide<1> on the same problem
    -- the cost of the patch-parallel shape where the lane kernel is at its
    best; the ratio is reported;
  * n = 128, 256 and 1024 under MDP_FUT_WIDE=auto.
One JSON line per case: ms, replicate-years/s, patch-updates/s (= n x
replicate-years/s), the per-year counts' checksum (the two n = 64 runs must
agree) and, under k_future_wide, the fraction of patches occupied after the
last year in the first 256 replicates.

Every case also times the summary path (mdp_future_time_summary: hist and
occ, every window's launch) beside the plain kernel of the same engine, with
the ratio and the window plan; hist[:, 0] must equal the plain counts.  Then
config 5 of bench.py (examples/input, 7 patches, the engine's own posterior
at s = 101, 10^6 replicates x 50 years), and the window length against
occupancy: n = 256 and 1024 again under MDP_FUT_SUM_YEARS = 1 and 2 (less LDS
per workgroup, more launches and record traffic).
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
    row[rng.choice(n, size=4, replace=False)] = -1
    post = np.zeros((11, 11))
    post[2:5, 3:9] = 1.0
    w = np.ones(11)
    w[0] = w[-1] = 0.5
    return row, post * (100.0 / float((np.outer(w, w) * post).sum()))


def summary_fields(f, n, nrep, tfut, reps, ms, counts):
    """time_summary beside time_kernel's `ms`, after checking the tables."""
    hist, occ = f.summary(nrep, tfut, seed=1)
    assert np.array_equal(hist[:, 0], counts), "hist[:, 0] differs from the plain counts"
    assert int((hist * np.arange(n + 1, dtype=np.uint64)).sum()) == int(occ.sum())
    sms = f.time_summary(nrep, tfut, seed=1, reps=reps)
    return {"summary_ms": sms, "summary_over_kernel": sms / ms, "mean_occupied_last": float(mdp.mean_occupied(hist)[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nrep", type=int, default=100_000)
    ap.add_argument("--tfut", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r09" / "future_summary" / "timing.jsonl"))
    a = ap.parse_args()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    lines = []
    ms64 = {}
    for n, options in [(64, "MDP_FUT_WIDE=0"), (64, "MDP_FUT_WIDE=1"), (128, "MDP_FUT_WIDE=auto"),
                       (256, "MDP_FUT_WIDE=auto"), (1024, "MDP_FUT_WIDE=auto")]:
        row, post = problem(n)
        with mdp.Future(row, post, m=400.0, d=100.0, KD=1.0, KS=0.0, options=options) as f:
            counts = f.simulate(a.nrep, a.tfut, seed=1)
            ms = f.time_kernel(a.nrep, a.tfut, seed=1, reps=a.reps)
            rec = {"n": n, "options": options, "kernel": f.kernel, "nrep": a.nrep, "tfut": a.tfut, "reps": a.reps,
                   "ms": ms, "replicate_years_per_s": a.nrep * a.tfut / (ms * 1e-3),
                   "patch_updates_per_s": n * a.nrep * a.tfut / (ms * 1e-3),
                   "counts_sum": int(counts.sum()), "counts_last": int(counts[-1])}
            if "wide" in rec["kernel"]:  # what the survivor walk sees: occupied patches per replicate
                rec["occupied_fraction"] = float(f.states(256, a.tfut, seed=1).mean())
            rec.update(summary_fields(f, n, a.nrep, a.tfut, a.reps, ms, counts))
        if n == 64:
            ms64[rec["kernel"]] = (ms, rec["counts_sum"])
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    (lane_ms, lane_sum), (wide_ms, wide_sum) = ms64["k_future<64>"], ms64["k_future_wide<1>"]
    assert lane_sum == wide_sum, "the two kernels disagree at n = 64"
    rec = {"n": 64, "ratio_wide_over_lane": wide_ms / lane_ms}
    lines.append(rec)
    print(json.dumps(rec), flush=True)
    # config 5 of bench.py: the lane kernel's best case
    inp = ROOT / "tests" / "golden" / "occupancies.txt"
    post_lik, ltot = mdp.run_file(inp, None, m=400.0, d=100.0, s=101)
    _, _, row = mdp.read_survey(inp)
    with mdp.Future(row, mdp.posterior(post_lik, ltot), m=400.0, d=100.0) as f:
        counts = f.simulate(1_000_000, 50, seed=20161014)
        ms = f.time_kernel(1_000_000, 50, seed=20161014, reps=a.reps)
        hist, occ = f.summary(1_000_000, 50, seed=20161014)
        assert np.array_equal(hist[:, 0], counts)
        sms = f.time_summary(1_000_000, 50, seed=20161014, reps=a.reps)
        rec = {"n": int(row.size), "case": "config5", "kernel": f.kernel, "nrep": 1_000_000, "tfut": 50, "reps": a.reps,
               "ms": ms, "summary_ms": sms, "summary_over_kernel": sms / ms, "counts_last": int(counts[-1]),
               "mean_occupied_last": float(mdp.mean_occupied(hist)[-1])}
    lines.append(rec)
    print(json.dumps(rec), flush=True)
    # window length against occupancy: shorter windows, less LDS per workgroup
    for n in (256, 1024):
        row, post = problem(n)
        for cap in (1, 2):
            with mdp.Future(row, post, m=400.0, d=100.0, KD=1.0, KS=0.0,
                            options=f"MDP_FUT_WIDE=auto;MDP_FUT_SUM_YEARS={cap}") as f:
                rec = {"n": n, "kernel": f.kernel, "sum_years": cap, "nrep": a.nrep, "tfut": a.tfut, "reps": a.reps,
                       "summary_ms": f.time_summary(a.nrep, a.tfut, seed=1, reps=a.reps)}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    out.write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
