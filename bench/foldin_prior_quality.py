#!/usr/bin/env python3
"""Does a per-IP topic prior from the saved model help fold-in scoring of a short batch? (CPU)

The day of tests/test_foldin_cpu.py (5000 synthetic flows, generator seed 21, K = 20, 12 training
sweeps) is trained once per model seed with every event ranked (maxresults = n, tol = 1) and saved
with its document profiles. The batch is every 5th row of that day: each IP keeps about a fifth of
its tokens. The yardstick is the training run's own ranking restricted to the batch rows, top 50;
the figure is the overlap of score_flow's top 50 with it, per prior mass (0 = no prior) and seed.

  python bench/foldin_prior_quality.py --out profiles/foldin/quality_prior_5000_k20.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=5000)
    ap.add_argument("--day-seed", type=int, default=21)
    ap.add_argument("--seeds", default="101,202,303")
    ap.add_argument("--masses", default="0,5,20,50,200")
    ap.add_argument("--step", type=int, default=5, help="the batch is every STEP-th row")
    ap.add_argument("--top", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np

    from oni355.models.saved import SavedModel
    from oni355.pipeline.flow import run_flow, score_flow
    from oni355.synth.flow import generate_flows

    day = generate_flows(a.flows, seed=a.day_seed)
    batch = {k: np.ascontiguousarray(v[::a.step]) for k, v in day.cols.items()}
    masses = [float(m) for m in a.masses.split(",")]
    out = {"day": f"generate_flows({a.flows}, seed={a.day_seed})", "K": 20, "train_sweeps": 12,
           "batch": f"rows[::{a.step}]", "top": a.top, "infer_sweeps": 30, "avg_last": 10, "overlap": {}}
    for seed in (int(s) for s in a.seeds.split(",")):
        res = run_flow(dict(day.cols), K=20, sweeps=12, tol=1.0, maxresults=day.n, device="cpu", seed=seed)
        model = SavedModel.from_run(res.lda, res.cuts, "flow")
        rows = res.rows
        yard = set((rows[rows % a.step == 0][: a.top] // a.step).tolist())
        out["overlap"][str(seed)] = {}
        for mass in masses:
            r = score_flow(dict(batch), model, tol=1.0, maxresults=a.top, device="cpu", seed=seed, prior_mass=mass)
            ov = len(yard & set(r.rows.tolist())) / a.top
            out["overlap"][str(seed)][str(mass)] = ov
            print(json.dumps({"seed": seed, "mass": mass, "overlap": ov}), flush=True)
    out["mean"] = {str(m): float(np.mean([v[str(m)] for v in out["overlap"].values()])) for m in masses}
    print(json.dumps({"mean": out["mean"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
