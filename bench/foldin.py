#!/usr/bin/env python3
"""Interleaved A/B of fold-in scoring against training on ONE generated flow day (one process):

  train    run_flow at the bench.py default shape (the day trains its own model)
  infer    score_flow against a model trained once (every sweep of a single-chunk document in one
           launch)
  unfused  score_flow with sweep fusion off (one launch per sweep)
  prior    score_flow, fused, with the model's per-IP topic profiles as priors (--prior-mass)

  python bench/foldin.py --flows 12500000 --topics 20 --rounds 3 --out profiles/foldin/bench.json

Prints one JSON line per day and a summary: median / min ms per day, ms per fold-in sweep (the
``foldin`` stage over the fold-in sweeps) and the run-to-run spread (max − min) of every variant.
The model is saved with its document profiles; ``model_bytes`` is the size of that file with and
without them. ``--variants`` picks the variants that alternate (default: all four).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=12_500_000)
    ap.add_argument("--topics", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=200, help="training sweeps")
    ap.add_argument("--infer-sweeps", type=int, default=30)
    ap.add_argument("--avg-last", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--prior-mass", type=float, default=5.0, help="the prior variant's mass")
    ap.add_argument("--variants", default="train,infer,unfused,prior")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--source", choices=["flow", "dns", "proxy"], default="flow",
                    help="the day's source (--flows events; --topics is 20 unless given: pass 50 for a default dns day)")
    a = ap.parse_args()
    import torch

    from oni355.models.saved import SavedModel

    dev = torch.device(a.device)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    kw = dict(tol=1.0, maxresults=3000, device=dev)
    if a.source == "flow":
        from oni355.pipeline.flow import run_flow, score_flow
        from oni355.synth.flow import generate_flows
        day = generate_flows(a.flows, seed=a.seed, n_hosts=max(64, a.flows // 25))
    elif a.source == "dns":
        from oni355.pipeline import dns
        from oni355.synth.dns import generate_dns
        day = generate_dns(a.flows, seed=a.seed, user_domain="intel")

        def run_flow(cols, **k):
            return dns.run_dns(cols, user_domain="intel", **k)
        score_flow = dns.score_dns
    else:
        from oni355.pipeline import proxy
        from oni355.synth.proxy import generate_proxy
        day = generate_proxy(a.flows, seed=a.seed)
        run_flow, score_flow = proxy.run_proxy, proxy.score_proxy
    print(f"generated {a.flows} {a.source} events in {time.perf_counter() - t0:.1f} s", flush=True)
    # the model is trained once (this untimed day is also the warm-up of the training variant)
    first = run_flow(day.cols, K=a.topics, sweeps=a.sweeps, **kw)
    if a.source == "flow":
        model = SavedModel.from_run(first.lda, first.cuts, "flow", {"day": "bench"})
    elif a.source == "dns":
        model = dns.model_from_result(first, None, "intel", {"day": "bench"})
    else:
        model = proxy.model_from_result(first, None, {"day": "bench"})
    with tempfile.TemporaryDirectory() as td:
        model_bytes = {"with_docs": os.path.getsize(model.save(os.path.join(td, "m.npz"))),
                       "without_docs": os.path.getsize(model.without_docs().save(os.path.join(td, "m0.npz")))}
    print(json.dumps({"model_bytes": model_bytes, "model_docs": int(model.doc_keys.shape[0]), "V": model.V}), flush=True)
    top_train = set(first.rows.tolist())
    del first
    ikw = dict(sweeps=a.infer_sweeps, avg_last=a.avg_last, **kw)
    variants = {"train": lambda: run_flow(day.cols, K=a.topics, sweeps=a.sweeps, **kw),
                "infer": lambda: score_flow(day.cols, model, **ikw),
                "unfused": lambda: score_flow(day.cols, model, fuse=False, **ikw),
                "prior": lambda: score_flow(day.cols, model, prior_mass=a.prior_mass, **ikw)}
    variants = {n: variants[n] for n in a.variants.split(",")}
    for n, fn in variants.items():  # untimed warm-up of the fold-in variants
        if n != "train":
            fn()
    days = {n: [] for n in variants}
    for r in range(a.rounds):
        for name, fn in variants.items():
            sync()
            ts = time.perf_counter()
            res = fn()
            sync()
            wall = time.perf_counter() - ts
            t = res.timings
            line = {"variant": name, "round": r, "day_ms": round(wall * 1e3, 2)}
            if name == "train":
                line["ms_per_sweep"] = round(t.get("train_dev_s", t.get("train_s", 0.0)) / a.sweeps * 1e3, 4)
            else:
                line["ms_per_sweep"] = round(t.get("foldin_dev_s", t.get("foldin_s", 0.0)) / max(a.infer_sweeps, 1) * 1e3, 4)
                # the stage that maps the batch's words into the model's vocabulary
                line["vocab_ms"] = round(t.get("vocab_dev_s", t.get("vocab_s", 0.0)) * 1e3, 4)
                line["vocab_wall_ms"] = round(t.get("vocab_s", 0.0) * 1e3, 4)  # host time of the stage
                line["launches"] = res.stats["foldin_launches"]
                if name == "prior":
                    line["n_prior_docs"] = res.stats["n_prior_docs"]
                line["overlap_with_training"] = round(len(top_train & set(res.rows.tolist())) / max(len(top_train), 1), 4)
            days[name].append(line)
            print(json.dumps(line), flush=True)
            del res

    def summ(v):
        d, s = [x["day_ms"] for x in v], [x["ms_per_sweep"] for x in v]
        out = {"day_ms_median": statistics.median(d), "day_ms_min": min(d), "day_ms_spread": round(max(d) - min(d), 2),
               "ms_per_sweep_median": statistics.median(s), "ms_per_sweep_min": min(s),
               "ms_per_sweep_spread": round(max(s) - min(s), 4)}
        if all("vocab_ms" in x for x in v):
            vo = [x["vocab_ms"] for x in v]
            out.update({"vocab_ms_median": statistics.median(vo), "vocab_ms_min": min(vo),
                        "vocab_ms_spread": round(max(vo) - min(vo), 4)})
        return out
    summary = {n: summ(v) for n, v in days.items()}
    out = {"source": a.source, "flows": a.flows, "topics": a.topics, "train_sweeps": a.sweeps, "infer_sweeps": a.infer_sweeps,
           "avg_last": a.avg_last, "rounds": a.rounds, "prior_mass": a.prior_mass, "model_bytes": model_bytes,
           "summary": summary, "days": days}
    print(json.dumps({"summary": summary}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
