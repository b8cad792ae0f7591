#!/usr/bin/env python3
"""Whole days of Gibbs and variational-EM training alternating in ONE process on ONE generated day:

  gibbs   run_flow / run_dns at the bench.py default shape (the collapsed-Gibbs sampler)
  vem     the same day with method="vem" (models.vem_gpu.VarLDA: --em-iters × --var-iters)

  python bench/vem_day.py --flows 12500000 --topics 20 --rounds 3 --out profiles/vem/flow_k20.json
  python bench/vem_day.py --source dns --flows 2000000 --topics 50 --out profiles/vem/dns_k50.json

Prints one JSON line per day (ms per day, ms of the train stage, planted recall in the top-N) and a
summary with the median / min / spread of each variant. After the timed days, untimed:

  * the likelihood trace of one vem day per EM iteration (eval_every=1);
  * the split of one EM iteration, each op timed alone with device events on the last vem day's
    corpus (median of --op-reps): E-step (ops.vfold), resp, wsum, table;
  * the overlap of the vem day's top-N with the Gibbs days' and the Gibbs days' among themselves
    (every Gibbs round runs its own seed).

``--em-tol X`` runs another comparison instead (no Gibbs days): the fixed ``--em-iters`` day, the day
with ``em_tol=X`` (at most ``--em-max`` iterations) and the fixed day with ``estimate_alpha``,
alternating in one process; per variant the iterations run, ms per day, the final variational bound,
the overlap of its top-N with the fixed day's and the planted recall; the α trace; and ops.vem_bound
timed alone with device events next to ops.doc_fit on the same pairs.

  python bench/vem_day.py --em-tol 1e-4 --out profiles/vem/bound_flow_12.5M_k20.json

``--var-tol X[,Y…]`` runs a third comparison (no Gibbs days): the fixed day and, per tolerance, the day
with ``var_tol`` alone and with ``var_tol`` + ``warm_start``, alternating in one process; per variant
ms per day and per EM iteration, the ``var_iters_trace``, the final bound, the overlap of its top-N
with the fixed day's and the planted recall. Then, with device events on the fixed day's final table:
ops.vfold against ops.vfold_exit(tol=0) (what the exit machinery costs), the E-step with each
tolerance from the cold start and from the previous γ, and what the lockstep of a round costs
(Σ n_it against Σ over rounds of documents × the round's largest n_it).

  python bench/vem_day.py --var-tol 1e-3,1e-5 --out profiles/vem/exit_flow_12.5M_k20.json

``--cvb-iters N`` runs a fourth comparison: Gibbs, vem (fixed ``--em-iters`` × ``--var-iters``) and batch
CVB0 (method="cvb0", N iterations) days alternating in one process; per variant ms per day and of the
train stage and the planted recall; the overlap of the cvb0 top-N with every Gibbs seed's and vem's next
to the Gibbs seed-to-seed overlap; the cvb0 likelihood trace per iteration; and, with device events,
ops.cvb0_update and the word sum each alone next to a device copy of the bytes an iteration must move.

  python bench/vem_day.py --cvb-iters 100 --out profiles/cvb0/flow_12.5M_k20.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def op_split(model, reps: int) -> dict:
    """Median device ms of the four ops of one EM iteration on ``model``'s corpus and table."""
    import torch

    from oni355 import ops
    pw, pc, ptr = model._pairs
    wm_ptr, wm_doc, wm_word, wm_pos = ops.vem_word_major(pw, model._pair_doc, model.V)
    _, gamma = ops.vfold(pw, pc, ptr, model.table, model.K, model.alpha, None, model.var_iters, want_gamma=True)
    e, q = ops.vem_resp(gamma, model.table, model._pair_doc, pw, pc, model.K, wm_pos)
    ss = ops.vem_wsum(e, q, model.table, wm_ptr, wm_doc, wm_word, model.V, model.K)
    steps = {"estep": lambda: ops.vfold(pw, pc, ptr, model.table, model.K, model.alpha, None, model.var_iters, want_gamma=True),
             "resp": lambda: ops.vem_resp(gamma, model.table, model._pair_doc, pw, pc, model.K, wm_pos),
             "wsum": lambda: ops.vem_wsum(e, q, model.table, wm_ptr, wm_doc, wm_word, model.V, model.K),
             "table": lambda: ops.vem_table(ss, model.K, model.beta)}
    out = {}
    for name, fn in steps.items():
        ms = []
        for _ in range(reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        ms = ms[2:]  # the first two warm the caches and the allocator
        out[name] = {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                     "ms_spread": round(max(ms) - min(ms), 4)}
    return out


def _timed(fn, reps: int) -> dict:
    import torch
    ms = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = ms[2:]  # the first two warm the caches and the allocator
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
            "ms_spread": round(max(ms) - min(ms), 4)}


def bound_ab(a, run, day, kw: dict, planted: set, dev) -> int:
    """The ``--em-tol`` comparison of the module text."""
    import torch

    from oni355 import ops
    base = dict(method="vem", var_iters=a.var_iters, **kw)
    variants = {"fixed": dict(em_iters=a.em_iters), "tol": dict(em_iters=a.em_max, em_tol=a.em_tol),
                "alpha": dict(em_iters=a.em_iters, estimate_alpha=True)}
    for v in variants.values():  # one untimed day each
        run(day.cols, **v, **base)
    days = {n: [] for n in variants}
    tops, models = {}, {}
    for r in range(a.rounds):
        for name, v in variants.items():
            torch.cuda.synchronize(dev)
            ts = time.perf_counter()
            res = run(day.cols, **v, **base)
            torch.cuda.synchronize(dev)
            wall = time.perf_counter() - ts
            m, rows = res.lda.model, set(res.rows.tolist())
            line = {"variant": name, "round": r, "day_ms": round(wall * 1e3, 2), "em_iters_done": int(m.sweeps_done),
                    "train_ms": round(res.timings.get("train_dev_s", res.timings.get("train_s", 0.0)) * 1e3, 3),
                    "bound": m.bound(), "loglik": res.stats["loglik"], "alpha": float(m.alpha),
                    "planted_recall_topN": round(len(rows & planted) / max(len(planted), 1), 4)}
            days[name].append(line)
            tops[name], models[name] = rows, m
            print(json.dumps(line), flush=True)
            del res
    n_top = max(len(tops["fixed"]), 1)
    summary = {n: {"day_ms_median": statistics.median(x["day_ms"] for x in v),
                   "day_ms_spread": round(max(x["day_ms"] for x in v) - min(x["day_ms"] for x in v), 2),
                   "em_iters_done": v[-1]["em_iters_done"], "bound": v[-1]["bound"], "alpha": v[-1]["alpha"],
                   "planted_recall_topN": v[-1]["planted_recall_topN"],
                   "top_overlap_with_fixed": round(len(tops[n] & tops["fixed"]) / n_top, 4)} for n, v in days.items()}
    m = models["fixed"]
    pw, pc, ptr = m._pairs
    theta, gamma = ops.vfold(pw, pc, ptr, m.table, m.K, m.alpha, None, m.var_iters, want_gamma=True)
    ops_ms = {"vem_bound": _timed(lambda: ops.vem_bound(gamma, m.table, m._pair_doc, pw, pc, m.K, m.alpha, ptr), a.op_reps),
              # the same γ without pairs: the row pass (ψ, lgamma) with the document and total passes
              "vem_bound_rows_only": _timed(lambda: ops.vem_bound(gamma, m.table, m._pair_doc[:0], pw[:0], pc[:0], m.K,
                                                                  m.alpha, torch.zeros_like(ptr)), a.op_reps),
              "doc_fit": _timed(lambda: ops.doc_fit(theta, m.table, m._pair_doc, pw, pc, m.c.D, m.V), a.op_reps),
              "estep": _timed(lambda: ops.vfold(pw, pc, ptr, m.table, m.K, m.alpha, None, m.var_iters), a.op_reps)}
    out = {"source": a.source, "flows": a.flows, "topics": a.topics, "em_iters": a.em_iters, "em_max": a.em_max,
           "em_tol": a.em_tol, "var_iters": a.var_iters, "rounds": a.rounds, "pairs": int(pw.numel()), "docs": int(m.c.D),
           "summary": summary, "ops_ms": ops_ms,
           "bound_trace_tol": [list(b) for b in models["tol"].bounds],
           "alpha_trace": [[int(i), float(al)] for i, _, _, al in models["alpha"].bounds] + [[int(models["alpha"].sweeps_done), float(models["alpha"].alpha)]],
           "days": days}
    print(json.dumps({"summary": summary, "ops_ms": ops_ms, "alpha_trace": out["alpha_trace"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


def lockstep(n_it, ptr) -> dict:
    """Updates the documents of the rounds needed against updates the rounds ran in lockstep: a wave
    owns 16 consecutive documents and packs them, in order, into rounds of at most 64 pairs
    (k_vfold_exit); a document over 64 pairs is the block path's and waits for nobody."""
    import numpy as np
    size = np.diff(ptr)
    need = ran = nbig = 0
    for w0 in range(0, size.size, 16):
        docs, used, top = 0, 0, 0
        for d in range(w0, min(w0 + 16, size.size)):
            if size[d] > 64:
                nbig += 1
                continue
            if docs and used + size[d] > 64:
                ran += docs * top
                docs, used, top = 0, 0, 0
            docs, used, top = docs + 1, used + int(size[d]), max(top, int(n_it[d]))
            need += int(n_it[d])
        ran += docs * top
    return {"updates_needed": need, "updates_in_lockstep": ran, "ratio": round(ran / max(need, 1), 4), "block_path_docs": nbig}


def exit_ab(a, run, day, kw: dict, planted: set, dev) -> int:
    """The ``--var-tol`` comparison of the module text."""
    import torch

    from oni355 import ops
    tols = [float(x) for x in a.var_tol.split(",")]
    base = dict(method="vem", em_iters=a.em_iters, var_iters=a.var_iters, **kw)
    variants = {"fixed": {}}
    for x in tols:
        variants[f"tol{x:g}"] = dict(var_tol=x)
        variants[f"tol{x:g}_warm"] = dict(var_tol=x, warm_start=True)
    for v in variants.values():  # one untimed day each
        run(day.cols, **v, **base)
    days = {n: [] for n in variants}
    tops, models = {}, {}
    for r in range(a.rounds):
        for name, v in variants.items():
            torch.cuda.synchronize(dev)
            ts = time.perf_counter()
            res = run(day.cols, **v, **base)
            torch.cuda.synchronize(dev)
            wall = time.perf_counter() - ts
            m, rows = res.lda.model, set(res.rows.tolist())
            train_ms = res.timings.get("train_dev_s", res.timings.get("train_s", 0.0)) * 1e3
            line = {"variant": name, "round": r, "day_ms": round(wall * 1e3, 2), "train_ms": round(train_ms, 3),
                    "ms_per_em_iter": round(train_ms / max(a.em_iters, 1), 4), "bound": m.bound(),
                    "loglik": res.stats["loglik"], "var_iters_trace": [round(x, 3) for x in m.var_iters_trace],
                    "planted_recall_topN": round(len(rows & planted) / max(len(planted), 1), 4)}
            days[name].append(line)
            tops[name], models[name] = rows, m
            print(json.dumps(line), flush=True)
            del res
    n_top = max(len(tops["fixed"]), 1)

    def med(v, key):
        return statistics.median(x[key] for x in v)
    summary = {n: {"day_ms_median": med(v, "day_ms"),
                   "day_ms_spread": round(max(x["day_ms"] for x in v) - min(x["day_ms"] for x in v), 2),
                   "ms_per_em_iter_median": med(v, "ms_per_em_iter"), "bound": v[-1]["bound"],
                   "var_iters_trace": v[-1]["var_iters_trace"], "planted_recall_topN": v[-1]["planted_recall_topN"],
                   "top_overlap_with_fixed": round(len(tops[n] & tops["fixed"]) / n_top, 4)} for n, v in days.items()}
    m = models["fixed"]
    pw, pc, ptr = m._pairs
    args = (pw, pc, ptr, m.table, m.K, m.alpha, None, m.var_iters)
    # the warm start's best case: the E-step restarted from its own fixed-count γ against the same table
    # (an EM that has converged); the days' var_iters_trace has what the real iterations needed
    _, g_prev = ops.vfold(*args, want_gamma=True)
    ops_ms = {"vfold": _timed(lambda: ops.vfold(*args, want_gamma=True), a.op_reps),
              "vfold_exit_tol0": _timed(lambda: ops.vfold_exit(*args, 0.0), a.op_reps)}
    lock = {}
    for x in tols:
        ops_ms[f"vfold_exit_tol{x:g}_cold"] = _timed(lambda: ops.vfold_exit(*args, x), a.op_reps)
        ops_ms[f"vfold_exit_tol{x:g}_from_converged"] = _timed(lambda: ops.vfold_exit(*args, x, g_prev), a.op_reps)
        n_cold = ops.vfold_exit(*args, x)[2].cpu().numpy()
        n_warm = ops.vfold_exit(*args, x, g_prev)[2].cpu().numpy()
        hp = ptr.cpu().numpy()
        lock[f"tol{x:g}_cold"] = dict(lockstep(n_cold, hp), n_it_mean=round(float(n_cold.mean()), 3))
        lock[f"tol{x:g}_from_converged"] = dict(lockstep(n_warm, hp), n_it_mean=round(float(n_warm.mean()), 3))
    out = {"source": a.source, "flows": a.flows, "topics": a.topics, "em_iters": a.em_iters, "var_iters": a.var_iters,
           "var_tol": tols, "rounds": a.rounds, "pairs": int(pw.numel()), "docs": int(m.c.D), "summary": summary,
           "ops_ms": ops_ms, "lockstep": lock, "days": days}
    print(json.dumps({"summary": summary, "ops_ms": ops_ms, "lockstep": lock}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


def cvb_ab(a, run, day, kw: dict, planted: set, dev) -> int:
    """The ``--cvb-iters`` comparison of the module text."""
    import torch

    from oni355 import ops
    vkw = dict(method="vem", em_iters=a.em_iters, var_iters=a.var_iters)
    ckw = dict(method="cvb0", cvb_iters=a.cvb_iters)
    variants = {"gibbs": lambda r: run(day.cols, sweeps=a.sweeps, seed=101 + r, **kw),
                "vem": lambda r: run(day.cols, **vkw, **kw), "cvb0": lambda r: run(day.cols, **ckw, **kw)}
    iters = {"gibbs": a.sweeps, "vem": a.em_iters, "cvb0": a.cvb_iters}
    for fn in variants.values():  # one untimed day each
        fn(0)
    days = {n: [] for n in variants}
    tops = {n: [] for n in variants}
    for r in range(a.rounds):
        for name, fn in variants.items():
            torch.cuda.synchronize(dev)
            ts = time.perf_counter()
            res = fn(r)
            torch.cuda.synchronize(dev)
            wall = time.perf_counter() - ts
            t = res.timings
            train_ms = t.get("train_dev_s", t.get("train_s", 0.0)) * 1e3
            rows = set(res.rows.tolist())
            line = {"variant": name, "round": r, "day_ms": round(wall * 1e3, 2), "train_ms": round(train_ms, 3),
                    "init_ms": round(t.get("init_dev_s", t.get("init_s", 0.0)) * 1e3, 3),
                    "ms_per_iter": round(train_ms / max(iters[name], 1), 4),
                    "planted_recall_topN": round(len(rows & planted) / max(len(planted), 1), 4),
                    "loglik": res.stats["loglik"]}
            days[name].append(line)
            tops[name].append(rows)
            print(json.dumps(line), flush=True)
            del res
    summary = {n: {"day_ms_median": statistics.median(x["day_ms"] for x in v),
                   "day_ms_spread": round(max(x["day_ms"] for x in v) - min(x["day_ms"] for x in v), 2),
                   "train_ms_median": statistics.median(x["train_ms"] for x in v),
                   "ms_per_iter_median": statistics.median(x["ms_per_iter"] for x in v),
                   "planted_recall_topN": [x["planted_recall_topN"] for x in v]} for n, v in days.items()}
    n_top, g, c = max(len(tops["cvb0"][0]), 1), tops["gibbs"], tops["cvb0"][0]
    overlap = {"cvb0_vs_cvb0": [round(len(c & x) / n_top, 4) for x in tops["cvb0"][1:]],
               "cvb0_vs_gibbs": [round(len(c & x) / n_top, 4) for x in g],
               "cvb0_vs_vem": round(len(c & tops["vem"][0]) / n_top, 4),
               "gibbs_vs_gibbs": [round(len(g[i] & g[j]) / n_top, 4) for i in range(len(g)) for j in range(i + 1, len(g))]}
    # one iteration's two ops, each alone with device events, and a device copy of the bytes the
    # iteration must move (r read and written by the update, read again by the word sum)
    traced = run(day.cols, eval_every=1, **ckw, **kw)
    m = traced.lda.model
    from oni355.models.cvb0_gpu import CvbLDA
    m = CvbLDA(m.c, m.K, m.alpha, m.beta).run(3)
    ptr, wm_src, wm_word, wm_cnt = m._wm
    P, KS = int(m._r.shape[0]), m.KS
    src, dst = torch.empty(P * KS * 3 // 2, dtype=torch.float32, device=dev), torch.empty(P * KS * 3 // 2, dtype=torch.float32, device=dev)
    ops_ms = {"cvb0_update": _timed(lambda: ops.cvb0_update(m._r, m.n_dk, m.n_wk, m.n_k, *m._pairs, m._ptr, m.K, m.alpha,
                                                            m.beta, m.V), a.op_reps),
              "word_sum": _timed(lambda: ops.vem_wsum(m._r, wm_cnt, m._ones, ptr, wm_src, wm_word, m.V, m.K), a.op_reps),
              "table": _timed(lambda: ops.vem_table(m.n_wk, m.K, m.beta), a.op_reps),
              "copy_same_bytes": _timed(lambda: dst.copy_(src), a.op_reps)}
    moved = 3 * P * KS * 4
    it_ms = ops_ms["cvb0_update"]["ms_median"] + ops_ms["word_sum"]["ms_median"]
    bw = {"bytes_per_iteration": moved, "copy_GBps": round(moved / ops_ms["copy_same_bytes"]["ms_median"] / 1e6, 1),
          "iteration_GBps": round(moved / it_ms / 1e6, 1),
          "fraction_of_copy": round(ops_ms["copy_same_bytes"]["ms_median"] / it_ms, 4)}
    trace = [[int(i), float(ll)] for i, ll in traced.lda.model.likelihoods]
    out = {"source": a.source, "flows": a.flows, "topics": a.topics, "gibbs_sweeps": a.sweeps, "em_iters": a.em_iters,
           "var_iters": a.var_iters, "cvb_iters": a.cvb_iters, "rounds": a.rounds, "pairs": P, "docs": int(m.c.D),
           "V": m.V, "KS": KS, "summary": summary, "top_overlap": overlap, "ops_ms": ops_ms, "bandwidth": bw,
           "loglik_trace": trace, "days": days}
    print(json.dumps({"summary": summary, "top_overlap": overlap, "ops_ms": ops_ms, "bandwidth": bw}), flush=True)
    print(json.dumps({"loglik_trace": trace}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cvb-iters", type=int, default=0, help="> 0: Gibbs, vem and cvb0 days alternating instead")
    ap.add_argument("--flows", type=int, default=12_500_000)
    ap.add_argument("--topics", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=200, help="Gibbs sweeps")
    ap.add_argument("--em-iters", type=int, default=30)
    ap.add_argument("--var-iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--maxresults", type=int, default=3000)
    ap.add_argument("--op-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--source", choices=["flow", "dns"], default="flow")
    ap.add_argument("--em-tol", type=float, default=0.0, help="> 0: the convergence-exit / α comparison instead")
    ap.add_argument("--em-max", type=int, default=100, help="--em-tol: the most EM iterations of the tol variant")
    ap.add_argument("--var-tol", default="", help="X[,Y…]: the per-document exit / warm start comparison instead")
    a = ap.parse_args()
    import numpy as np
    import torch

    dev = torch.device(a.device)
    t0 = time.perf_counter()
    kw = dict(K=a.topics, tol=1.0, maxresults=a.maxresults, device=dev)
    if a.source == "flow":
        from oni355.pipeline.flow import run_flow as run
        from oni355.synth.flow import generate_flows
        day = generate_flows(a.flows, seed=a.seed, n_hosts=max(64, a.flows // 25))
    else:
        from oni355.pipeline import dns
        from oni355.synth.dns import generate_dns
        day = generate_dns(a.flows, seed=a.seed, n_clients=max(32, a.flows // 40))

        def run(cols, **k):
            return dns.run_dns(cols, user_domain="intel", **k)
    planted = set(np.asarray(day.anomaly_rows).tolist())
    print(f"generated {a.flows} {a.source} events in {time.perf_counter() - t0:.1f} s", flush=True)
    if a.cvb_iters > 0:
        return cvb_ab(a, run, day, kw, planted, dev)
    if a.em_tol > 0:
        return bound_ab(a, run, day, kw, planted, dev)
    if a.var_tol:
        return exit_ab(a, run, day, kw, planted, dev)
    vkw = dict(method="vem", em_iters=a.em_iters, var_iters=a.var_iters)
    variants = {"gibbs": lambda r: run(day.cols, sweeps=a.sweeps, seed=101 + r, **kw),
                "vem": lambda r: run(day.cols, **vkw, **kw)}
    for fn in variants.values():  # one untimed day each: allocator, graphs, code objects
        fn(0)
    days = {n: [] for n in variants}
    tops = {n: [] for n in variants}
    last_vem = None
    for r in range(a.rounds):
        for name, fn in variants.items():
            torch.cuda.synchronize(dev)
            ts = time.perf_counter()
            res = fn(r)
            torch.cuda.synchronize(dev)
            wall = time.perf_counter() - ts
            t = res.timings
            train_ms = t.get("train_dev_s", t.get("train_s", 0.0)) * 1e3
            rows = set(res.rows.tolist())
            line = {"variant": name, "round": r, "day_ms": round(wall * 1e3, 2), "train_ms": round(train_ms, 3),
                    "init_ms": round(t.get("init_dev_s", t.get("init_s", 0.0)) * 1e3, 3),
                    "ms_per_iter": round(train_ms / max(a.em_iters if name == "vem" else a.sweeps, 1), 4),
                    "planted_recall_topN": round(len(rows & planted) / max(len(planted), 1), 4),
                    "loglik": res.stats["loglik"]}
            days[name].append(line)
            tops[name].append(rows)
            print(json.dumps(line), flush=True)
            if name == "vem":
                last_vem = res.lda.model
            del res

    def summ(v):
        d, s = [x["day_ms"] for x in v], [x["ms_per_iter"] for x in v]
        return {"day_ms_median": statistics.median(d), "day_ms_min": min(d), "day_ms_spread": round(max(d) - min(d), 2),
                "ms_per_iter_median": statistics.median(s), "ms_per_iter_min": min(s),
                "ms_per_iter_spread": round(max(s) - min(s), 4),
                "planted_recall_topN": [x["planted_recall_topN"] for x in v]}
    summary = {n: summ(v) for n, v in days.items()}
    n_top = max(len(tops["vem"][0]), 1)
    g = tops["gibbs"]
    overlap = {"vem_vs_vem": [round(len(tops["vem"][0] & x) / n_top, 4) for x in tops["vem"][1:]],
               "vem_vs_gibbs": [round(len(tops["vem"][0] & x) / n_top, 4) for x in g],
               "gibbs_vs_gibbs": [round(len(g[i] & g[j]) / n_top, 4) for i in range(len(g)) for j in range(i + 1, len(g))]}
    split = op_split(last_vem, a.op_reps)
    traced = run(day.cols, eval_every=1, **vkw, **kw)
    trace = [[int(i), float(ll)] for i, ll in traced.lda.model.likelihoods]
    out = {"source": a.source, "flows": a.flows, "topics": a.topics, "gibbs_sweeps": a.sweeps, "em_iters": a.em_iters,
           "var_iters": a.var_iters, "rounds": a.rounds,
           "stats": {k: v for k, v in traced.stats.items() if isinstance(v, (int, float, str))},
           "summary": summary, "top_overlap": overlap, "op_split_ms": split, "loglik_trace": trace, "days": days}
    print(json.dumps({"summary": summary, "top_overlap": overlap, "op_split_ms": split}), flush=True)
    print(json.dumps({"loglik_trace": trace}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
