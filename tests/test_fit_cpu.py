"""The NumPy specification of ops.doc_fit against the fsum / long-double reference of
tests/fit_inputs.py, score_flow / score_dns with fit=True, and oni-ml --infer-fit."""
from __future__ import annotations

import csv
import json
import math
import os

import numpy as np
import pytest
import torch

import fit_inputs as fx
from oni355 import ops
from oni355.models.saved import SavedModel


@pytest.mark.parametrize("KS", [4, 20])
def test_spec_against_the_reference(KS):
    pd, pw, pc, D = fx.pair_list()
    th, tb = fx.model(KS, D)
    out = ops.doc_fit(*(torch.from_numpy(x) for x in (th, tb, pd, pw, pc)), D, fx.V)
    fx.check([t.numpy() for t in out], fx.reference(th, tb, pd, pw, pc, D), D)


def _check_batch(res, n_tokens):
    """Token counts, and the totals against the fsum of the document values (P ≤ tokens)."""
    f, st = res.fit, res.stats
    assert int(f.tokens.sum()) == n_tokens == st["batch_tokens"]
    assert st["batch_oov_tokens"] == st["n_oov_tokens"] == int(f.oov_tokens.sum())
    ll = f.loglik.tolist()
    tol = (4 + math.ceil(math.log2(n_tokens))) * 2.0**-52 * math.fsum(abs(x) for x in ll)
    assert abs(st["batch_loglik"] - math.fsum(ll)) <= tol and st["batch_loglik"] < 0
    assert st["batch_loglik_per_token"] == st["batch_loglik"] / n_tokens
    assert st["batch_perplexity"] == math.exp(-st["batch_loglik_per_token"])
    assert st["loglik"] is None and res.timings["fit_s"] > 0
    assert f.doc_keys.numel() == f.loglik.numel() and bool((f.min_score > 0).all())


def test_score_flow_fit():
    from oni355.pipeline.flow import run_flow, score_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(5000, seed=21)
    res = run_flow(dict(day.cols), K=20, sweeps=12, maxresults=100, device="cpu", seed=101)
    m = SavedModel.from_run(res.lda, res.cuts, "flow")
    a = score_flow(dict(day.cols), m, maxresults=100, device="cpu", seed=101)
    b = score_flow(dict(day.cols), m, maxresults=100, device="cpu", seed=101, fit=True)
    assert a.fit is None and "batch_loglik" not in a.stats and "fit_s" not in a.timings
    assert np.array_equal(a.rows, b.rows) and a.scores.tobytes() == b.scores.tobytes()  # bitwise as without
    assert a.src_scores.tobytes() == b.src_scores.tobytes() and a.dst_scores.tobytes() == b.dst_scores.tobytes()
    _check_batch(b, 2 * 5000)


def test_score_dns_fit():
    from oni355.pipeline import dns
    from oni355.synth.dns import generate_dns
    day = generate_dns(2000, seed=21, user_domain="intel")
    res = dns.run_dns(dict(day.cols), user_domain="intel", K=20, sweeps=6, maxresults=50, device="cpu", seed=101)
    m = dns.model_from_result(res, None, "intel")
    a = dns.score_dns(dict(day.cols), m, maxresults=50, device="cpu", sweeps=6, avg_last=3)
    b = dns.score_dns(dict(day.cols), m, maxresults=50, device="cpu", sweeps=6, avg_last=3, fit=True)
    assert a.fit is None and np.array_equal(a.rows, b.rows) and a.scores.tobytes() == b.scores.tobytes()
    _check_batch(b, 2000)


def test_cli_infer_fit(tmp_path):
    from oni355.cli import ml
    lp, md = str(tmp_path / "lp"), str(tmp_path / "models")
    base = ["20160708", "flow", "1.0", "40", "--synthetic", "3000", "--device", "cpu", "--lpath", lp, "--quiet"]
    with pytest.raises(SystemExit) as e:
        ml.main(base + ["--infer-fit"])
    assert e.value.code not in (0, None) and "--model" in str(e.value.code)
    assert ml.main(base + ["--sweeps", "6", "--save-model", md]) == 0
    assert ml.main(base + ["--model", os.path.join(md, "flow_model.npz"), "--infer-sweeps", "6", "--infer-avg-last",
                           "3", "--infer-fit"]) == 0
    with open(os.path.join(lp, "flow", "20160708", "metrics.jsonl")) as f:
        last = json.loads(f.readlines()[-1])
    assert last["batch_tokens"] == 6000 and last["batch_oov_tokens"] == 0 and last["loglik"] is None
    assert last["batch_loglik_per_token"] == last["batch_loglik"] / 6000 < 0
    assert last["batch_perplexity"] == math.exp(-last["batch_loglik_per_token"])
    with open(os.path.join(lp, "flow", "20160708", "flow_fit.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["ip", "tokens", "oov_tokens", "loglik", "loglik_per_token", "min_score"]
    body = rows[1:]
    assert len(body) == 40 and all(int(r[1]) > 0 and float(r[4]) == float(r[3]) / int(r[1]) for r in body)
    key = [(float(r[4]), [int(x) for x in r[0].split(".")]) for r in body]  # per token, ties by address
    assert key == sorted(key)
