"""The warm-started, per-document-exit fold-in on the CPU: its specification
(oni355/ref/vfold_exit_spec.py) against vfold_spec, the off-by-default promise of run_flow, and the
usage errors of the new options."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oni355.ref import vfold_exit_spec, vfold_spec


def _case(K, KS, seed=0):
    r = np.random.default_rng(seed)
    sizes = [0, 1, 5, 70, 3, 0, 12]
    pw = np.concatenate([np.sort(r.choice(300, n, replace=False)) for n in sizes]).astype(np.int32)
    pc = r.integers(1, 30, pw.size).astype(np.int32)
    pc[2] = 10 ** 6
    t = np.zeros((300, KS), np.float32)
    t[:, :K] = r.random((300, K)) ** 4 + 1e-7
    t[:, :K] /= t[:, :K].sum(0, keepdims=True)
    return pw, pc, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), t, K, 0.3


@pytest.mark.parametrize("K,KS,iters", [(3, 4, 0), (20, 20, 1), (7, 8, 25)])
def test_tol_zero_is_vfold_spec(K, KS, iters):
    c = _case(K, KS)
    th, g, n_it, _ = vfold_exit_spec.vfold_exit(*c, max_iters=iters, tol=0.0)
    th0, g0 = vfold_spec.vfold(*c, iters=iters)
    assert np.array_equal(th, th0) and np.array_equal(g, g0)
    assert n_it.dtype == np.int32 and n_it.min() >= min(1, iters) and n_it.max() <= iters


@pytest.mark.parametrize("warm", [False, True])
def test_force_iters_replays_the_rule(warm):
    c = _case(20, 20)
    g0 = vfold_spec.vfold(*c, iters=2)[1] if warm else None
    th, g, n_it, tr = vfold_exit_spec.vfold_exit(*c, max_iters=40, tol=1e-2, gamma0=g0)
    assert 1 <= n_it.min() and n_it.max() <= 40 and len(set(n_it.tolist())) > 2  # documents stop apart
    assert n_it[0] == 1 and np.array_equal(g[0, :20], np.full(20, 0.3))  # no pairs: γ = a at once
    assert np.array_equal(np.isfinite(tr).sum(1), n_it)
    for d, n in enumerate(n_it):  # a document stops at its first update within the tolerance
        assert (tr[d, n - 1] <= 1e-2 or n == 40) and np.all(tr[d, :n - 1] > 1e-2)
    th2, g2, n2, _ = vfold_exit_spec.vfold_exit(*c, max_iters=40, gamma0=g0, force_iters=n_it)
    assert np.array_equal(th, th2) and np.array_equal(g, g2) and np.array_equal(n_it, n2)


@pytest.fixture(scope="module")
def day():
    from oni355.synth.flow import generate_flows
    return generate_flows(1500, seed=4)


def test_defaults_leave_vem_as_it_was(day):
    from oni355.pipeline.flow import run_flow
    kw = dict(K=20, maxresults=100, device="cpu", method="vem", em_iters=2, var_iters=3)
    a, b = run_flow(dict(day.cols), **kw), run_flow(dict(day.cols), var_tol=0.0, warm_start=False, **kw)
    assert a.rows.tobytes() == b.rows.tobytes() and a.scores.tobytes() == b.scores.tobytes() and a.stats == b.stats
    assert torch.equal(a.lda.model.theta(), b.lda.model.theta()) and torch.equal(a.lda.model.table, b.lda.model.table)
    assert "var_tol" not in a.stats and a.lda.model.var_iters_trace == []
    c = run_flow(dict(day.cols), var_tol=1e-2, warm_start=True, **dict(kw, var_iters=20))
    tr = c.lda.model.var_iters_trace
    assert len(tr) == 2 and all(1 <= x <= 20 for x in tr) and tr[1] < 20
    assert c.stats["var_tol"] == 1e-2 and c.stats["warm_start"] is True
    assert (c.stats["var_iters_mean_first"], c.stats["var_iters_mean_last"]) == (tr[0], tr[1])


def test_usage_errors(day, tmp_path):
    from oni355.cli import ml
    from oni355.models.saved import SavedModel
    from oni355.pipeline.flow import run_flow, score_flow
    for kw in (dict(var_tol=1e-3), dict(warm_start=True)):
        with pytest.raises(ValueError, match="method='vem'"):
            run_flow(dict(day.cols), K=20, sweeps=2, device="cpu", **kw)
    with pytest.raises(ValueError, match="var_tol"):
        run_flow(dict(day.cols), K=20, device="cpu", method="vem", var_tol=-1.0)
    tr = run_flow(dict(day.cols), K=20, sweeps=2, maxresults=50, device="cpu")
    m = SavedModel.load(SavedModel.from_run(tr.lda, tr.cuts, "flow").save(str(tmp_path / "m.npz")))
    with pytest.raises(ValueError, match="infer_tol"):
        score_flow(dict(day.cols), m, device="cpu", infer_tol=1e-3)
    base = ["20160708", "flow", "1.0", "50", "--synthetic", "600", "--device", "cpu", "--lpath", str(tmp_path), "--quiet"]
    for extra, flag, needs in ((["--var-tol", "1e-3"], "--var-tol", "--train-method vem"),
                               (["--warm-start"], "--warm-start", "--train-method vem"),
                               (["--model", str(tmp_path / "m.npz"), "--infer-tol", "1e-3"], "--infer-tol", "--infer-method vb")):
        with pytest.raises(SystemExit) as e:
            ml.main(base + extra)
        assert e.value.code not in (0, None) and flag in str(e.value.code) and needs in str(e.value.code)
