"""The variational bound, the EM convergence exit and α estimation of method="vem" on the CPU path:
ops.vem_bound runs its specification, alpha_newton returns a root, em_tol stops where lda-c's loop
stops, and with both options off nothing changes."""
from __future__ import annotations

import mpmath as mp
import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.ref import vem_spec


def test_ops_vem_bound_on_cpu_runs_the_specification():
    r = np.random.default_rng(3)
    D, V, K, KS, P = 9, 7, 3, 4, 40
    gamma = np.zeros((D, KS), np.float32)
    gamma[:, :K] = r.uniform(0.05, 30.0, (D, K))
    table = np.zeros((V + 1, KS), np.float32)
    table[:, :K] = r.random((V + 1, K)) + 1e-3
    pd = np.sort(r.integers(0, D, P)).astype(np.int32)
    pw, pc = r.integers(0, V + 1, P).astype(np.int32), r.integers(1, 9, P).astype(np.int32)
    got = ops.vem_bound(*(torch.from_numpy(x) for x in (gamma, table, pd, pw, pc)), K, 0.7)
    doc, tot = vem_spec.bound(gamma, table, pd, pw, pc, K, 0.7)
    assert got.doc.dtype == torch.float64 and np.array_equal(got.doc.numpy(), doc) and np.array_equal(got.tot.numpy(), tot)
    assert np.isfinite(doc).all() and tot[0] == doc.sum() and tot[1] < 0


@pytest.mark.parametrize("K", [3, 20, 100])
@pytest.mark.parametrize("a0", [0.05, 2.5])
def test_alpha_newton_returns_a_root(K, a0):
    r = np.random.default_rng(K)
    D = 200
    g = torch.from_numpy(a0 + 50.0 * r.dirichlet(np.full(K, a0), D))
    ss = float((torch.digamma(g).sum(1) - K * torch.digamma(g.sum(1))).sum())
    a = vem_spec.alpha_newton(ss, D, K)
    mp.mp.dps = 40
    df = D * (K * mp.digamma(K * mp.mpf(a)) - K * mp.digamma(mp.mpf(a))) + mp.mpf(ss)
    print(f"K={K} a0={a0}: alpha {a:.6g} df {float(df):.3e}")
    assert 0 < a < 100 and abs(df) <= 1e-5


@pytest.fixture(scope="module")
def day():
    from oni355.synth.flow import generate_flows
    return generate_flows(5000, seed=21)


def test_em_tol_stops_at_the_first_converged_iteration(day):
    from oni355.pipeline.flow import run_flow
    r = run_flow(dict(day.cols), K=20, maxresults=100, device="cpu", method="vem", em_iters=50, var_iters=5, em_tol=1e-4)
    m, st = r.lda.model, r.stats
    conv = [c for _, _, c, _ in m.bounds]
    first = next(i for i, c in enumerate(conv) if i >= 2 and 0 <= c <= 1e-4)
    print(f"stopped after {st['em_iters_done']} iterations, conv {conv[-1]:.3e}, bound/token {st['elbo_per_token']:.6f}")
    assert st["em_iters_done"] == len(conv) == first + 1 < 50 and st["em_converged"] is True
    assert [i for i, *_ in m.bounds] == list(range(len(conv))) and conv[0] == 1.0
    assert st["alpha_final"] == m.alpha == m.bounds[0][3] and st["elbo"] == m.bound()  # α stays without estimate_alpha
    assert m.bounds[-1][1] > m.bounds[0][1] and np.isfinite(st["elbo"])


def test_options_off_change_nothing(day):
    from oni355.pipeline.flow import run_flow
    kw = dict(K=20, maxresults=100, device="cpu", method="vem", em_iters=2, var_iters=3)
    a, b = run_flow(dict(day.cols), **kw), run_flow(dict(day.cols), em_tol=0.0, estimate_alpha=False, **kw)
    assert a.rows.tobytes() == b.rows.tobytes() and a.scores.tobytes() == b.scores.tobytes() and a.stats == b.stats
    assert torch.equal(a.lda.model.theta(), b.lda.model.theta()) and torch.equal(a.lda.model.table, b.lda.model.table)
    assert a.lda.model.bounds == [] and "elbo" not in a.stats and a.lda.model.sweeps_done == 2


def test_cli_refuses_em_tol_without_vem(tmp_path):
    from oni355.cli import ml
    with pytest.raises(SystemExit) as e:
        ml.main(["20160708", "flow", "1.0", "50", "--synthetic", "600", "--device", "cpu", "--lpath", str(tmp_path),
                 "--quiet", "--em-tol", "1e-4"])
    assert e.value.code not in (0, None) and "--em-tol" in str(e.value.code) and "--train-method vem" in str(e.value.code)
