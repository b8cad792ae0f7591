"""Variational-EM training (method="vem") on the CPU path: the specification improves the
likelihood, the pipelines ignore the seed, a saved model reproduces the training day under the
variational fold-in, and the CLI refuses what vem does not combine with."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oni355.models.saved import SavedModel
from oni355.ref import vem_spec

EM, VAR = 4, 6


def test_em_improves_the_likelihood_of_a_planted_corpus():
    r = np.random.default_rng(5)
    D, V, K = 60, 30, 3
    pd, pw, pc = [], [], []
    for d in range(D):  # topic t owns words 10t .. 10t + 9
        cnt = np.bincount(10 * (d % K) + r.integers(0, 10, 40), minlength=V)
        w = np.nonzero(cnt)[0]
        pd += [d] * w.size
        pw += w.tolist()
        pc += cnt[w].tolist()
    pd, pw, pc = (np.asarray(x, np.int32) for x in (pd, pw, pc))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(pd, minlength=D))]).astype(np.int64)

    def final(k, iters):
        tr = []
        vem_spec.vem(pd, pw, pc, ptr, V, k, 4, 50.0 / k, 0.01, iters, 20, trace=tr)
        return tr

    tr = final(K, 30)
    assert [i for i, _ in tr] == list(range(31))
    assert tr[-1][1] > tr[0][1] and tr[-1][1] > final(1, 30)[-1][1]


@pytest.fixture(scope="module")
def day():
    from oni355.synth.flow import generate_flows
    return generate_flows(5000, seed=21)


@pytest.fixture(scope="module")
def trained(day):
    from oni355.pipeline.flow import run_flow
    return run_flow(dict(day.cols), K=20, maxresults=200, device="cpu", method="vem", em_iters=EM, var_iters=VAR, seed=1)


def test_vem_ignores_the_seed_and_gibbs_stays_the_default(day, trained):
    from oni355.pipeline.flow import run_flow
    b = run_flow(dict(day.cols), K=20, maxresults=200, device="cpu", method="vem", em_iters=EM, var_iters=VAR, seed=2)
    assert np.array_equal(trained.rows, b.rows) and trained.scores.tobytes() == b.scores.tobytes()
    assert (trained.stats["train_method"], trained.stats["em_iters"], trained.stats["var_iters"]) == ("vem", EM, VAR)
    assert trained.lda.model.sweeps_done == EM and np.isfinite(trained.stats["loglik"])
    g0 = run_flow(dict(day.cols), K=20, sweeps=6, maxresults=200, device="cpu")
    g1 = run_flow(dict(day.cols), K=20, sweeps=6, maxresults=200, device="cpu", method="gibbs")
    assert np.array_equal(g0.rows, g1.rows) and g0.scores.tobytes() == g1.scores.tobytes()
    assert g0.stats == g1.stats and "train_method" not in g0.stats


def test_saved_vem_model_reproduces_the_day_under_vb(day, trained, tmp_path):
    from oni355.pipeline.flow import score_flow
    m = SavedModel.load(SavedModel.from_run(trained.lda, trained.cuts, "flow").save(str(tmp_path / "m.npz")))
    assert m.provenance["train_method"] == "vem" and m.provenance["em_iters"] == EM and m.provenance["var_iters"] == VAR
    assert np.array_equal(m.phi_oov, trained.lda.model.phi_oov().numpy())
    r = score_flow(dict(day.cols), m, maxresults=200, device="cpu", method="vb", iters=VAR)
    assert torch.equal(r.lda.theta(), trained.lda.model.theta())
    assert np.array_equal(r.rows, trained.rows) and r.scores.tobytes() == trained.scores.tobytes()


@pytest.mark.parametrize("extra,msg", [(["--gpus", "2"], "single-GPU"), (["--ckpt-dir", "ck"], "--ckpt-dir"),
                                       (["--model", "m.npz"], "--model")])
def test_cli_refuses_what_vem_does_not_combine_with(tmp_path, extra, msg):
    from oni355.cli import ml
    base = ["20160708", "flow", "1.0", "50", "--synthetic", "600", "--device", "cpu", "--lpath", str(tmp_path),
            "--quiet", "--train-method", "vem"]
    with pytest.raises(SystemExit) as e:
        ml.main(base + extra)
    assert e.value.code not in (0, None) and "vem" in str(e.value.code) and msg in str(e.value.code)
