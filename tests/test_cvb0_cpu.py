"""Batch CVB0 without a device: the specification's invariants, run_flow(method="cvb0") on the CPU
path (ops → oni355/ref/cvb0_spec.py), the saved model's provenance and the usage errors."""
from __future__ import annotations

import numpy as np
import pytest

from oni355.models.saved import SavedModel
from oni355.ref import cvb0_spec, vem_spec


def test_spec_invariants_and_monotone_likelihood():
    r = np.random.default_rng(5)
    D, V, K = 60, 30, 3
    topics = r.dirichlet(np.full(V, 0.05), K)
    cnt = np.stack([r.multinomial(80, r.dirichlet(np.full(K, 0.2)) @ topics) for _ in range(D)])
    pd, pw = (x.astype(np.int32) for x in np.nonzero(cnt))
    pc = cnt[pd, pw].astype(np.int32)
    rows = cvb0_spec.init(pw, V, K, 4)
    n_dk, n_wk, n_k = cvb0_spec.counts(rows, pd, pw, pc, D, V)
    rows, n_dk2 = cvb0_spec.update(rows, n_dk, n_wk, n_k, pd, pw, pc, K, 0.5, 0.1, V)
    assert np.allclose(rows[:, :K].sum(1), 1, atol=1e-12) and np.all(rows[:, K:] == 0)
    n_dk, n_wk, n_k = cvb0_spec.counts(rows, pd, pw, pc, D, V)
    assert np.array_equal(n_dk, n_dk2)
    T = float(pc.sum())
    assert abs(n_dk.sum() - T) <= 1e-9 * T and abs(n_wk.sum() - T) <= 1e-9 * T and abs(n_k.sum() - T) <= 1e-9 * T
    tr = []
    cvb0_spec.cvb0(pd, pw, pc, cnt.sum(1), V, K, 4, 0.5, 0.1, 20, trace=tr)
    ll = [x for _, x in tr]
    assert len(ll) == 21 and all(b >= a for a, b in zip(ll, ll[1:])) and ll[-1] > ll[0]


@pytest.fixture(scope="module")
def day():
    from oni355.synth.flow import generate_flows
    return generate_flows(5000, seed=21)


def test_run_flow_cvb0_ignores_the_seed_and_saves_its_provenance(day, tmp_path):
    from oni355.pipeline.flow import run_flow, score_flow
    from oni355.synth.flow import generate_flows
    kw = dict(K=20, maxresults=200, device="cpu", method="cvb0", cvb_iters=4)
    a, b = run_flow(dict(day.cols), seed=1, **kw), run_flow(dict(day.cols), seed=2, **kw)
    assert np.array_equal(a.rows, b.rows) and a.scores.tobytes() == b.scores.tobytes()
    assert a.stats["train_method"] == "cvb0" and a.stats["cvb_iters"] == 4
    m = SavedModel.load(SavedModel.from_run(a.lda, a.cuts, "flow").save(str(tmp_path / "m.npz")))
    assert m.provenance["train_method"] == "cvb0" and m.provenance["cvb_iters"] == 4
    assert "seed" not in m.provenance and "em_iters" not in m.provenance
    assert np.array_equal(m.phi_oov, a.lda.model.phi_oov().numpy())
    r = score_flow(dict(generate_flows(5000, seed=22).cols), m, maxresults=200, device="cpu", method="vb", iters=5)
    assert len(r.rows) == 200 and np.all(np.diff(r.scores) >= 0)


def test_a_vem_model_records_what_it_did_before(day):
    from oni355.pipeline.flow import run_flow
    v = run_flow(dict(day.cols), K=20, maxresults=50, device="cpu", method="vem", em_iters=1, var_iters=2)
    p = SavedModel.from_run(v.lda, v.cuts, "flow").provenance
    assert p["train_method"] == "vem" and p["em_iters"] == 1 and p["var_iters"] == 2 and "cvb_iters" not in p
    assert "cvb_iters" not in v.stats and v.stats["train_method"] == "vem"


@pytest.mark.parametrize("kw", [dict(em_tol=1e-4), dict(estimate_alpha=True), dict(var_tol=1e-3),
                                dict(warm_start=True), dict(cvb_iters=-1)])
def test_run_flow_refuses_what_cvb0_does_not_combine_with(day, kw):
    from oni355.pipeline.flow import run_flow
    with pytest.raises(ValueError):
        run_flow(dict(day.cols), K=20, maxresults=50, device="cpu", method="cvb0", **kw)


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--ckpt-dir", "x"], ["--ldac-out", "x"], ["--em-iters", "3"]])
def test_cli_refuses_what_cvb0_does_not_combine_with(tmp_path, extra):
    from oni355.cli import ml
    base = ["20160708", "flow", "1.0", "50", "--synthetic", "600", "--device", "cpu", "--lpath", str(tmp_path),
            "--quiet", "--train-method", "cvb0"]
    with pytest.raises(SystemExit) as e:
        ml.main(base + extra)
    assert e.value.code not in (0, None) and extra[0] in str(e.value.code)
