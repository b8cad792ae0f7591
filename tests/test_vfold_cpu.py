"""The variational fold-in on the CPU (oni355/ref/vfold_spec.py through ops.vfold): its fixed point,
score_flow(method="vb") on the day of tests/test_foldin_cpu.py, and the oni-ml options."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from oni355.models.foldin import VarFoldIn
from oni355.models.saved import SavedModel
from oni355.ref import vfold_spec

N_TOP = 100
# the seed-to-seed noise floor of this day's top-100 (tests/test_foldin_cpu.py, docs/foldin.md)
FLOOR = [0.30, 0.24, 0.37, 0.21, 0.29]


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    from oni355.pipeline.flow import run_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(5000, seed=21)
    res = run_flow(dict(day.cols), K=20, sweeps=12, maxresults=N_TOP, device="cpu", seed=101)
    m = SavedModel.from_run(res.lda, res.cuts, "flow").save(str(tmp_path_factory.mktemp("m") / "m.npz"))
    return day, res, SavedModel.load(m)


def test_vb_top100_overlap_and_fixed_point(trained):
    from oni355.pipeline.flow import score_flow
    day, res, m = trained
    r = score_flow(dict(day.cols), m, maxresults=N_TOP, device="cpu", method="vb", seed=101)
    assert isinstance(r.lda, VarFoldIn) and r.lda.launches == {"vfold": 1}
    assert r.stats["infer_method"] == "vb" and r.stats["infer_iters"] == 20 and r.stats["foldin_launches"] == 1
    overlap = len(set(r.rows.tolist()) & set(res.rows.tolist())) / N_TOP
    print("vb fold-in overlap", overlap, "floor", FLOOR)
    assert overlap >= min(FLOOR)
    # the specification reaches a fixed point: one more iteration after 200 moves θ by < 1e-9
    c, f = r.lda.c, r.lda
    args = (c.pair_word.numpy(), c.pair_cnt.numpy(), c.doc_pair_ptr.numpy(), f.table.numpy(), f.K, f.alpha)
    t200, t201 = (vfold_spec.vfold(*args, iters=n)[0] for n in (200, 201))
    assert np.abs(t201 - t200).max() < 1e-9
    assert np.all(t200[:, f.K:] == 0) and np.allclose(t200.sum(1), 1, atol=1e-12)


def test_method_gibbs_is_the_call_without_the_argument(trained):
    from oni355.pipeline.flow import score_flow
    day, _, m = trained
    a = score_flow(dict(day.cols), m, maxresults=N_TOP, device="cpu", sweeps=4, avg_last=2)
    b = score_flow(dict(day.cols), m, maxresults=N_TOP, device="cpu", sweeps=4, avg_last=2, method="gibbs", iters=3)
    for k in ("rows", "scores", "src_scores", "dst_scores", "src_words", "dst_words"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes()
    assert a.stats == b.stats and "infer_method" not in a.stats
    assert a.lda.ndk_sum.numpy().tobytes() == b.lda.ndk_sum.numpy().tobytes()
    with pytest.raises(ValueError, match="gibbs"):
        score_flow(dict(day.cols), m, device="cpu", method="em")


def test_cli_infer_method(trained, tmp_path):
    from oni355.cli import ml
    _, _, m = trained
    mp, lp = m.save(str(tmp_path / "flow_model.npz")), str(tmp_path / "lp")
    base = ["20160708", "flow", "1.0", "50", "--synthetic", "3000", "--device", "cpu", "--lpath", lp, "--quiet"]
    assert ml.main(base + ["--model", mp, "--infer-method", "vb", "--infer-iters", "5"]) == 0
    assert os.path.exists(os.path.join(lp, "flow", "20160708", "flow_results.csv"))
    with open(os.path.join(lp, "flow", "20160708", "metrics.jsonl")) as f:
        last = json.loads(f.readlines()[-1])
    assert last["infer_method"] == "vb" and last["infer_iters"] == 5 and last["mode"] == "infer"
    for extra in (["--infer-method", "vb"], ["--infer-iters", "5"]):
        with pytest.raises(SystemExit) as e:
            ml.main(base + extra)
        assert e.value.code not in (0, None) and "needs --model" in str(e.value.code)
