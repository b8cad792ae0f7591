"""k_vfold (csrc/kernels/vfold.hip) through ops.vfold against its specification
(oni355/ref/vfold_spec.py) in float64, and score_flow(method="vb") on the device.

The tolerance is the specification's own f32 error: 4 · max|spec32 − spec64| + 2^-24 per case (the
factor covers a device expf / logf / division a few ulp from NumPy's and another fixed sum order).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.ref import vfold_spec

pytestmark = pytest.mark.gpu

V = 1100  # model words; id V = the out-of-vocabulary row
# pairs per document: none, 1, 1, exactly 64 and 65, small documents one of which straddles the pair
# index 192 with another right behind it, ~1000 (four waves, several strides), a wave of 16 whose pairs
# need several rounds, a second block of documents, a last one without pairs
SIZES = [0, 1, 1, 64, 65, 7, 7, 7, 7, 7, 7, 7, 7, 9, 5, 3, 1000, 3, 0, 12, 64, 2, 1, 70, 40, 30, 33, 31, 1, 63, 2, 5]
SIZES += np.random.default_rng(3).integers(1, 12, 70).tolist() + [66, 4, 0]


def _corpus():
    r = np.random.default_rng(11)
    words = [np.sort(r.choice(V, n, replace=False)) for n in SIZES]
    for d in (1, 4, 16, 20, 40):  # out-of-vocabulary pairs, also in the block path
        words[d][-1] = V
    pw = np.concatenate(words).astype(np.int32)
    pc = r.integers(1, 30, pw.size).astype(np.int32)
    pc[::7] = 1
    pc[3::50] = 10 ** 6
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    assert ptr[13] < 192 < ptr[14] and pw.size % 64 != 0
    return pw, pc, ptr


def _table(K, KS):
    t = np.zeros((V + 1, KS), np.float32)
    t[:, :K] = (np.random.default_rng(K).random((V + 1, K)) ** 4 + 1e-7).astype(np.float32)
    t[:, :K] /= t[:, :K].sum(0, keepdims=True)
    return t


def _bound(args, kw):
    t64 = vfold_spec.vfold(*args, **kw)[0]
    t32 = vfold_spec.vfold(*args, dtype=np.float32, **kw)[0]
    return t64, 4 * float(np.abs(t32 - t64).max()) + 2.0 ** -24


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("iters", [0, 1, 20])
@pytest.mark.parametrize("alpha", [0.01, 2.5])
@pytest.mark.parametrize("K,KS", [(3, 4), (20, 20), (50, 52), (100, 104), (33, 64)])
def test_device_against_the_spec(gpu, K, KS, alpha, iters, with_prior):
    pw, pc, ptr = _corpus()
    D, table, prior = len(SIZES), _table(K, KS), None
    if with_prior:
        prior = np.full((D, KS), alpha, np.float32)
        prior[::3, :K] += (5 * np.random.default_rng(5).dirichlet(np.ones(K) * 0.2, len(prior[::3]))).astype(np.float32)
    want, tol = _bound((pw, pc, ptr, table, K, alpha), dict(prior=prior, iters=iters))
    dev = [torch.from_numpy(x).to(gpu) for x in (pw, pc, ptr, table)]
    pr = None if prior is None else torch.from_numpy(prior).to(gpu)
    th, g = ops.vfold(*dev, K, alpha, pr, iters, want_gamma=True)
    got = th.cpu().numpy()
    err = float(np.abs(got - want).max())
    print(f"K={K} KS={KS} alpha={alpha} iters={iters} prior={with_prior}: err {err:.3e} tol {tol:.3e} "
          f"ratio to f32 spec error {err / ((tol - 2.0 ** -24) / 4 + 1e-300):.2f}")
    assert np.all(got[:, K:] == 0) and np.all(g.cpu().numpy()[:, K:] == 0)
    # a fixed-order f32 sum of K/4 terms per lane and two joins: at most (K/4 + 2) roundings, one more
    # for each quotient and for the f64 sum of the rounded quotients
    assert np.abs(got.astype(np.float64).sum(1) - 1).max() <= (K // 4 + 4) * 2.0 ** -24
    assert err <= tol
    assert torch.equal(ops.vfold(*dev, K, alpha, pr, iters), th)  # same inputs, same bits


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    from oni355.models.saved import SavedModel
    from oni355.pipeline.flow import run_flow
    from oni355.synth.flow import generate_flows
    tr = run_flow(dict(generate_flows(5000, seed=21).cols), K=20, sweeps=8, maxresults=100, device="cpu")
    m = SavedModel.from_run(tr.lda, tr.cuts, "flow").save(str(tmp_path_factory.mktemp("m") / "m.npz"))
    return SavedModel.load(m), generate_flows(5000, seed=22)  # a day with unseen words


def test_score_flow_vb_gpu_matches_cpu(gpu, saved):
    from oni355.pipeline.flow import score_flow
    m, day = saved
    rc = score_flow(dict(day.cols), m, maxresults=200, device="cpu", method="vb", prior_mass=5.0)
    rg = score_flow(dict(day.cols), m, maxresults=200, device=gpu, method="vb", prior_mass=5.0)
    assert rg.stats["infer_method"] == "vb" and rg.stats["infer_iters"] == 20 and rg.stats["foldin_launches"] == 1
    c, f = rc.lda.c, rc.lda
    _, tol = _bound((c.pair_word.numpy(), c.pair_cnt.numpy(), c.doc_pair_ptr.numpy(), f.table.numpy(), f.K, f.alpha),
                    dict(prior=f.prior.numpy(), iters=20))
    assert np.abs(rg.lda.theta().cpu().numpy() - f.theta().numpy()).max() <= tol
    # the lists agree except where scores tie within the tolerance
    assert np.abs(rc.scores - rg.scores).max() <= tol
    sc = dict(zip(rc.rows.tolist(), rc.scores.tolist()))
    sg = dict(zip(rg.rows.tolist(), rg.scores.tolist()))
    for row in set(sc) ^ set(sg):
        assert abs(sc.get(row, sg.get(row)) - rc.scores[-1]) <= tol
    for row in set(sc) & set(sg):
        assert abs(sc[row] - sg[row]) <= tol


def test_vb_scores_do_not_depend_on_the_seed(gpu, saved):
    from oni355.pipeline.flow import score_flow
    m, day = saved
    a = score_flow(dict(day.cols), m, maxresults=200, device=gpu, method="vb", seed=1)
    b = score_flow(dict(day.cols), m, maxresults=200, device=gpu, method="vb", seed=2)
    assert np.array_equal(a.rows, b.rows) and a.scores.tobytes() == b.scores.tobytes()
    assert torch.equal(a.lda.theta(), b.lda.theta())
