"""k_vfold_exit (csrc/kernels/vfold_exit.hip) through ops.vfold_exit: bit for bit k_vfold with the exit
off, its per-document exit and warm start against the float64 specification
(oni355/ref/vfold_exit_spec.py), independence of a document from its neighbours, and vem training
with both options on the device. Corpus and table are those of test_gpu_vfold.py.

A document is *undecided* where some entry of its f64 change/total trace lies within 1 % of the
tolerance: there f32 arithmetic may stop one update apart. Every other document must stop exactly
where the specification does, and at most 12 of the 105 may be undecided. θ is then compared with
the specification replaying the device's own counts, within 4 · max|spec32 − spec64| + 2^-24.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.ref import vfold_exit_spec as spec

pytestmark = pytest.mark.gpu

V = 1100
SIZES = [0, 1, 1, 64, 65, 7, 7, 7, 7, 7, 7, 7, 7, 9, 5, 3, 1000, 3, 0, 12, 64, 2, 1, 70, 40, 30, 33, 31, 1, 63, 2, 5]
SIZES += np.random.default_rng(3).integers(1, 12, 70).tolist() + [66, 4, 0]
D = len(SIZES)
SHAPES = pytest.mark.parametrize("K,KS", [(3, 4), (20, 20), (50, 52), (100, 104), (33, 64)])
ALPHAS = pytest.mark.parametrize("alpha", [0.01, 2.5])


@functools.lru_cache(None)
def _corpus():
    r = np.random.default_rng(11)
    words = [np.sort(r.choice(V, n, replace=False)) for n in SIZES]
    for d in (1, 4, 16, 20, 40):  # out-of-vocabulary pairs, also in the block path
        words[d][-1] = V
    pw = np.concatenate(words).astype(np.int32)
    pc = r.integers(1, 30, pw.size).astype(np.int32)
    pc[::7] = 1
    pc[3::50] = 10 ** 6
    return pw, pc, np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)


@functools.lru_cache(None)
def _table(K, KS):
    t = np.zeros((V + 1, KS), np.float32)
    t[:, :K] = (np.random.default_rng(K).random((V + 1, K)) ** 4 + 1e-7).astype(np.float32)
    t[:, :K] /= t[:, :K].sum(0, keepdims=True)
    return t


def _dev(gpu, *xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(gpu) for x in xs]


def _check_exit(gpu, K, KS, alpha, tol, gamma0):
    """The two checks of the exit: stopping counts against the f64 rule, θ against the f64 replay."""
    pw, pc, ptr = _corpus()
    args = (pw, pc, ptr, _table(K, KS), K, alpha)
    trace = spec.vfold_exit(*args, max_iters=40, tol=tol, gamma0=gamma0)[3]
    n64 = np.isfinite(trace).sum(1)
    undecided = (np.abs(np.nan_to_num(trace, nan=np.inf) - tol) <= 0.01 * tol).any(1)
    g0, = _dev(gpu, gamma0)
    th, g, n_it = ops.vfold_exit(*_dev(gpu, *args[:4]), K, alpha, None, 40, tol, g0)
    th, g, n = th.cpu().numpy(), g.cpu().numpy(), n_it.cpu().numpy()
    t64 = spec.vfold_exit(*args, max_iters=40, gamma0=gamma0, force_iters=n)[0]
    t32 = spec.vfold_exit(*args, max_iters=40, gamma0=gamma0, force_iters=n, dtype=np.float32)[0]
    bound = 4 * float(np.abs(t32 - t64).max()) + 2.0 ** -24
    err = float(np.abs(th - t64).max())
    print(f"K={K} KS={KS} alpha={alpha} tol={tol} warm={gamma0 is not None}: undecided {int(undecided.sum())}, "
          f"count mismatches {int((n != n64).sum())}, mean n_it {n.mean():.2f}, err {err:.3e} bound {bound:.3e}")
    assert undecided.sum() <= 12
    assert np.array_equal(n[~undecided], n64[~undecided])
    assert n.min() >= 1 and n.max() <= 40
    assert np.all(th[:, K:] == 0) and np.all(g[:, K:] == 0)
    assert err <= bound
    return th, g, n


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("max_iters", [0, 1, 20])
@ALPHAS
@SHAPES
def test_fixed_count_is_k_vfold(gpu, K, KS, alpha, max_iters, with_prior):
    prior = None
    if with_prior:
        prior = np.full((D, KS), alpha, np.float32)
        prior[::3, :K] += (5 * np.random.default_rng(5).dirichlet(np.ones(K) * 0.2, len(prior[::3]))).astype(np.float32)
    dev = _dev(gpu, *_corpus(), _table(K, KS))
    pr, = _dev(gpu, prior)
    th, g, n_it = ops.vfold_exit(*dev, K, alpha, pr, max_iters, 0.0)
    th0, g0 = ops.vfold(*dev, K, alpha, pr, max_iters, want_gamma=True)
    assert torch.equal(th, th0) and torch.equal(g, g0)
    assert n_it.dtype == torch.int32 and int(n_it.min()) >= min(1, max_iters) and int(n_it.max()) <= max_iters


@pytest.mark.parametrize("tol", [1e-3, 1e-5])
@ALPHAS
@SHAPES
def test_exit_against_float64(gpu, K, KS, alpha, tol):
    _check_exit(gpu, K, KS, alpha, tol, None)


@ALPHAS
@SHAPES
def test_warm_start(gpu, K, KS, alpha):
    dev = _dev(gpu, *_corpus(), _table(K, KS))
    g0 = ops.vfold(*dev, K, alpha, None, 3, want_gamma=True)[1]
    th, g, n = _check_exit(gpu, K, KS, alpha, 1e-3, g0.cpu().numpy())
    th0, gz, nz = ops.vfold_exit(*dev, K, alpha, None, 0, 1e-3, g0)
    assert torch.equal(gz, g0) and int(nz.max()) == 0  # no update: γ is gamma0 and θ = γ / Σγ
    ref = g0[:, :K].double() / g0[:, :K].double().sum(1, keepdim=True)
    # the device's f32 sum of K terms (K/4 per lane and two joins) and one quotient, as in test_gpu_vfold.py
    assert float((th0[:, :K].double() - ref).abs().max()) <= (K // 4 + 4) * 2.0 ** -24 and bool((th0[:, K:] == 0).all())
    if KS > K:  # garbage in the padding columns of gamma0 changes nothing
        bad = g0.clone()
        bad[:, K:] = torch.tensor([float("nan"), -7.0, float("inf"), 1e30], device=gpu).repeat(KS)[: KS - K]
        th2, g2, n2 = ops.vfold_exit(*dev, K, alpha, None, 40, 1e-3, bad)
        assert np.array_equal(th2.cpu().numpy(), th) and np.array_equal(g2.cpu().numpy(), g)
        assert np.array_equal(n2.cpu().numpy(), n)


@ALPHAS
@SHAPES
def test_a_document_does_not_depend_on_its_neighbours(gpu, K, KS, alpha):
    pw, pc, ptr = _corpus()
    order = np.arange(D)[::-1]
    rw = np.concatenate([pw[ptr[d]:ptr[d + 1]] for d in order])
    rc = np.concatenate([pc[ptr[d]:ptr[d + 1]] for d in order])
    rptr = np.concatenate([[0], np.cumsum(np.diff(ptr)[order])]).astype(np.int64)
    tab, = _dev(gpu, _table(K, KS))
    fwd = ops.vfold_exit(*_dev(gpu, pw, pc, ptr), tab, K, alpha, None, 40, 1e-3)
    rev = ops.vfold_exit(*_dev(gpu, rw, rc, rptr), tab, K, alpha, None, 40, 1e-3)
    again = ops.vfold_exit(*_dev(gpu, pw, pc, ptr), tab, K, alpha, None, 40, 1e-3)
    flip = torch.from_numpy(order.copy()).to(gpu)
    for a, b, c in zip(fwd, rev, again):
        assert torch.equal(a, b[flip]) and torch.equal(a, c)


def test_training_with_exit_and_warm_start(gpu, tmp_path):
    from oni355.models.saved import SavedModel
    from oni355.pipeline.flow import run_flow, score_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(3000, seed=21)
    kw = dict(K=20, maxresults=100, device=gpu, method="vem", em_iters=4, var_iters=20, var_tol=1e-3, warm_start=True)
    a, b = run_flow(dict(day.cols), **kw), run_flow(dict(day.cols), **kw)
    ma, mb = a.lda.model, b.lda.model
    assert torch.equal(ma.theta(), mb.theta()) and torch.equal(ma.table, mb.table)
    assert a.rows.tobytes() == b.rows.tobytes() and a.scores.tobytes() == b.scores.tobytes()
    tr = ma.var_iters_trace
    print("var_iters_trace", tr)
    assert len(tr) == 4 and all(1 <= x <= 20 for x in tr)
    m = SavedModel.load(SavedModel.from_run(a.lda, a.cuts, "flow").save(str(tmp_path / "m.npz")))
    assert m.provenance["var_tol"] == 1e-3 and bool(m.provenance["warm_start"])
    s = score_flow(dict(day.cols), m, maxresults=100, device=gpu, method="vb", iters=20, infer_tol=1e-3)
    assert torch.equal(s.lda.theta(), ma.theta())
    assert s.stats["infer_tol"] == 1e-3 and 1 <= s.stats["infer_iters_mean"] <= 20
