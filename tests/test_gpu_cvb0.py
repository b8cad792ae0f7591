"""The kernels of csrc/kernels/cvb0.hip through ops.cvb0_init / cvb0_update / cvb0_theta against their
specification (oni355/ref/cvb0_spec.py) in float64, and CvbLDA end to end on the device.

Bounds. One step's r and n_dk repeat the f32 specification's arithmetic, so they get the project's
allowance: 4 × the f32 specification's own error against float64 plus 2^-24 (absolute on r, relative
to the document's length on its n_dk row). init and θ are one f64 expression rounded once: 2^-23.
Float32 trajectories drift (8e-6 in r after 100 steps), so single steps are compared, not runs.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.ref import cvb0_spec

pytestmark = pytest.mark.gpu

# pairs per document. Offsets: 0 | 0..1 (a single pair, count 1) | 1..64 (ends on a wave's last
# lane: a tail record) | 64..128 (exactly a wave: a head record) | 128..193 (a head and one more
# pair) | 193..1193 (sixteen records) | small documents inside waves, empty ones between them | a
# last document ending on a partial wave
SIZES = [0, 1, 63, 64, 65, 1000, 3, 0, 17, 40, 2, 31, 0, 9] + [5, 12, 0, 26, 1, 8, 33, 4] * 3 + [20, 7]
D, V = len(SIZES), 1200  # words 1100.. have no pairs
SHAPES = [(3, 4), (20, 20), (50, 52), (100, 100), (256, 256)]
PRIORS = [(0.01, 0.01), (2.5, 0.1)]


@functools.lru_cache(maxsize=None)
def _pairs():
    r = np.random.default_rng(11)
    pd = np.repeat(np.arange(D), SIZES).astype(np.int32)
    pw = np.concatenate([np.sort(r.choice(1100, n, replace=False)) for n in SIZES]).astype(np.int32)
    pc = r.integers(1, 30, pd.size).astype(np.int32)
    pc[5::50] = 10 ** 6
    pc[pd == 1] = 1
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    assert D == 40 and pd.size % 64 not in (0, 63)
    return pd, pw, pc, ptr


@functools.lru_cache(maxsize=None)
def _state(K, KS):
    """f32 rows r (random, normalised) and their counts: shared by the cases, never changed."""
    pd, pw, pc, _ = _pairs()
    r = np.zeros((pd.size, KS), np.float32)
    x = np.random.default_rng(K).random((pd.size, K)) ** 6 + 1e-9
    r[:, :K] = (x / x.sum(1, keepdims=True)).astype(np.float32)
    return (r,) + cvb0_spec.counts(r, pd, pw, pc, D, V, np.float32)


def _dev(gpu, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(gpu) for x in xs]


@pytest.mark.parametrize("alpha,beta", PRIORS)
@pytest.mark.parametrize("K,KS", SHAPES)
def test_update_against_float64(gpu, K, KS, alpha, beta):
    pd, pw, pc, ptr = _pairs()
    r0, n_dk, n_wk, n_k = _state(K, KS)
    N = np.add.reduceat(np.append(pc, 0).astype(np.float64), ptr[:-1]) * (np.diff(ptr) > 0)
    r64, n64 = cvb0_spec.update(r0, n_dk, n_wk, n_k, pd, pw, pc, K, alpha, beta, V)
    r32, n32 = cvb0_spec.update(r0, n_dk, n_wk, n_k, pd, pw, pc, K, alpha, beta, V, dtype=np.float32)
    scale = np.maximum(N, 1.0)[:, None]
    own_r, own_n = float(np.abs(r32 - r64).max()), float((np.abs(n32 - n64) / scale).max())
    tol_r, tol_n = 4 * own_r + 2.0 ** -24, 4 * own_n + 2.0 ** -24

    def step(grid=None):
        rows, *rest = _dev(gpu, r0.copy(), n_dk, n_wk, n_k, pd, pw, pc, ptr)
        return rows, ops.cvb0_update(rows, *rest, K, alpha, beta, V, grid=grid)

    rows, nd = step()
    r, n = rows.cpu().numpy().astype(np.float64), nd.cpu().numpy().astype(np.float64)
    err_r, err_n = float(np.abs(r - r64).max()), float((np.abs(n - n64) / scale).max())
    print(f"K={K} KS={KS} α={alpha} β={beta}: r err {err_r:.3e} tol {tol_r:.3e} ratio {err_r / (own_r + 1e-300):.2f}; "
          f"n_dk rel err {err_n:.3e} tol {tol_n:.3e} ratio {err_n / (own_n + 1e-300):.2f}")
    assert err_r <= tol_r and err_n <= tol_n
    assert np.all(np.abs(r[:, :K].sum(1) - 1) <= K * 2.0 ** -23) and np.all(r[:, K:] == 0)
    assert np.all(np.abs(n.sum(1) - N) <= tol_n * scale[:, 0]) and np.all(n[:, K:] == 0) and np.all(n[N == 0] == 0)
    for other in (step(grid=1), step()):  # whatever the grid, and from run to run
        assert torch.equal(other[0], rows) and torch.equal(other[1], nd)


@pytest.mark.parametrize("K,KS", SHAPES)
def test_init_and_theta_against_float64(gpu, K, KS):
    pd, pw, pc, ptr = _pairs()
    bad = pw.copy()
    bad[7] = V  # a word out of range: a zero row
    want = cvb0_spec.init(bad, V, K, KS)
    got = ops.cvb0_init(torch.from_numpy(bad).to(gpu), V, K, KS).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * want) and np.all(got[7] == 0) and np.all(got[:, K:] == 0)
    n_dk = _state(K, KS)[1]
    doc_len = np.add.reduceat(np.append(pc, 0).astype(np.int64), ptr[:-1]) * (np.diff(ptr) > 0)
    want = cvb0_spec.theta(n_dk, doc_len, K, 0.37)
    got = ops.cvb0_theta(*_dev(gpu, n_dk, doc_len), K, 0.37).cpu().numpy()
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * want) and np.all(got[:, K:] == 0)
    assert np.array_equal(got[0, :K], np.full(K, np.float32(1.0 / K)))  # the empty document


def test_cvblda_end_to_end(gpu):
    from oni355.pipeline.flow import run_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(5000, seed=21)
    kw = dict(K=20, maxresults=100, device=gpu, method="cvb0", cvb_iters=5, eval_every=5)
    a, b = run_flow(dict(day.cols), seed=1, **kw), run_flow(dict(day.cols), seed=2, **kw)
    ma, mb = a.lda.model, b.lda.model
    assert torch.equal(ma.theta(), mb.theta()) and torch.equal(ma.table, mb.table)
    assert np.array_equal(a.rows, b.rows) and a.scores.tobytes() == b.scores.tobytes()
    c = a.lda.corpus
    args = [x.cpu().numpy() for x in (c.pair_doc, c.pair_word, c.pair_cnt, c.doc_lengths())]
    ll = {}
    for dt in (np.float64, np.float32):
        tr = []
        cvb0_spec.cvb0(*args, c.V, 20, ma.KS, ma.alpha, ma.beta, 5, dtype=dt, trace=tr)
        ll[dt] = tr[-1][1] / c.T
    (it0, ll0), (it5, ll5) = ma.likelihoods[0], ma.likelihoods[-1]
    got = ll5 / c.T
    own = abs(ll[np.float32] - ll[np.float64])
    tol = 4 * own + 1e-6 * abs(ll[np.float64])
    print(f"per-token loglik start {ll0 / c.T:.9f} device {got:.9f} spec64 {ll[np.float64]:.9f} spec32 "
          f"{ll[np.float32]:.9f}: err {abs(got - ll[np.float64]):.3e} tol {tol:.3e}")
    assert (it0, it5) == (0, 5) and ll5 > ll0
    assert abs(got - ll[np.float64]) <= tol
