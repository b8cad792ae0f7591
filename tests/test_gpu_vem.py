"""The M-step kernels of csrc/kernels/vem.hip through ops.vem_resp / vem_wsum / vem_table against
their specification (oni355/ref/vem_spec.py) in float64, and VarLDA end to end on the device.

Bounds: the segmented sum adds exact products of non-negative terms in f64 and rounds once after one
f64 multiply, so 2^-23 relative per element; the table is one f64 expression rounded once; e and q
repeat k_vfold's ψ series and dot, so they get that test's allowance, 4 × the f32 specification's
own error plus a 2^-24-scaled term.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.ref import vem_spec

pytestmark = pytest.mark.gpu

D = 40
# pairs per word, in word order. Cumulative: 1 | 64 (a word ending on a tile boundary) | 128 (one
# starting and ending on one) | 193 | 322 (across the span boundary 256) | 512 (ending on a span
# boundary) | 1512 (1000 pairs from a span boundary: four records, the wave combine) | 1536 (a tail
# ending on a span boundary) | 1792 (exactly one span) | 1795 (a head that ends inside its span) |
# 2095 (two records: the lane group's own combine) | 2100 | 2107: a last tile of 59 pairs, then a
# last word without pairs
SIZES = [0, 1, 63, 64, 65, 129, 190, 1000, 24, 256, 3, 300, 5, 0, 7, 0]
V = len(SIZES)
SHAPES = [(3, 4), (20, 20), (50, 52), (100, 100), (256, 256)]


@functools.lru_cache(maxsize=None)
def _pairs():
    """Doc-major (pair_doc, pair_word, pair_cnt) whose word-major list has SIZES, and that list."""
    r = np.random.default_rng(7)
    word = np.repeat(np.arange(V), SIZES)
    doc = np.concatenate([np.sort(r.integers(0, D, n)) for n in SIZES])
    o = np.argsort(doc, kind="stable")
    pd, pw = doc[o].astype(np.int32), word[o].astype(np.int32)
    pc = r.integers(1, 30, pd.size).astype(np.int32)
    pc[3::50] = 10 ** 6
    wm = vem_spec.word_major(pw, pd, V)
    assert np.array_equal(np.diff(wm[0]), SIZES) and pd.size % 64 == 59
    return pd, pw, pc, wm


@functools.lru_cache(maxsize=None)
def _inputs(K, KS):
    """f32 table [V + 1, KS], γ and e [D, KS], word-major q [P]: shared by the cases, never changed."""
    r = np.random.default_rng(K)
    P = sum(SIZES)
    table = np.zeros((V + 1, KS), np.float32)
    table[:, :K] = (r.random((V + 1, K)) ** 4 + 1e-7).astype(np.float32)
    table[:, :K] /= table[:, :K].sum(0, keepdims=True)
    gamma = np.zeros((D, KS), np.float32)
    gamma[:, :K] = np.exp(r.uniform(np.log(0.01), np.log(3000.0), (D, K))).astype(np.float32)
    e = np.zeros((D, KS), np.float32)
    e[:, :K] = r.random((D, K)).astype(np.float32) ** 3
    q = np.exp(r.uniform(np.log(1e-3), np.log(1e7), P)).astype(np.float32)
    return table, gamma, e, q


def _dev(gpu, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(gpu) for x in xs]


@pytest.mark.parametrize("K,KS", SHAPES)
def test_wsum_against_float64(gpu, K, KS):
    _, _, _, (ptr, wm_doc, wm_word, _) = _pairs()
    table, _, e, q = _inputs(K, KS)
    want = vem_spec.wsum(e, q, table, ptr, wm_doc, K)
    args = _dev(gpu, e, q, table, ptr, wm_doc, wm_word)
    got = ops.vem_wsum(*args, V, K)
    g = got.cpu().numpy().astype(np.float64)
    rel = np.abs(g - want) / np.where(want > 0, want, 1.0)
    print(f"K={K} KS={KS}: max relative error {rel.max():.3e} (bound {2.0 ** -23:.3e})")
    assert np.all(g[np.asarray(SIZES) == 0] == 0) and np.all(g[:, K:] == 0)
    assert np.all(np.abs(g - want) <= 2.0 ** -23 * want)
    assert torch.equal(ops.vem_wsum(*args, V, K, grid=1), got)  # whatever the grid
    assert torch.equal(ops.vem_wsum(*args, V, K), got)          # and from run to run


@pytest.mark.parametrize("K,KS", SHAPES)
def test_table_against_float64(gpu, K, KS):
    Vt, beta = 600, 0.01  # three column tiles, the last one short
    ss = np.zeros((Vt, KS), np.float32)
    ss[:, :K] = np.random.default_rng(KS).random((Vt, K)).astype(np.float32) ** 8 * 1e4
    ss[5::7] = 0
    want, ssk = vem_spec.table(ss, K, beta)
    got, gk = (x.cpu().numpy() for x in ops.vem_table(torch.from_numpy(ss).to(gpu), K, beta))
    assert got.shape == (Vt + 1, KS) and got.dtype == np.float32 and gk.dtype == np.float64
    assert np.all(got[:, K:] == 0) and np.all(gk[K:] == 0)
    assert np.all(np.abs(gk[:K] - ssk[:K]) <= Vt * 2.0 ** -53 * ssk[:K])  # f64 sums of Vt terms, another order
    assert np.all(np.abs(got[:, :K] - want[:, :K]) <= 2.0 ** -23 * want[:, :K])
    assert np.abs(got[:Vt, :K].astype(np.float64).sum(0) - want[:Vt, :K].sum(0)).max() <= Vt * 2.0 ** -23
    assert np.array_equal(got[Vt, :K], (beta / (gk[:K] + Vt * beta)).astype(np.float32))
    again = ops.vem_table(torch.from_numpy(ss).to(gpu), K, beta, grid=1)[0]
    assert np.array_equal(again.cpu().numpy(), got)


@pytest.mark.parametrize("K,KS", SHAPES)
def test_resp_against_float64(gpu, K, KS):
    pd, pw, pc, (_, _, _, wm_pos) = _pairs()
    table, gamma, _, _ = _inputs(K, KS)
    e64, q64 = vem_spec.resp(gamma, table, pd, pw, pc, K)
    e32, q32 = vem_spec.resp(gamma, table, pd, pw, pc, K, dtype=np.float32)
    tol_e = 4 * float(np.abs(e32 - e64).max()) + 2.0 ** -24
    tol_q = 4 * float((np.abs(q32 - q64) / q64).max()) + 2.0 ** -24
    args = _dev(gpu, gamma, table, pd, pw, pc)
    e, q = (x.cpu().numpy() for x in ops.vem_resp(*args, K))
    err_e = float(np.abs(e - e64).max())
    err_q = float((np.abs(q - q64) / q64).max())
    print(f"K={K} KS={KS}: e err {err_e:.3e} tol {tol_e:.3e} ratio {err_e / ((tol_e - 2.0 ** -24) / 4 + 1e-300):.2f}; "
          f"q rel err {err_q:.3e} tol {tol_q:.3e} ratio {err_q / ((tol_q - 2.0 ** -24) / 4 + 1e-300):.2f}")
    assert np.all(e[:, K:] == 0) and e[:, :K].max(1).min() == 1.0
    assert err_e <= tol_e and err_q <= tol_q
    qw = ops.vem_resp(*args, K, torch.from_numpy(wm_pos).to(gpu))[1].cpu().numpy()
    assert np.array_equal(qw[wm_pos], q)  # the same values, at their word-major positions


def test_varlda_end_to_end(gpu):
    from oni355.pipeline.flow import run_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(5000, seed=21)
    kw = dict(K=20, maxresults=100, device=gpu, method="vem", em_iters=3, var_iters=5)
    a, b = run_flow(dict(day.cols), seed=1, **kw), run_flow(dict(day.cols), seed=2, **kw)
    ma, mb = a.lda.model, b.lda.model
    assert torch.equal(ma.theta(), mb.theta()) and torch.equal(ma.table, mb.table)
    assert np.array_equal(a.rows, b.rows) and a.scores.tobytes() == b.scores.tobytes()
    c = a.lda.corpus
    pairs = [x.cpu().numpy() for x in (c.pair_doc, c.pair_word, c.pair_cnt, c.doc_pair_ptr)]
    ll = {}
    for dt in (np.float64, np.float32):
        tr = []
        vem_spec.vem(*pairs, c.V, 20, ma.KS, ma.alpha, ma.beta, 3, 5, dtype=dt, trace=tr)
        ll[dt] = tr[-1][1] / c.T
    got = a.stats["loglik"] / c.T
    own = abs(ll[np.float32] - ll[np.float64])
    tol = 4 * own + 1e-6 * abs(ll[np.float64])
    print(f"per-token loglik device {got:.9f} spec64 {ll[np.float64]:.9f} spec32 {ll[np.float32]:.9f}: "
          f"err {abs(got - ll[np.float64]):.3e} tol {tol:.3e} ratio to the f32 spec's error "
          f"{abs(got - ll[np.float64]) / (own + 1e-300):.2f}")
    assert abs(got - ll[np.float64]) <= tol
