"""ops.vem_bound (csrc/kernels/vem_bound.hip) against an mpmath reference at 40 digits, and VarLDA with
α estimation end to end on the device.

Allowance per document, and for both totals with log2 P and log2 D:

    |device − ref| ≤ (4·r_spec + 4 + ⌈log2 max(P_d, 2)⌉ + ⌈log2 KS⌉) · 2^-52 · M_d

M_d is the sum of the magnitudes the result is built from (an absolute error in E = ψ(γ) − ψ(S)
passes straight into log s, so every pair also counts max_k|ψ(γ_k)| + |ψ(S_d)|), and r_spec is the
float64 specification's own largest error over the case's documents in the same unit: the project's
"4 × the specification's own error" rule, one precision up.
"""
from __future__ import annotations

import functools
import math

import mpmath as mp
import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.ref import vem_spec

pytestmark = pytest.mark.gpu

mp.mp.dps = 40
V = 40
# pairs per document, in document order. Cumulative: 0 | 1 | 64 (ends on a wave boundary) | 128
# (exactly one wave) | 193 (head plus one lane) | 323 | 1023 (700 pairs over waves 5 .. 15: eleven
# records, the whole-wave combine) | 20 empty documents | 3 .. 7 pairs each up to 1048 | empty up to
# document 279 | 5 and 6 pairs in the short third tile of 256 documents. P = 1059 = 16·64 + 35
SIZES = [0, 1, 63, 64, 65, 130, 700] + [0] * 20 + [3, 5, 7, 4, 6] + [0] * 247 + [5] + [0] * 18 + [6, 0]
D = len(SIZES)
SHAPES = [(3, 4), (20, 20), (50, 52), (100, 100), (256, 256)]


@functools.lru_cache(maxsize=None)
def _pairs():
    r = np.random.default_rng(11)
    pd = np.repeat(np.arange(D), SIZES).astype(np.int32)
    pw = r.integers(0, V, pd.size).astype(np.int32)
    pw[200] = V  # the table's last row
    pc = r.integers(1, 31, pd.size).astype(np.int32)
    pc[3::50] = 10 ** 6
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    assert D == 300 and pd.size % 64 == 35
    return pd, pw, pc, ptr


@functools.lru_cache(maxsize=None)
def _inputs(K, KS):
    """f32 table [V + 1, KS] and γ [D, KS] drawn from a pool of 300 values: shared, never changed."""
    r = np.random.default_rng(K)
    table = np.zeros((V + 1, KS), np.float32)
    table[:, :K] = (r.random((V + 1, K)) ** 4 + 1e-7).astype(np.float32)
    table[:, :K] /= table[:, :K].sum(0, keepdims=True)
    pool = np.exp(r.uniform(np.log(0.01), np.log(3000.0), 300)).astype(np.float32)
    gamma = np.zeros((D, KS), np.float32)
    gamma[:, :K] = pool[r.integers(0, pool.size, (D, K))]
    gamma[[4, 6, 150, 299], :K] = 1e6
    return table, gamma


@functools.lru_cache(maxsize=None)
def _ref(K, KS):
    """What does not depend on α, in mpmath: per document γ, E, lgamma(S), Σ lgamma(γ), Σ ψ(γ), ψ(S),
    max|ψ(γ)|, and per pair log s."""
    pd, pw, pc, ptr = _pairs()
    table, gamma = _inputs(K, KS)
    psi, lg = functools.lru_cache(None)(lambda v: mp.digamma(v)), functools.lru_cache(None)(lambda v: mp.loggamma(v))
    epsi = functools.lru_cache(None)(lambda v: mp.exp(psi(v)))
    tab = [[mp.mpf(float(v)) for v in row[:K]] for row in table]
    docs = []
    for d in range(D):
        g = [float(v) for v in gamma[d, :K]]
        S = mp.fsum(g)
        pS, eS = mp.digamma(S), mp.exp(mp.digamma(S))
        x = [epsi(v) / eS for v in g]
        logs = [mp.log(mp.fsum(t * y for t, y in zip(tab[pw[p]], x))) for p in range(ptr[d], ptr[d + 1])]
        docs.append(dict(g=g, E=[psi(v) - pS for v in g], lgS=mp.loggamma(S), lg=[lg(v) for v in g],
                         spsi=mp.fsum(psi(v) for v in g), pS=pS, mpsi=max(abs(psi(v)) for v in g), logs=logs,
                         apsi=mp.fsum(abs(psi(v)) for v in g)))
    return docs


def _bound_ref(K, KS, alpha):
    """(L_d, M_d for L, A_d, M_d for A) as float64 arrays, rounded once from mpmath."""
    _, _, pc, ptr = _pairs()
    a, c0 = mp.mpf(alpha), mp.loggamma(K * mp.mpf(alpha)) - K * mp.loggamma(mp.mpf(alpha))
    m0 = abs(mp.loggamma(K * a)) + K * abs(mp.loggamma(a))
    out = []
    for d, r in enumerate(_ref(K, KS)):
        c = [int(v) for v in pc[ptr[d]: ptr[d + 1]]]
        L = c0 - r["lgS"] + mp.fsum((a - g) * e + l for g, e, l in zip(r["g"], r["E"], r["lg"])) \
            + mp.fsum(n * s for n, s in zip(c, r["logs"]))
        ML = m0 + abs(r["lgS"]) + mp.fsum(abs(a - g) * abs(e) + abs(l) for g, e, l in zip(r["g"], r["E"], r["lg"])) \
            + mp.fsum(n * (abs(s) + r["mpsi"] + abs(r["pS"])) for n, s in zip(c, r["logs"]))
        out.append((L, ML, r["spsi"] - K * r["pS"], r["apsi"] + K * abs(r["pS"])))
    return out


@pytest.mark.parametrize("alpha", [0.01, 2.5])
@pytest.mark.parametrize("K,KS", SHAPES)
def test_bound_against_mpmath(gpu, K, KS, alpha):
    pd, pw, pc, ptr = _pairs()
    table, gamma = _inputs(K, KS)
    ref = _bound_ref(K, KS, alpha)
    L, ML, A, MA = (np.array([float(r[i]) for r in ref]) for i in range(4))
    u = 2.0 ** -52 * ML
    spec_doc, spec_tot = vem_spec.bound(gamma, table, pd, pw, pc, K, alpha)
    r_spec = float(max(abs(mp.mpf(float(s)) - r[0]) / (mp.mpf(2) ** -52 * r[1]) for s, r in zip(spec_doc, ref)))
    args = [torch.from_numpy(x).to(gpu) for x in (gamma, table, pd, pw, pc)]
    got = ops.vem_bound(*args, K, alpha, torch.from_numpy(ptr).to(gpu))
    doc, tot = got.doc.cpu().numpy(), got.tot.cpu().numpy()
    lks = math.ceil(math.log2(KS))
    allow = 4 * r_spec + 4 + np.ceil(np.log2(np.maximum(np.asarray(SIZES), 2))) + lks
    err = np.array([float(abs(mp.mpf(float(v)) - r[0])) for v, r in zip(doc, ref)])
    allow_t = 4 * r_spec + 4 + math.ceil(math.log2(pd.size)) + math.ceil(math.log2(D)) + lks
    tL, tA = mp.fsum(r[0] for r in ref), mp.fsum(r[2] for r in ref)
    uL, uA = 2.0 ** -52 * float(mp.fsum(r[1] for r in ref)), 2.0 ** -52 * float(mp.fsum(r[3] for r in ref))
    eL, eA = float(abs(mp.mpf(float(tot[0])) - tL)), float(abs(mp.mpf(float(tot[1])) - tA))
    print(f"K={K} KS={KS} alpha={alpha}: r_spec {r_spec:.2f}; device per document max {np.max(err / u):.2f} u "
          f"(smallest allowance {allow.min():.1f}); totals L {eL / uL:.2f} u, A {eA / uA:.2f} u (allowance {allow_t:.1f}); "
          f"spec totals L {float(abs(mp.mpf(float(spec_tot[0])) - tL)) / uL:.2f} u A "
          f"{float(abs(mp.mpf(float(spec_tot[1])) - tA)) / uA:.2f} u")
    assert np.all(err <= allow * u)
    assert eL <= allow_t * uL and eA <= allow_t * uA
    for again in (ops.vem_bound(*args, K, alpha, torch.from_numpy(ptr).to(gpu), grid=1), ops.vem_bound(*args, K, alpha)):
        assert torch.equal(again.doc, got.doc) and torch.equal(again.tot, got.tot)  # whatever the grid, run to run


def test_varlda_with_alpha_estimation_end_to_end(gpu, tmp_path):
    from oni355.models.saved import SavedModel
    from oni355.pipeline.flow import run_flow, score_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(5000, seed=21)
    kw = dict(K=20, maxresults=100, device=gpu, method="vem", em_iters=6, var_iters=5, estimate_alpha=True, em_tol=0)
    a, b = run_flow(dict(day.cols), seed=1, **kw), run_flow(dict(day.cols), seed=2, **kw)
    ma, mb = a.lda.model, b.lda.model
    assert torch.equal(ma.theta(), mb.theta()) and torch.equal(ma.table, mb.table) and ma.bounds == mb.bounds
    assert np.array_equal(a.rows, b.rows) and a.scores.tobytes() == b.scores.tobytes() and a.stats == b.stats
    assert a.stats["em_iters_done"] == 6 and a.stats["em_converged"] is False and a.stats["alpha_final"] == ma.alpha
    c = a.lda.corpus
    pairs = [x.cpu().numpy() for x in (c.pair_doc, c.pair_word, c.pair_cnt, c.doc_pair_ptr)]
    want = {}
    for dt in (np.float64, np.float32):
        tr = []
        vem_spec.vem(*pairs, c.V, 20, ma.KS, ma.bounds[0][3], ma.beta, 6, 5, dtype=dt, estimate_alpha=True, bounds=tr)
        want[dt] = (tr[-1][1] / c.T, tr[-1][3])
    for name, got, i in (("elbo_per_token", a.stats["elbo_per_token"], 0), ("alpha_final", a.stats["alpha_final"], 1)):
        w64, w32 = want[np.float64][i], want[np.float32][i]
        tol = 4 * abs(w32 - w64) + 1e-6 * abs(w64)
        print(f"{name}: device {got:.9f} spec64 {w64:.9f} spec32 {w32:.9f}: err {abs(got - w64):.3e} tol {tol:.3e}")
        assert abs(got - w64) <= tol
    m = SavedModel.load(SavedModel.from_run(a.lda, a.cuts, "flow").save(str(tmp_path / "m.npz")))
    assert m.alpha == ma.alpha and m.provenance["estimate_alpha"] is True and m.provenance["elbo"] == a.stats["elbo"]
    r = score_flow(dict(day.cols), m, maxresults=100, device=gpu, method="vb", iters=5)
    assert torch.equal(r.lda.theta(), ma.theta())
