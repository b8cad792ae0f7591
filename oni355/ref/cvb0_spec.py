"""Specification of batch CVB0 training on the device (csrc/kernels/cvb0.hip, ops.cvb0_init /
cvb0_update / cvb0_theta, models.cvb0_gpu.CvbLDA): collapsed variational Bayes, zeroth order
(Asuncion et al. 2009), the deterministic mean-field counterpart of the collapsed Gibbs sampler,
over the corpus' doc-major distinct (doc, word, count) pairs ``(d_p, w_p, c_p)``. No seed anywhere::

    init    t0[w,k] = 1/V + u(w,k)                 u = vem_spec.init_u
            r_pk = t0[w_p,k] / Σ_j t0[w_p,j]       k < K, 0 past K
    counts  n_dk = Σ_{p in d} c_p·r_pk     n_wk = Σ_{p : w_p = w} c_p·r_pk     n_k = Σ_w n_wk
    step    u_k = (max(n_dk − r_pk, 0) + α) · (max(n_wk − r_pk, 0) + β) / (max(n_k − r_pk, 0) + Vβ)
            r_pk ← u_k / Σ_j u_j                   every pair from the OLD counts, then recount
    end     θ_dk = (n_dk + α) / (N_d + Kα), 0 past K; a document without pairs gets 1/K
            table = vem_spec.table(n_wk, K, β)

All tokens of a pair share one responsibility row, so the pair's own "one token" is r_pk. The counts
are summed in float64 and rounded once to ``dtype``; pairs naming a document outside [0, D) or a
word outside [0, V) contribute nothing and keep their row. The likelihood reported is the plug-in
one of :func:`oni355.ref.fit_spec.doc_fit`.

Everything is vectorised NumPy on ``dtype``: float64 is the reference, float32 shows what f32
arithmetic alone costs.
"""
from __future__ import annotations

import numpy as np

from . import vem_spec


def init(pair_word, V: int, K: int, KS: int, dtype=np.float64):
    """r ``dtype`` [P, KS] of the hash init; a pair with a word outside [0, V) gets a zero row."""
    pw = np.asarray(pair_word).astype(np.int64)
    ok = (pw >= 0) & (pw < int(V))
    t0 = 1.0 / float(V) + vem_spec.init_u(V, K).astype(np.float64)
    r = np.zeros((pw.size, int(KS)), dtype)
    r[ok, : int(K)] = (t0 / t0.sum(1, keepdims=True))[pw[ok]].astype(dtype)
    return r


def _live(pair_doc, pair_word, D: int, V: int):
    pd = np.asarray(pair_doc).astype(np.int64)
    pw = np.asarray(pair_word).astype(np.int64)
    return pd, pw, (pd >= 0) & (pd < int(D)) & (pw >= 0) & (pw < int(V))


def counts(r, pair_doc, pair_word, pair_cnt, D: int, V: int, dtype=np.float64):
    """(n_dk ``dtype`` [D, KS], n_wk ``dtype`` [V, KS], n_k float64 [KS]) of the rows ``r``: float64
    sums rounded once; n_k is the float64 sum of the rounded n_wk (vem_spec.table's ss_k)."""
    r = np.asarray(r)
    pd, pw, ok = _live(pair_doc, pair_word, D, V)
    cr = np.asarray(pair_cnt).astype(np.float64)[ok, None] * r[ok].astype(np.float64)
    ndk = np.zeros((int(D), r.shape[1]))
    nwk = np.zeros((int(V), r.shape[1]))
    np.add.at(ndk, pd[ok], cr)
    np.add.at(nwk, pw[ok], cr)
    nwk = nwk.astype(dtype)
    return ndk.astype(dtype), nwk, nwk.astype(np.float64).sum(0)


def update(r, n_dk, n_wk, n_k, pair_doc, pair_word, pair_cnt, K: int, alpha: float, beta: float, V: int,
           dtype=np.float64):
    """(r_new ``dtype`` [P, KS], n_dk_new ``dtype`` [D, KS]): one Jacobi step from the old counts and
    the document counts of the new rows."""
    r = np.asarray(r).astype(dtype)
    n_dk, n_wk = np.asarray(n_dk).astype(dtype), np.asarray(n_wk).astype(dtype)
    K, D = int(K), n_dk.shape[0]
    pd, pw, ok = _live(pair_doc, pair_word, D, V)
    ro = r[ok, :K]
    zero = dtype(0)
    x = np.maximum(n_dk[pd[ok], :K] - ro, zero) + dtype(alpha)
    y = np.maximum(n_wk[pw[ok], :K] - ro, zero) + dtype(beta)
    z = np.maximum(np.asarray(n_k).astype(dtype)[:K] - ro, zero) + dtype(float(V) * float(beta))
    u = (x * y) / z
    out = r.copy()
    out[ok, :K] = u / u.sum(1, keepdims=True)
    cr = np.asarray(pair_cnt).astype(np.float64)[ok, None] * out[ok].astype(np.float64)
    ndk = np.zeros(n_dk.shape)
    np.add.at(ndk, pd[ok], cr)
    return out, ndk.astype(dtype)


def theta(n_dk, doc_len, K: int, alpha: float, dtype=np.float64):
    """θ ``dtype`` [D, KS]: (n_dk + α)/(N_d + Kα), 1/K for a document of length 0, zero past K."""
    n = np.asarray(n_dk).astype(np.float64)
    N = np.asarray(doc_len).astype(np.float64)
    K = int(K)
    th = np.zeros(n.shape)
    th[:, :K] = (n[:, :K] + float(alpha)) / (N[:, None] + K * float(alpha))
    th[N <= 0, :K] = 1.0 / K
    return th.astype(dtype)


def cvb0(pair_doc, pair_word, pair_cnt, doc_len, V: int, K: int, KS: int, alpha: float, beta: float, iters: int,
         dtype=np.float64, trace=None):
    """(θ [D, KS], table [V + 1, KS], n_k [KS]) after ``iters`` steps from the hash init. ``trace``: a
    list that receives (iteration, plug-in log-likelihood) before every step and after the last."""
    D = np.asarray(doc_len).size
    r = init(pair_word, V, K, KS, dtype)
    n_dk, n_wk, n_k = counts(r, pair_doc, pair_word, pair_cnt, D, V, dtype)

    def _ll(it):
        if trace is not None:
            tab = vem_spec.table(n_wk, K, beta, dtype)[0]
            trace.append((it, vem_spec.loglik(theta(n_dk, doc_len, K, alpha, dtype), tab, pair_doc, pair_word,
                                              pair_cnt, V)))

    for it in range(int(iters)):
        _ll(it)
        r, _ = update(r, n_dk, n_wk, n_k, pair_doc, pair_word, pair_cnt, K, alpha, beta, V, dtype)
        n_dk, n_wk, n_k = counts(r, pair_doc, pair_word, pair_cnt, D, V, dtype)
    _ll(int(iters))
    tab, n_k = vem_spec.table(n_wk, K, beta, dtype)
    return theta(n_dk, doc_len, K, alpha, dtype), tab, n_k
