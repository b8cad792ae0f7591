"""Specification of variational-EM training on the device (csrc/kernels/vem.hip, ops.vem_resp /
vem_wsum / vem_table, models.vem_gpu.VarLDA): smoothed (MAP) variational EM with fixed α and β over
the corpus' distinct (doc, word, count) pairs ``(d_p, w_p, c_p)``, lda-c's ``lda est`` without its
α estimation, its ELBO and its convergence exits. No seed anywhere::

    init      ss0[w,k] = 1/V + u(w,k)        u = top 24 bits of mix32(w·K + k) · 2^-24
              table    = table(ss0)
    em_iters times:
      E-step  γ = vfold(pairs, table, K, α, iters=var_iters)            (vfold_spec, unchanged)
      resp    e_dk = exp(ψ(γ_dk) − max_j ψ(γ_dj))      k < K, 0 past K
              s_p  = Σ_k table[w_p,k] · e_{d_p,k}       q_p = c_p / s_p
      stats   ss[w,k] = table[w,k] · Σ_{p : w_p = w} q_p · e_{d_p,k}    (pairs of a word in ascending
                                                                         pair index; none: 0)
      table   ss_k = Σ_w ss[w,k]
              table[w,k] = (ss[w,k] + β) / (ss_k + Vβ)    w < V, k < K
              table[V,k] = β / (ss_k + Vβ)                the row of an unseen word
              columns K .. KS−1 are zero
    θ = vfold(pairs, table, ...)                          one final E-step against the final table

Both iteration counts are fixed: no result depends on a threshold. Scoring the training day against
the saved table with the variational fold-in (``var_iters`` iterations, no prior) therefore
reproduces θ. The likelihood reported is the plug-in one of :func:`oni355.ref.fit_spec.doc_fit`.

Everything is vectorised NumPy on ``dtype``: float64 is the reference, float32 shows what f32
arithmetic alone costs.
"""
from __future__ import annotations

import numpy as np
import torch

from . import fit_spec, vfold_spec

_M32 = 0xFFFFFFFF


def _mul32(x, c: int):
    """x · c mod 2^32 on int64 values below 2^32 without leaving int64 (c in two 16-bit halves)."""
    return ((((x * (c >> 16)) & 0xFFFF) << 16) + x * (c & 0xFFFF)) & _M32


def init_u(V: int, K: int, device=None):
    """u(w,k) ∈ [0,1), float32 [V, K]: the top 24 bits of lowbias32(w·K + k) (oni::mix32) times
    2^-24, in masked int64 arithmetic. NumPy without ``device``, else a torch tensor computed on
    that device: the same bits everywhere. ``V·K`` must stay below 2^32."""
    if int(V) * int(K) > _M32:
        raise ValueError("init_u: V·K must be below 2^32")
    if device is None:
        x = np.arange(int(V) * int(K), dtype=np.int64)
    else:
        x = torch.arange(int(V) * int(K), dtype=torch.int64, device=device)
    x = x & _M32
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    x = x ^ (x >> 16)
    x = x >> 8
    if isinstance(x, np.ndarray):
        return (x.astype(np.float32) * np.float32(2.0 ** -24)).reshape(int(V), int(K))
    return (x.to(torch.float32) * (2.0 ** -24)).reshape(int(V), int(K))


def init_ss(V: int, K: int, KS: int, dtype=np.float64):
    """ss0 ``dtype`` [V, KS]: 1/V + u(w,k), zero past K."""
    ss = np.zeros((int(V), int(KS)), dtype)
    ss[:, :K] = dtype(1.0) / dtype(V) + init_u(V, K).astype(dtype)
    return ss


def table(ss, K: int, beta: float, dtype=np.float64):
    """(table ``dtype`` [V + 1, KS], ss_k ``dtype`` [KS]) from the statistics ``ss`` [V, KS]."""
    ss = np.asarray(ss).astype(dtype)
    V, KS = ss.shape
    K = int(K)
    ssk = np.zeros(KS, dtype)
    ssk[:K] = ss[:, :K].sum(0)
    den = ssk[:K] + dtype(V) * dtype(beta)
    t = np.zeros((V + 1, KS), dtype)
    t[:V, :K] = (ss[:, :K] + dtype(beta)) / den
    t[V, :K] = dtype(beta) / den
    return t, ssk


def resp(gamma, tab, pair_doc, pair_word, pair_cnt, K: int, dtype=np.float64):
    """(e ``dtype`` [D, KS], q ``dtype`` [P] in the pairs' own order) from the E-step's γ."""
    g = np.asarray(gamma).astype(dtype)
    D, KS = g.shape
    K = int(K)
    pd = np.asarray(pair_doc).astype(np.int64)
    pw = np.asarray(pair_word).astype(np.int64)
    e = np.zeros((D, KS), dtype)
    if D:
        psi = torch.digamma(torch.from_numpy(np.ascontiguousarray(g[:, :K]))).numpy()
        e[:, :K] = np.exp(psi - psi.max(1, keepdims=True))
    s = (np.asarray(tab).astype(dtype)[pw, :K] * e[pd, :K]).sum(1)
    return e, (np.asarray(pair_cnt).astype(dtype) / s).astype(dtype)


def word_major(pair_word, pair_doc, V: int):
    """The word-major pair order, built once per model: (word_pair_ptr int64 [V + 1], wm_doc int32
    [P], wm_word int32 [P], wm_pos int32 [P]) with ``wm_pos[p]`` the word-major position of
    doc-major pair p. The sort is stable: a word's pairs stay in ascending document order."""
    pw = np.asarray(pair_word).astype(np.int64)
    order = np.argsort(pw, kind="stable")
    pos = np.empty(pw.size, np.int32)
    pos[order] = np.arange(pw.size, dtype=np.int32)
    ptr = np.zeros(int(V) + 1, np.int64)
    np.cumsum(np.bincount(pw, minlength=int(V))[: int(V)], out=ptr[1:])
    return ptr, np.asarray(pair_doc).astype(np.int32)[order], pw[order].astype(np.int32), pos


def wsum(e, q_wm, tab, word_pair_ptr, wm_doc, K: int, dtype=np.float64):
    """ss ``dtype`` [V, KS] from e [D, KS], the word-major q and documents and the table."""
    e = np.asarray(e).astype(dtype)
    ptr = np.asarray(word_pair_ptr).astype(np.int64)
    V, KS = ptr.size - 1, e.shape[1]
    ww = np.repeat(np.arange(V), np.diff(ptr))
    acc = np.zeros((V, KS), dtype)
    np.add.at(acc, ww, np.asarray(q_wm).astype(dtype)[:, None] * e[np.asarray(wm_doc).astype(np.int64)])
    return (np.asarray(tab).astype(dtype)[:V] * acc).astype(dtype)


def loglik(theta, tab, pair_doc, pair_word, pair_cnt, V: int) -> float:
    """The plug-in log-likelihood Σ c · log(θ_d·φ_w) of ops.doc_fit, from f32-rounded θ and table."""
    th = np.asarray(theta).astype(np.float32)
    return float(fit_spec.doc_fit(th, np.asarray(tab).astype(np.float32), pair_doc, pair_word, pair_cnt,
                                  th.shape[0], int(V))[4][0])


def vem(pair_doc, pair_word, pair_cnt, doc_pair_ptr, V: int, K: int, KS: int, alpha: float, beta: float,
        em_iters: int, var_iters: int, dtype=np.float64, trace=None):
    """(θ [D, KS], table [V + 1, KS], ss_k [KS]) after ``em_iters`` EM iterations and the final
    E-step. ``trace``: a list that receives (iteration, plug-in log-likelihood) before every
    iteration's M-step and after the last E-step."""
    wm_ptr, wm_doc, _, wm_pos = word_major(pair_word, pair_doc, V)
    tab, ssk = table(init_ss(V, K, KS, dtype), K, beta, dtype)
    for it in range(int(em_iters)):
        theta, g = vfold_spec.vfold(pair_word, pair_cnt, doc_pair_ptr, tab, K, alpha, None, var_iters, dtype)
        if trace is not None:
            trace.append((it, loglik(theta, tab, pair_doc, pair_word, pair_cnt, V)))
        e, q = resp(g, tab, pair_doc, pair_word, pair_cnt, K, dtype)
        q_wm = np.empty_like(q)
        q_wm[wm_pos] = q
        tab, ssk = table(wsum(e, q_wm, tab, wm_ptr, wm_doc, K, dtype), K, beta, dtype)
    theta, _ = vfold_spec.vfold(pair_word, pair_cnt, doc_pair_ptr, tab, K, alpha, None, var_iters, dtype)
    if trace is not None:
        trace.append((int(em_iters), loglik(theta, tab, pair_doc, pair_word, pair_cnt, V)))
    return theta, tab, ssk
