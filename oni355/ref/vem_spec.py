"""Specification of variational-EM training on the device (csrc/kernels/vem.hip, ops.vem_resp /
vem_wsum / vem_table, models.vem_gpu.VarLDA): smoothed (MAP) variational EM with fixed α and β over
the corpus' distinct (doc, word, count) pairs ``(d_p, w_p, c_p)``: lda-c's ``lda est``. Its variational
bound, its EM convergence exit and its α estimation are options (:func:`bound`, :func:`alpha_newton`,
``em_tol`` / ``estimate_alpha`` of :func:`vem`), off by default. No seed anywhere::

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

``var_iters`` is fixed, and so is ``em_iters`` unless ``em_tol`` > 0. Scoring the training day against
the saved table with the variational fold-in (``var_iters`` iterations, no prior, the saved α)
therefore reproduces θ. The likelihood reported is the plug-in one of
:func:`oni355.ref.fit_spec.doc_fit`; the bound EM climbs is :func:`bound`::

    S_d = Σ_{k<K} γ_dk      E_dk = ψ(γ_dk) − ψ(S_d)      x_dk = exp(E_dk)
    A_d = Σ_{k<K} ψ(γ_dk) − K·ψ(S_d)                                 (α statistic of the document)
    T_d = lgamma(Kα) − K·lgamma(α) − lgamma(S_d) + Σ_{k<K} [(α − γ_dk)·E_dk + lgamma(γ_dk)]
    L_d = T_d + Σ_{p in d} c_p · log(Σ_{k<K} table[w_p,k] · x_{d_p,k})

(the pair term is lda-c's Σ_k φ_pk(E_k − log φ_pk + log β_kw) at the optimal φ, where it is log s_p).

Everything is vectorised NumPy on ``dtype``: float64 is the reference, float32 shows what f32
arithmetic alone costs.
"""
from __future__ import annotations

import math

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


def bound(gamma, tab, pair_doc, pair_word, pair_cnt, K: int, alpha: float):
    """(L_d float64 [D], float64 [2] = Σ_d L_d, Σ_d A_d): the variational bound per document and the α
    sufficient statistic, in float64 from γ [D, KS] and the table as given (see the module text).
    A pair whose s_p is 0 gives −inf; pairs naming a document outside [0, D) or a word outside the
    table's rows contribute nothing."""
    g = np.asarray(gamma).astype(np.float64)[:, : int(K)]
    tab = np.asarray(tab)
    D, K, alpha = g.shape[0], int(K), float(alpha)
    pd = np.asarray(pair_doc).astype(np.int64)
    pw = np.asarray(pair_word).astype(np.int64)
    ok = (pd >= 0) & (pd < D) & (pw >= 0) & (pw < tab.shape[0])
    pd, pw, c = pd[ok], pw[ok], np.asarray(pair_cnt).astype(np.float64)[ok]
    S = g.sum(1)
    psi = torch.digamma(torch.from_numpy(np.ascontiguousarray(g))).numpy()
    pS = torch.digamma(torch.from_numpy(S)).numpy()
    lg = torch.lgamma(torch.from_numpy(np.ascontiguousarray(g))).numpy()
    E = psi - pS[:, None]
    A = psi.sum(1) - K * pS
    L = (math.lgamma(K * alpha) - K * math.lgamma(alpha)) - torch.lgamma(torch.from_numpy(S)).numpy() \
        + ((alpha - g) * E + lg).sum(1)
    s = (tab[pw, :K].astype(np.float64) * np.exp(E)[pd]).sum(1)
    with np.errstate(divide="ignore"):
        np.add.at(L, pd, c * np.log(s))
    return L, np.array([L.sum(), A.sum()], np.float64)


def _f64(fn, x: float) -> float:
    return float(fn(torch.tensor(float(x), dtype=torch.float64)))


def alpha_newton(alpha_ss: float, D: int, K: int) -> float:
    """The symmetric α that maximises the bound given Σ_d A_d: lda-c's Newton iteration on log α
    from 100 (``mle`` of csrc/lda_cpu/lda_vem.cpp), float64, at most 1000 steps, until |df| ≤ 1e-5,
    with its ×10 restart when a step leaves the representable range."""
    D, K, ss = float(D), float(K), float(alpha_ss)
    init_a = 100.0
    log_a, df = math.log(init_a), 1.0
    for _ in range(1000):
        if abs(df) <= 1e-5:
            break
        try:
            a = math.exp(log_a)
        except OverflowError:
            a = float("nan")
        if math.isnan(a) or math.isinf(a) or a <= 0.0:
            init_a *= 10.0
            a = init_a
            log_a = math.log(a)
        df = D * (K * _f64(torch.digamma, K * a) - K * _f64(torch.digamma, a)) + ss
        d2f = D * (K * K * _f64(lambda t: torch.polygamma(1, t), K * a) - K * _f64(lambda t: torch.polygamma(1, t), a))
        log_a -= df / (d2f * a + df)
    return math.exp(log_a)


def vem(pair_doc, pair_word, pair_cnt, doc_pair_ptr, V: int, K: int, KS: int, alpha: float, beta: float,
        em_iters: int, var_iters: int, dtype=np.float64, trace=None, em_tol: float = 0.0,
        estimate_alpha: bool = False, bounds=None):
    """(θ [D, KS], table [V + 1, KS], ss_k [KS]) after ``em_iters`` EM iterations and the final
    E-step. ``trace``: a list that receives (iteration, plug-in log-likelihood) before every
    iteration's M-step and after the last E-step.

    With ``em_tol`` > 0 or ``estimate_alpha`` every iteration's E-step is followed by :func:`bound`
    (float64, from the ``dtype`` γ and table, as the device computes it from f32 ones) and
    ``bounds`` (a list) receives (iteration, L, conv, α) with conv = (L_old − L)/L_old, 1.0 for the
    first, then (iterations run, L of the final E-step, None, final α). ``estimate_alpha``: after
    the table update α ← :func:`alpha_newton` rounded to float32 (what a saved model carries).
    ``em_tol`` > 0: ``em_iters`` is the maximum; EM stops after the M-step of an iteration that
    is at least the third and has 0 ≤ conv ≤ em_tol."""
    wm_ptr, wm_doc, _, wm_pos = word_major(pair_word, pair_doc, V)
    tab, ssk = table(init_ss(V, K, KS, dtype), K, beta, dtype)
    track = em_tol > 0 or estimate_alpha
    L_old, done = 0.0, 0
    for it in range(int(em_iters)):
        theta, g = vfold_spec.vfold(pair_word, pair_cnt, doc_pair_ptr, tab, K, alpha, None, var_iters, dtype)
        if trace is not None:
            trace.append((it, loglik(theta, tab, pair_doc, pair_word, pair_cnt, V)))
        conv = 1.0
        if track:
            _, (L, a_ss) = bound(g, tab, pair_doc, pair_word, pair_cnt, K, alpha)
            conv = 1.0 if L_old == 0 else (L_old - L) / L_old
            L_old = L
            if bounds is not None:
                bounds.append((it, float(L), float(conv), float(alpha)))
        e, q = resp(g, tab, pair_doc, pair_word, pair_cnt, K, dtype)
        q_wm = np.empty_like(q)
        q_wm[wm_pos] = q
        tab, ssk = table(wsum(e, q_wm, tab, wm_ptr, wm_doc, K, dtype), K, beta, dtype)
        if estimate_alpha:
            alpha = float(np.float32(alpha_newton(a_ss, g.shape[0], K)))
        done = it + 1
        if em_tol > 0 and done >= 3 and 0 <= conv <= em_tol:
            break
    theta, g = vfold_spec.vfold(pair_word, pair_cnt, doc_pair_ptr, tab, K, alpha, None, var_iters, dtype)
    if trace is not None:
        trace.append((done if track else int(em_iters), loglik(theta, tab, pair_doc, pair_word, pair_cnt, V)))
    if track and bounds is not None:
        bounds.append((done, float(bound(g, tab, pair_doc, pair_word, pair_cnt, K, alpha)[1][0]), None, float(alpha)))
    return theta, tab, ssk
