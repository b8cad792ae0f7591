"""Specification of the variational fold-in with a warm start and a per-document exit
(csrc/kernels/vfold_exit.hip, ops.vfold_exit): :mod:`oni355.ref.vfold_spec`'s update, started from a
given γ and stopped per document.

Per document, with γ_old → γ_new exactly one iteration of ``vfold_spec.vfold``::

    γ ← gamma0[d, :K]  if given, else a_d + N_d / K
    up to max_iters times, while the document is not frozen:
        γ_new = update(γ_old)
        change = Σ_k |γ_new,k − γ_old,k|        total = Σ_k γ_new,k
        γ ← γ_new;  freeze when change ≤ tol · total

The change is relative to Σγ (= Σa + N_d up to rounding), not an absolute mean change: a document
of 10⁶ events has γ of 10⁵ whose f32 spacing alone is 0.008. ``tol = 0`` freezes only on an exact
fixed point, which loses nothing because the update is a function of γ_old alone. This is NOT
lda-c's ``var converged`` on the relative change of the per-document likelihood (a lgamma row per
iteration): it is the γ-change rule above.

``n_it[d]`` is the number of updates the document received (1 ≤ n_it ≤ max_iters for
max_iters ≥ 1; a document without pairs has γ = a_d after one update and freezes after at most
two). ``force_iters`` (int [D]) replaces the rule by given counts, to replay decisions taken in
another precision. ``trace`` [D, max_iters] is change/total per update, NaN after the freeze.
"""
from __future__ import annotations

import numpy as np
import torch


def vfold_exit(pair_word, pair_cnt, doc_pair_ptr, table, K: int, alpha: float, prior=None, max_iters: int = 20,
               tol: float = 0.0, gamma0=None, force_iters=None, dtype=np.float64):
    """(θ, γ, n_it, trace): θ, γ ``dtype`` [D, KS], n_it int32 [D], trace ``dtype`` [D, max_iters]."""
    ptr = np.asarray(doc_pair_ptr).astype(np.int64)
    D, K, max_iters = ptr.size - 1, int(K), int(max_iters)
    table = np.asarray(table)
    KS = table.shape[1]
    if not 1 <= K <= KS or max_iters < 0 or D < 0:
        raise ValueError("vfold_exit: 1 ≤ K ≤ KS, max_iters ≥ 0")
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError("vfold_exit: tol must be finite and ≥ 0")
    pw = np.asarray(pair_word).astype(np.int64)
    c = np.asarray(pair_cnt).astype(dtype)
    pd = np.repeat(np.arange(D), np.diff(ptr))
    if pd.size != pw.size or (ptr.size and ptr[0] != 0):
        raise ValueError("vfold_exit: doc_pair_ptr must run from 0 to the number of pairs")
    phi = table[pw, :K].astype(dtype)
    a = np.full((D, K), alpha, dtype) if prior is None else np.asarray(prior)[:, :K].astype(dtype)
    if gamma0 is None:
        N = np.zeros(D, dtype)
        np.add.at(N, pd, c)
        g = a + (N / dtype(K))[:, None]
    else:
        g = np.asarray(gamma0)[:, :K].astype(dtype)
    force = None if force_iters is None else np.asarray(force_iters).astype(np.int64)
    tol = dtype(tol)
    active = np.full(D, max_iters > 0) if force is None else force > 0
    n_it = np.zeros(D, np.int32)
    trace = np.full((D, max_iters), np.nan, dtype)
    for it in range(max_iters):
        if not active.any():
            break
        psi = torch.digamma(torch.from_numpy(g)).numpy()
        e = np.exp(psi - psi.max(1, keepdims=True))
        s = (phi * e[pd]).sum(1)
        r = np.zeros((D, K), dtype)
        np.add.at(r, pd, (c / s)[:, None] * phi)
        new = (a + e * r).astype(dtype)
        change, total = np.abs(new - g).sum(1), new.sum(1)
        g = np.where(active[:, None], new, g)
        n_it[active] += 1
        trace[active, it] = (change / total)[active]
        active = active & ~(change <= tol * total) if force is None else n_it < force
    theta = np.zeros((D, KS), dtype)
    gamma = np.zeros((D, KS), dtype)
    gamma[:, :K] = g
    theta[:, :K] = g / g.sum(1, keepdims=True)
    return theta, gamma, n_it, trace
