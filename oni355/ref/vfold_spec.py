"""Specification of the variational fold-in (csrc/kernels/vfold.hip, ops.vfold): mean-field θ of
new documents against a frozen word table, over the doc-major distinct (doc, word, count) pairs.

Per document d with pairs p = (w_p, c_p) in corpus order, table rows φ_w and prior row a_d::

    γ_k ← a_dk + N_d / K                          N_d = Σ c_p, k < K
    iters times:  e_k = exp(ψ(γ_k) − max_j ψ(γ_j))
                  s_p = Σ_k φ_{w_p,k} · e_k
                  r_k = Σ_p (c_p / s_p) · φ_{w_p,k}      (pairs in corpus order)
                  γ_k ← a_dk + e_k · r_k
    θ_dk = γ_k / Σ_j γ_j  (k < K), 0 for K ≤ k < KS

This is the batch (Jacobi) form of lda-c's E-step: the same fixed point as the in-place update of
csrc/lda_cpu/lda_vem.cpp ``infer_doc``, without that function's per-word update order and without
its likelihood-based stopping rule -- the iteration count is fixed. A document without pairs gets
θ = a_d / Σ a_d. ψ is ``torch.digamma`` on ``dtype`` (independent of the device's own series);
float64 is the reference, float32 shows what f32 arithmetic alone costs.
"""
from __future__ import annotations

import numpy as np
import torch


def vfold(pair_word, pair_cnt, doc_pair_ptr, table, K: int, alpha: float, prior=None, iters: int = 20,
          dtype=np.float64):
    """(θ, γ), both ``dtype`` [D, KS]. ``table`` [rows, KS], ``prior`` [D, KS] or None (the flat α)."""
    ptr = np.asarray(doc_pair_ptr).astype(np.int64)
    D, K, iters = ptr.size - 1, int(K), int(iters)
    table = np.asarray(table)
    KS = table.shape[1]
    if not 1 <= K <= KS or iters < 0 or D < 0:
        raise ValueError("vfold: 1 ≤ K ≤ KS, iters ≥ 0")
    pw = np.asarray(pair_word).astype(np.int64)
    c = np.asarray(pair_cnt).astype(dtype)
    pd = np.repeat(np.arange(D), np.diff(ptr))
    if pd.size != pw.size or (ptr.size and ptr[0] != 0):
        raise ValueError("vfold: doc_pair_ptr must run from 0 to the number of pairs")
    phi = table[pw, :K].astype(dtype)
    a = np.full((D, K), alpha, dtype) if prior is None else np.asarray(prior)[:, :K].astype(dtype)
    N = np.zeros(D, dtype)
    np.add.at(N, pd, c)
    g = a + (N / dtype(K))[:, None]
    for _ in range(iters):
        psi = torch.digamma(torch.from_numpy(g)).numpy()
        e = np.exp(psi - psi.max(1, keepdims=True))
        s = (phi * e[pd]).sum(1)
        r = np.zeros((D, K), dtype)
        np.add.at(r, pd, (c / s)[:, None] * phi)
        g = (a + e * r).astype(dtype)
    theta = np.zeros((D, KS), dtype)
    gamma = np.zeros((D, KS), dtype)
    gamma[:, :K] = g
    theta[:, :K] = g / g.sum(1, keepdims=True)
    return theta, gamma
