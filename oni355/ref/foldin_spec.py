"""NumPy specification oracle of fold-in inference (csrc/kernels/foldin.hip, k_foldin).

Fold-in estimates the doc-topic counts of NEW documents against a frozen word table φ (a saved
model, :mod:`oni355.models.saved`): the `lda inf` half of the reference's LDA engine. A token of
word w in document d draws topic k with weight

    p_k ∝ (n_dk^¬t + α) · φ_wk

-- the doc side is exact within a chunk (sequential updates, the token removed), the word side is
the frozen row used as is (the token was never counted in it: no exclusion). Row V of φ is the row
of a word the model never saw (``phi_oov``). Like :func:`oni355.ref.spec.gibbs_pass` this replays
the kernel bit for bit: same f32 operation order, the same fma chain, the same Philox stream.

Philox streams: 2 for the init pass (sweep counter 0), 3 for the sweeps; training draws from
streams 0 and 1. (The MH training sampler's word move also names stream 2, but with the token
position -- not position / 4 -- as the first counter word and sweep ≥ 1, so no counter is shared
with the fold-in init pass at sweep 0.)
"""
from __future__ import annotations

import numpy as np

from . import spec
from .spec import F32, U32, fma_f32, token_rand

SELECT_ALL, SELECT_SINGLE, SELECT_MULTI = 0, 1, 2
# document keys from here up are ids of a per-day IPv6 dictionary (pipeline.flow.with_ipv6_keys):
# they name another address on another day, so they carry no prior
V6_KEY_BASE = 0xF0000000


def prior_rows(doc_keys_model: np.ndarray, doc_theta: np.ndarray, doc_tokens: np.ndarray,
               batch_doc_keys: np.ndarray, K: int, KS: int, alpha: float, mass: float) -> np.ndarray:
    """Per-document Dirichlet prior rows of a batch from a saved model's document profiles
    (k_prior_rows, csrc/kernels/foldin.hip), f32 [D, KS].

    ``doc_keys_model`` int64 [Dm] strictly ascending, ``doc_theta`` f32 [Dm, ≥ K], ``doc_tokens``
    int64 [Dm]; ``batch_doc_keys`` int64 [D]. A batch key found in the model (binary search) below
    :data:`V6_KEY_BASE` gets pr_j = fma(m, θ_ij, f32(α)) for j < K with m = min(f32(tokens_i),
    f32(mass)): the training day's θ weighted by at most ``mass`` pseudo-tokens, never by more than
    the document had. Every other element (unknown keys, per-day IPv6 ids, columns ≥ K) is f32(α)."""
    keys = np.asarray(batch_doc_keys, dtype=np.int64)
    mk = np.asarray(doc_keys_model, dtype=np.int64)
    a32 = F32(alpha)
    out = np.full((keys.shape[0], KS), a32, dtype=F32)
    if mk.shape[0] == 0 or keys.shape[0] == 0:
        return out
    pos = np.minimum(np.searchsorted(mk, keys), mk.shape[0] - 1)
    hit = np.nonzero((mk[pos] == keys) & (keys < V6_KEY_BASE))[0]
    row = pos[hit]
    m = np.minimum(np.asarray(doc_tokens, dtype=np.int64)[row].astype(F32), F32(mass))
    th = np.asarray(doc_theta, dtype=F32)[row, :K]
    out[hit, :K] = fma_f32(np.broadcast_to(m[:, None], th.shape), th, np.full(th.shape, a32, dtype=F32))
    return out


def theta_rows_prior(ndk_sum: np.ndarray, prior: np.ndarray, K: int, S: float) -> np.ndarray:
    """θ of documents folded in under per-document prior rows (k_theta_rows_prior,
    csrc/kernels/day_tail.hip), f32 [D, KS]: with S32 = f32(S) window samples,
    num_j = fma(S32, pr_j, f32(Σn_dj)), sp = pr_0 + pr_1 + … + pr_{K−1} added in that order in f32,
    den = fma(S32, sp, f32(n_d)) with n_d the int64 row sum over j < K, θ_j = num_j / den; columns
    ≥ K zero."""
    n = np.asarray(ndk_sum)
    pr = np.asarray(prior, dtype=F32)
    D, KS = n.shape
    S32 = np.full(D, F32(S), dtype=F32)
    sp = np.zeros(D, dtype=F32)
    for j in range(K):
        sp = sp + pr[:, j]
    nd = n[:, :K].astype(np.int64).sum(1).astype(F32)
    den = fma_f32(S32, sp, nd)
    th = np.zeros((D, KS), dtype=F32)
    for j in range(K):
        th[:, j] = fma_f32(S32, pr[:, j], n[:, j].astype(F32)) / den
    return th


def foldin_pass(st: dict, G: int, KP: int, K: int, alpha: float, seed0: int, seed1: int, init: bool,
                sweep: int, chunk_len: np.ndarray, select: int = SELECT_ALL, prior: np.ndarray | None = None) -> None:
    """One init (``init``) or sweep pass over numpy state arrays, in place.

    Per chunk: ``n`` starts at zero (init) or at ``ndk_src[doc]``; tokens are taken in chunk order.
    Per token: on a sweep ``n[zo] -= 1``; a_j = f32(n_j) + f32(α); lane g chains its KP topics,
    P_j = fma(a_j, φ_wj, P_{j−1}); lanes are combined, and the topic drawn, by the training oracle's
    own :func:`spec.unit_draw`: thr = u01(r)·total; zn = min(#{cum ≤ thr}, K − 1); ``n[zn] += 1``,
    ``tok_z = zn``. The init pass is the same code without the decrement: a chunk's tokens are drawn
    one after another from (n_so_far + α)·φ_w. Epilogue as in gibbs_pass: a single-chunk document
    writes its row to ``ndk_dst``, a multi-chunk document adds its Δ.

    ``select``: 0 every chunk, 1 only chunks of single-chunk documents, 2 only chunks of
    multi-chunk documents (the kernel's launch selections).

    st keys: tok_word u32 (ids into φ, V = out of vocabulary), tok_z u8, slice_off i64, chunk_doc
    i32, chunk_pos0 i32, chunk_key u32, chunk_multi u8, ndk_src i32 [D, KS], ndk_dst i32 [D, KS],
    phi f32 [V + 1, KS] (columns ≥ K zero).

    ``prior`` (f32 [D, KS], :func:`prior_rows`): a_j = f32(n_j) + prior[doc, j] in place of + f32(α),
    the same row in every chunk of a document; nothing else changes.
    """
    S = 64 // G
    KS = G * KP
    doc = st["chunk_doc"]
    C = doc.shape[0]
    cid = np.arange(C)
    slc, lane = cid // S, cid % S
    multi_c = st["chunk_multi"] != 0
    live = doc >= 0
    if select == SELECT_SINGLE:
        live = live & ~multi_c
    elif select == SELECT_MULTI:
        live = live & multi_c
    n = np.zeros((C, KS), dtype=np.int32)
    if not init:
        n[live] = st["ndk_src"][doc[live]]
    n_start = n.copy()
    clen = np.where(live, chunk_len, 0)
    alpha32 = F32(alpha)
    stream = 2 if init else 3
    sw = 0 if init else sweep
    phi = st["phi"]
    for s in range(int(clen.max(initial=0))):
        act = np.nonzero(clen > s)[0]
        idx = st["slice_off"][slc[act]] + s * S + lane[act]
        w = st["tok_word"][idx].astype(np.int64)
        pos = st["chunk_pos0"][act].astype(U32) + U32(s)
        rr = token_rand(pos, st["chunk_key"][act], sw, stream, seed0, seed1)
        if not init:
            zo = st["tok_z"][idx].astype(np.int64)
            n[act, zo] -= 1
        add = alpha32 if prior is None else prior[doc[act]]
        av = (n[act].astype(F32) + add).reshape(-1, G, KP)
        zn = spec.unit_draw(av, phi[w].reshape(-1, G, KP), rr, K)
        n[act, zn] += 1
        st["tok_z"][idx] = zn.astype(np.uint8)
    d = n - n_start
    multi = live & multi_c
    single = live & ~multi_c
    st["ndk_dst"][doc[single]] = n[single]
    np.add.at(st["ndk_dst"], doc[multi], d[multi])


def window(sweeps: int, avg_last: int) -> tuple[int, int]:
    """(avg_from, samples): the window sums take the rows after sweeps avg_from..sweeps (the last
    ``avg_last``, at least one, at most all). No sweeps: the init counts are the one sample."""
    if sweeps <= 0:
        return 1, 1
    s = max(1, min(int(avg_last), int(sweeps)))
    return sweeps - s + 1, s


def foldin_run(st: dict, G: int, KP: int, K: int, alpha: float, seed0: int, seed1: int, sweeps: int,
               avg_last: int, chunk_len: np.ndarray, prior: np.ndarray | None = None):
    """Init pass + ``sweeps`` sweeps (numbered 1..sweeps) over ``st`` (``ndk_src`` / ``ndk_dst``
    give the [D, KS] shape; their contents are replaced). Returns (ndk_sum, ndk): the sum of the
    doc rows after each of the last ``avg_last`` sweeps (int32 [D, KS]) and the final rows."""
    ndk = np.zeros_like(st["ndk_dst"])
    st["ndk_src"] = st["ndk_dst"] = ndk
    foldin_pass(st, G, KP, K, alpha, seed0, seed1, True, 0, chunk_len, prior=prior)
    avg_from, _ = window(sweeps, avg_last)
    ndk_sum = np.zeros_like(ndk)
    for sweep in range(1, sweeps + 1):
        st["ndk_src"], st["ndk_dst"] = ndk, ndk.copy()  # multi-chunk rows: Δ into the pre-copied row
        foldin_pass(st, G, KP, K, alpha, seed0, seed1, False, sweep, chunk_len, prior=prior)
        ndk = st["ndk_dst"]
        if sweep >= avg_from:
            ndk_sum += ndk
    if sweeps <= 0:
        ndk_sum += ndk
    st["ndk_src"] = st["ndk_dst"] = ndk
    return ndk_sum, ndk


__all__ = ["foldin_pass", "foldin_run", "window", "prior_rows", "theta_rows_prior", "V6_KEY_BASE", "SELECT_ALL", "SELECT_SINGLE", "SELECT_MULTI", "spec"]
