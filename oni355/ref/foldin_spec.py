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
from .spec import F32, U32, token_rand

SELECT_ALL, SELECT_SINGLE, SELECT_MULTI = 0, 1, 2


def foldin_pass(st: dict, G: int, KP: int, K: int, alpha: float, seed0: int, seed1: int, init: bool,
                sweep: int, chunk_len: np.ndarray, select: int = SELECT_ALL) -> None:
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
        av = (n[act].astype(F32) + alpha32).reshape(-1, G, KP)
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
               avg_last: int, chunk_len: np.ndarray):
    """Init pass + ``sweeps`` sweeps (numbered 1..sweeps) over ``st`` (``ndk_src`` / ``ndk_dst``
    give the [D, KS] shape; their contents are replaced). Returns (ndk_sum, ndk): the sum of the
    doc rows after each of the last ``avg_last`` sweeps (int32 [D, KS]) and the final rows."""
    ndk = np.zeros_like(st["ndk_dst"])
    st["ndk_src"] = st["ndk_dst"] = ndk
    foldin_pass(st, G, KP, K, alpha, seed0, seed1, True, 0, chunk_len)
    avg_from, _ = window(sweeps, avg_last)
    ndk_sum = np.zeros_like(ndk)
    for sweep in range(1, sweeps + 1):
        st["ndk_src"], st["ndk_dst"] = ndk, ndk.copy()  # multi-chunk rows: Δ into the pre-copied row
        foldin_pass(st, G, KP, K, alpha, seed0, seed1, False, sweep, chunk_len)
        ndk = st["ndk_dst"]
        if sweep >= avg_from:
            ndk_sum += ndk
    if sweeps <= 0:
        ndk_sum += ndk
    st["ndk_src"] = st["ndk_dst"] = ndk
    return ndk_sum, ndk


__all__ = ["foldin_pass", "foldin_run", "window", "SELECT_ALL", "SELECT_SINGLE", "SELECT_MULTI", "spec"]
