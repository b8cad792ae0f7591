"""Inputs and the reference shared by tests/test_fit_cpu.py and tests/test_gpu_fit.py: one doc-major
pair list with a document at every place of the 64-pair waves of k_fit_pairs that takes another
branch. Pair counts (first pair index): doc 0 none | 1: 1 (0) | 2: 63 (1), ends on lane 63 | 3: 64
(64), a whole wave | 4: 65 (128) | 5 none | 6: 62 (193), inside a wave | 7: 2 (255), starts on a last
lane | 8: 94 (257), exactly two waves | 9: 492 (351), nine waves, one more than kHeavyWaves: the
wave-wide branch of k_fit_docs | 10: 443 (843), eight waves, the longest one-lane combine | 11: 3 |
12..311: 1..3 pairs each (a second tile of 256 documents) | 312, 313 none. Counts are 1..5 with a 1
and a 2^20 forced; some words are the out-of-vocabulary row V; word V - 1 is in document 11 only."""
from __future__ import annotations

import math

import numpy as np

from oni355.ref import spec

V = 700
HEAD = [0, 1, 63, 64, 65, 0, 62, 2, 94, 492, 443, 3]
ZERO_DOC = 11
K_OF = {4: 3, 20: 20, 56: 50, 112: 100}


def pair_list():
    r = np.random.default_rng(5)
    sizes = np.array(HEAD + r.integers(1, 4, 300).tolist() + [0, 0])
    D = sizes.size
    pd = np.repeat(np.arange(D), sizes).astype(np.int32)
    words = np.concatenate([np.arange(V - 1), [V]])  # everything but V - 1
    pw = np.concatenate([np.sort(r.choice(words, n, replace=False)) for n in sizes]).astype(np.int32)
    pc = r.integers(1, 6, pd.size).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(sizes)])
    pw[0], pw[first[ZERO_DOC]] = V, V - 1  # document 1 is one out-of-vocabulary pair
    pc[3], pc[200], pc[400] = 1, 2**20, 2**20
    return pd, pw, pc, D


def model(KS: int, D: int, seed: int = 9):
    """θ [D, KS] and table [V + 1, KS]: positive over K columns, zero pads."""
    r = np.random.default_rng(seed + KS)
    K = K_OF[KS]
    th, tb = np.zeros((D, KS), np.float32), np.zeros((V + 1, KS), np.float32)
    th[:, :K] = r.dirichlet(np.full(K, 0.3), D).astype(np.float32) + np.float32(1e-6)
    tb[:, :K] = (r.dirichlet(np.full(V + 1, 0.1), K).T).astype(np.float32) + np.float32(1e-9)
    return th, tb


def reference(th, tb, pd, pw, pc, D):
    """Per document: math.fsum of count · log(score), score the f32 pair score of the spec, the log
    in np.longdouble; and the derived tolerance (4 + ⌈log2 max(P_d, 2)⌉) · 2^-52 · Σ c·|log s|. The
    last entry of each is the total's (the same form with P)."""
    s = spec.dot_rows(th[pd], tb[pw])
    with np.errstate(divide="ignore"):
        term = [float(t) for t in pc.astype(np.longdouble) * np.log(s.astype(np.longdouble))]
    ll, tol = [], []
    first = np.searchsorted(pd, np.arange(D + 1))
    for a, b in list(zip(first[:-1], first[1:])) + [(0, pd.size)]:
        ll.append(math.fsum(term[a:b]))
        tol.append((4 + math.ceil(math.log2(max(b - a, 2)))) * 2.0**-52 * math.fsum(abs(t) for t in term[a:b]))
    tok = np.bincount(pd, weights=pc, minlength=D).astype(np.int64)
    oov = np.bincount(pd, weights=np.where(pw == V, pc, 0), minlength=D).astype(np.int64)
    mn = np.full(D, np.inf, np.float32)
    np.minimum.at(mn, pd, s)
    return np.array(ll), np.array(tol), tok, oov, mn


def check(out, ref, D):
    ll, tol, tok, oov, mn = ref
    err = np.abs(out[0] - ll[:D])
    print("max |ll - ref| / tol over the documents:", float(np.max(err[tol[:D] > 0] / tol[:D][tol[:D] > 0])),
          "total:", abs(out[4][0] - ll[D]) / tol[D])
    assert np.all(err <= tol[:D])
    assert np.array_equal(out[1], tok) and np.array_equal(out[2], oov)
    assert out[3].dtype == np.float32 and out[3].tobytes() == mn.tobytes()
    assert abs(out[4][0] - ll[D]) <= tol[D]
    assert out[4][1:].tolist() == [float(tok.sum()), float(oov.sum()), float(np.count_nonzero(tok))]
