"""NumPy specification of ``ops.doc_fit`` (csrc/kernels/fit.hip): how well a model table fits a
batch, per document.

    ll_d = Σ_{pairs (d,w)} c_dw · log( Σ_k θ_dk · φ_wk )

The pair score is :func:`oni355.ref.spec.dot_rows` (f32, fixed k order), exactly what
``ops.pair_score`` returns; the log is ``np.log`` on float64 and each document's sum is taken in
float64 over its pairs in list order. The device adds the same terms in another (fixed) order, so
``ll`` agrees within the summation tolerance of ``tests/test_gpu_fit.py``; the integers and
``min_score`` agree exactly.
"""
from __future__ import annotations

import numpy as np

from . import spec


def doc_fit(theta, table, pair_doc, pair_word, pair_count, D: int, oov_id: int):
    """(ll f64 [D], tokens i64 [D], oov_tokens i64 [D], min_score f32 [D], tot f64 [4]).

    ``pair_doc`` is non-decreasing (doc-major pairs). A document without pairs gets 0, 0, 0, +inf;
    a pair score of exactly 0 gives -inf for its document and for ``tot[0]``. ``tot`` = Σ ll,
    Σ tokens, Σ oov_tokens, the number of documents with at least one token."""
    pd = np.asarray(pair_doc).astype(np.int64)
    pw = np.asarray(pair_word).astype(np.int64)
    c = np.asarray(pair_count).astype(np.int64)
    D = int(D)
    if pd.size and (np.any(np.diff(pd) < 0) or pd[0] < 0 or pd[-1] >= D):
        raise ValueError("doc_fit: pair_doc must be non-decreasing in [0, D)")
    ll = np.zeros(D, np.float64)
    tok = np.zeros(D, np.int64)
    oov = np.zeros(D, np.int64)
    mn = np.full(D, np.inf, np.float32)
    if pd.size:
        s = spec.dot_rows(np.asarray(theta)[pd], np.asarray(table)[pw])
        with np.errstate(divide="ignore", invalid="ignore"):
            term = c.astype(np.float64) * np.log(s.astype(np.float64))
        docs, start = np.unique(pd, return_index=True)  # the documents with pairs, each one's first pair
        ll[docs] = np.add.reduceat(term, start)
        tok[docs] = np.add.reduceat(c, start)
        oov[docs] = np.add.reduceat(np.where(pw == int(oov_id), c, 0), start)
        mn[docs] = np.minimum.reduceat(s, start)
    with np.errstate(invalid="ignore"):
        tot = np.array([ll.sum(), float(tok.sum()), float(oov.sum()), float(np.count_nonzero(tok > 0))], np.float64)
    return ll, tok, oov, mn, tot
