"""CPU side of the fused doc-and-pair build: ``ops.corpus.doc_pair_build`` on CPU tensors is the
torch reference (``encode_docs`` + ``torch_pairs``), and ``build_and_train`` on a CPU day still
builds the corpus the two separate calls give."""
import numpy as np
import pytest
import torch

from oni355.models.corpus import build_corpus
from oni355.models.gibbs import tiling_for
from oni355.ops import corpus as oc
from oni355.pipeline import common

FIELDS = ("pair_doc", "pair_word", "pair_cnt", "doc_pair_ptr", "doc_tok_ptr", "pair_tokoff", "slice_off",
          "slice_len", "chunk_doc", "chunk_pos0", "chunk_len", "chunk_key", "chunk_multi", "tok_word", "long_rows",
          "wsorted", "wslot", "tile_wlo", "tile_whi", "wpos", "doc_keys")


def _day(n, D, V, seed):
    r = np.random.default_rng(seed)
    table = np.unique(r.integers(0, 2**32, 2 * D + 16, dtype=np.int64))
    table = table[r.permutation(table.size)[:D]]
    table[0] |= 0x80000000
    p = 1.0 / np.arange(1, D + 1) ** 1.1
    keys = torch.from_numpy(table[r.choice(D, n, p=p / p.sum())])
    word = torch.from_numpy(np.minimum(r.zipf(1.3, n) - 1, V - 1).astype(np.int32))
    return keys, word


@pytest.mark.parametrize("n,D,V,weighted,form", [(1, 1, 1, False, "i64"), (65, 20, 2, True, "halves"),
                                                 (5000, 300, 200, False, "i32"), (5000, 300, 5740, True, "i64")])
def test_cpu_doc_pair_build_is_the_torch_reference(n, D, V, weighted, form):
    keys, word = _day(n, D, V, seed=n + V)
    w = None
    if weighted:
        w = torch.ones(n, dtype=torch.int32)
        w[::7] = 1000
    k32 = (keys & 0xFFFFFFFF).to(torch.int32)
    dk = {"i64": keys, "i32": k32, "halves": (k32[: n // 3].contiguous(), k32[n // 3:].contiguous())}[form]
    n0 = n // 2
    udoc, ps = oc.doc_pair_build(dk, word, V, w, n0=n0)
    ru, rinv = common.encode_docs(keys)
    rp = common.torch_pairs(rinv, word, V)
    assert torch.equal(udoc, ru) and ps.D == ru.numel() and ps.V == V and ps.nnz == rp.pair_doc.numel()
    for f in ("pair_doc", "pair_word", "tok_pair"):
        a, b = getattr(rp, f), getattr(ps, f)
        assert a.dtype == b.dtype and torch.equal(a, b), f
    wt = w.long() if w is not None else torch.ones(n, dtype=torch.int64)
    assert torch.equal(ps.pair_cnt.long(), torch.zeros(ps.nnz, dtype=torch.int64).index_add_(0, rp.tok_pair.long(), wt))
    if n0:
        assert torch.equal(ps.order0, torch.argsort(rp.tok_pair[:n0], stable=True))
    else:
        assert ps.order0 is None
    assert oc.doc_pair_build(dk, word, V, w)[1].order0 is None


@pytest.mark.parametrize("weighted", [False, True])
def test_cpu_build_and_train_corpus_equals_separate_calls(weighted):
    n, D, V, K, L = 4000, 250, 120, 20, 32
    keys, word = _day(n, D, V, seed=17)
    vocab = torch.arange(V, dtype=torch.int64) * 3 + 1
    w = None
    if weighted:
        w = torch.ones(n, dtype=torch.int32)
        w[::11] = 1000
    run = common.build_and_train(keys, vocab[word.long()], w, vocab, K, None, 0.01, 7, 0, L, None, train=False,
                                 n_event0=n // 2)
    udoc, inv = common.encode_docs(keys)
    ref = build_corpus(inv, word, int(udoc.numel()), V, common.i64_to_u32bits(udoc), tiling_for(K)[0], L, weight=w)
    assert torch.equal(run.doc_keys64, udoc) and run.route is None and run.pairs is None
    got = run.corpus
    assert (got.D, got.V, got.T, got.G, got.L) == (ref.D, ref.V, ref.T, ref.G, ref.L)
    for f in FIELDS:
        a, b = getattr(ref, f), getattr(got, f)
        assert a.dtype == b.dtype and torch.equal(a, b), f
