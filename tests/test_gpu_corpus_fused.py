"""The fused doc-and-pair build (csrc/kernels/corpus.hip ``oni_doc_pair_build``) == ``dict_encode`` of
the doc keys followed by ``pair_build`` of the ids, output by output, at the sizes where its paths
part: one token, one wave + 1, either side of the sort-back threshold, a size that is no multiple
of the block; doc keys with the top bit set, one doc, one doc per token; V = 1 (zero word bits), 2,
5740 and D·V > 2^32; every ``n0``; weights; and a second call that reuses the scratch arena."""
import numpy as np
import pytest
import torch

from oni355.ops import corpus as oc

pytestmark = pytest.mark.gpu

BACK = 1 << 21  # kSortBackMin


def _tokens(n, D, V, seed, docs="zipf"):
    """Seeded Zipf tokens: (u32 doc keys as int64, with the top bit set on about half; int32 words)."""
    r = np.random.default_rng(seed)
    if docs == "one":
        doc = np.zeros(n, dtype=np.int64)
    elif docs == "own":
        doc = r.permutation(n).astype(np.int64)
    else:
        p = 1.0 / np.arange(1, D + 1) ** 1.1
        doc = r.choice(D, n, p=p / p.sum())
        if n >= D:
            doc[:D] = np.arange(D)  # every doc present: D is the dictionary's size
    nd = n if docs == "own" else D
    u = np.unique(r.integers(0, 2**32, 2 * nd + 16, dtype=np.int64))
    table = u[r.permutation(u.size)[:nd]]
    table[0] |= 0x80000000  # the heaviest doc is a real-looking address: u32 >= 2^31
    word = np.minimum(r.zipf(1.3, n) - 1, V - 1)
    return torch.from_numpy(table[doc]), torch.from_numpy(word.astype(np.int32))


def _weights(n):
    w = torch.ones(n, dtype=torch.int32)
    w[::7] = 1000
    return w


def _check(gpu, keys, word, V, weight, n0, form="i64"):
    n = keys.numel()
    k, w = keys.to(gpu), word.to(gpu)
    wt = weight.to(gpu) if weight is not None else None
    ud, ids = oc.dict_encode(k.contiguous(), 32)
    ref = oc.pair_build(ids, w, int(ud.numel()), V, wt, n0=n0)
    if form == "i64":
        dk = k
    else:
        k32 = (k & 0xFFFFFFFF).to(torch.int32)  # u32 bits
        dk = k32 if form == "i32" else (k32[: n // 3].contiguous(), k32[n // 3:].contiguous())
    fu, got = oc.doc_pair_build(dk, w, V, wt, n0=n0)
    assert got.D == ref.D == int(ud.numel()) and got.nnz == ref.nnz and got.V == ref.V
    assert fu.dtype == ud.dtype and torch.equal(fu, ud)
    for f in ("pair_doc", "pair_word", "pair_cnt", "tok_pair"):
        a, b = getattr(ref, f), getattr(got, f)
        assert a.dtype == b.dtype and torch.equal(a, b), f
    if n0 == 0:
        assert got.order0 is None
    else:
        assert got.order0.dtype == ref.order0.dtype and torch.equal(got.order0, ref.order0)
    return fu, got


# n, D, V, docs, weighted, n0 ("half" = n // 2, "all" = n), form of the doc keys
CASES = [
    (1, 1, 1, "zipf", False, 0, "i64"),
    (1, 1, 2, "zipf", False, "all", "i32"),
    (65, 20, 64, "zipf", True, "half", "halves"),
    (65, 20, 1, "zipf", False, "all", "i64"),            # V = 1: zero word bits
    (65, 20, 2, "one", True, 0, "i32"),                  # all tokens in one doc
    (5000, 300, 5740, "own", False, "half", "halves"),   # every token its own doc
    (200_003, 100_000, 70_001, "zipf", False, "all", "i64"),  # D·V > 2^32: the two-call form sorts u64 keys
    (BACK - 1, 60_000, 5740, "zipf", False, "half", "halves"),
    (BACK, 60_000, 5740, "zipf", True, "all", "i64"),
    (BACK, 1, 2, "one", False, 0, "i32"),
    (3_000_001, 370_000, 5740, "zipf", False, "half", "halves"),
]


@pytest.mark.parametrize("n,D,V,docs,weighted,n0,form", CASES)
def test_fused_equals_dict_encode_then_pair_build(gpu, n, D, V, docs, weighted, n0, form):
    keys, word = _tokens(n, D, V, seed=n + V, docs=docs)
    n0 = {"half": n // 2, "all": n}.get(n0, n0)
    _check(gpu, keys, word, V, _weights(n) if weighted else None, n0, form)


def test_fused_equals_torch_unique(gpu):
    n, D, V = 100_001, 3000, 700
    keys, word = _tokens(n, D, V, seed=3)
    assert int((keys >= 2**31).sum()) > 0
    fu, got = _check(gpu, keys, word, V, None, n, "halves")
    u, inv = torch.unique(keys, return_inverse=True)
    pu, pinv = torch.unique(inv * V + word.to(torch.int64), return_inverse=True)
    assert torch.equal(fu.cpu(), u)
    assert torch.equal(got.pair_doc.cpu(), (pu // V).to(torch.int32))
    assert torch.equal(got.pair_word.cpu(), (pu % V).to(torch.int32))
    assert torch.equal(got.tok_pair.cpu(), pinv.to(torch.int32))
    assert torch.equal(got.pair_cnt.cpu(), torch.bincount(pinv, minlength=pu.numel()).to(torch.int32))
    assert torch.equal(got.order0.cpu(), torch.argsort(pinv, stable=True))


def test_second_call_reuses_scratch(gpu):
    """Two calls on one stream, a large then a small one and a large one again: the caching
    allocator hands the first call's scratch out again, stale words, flags and ranks included."""
    a = _tokens(BACK + 5, 50_000, 5740, seed=11)
    b = _tokens(70_001, 900, 3, seed=12)
    _check(gpu, *a, 5740, None, BACK // 2, "halves")
    _check(gpu, *b, 3, _weights(70_001), 70_001, "i64")
    _check(gpu, *a, 5740, _weights(BACK + 5), 0, "i32")


def test_device_ops_refuse_mixed_devices(gpu):
    keys, word = _tokens(65, 20, 64, seed=1)
    with pytest.raises(TypeError):
        oc.doc_pair_build(keys, word.to(gpu), 64)
