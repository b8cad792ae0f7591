"""k_table_lookup (csrc/kernels/lookup.hip) against its oracle (oni355/ref/lookup_spec.py), bit for
bit in id mode and value mode, miss counter included.

Table sizes 0, 1, 2, 255 and 4097 (the last one past the 2048 samples of the coarse LDS level:
sampling stride 3, a short last run) and one of 150k keys (stride 74, one block's LDS level full);
query counts 0, 1, 63, 64, 65 and 1000 (below, at and past a wave, several blocks with a ragged last
one). Keys are negative and positive int64; the queries mix hits, repeated hits, the values just
beside a key, values below the first and above the last key and the int64 extremes; all-hit and
all-miss batches; values above 2^31 − 1 clamp, negative values pass through their low 32 bits.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.ref import lookup_spec

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
M_SIZES = [0, 1, 2, 255, 4097]
N_SIZES = [0, 1, 63, 64, 65, 1000]


def _table(M: int):
    r = np.random.default_rng(1000 + M)
    # signed order, both signs, gaps of at least 3 (key ± 1 is never a key), the extremes included
    keys = np.sort(r.choice(np.arange(-3 * M, 3 * M + 3, 3, dtype=np.int64), M, replace=False)) * 1_000_003
    if M >= 2:
        keys[0], keys[-1] = I64.min + 1, I64.max - 1
    values = r.integers(0, 5000, M).astype(np.int64)
    values[r.random(M) < 0.2] += 2**31 - 2500  # around and above the clamp
    if M:
        values[M // 2] = 2**40
        values[0] = -7
    return keys, values


def _queries(keys: np.ndarray, n: int, kind: str):
    r = np.random.default_rng(n * 31 + keys.size)
    M = keys.size
    if kind == "hit" and M:
        return keys[r.integers(0, M, n)]
    if kind == "miss" or M == 0:
        q = r.integers(-2**40, 2**40, n) * 3 + 1
        return q[~np.isin(q, keys)] if M else q
    q = keys[r.integers(0, M, n)].copy()           # hits, many of them repeated
    near = r.random(n)
    q[near < 0.15] += 1                             # just above a key
    q[(near >= 0.15) & (near < 0.3)] -= 1           # just below a key
    edge = np.array([I64.min, I64.max, keys[0] - 1, keys[-1] + 1, keys[0], keys[-1], 0], dtype=np.int64)
    k = min(n, edge.size)
    q[r.choice(n, k, replace=False)] = edge[:k]
    if n > 8:
        q[-4:] = q[0]                               # one query repeated inside a wave and across blocks
    return q


def _check(gpu, keys, values, q):
    dk, dv, dq = (torch.from_numpy(np.ascontiguousarray(x)).to(gpu) for x in (keys, values, q))
    for vals, dvals in ((None, None), (values, dv)):
        want, miss = lookup_spec.table_lookup(keys, q, vals)
        got, cnt = ops.table_lookup(dk, dq, dvals)
        assert got.dtype == torch.int32 and got.shape == (q.size,) and cnt.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), want)
        assert int(cnt.item()) == miss
    return want, miss


@pytest.mark.parametrize("n", N_SIZES)
@pytest.mark.parametrize("M", M_SIZES)
def test_lookup_equals_its_oracle(gpu, M, n):
    keys, values = _table(M)
    q = _queries(keys, n, "mixed")
    _, miss = _check(gpu, keys, values, q)
    if M and n >= 64:
        assert 0 < miss < q.size  # the batch holds hits and misses


@pytest.mark.parametrize("M", [1, 255, 4097])
def test_all_hit_and_all_miss(gpu, M):
    keys, values = _table(M)
    want, miss = _check(gpu, keys, values, _queries(keys, 1000, "hit"))
    assert miss == 0
    q = _queries(keys, 1000, "miss")
    want, miss = _check(gpu, keys, values, q)
    assert miss == q.size > 900 and not want.any()
    # every key once, in order: id mode is the identity, value mode the clamped column
    ids, _ = ops.table_lookup(torch.from_numpy(keys).to(gpu), torch.from_numpy(keys).to(gpu))
    assert np.array_equal(ids.cpu().numpy(), np.arange(M, dtype=np.int32))
    got, _ = ops.table_lookup(torch.from_numpy(keys).to(gpu), torch.from_numpy(keys).to(gpu),
                              torch.from_numpy(values).to(gpu))
    assert np.array_equal(got.cpu().numpy(), np.minimum(values, 2**31 - 1).astype(np.int32))
    assert int(got[0]) == -7 and (M < 2 or int(got.max()) == 2**31 - 1)


def test_a_table_past_one_block_of_samples_per_stride(gpu):
    """150k keys, as a large flow vocabulary: stride 74, the LDS level full, 7 steps in memory."""
    r = np.random.default_rng(9)
    keys = np.unique(r.integers(-2**45, 2**45, 150_500))[:150_000]
    values = r.integers(0, 2**33, keys.size)
    q = np.concatenate([keys[r.integers(0, keys.size, 3000)], r.integers(-2**45, 2**45, 1000), keys[::74][:500],
                        keys[73::74][:500], keys[-3:]])
    _, miss = _check(gpu, keys, values, q)
    assert 900 < miss <= 1000


def test_the_counter_accumulates_and_arguments_are_checked(gpu):
    keys, values = _table(255)
    dk = torch.from_numpy(keys).to(gpu)
    q1, q2 = _queries(keys, 1000, "mixed"), _queries(keys, 65, "miss")
    cnt = torch.zeros(1, dtype=torch.int64, device=gpu)
    ops.table_lookup(dk, torch.from_numpy(q1).to(gpu), misses=cnt)
    _, same = ops.table_lookup(dk, torch.from_numpy(q2).to(gpu), misses=cnt)
    assert same is cnt
    assert int(cnt.item()) == lookup_spec.table_lookup(keys, q1)[1] + q2.size
    with pytest.raises(TypeError):
        ops.table_lookup(dk.to(torch.int32), torch.from_numpy(q1).to(gpu))
    with pytest.raises(ValueError):
        ops.table_lookup(dk, torch.from_numpy(q1).to(gpu), torch.from_numpy(values[:-1]).to(gpu))
    with pytest.raises(ValueError):
        ops.table_lookup(dk, torch.from_numpy(q1))
