"""NumPy specification oracle of the sorted-table lookup (csrc/kernels/lookup.hip, k_table_lookup).

Fold-in scoring looks every event's key up in a table saved with the model: a word key in the
model's vocabulary (id mode), a proxy user-agent hash in the model's frequency table (value mode).
All quantities are integers, so the kernel equals this bit for bit.
"""
from __future__ import annotations

import numpy as np

I32_MAX = 2**31 - 1


def table_lookup(keys: np.ndarray, queries: np.ndarray, values: np.ndarray | None = None) -> tuple[np.ndarray, int]:
    """(out int32 [n], number of queries absent from ``keys``).

    ``keys`` int64 [M] strictly ascending in signed order, ``queries`` int64 [n].
    Id mode (``values`` None): out[i] = the position of queries[i] in ``keys``, M on a miss.
    Value mode (``values`` int64 [M]): out[i] = int32(min(values[pos], 2^31 − 1)), 0 on a miss."""
    k = np.asarray(keys, dtype=np.int64)
    q = np.asarray(queries, dtype=np.int64)
    M = int(k.shape[0])
    if M > I32_MAX:
        raise ValueError("table_lookup: at most 2^31 - 1 keys")
    if M == 0:
        return np.zeros(q.shape[0], dtype=np.int32), int(q.shape[0])
    pos = np.minimum(np.searchsorted(k, q), M - 1)
    hit = k[pos] == q
    if values is None:
        out = np.where(hit, pos, M)
    else:
        v = np.asarray(values, dtype=np.int64)
        if v.shape[0] != M:
            raise ValueError("table_lookup: one value per key")
        out = np.where(hit, np.minimum(v[pos], I32_MAX), 0)
    return out.astype(np.int32), int(q.shape[0] - int(hit.sum()))


__all__ = ["table_lookup", "I32_MAX"]
