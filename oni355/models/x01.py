"""Packed X01 payload: the sweep's Δ buffer as it travels through the all-reduce."""
from __future__ import annotations

import os

import torch

from .. import ops

# X01 payload packing pays only once the all-reduce is bandwidth-bound (see X01Payload.wanted)
X01_PACK_MIN_BYTES = 4 << 20


class X01Payload:
    """Packed X01 payload (csrc/kernels/x01.hip). A word's per-rank value (an absolute local
    count in recount sweeps, a delta otherwise) is bounded by its local token count c_{w,r}, so
    words with max_r c_{w,r} ≤ O8 = ⌊127 / W⌋ travel as four offset bytes per int32 word, words
    up to O = ⌊32767 / W⌋ as two offset 16-bit halves, and the ring sum stays exact; the rest
    stays int32. A realistic vocabulary is mostly rare words: 13.6 MB → ~3.4 MB per sweep at
    V = 170k, K = 20 (dense → 8-bit)."""

    @staticmethod
    def wanted(dense: torch.Tensor) -> bool:
        """``ONI_X01_PACK``: "1" always packs, "0" never, "auto" (default) packs when the dense Δ
        buffer is at least ``ONI_X01_PACK_MIN_BYTES`` (default 4 MiB). Below that the all-reduce
        is latency-bound (a 0.46 MB flow-day buffer costs about the same as half of it) and the
        pack + unpack kernels would be two extra graph nodes per sweep for nothing."""
        mode = os.environ.get("ONI_X01_PACK", "auto")
        if mode in ("0", "1"):
            return mode == "1"
        min_bytes = int(os.environ.get("ONI_X01_PACK_MIN_BYTES", str(X01_PACK_MIN_BYTES)))
        return dense.numel() * dense.element_size() >= min_bytes

    @classmethod
    def build(cls, dense: torch.Tensor, wsorted: torch.Tensor, V: int, KS: int, comm) -> "X01Payload | None":
        """For the Δ buffer ``dense`` ([V·KS | tail]); None when not wanted or no smaller than it."""
        if KS % 2 or not cls.wanted(dense):
            return None
        W = comm.world
        O = 32767 // W
        O8 = 127 // W
        if os.environ.get("ONI_X01_LIGHT_MAX"):  # tests: force a tiny/light/heavy mix on small days
            O = min(O, int(os.environ["ONI_X01_LIGHT_MAX"]))
        if os.environ.get("ONI_X01_TINY_MAX"):
            O8 = min(O8, int(os.environ["ONI_X01_TINY_MAX"]))
        O8 = min(O8, O)
        dev = dense.device
        cnt = torch.zeros(V, dtype=torch.int64, device=dev)
        if wsorted.numel():  # wsorted is sorted: run lengths by binary search, no contended histogram
            ws = wsorted.to(torch.int64)
            edges = torch.searchsorted(ws, torch.arange(V + 1, dtype=torch.int64, device=dev))
            cnt += edges[1:] - edges[:-1]
        comm.allreduce_(cnt, op="max")
        if KS % 4:
            O8 = -1  # four counts per word need KS % 4 == 0 (always true for choose_tiling)
        x = cls()
        x.tiny = torch.nonzero(cnt <= O8).flatten().to(torch.int32).contiguous()
        x.light = torch.nonzero((cnt > O8) & (cnt <= O)).flatten().to(torch.int32).contiguous()
        x.heavy = torch.nonzero(cnt > O).flatten().to(torch.int32).contiguous()
        x.KS = KS
        x.tail_off, x.tail_len = V * KS, dense.numel() - V * KS
        n = ops.x01_packed_len(x.tiny.numel(), x.light.numel(), x.heavy.numel(), KS, x.tail_len)
        if n >= dense.numel():
            return None
        x.O8, x.O = max(O8, 0), O
        x.WO8, x.WO = W * x.O8, W * O
        x.buf = torch.zeros(n, dtype=torch.int32, device=dev)
        return x

    def __getitem__(self, name: str):
        return getattr(self, name)

    def pack(self, dn: torch.Tensor) -> None:  # buf := this rank's Δ buffer ``dn``, packed
        ops.x01_pack(dn, self.tiny, self.light, self.heavy, self.KS, self.tail_off, self.tail_len, self.O8, self.O,
                     self.buf)

    def unpack(self, out: torch.Tensor) -> None:  # ``out`` := the dense Δ buffer of the summed buf
        ops.x01_unpack(self.buf, self.tiny, self.light, self.heavy, self.KS, self.tail_off, self.tail_len, self.WO8,
                       self.WO, out)
