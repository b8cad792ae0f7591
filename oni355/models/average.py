"""Posterior averaging: θ and φ from the count sums of the last samples of a chain."""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import ops

# largest global token count a model takes: every int32 count (n_wk, n_k, n_dk, Δ) is ≤ the token
# count, and the Δn_k replicas hold partial sums of it
INT32_COUNT_MAX = 2**31 - 1


def theta_rows(ndk: torch.Tensor, K: int, add: float, den_add: float) -> torch.Tensor:
    """θ[d,k] = (n_dk + add)/(n_d + den_add) over the K real topics, the padding columns zero
    (k_theta_rows on a GPU; its float expression here: CPU and GPU θ agree bit for bit)."""
    if ndk.device.type == "cuda":
        return ops.theta_rows(ndk, K, add, den_add)
    nd = ndk[:, :K].to(torch.int64).sum(1, keepdim=True).to(torch.float32)  # as k_theta_rows
    th = (ndk.to(torch.float32) + add) / (nd + den_add)
    th[:, K:] = 0
    return th.contiguous()


def theta_rows_prior(ndk_sum: torch.Tensor, prior: torch.Tensor, K: int, S: float) -> torch.Tensor:
    """θ[d,k] = (Σn_dk + S·pr_dk)/(Σn_d + S·Σ_k pr_dk) of documents folded in under per-document prior
    rows ``prior`` (f32 [D, KS]) over S window samples, the padding columns zero. Numerator and
    denominator are single f32 fmas (k_theta_rows_prior on a GPU); torch has no fma whose rounding
    is pinned on the CPU, so CPU tensors take the NumPy expression of
    :func:`oni355.ref.foldin_spec.theta_rows_prior`: CPU and GPU θ agree bit for bit."""
    return ops.theta_rows_prior(ndk_sum, prior, K, S)


class PosteriorAverage:
    """The averaging schedule (``at``: the sweep counts at which a sample is added), the sample
    sums ``wk``, ``k``, ``dk`` of n_wk, n_k, n_dk (allocated at the first sample), the number
    ``n`` of samples in them and the cached (θ, φ) of the completed average."""

    def __init__(self, K: int, KS: int, alpha: float, beta: float, vbeta: float, device):
        self.K, self.KS, self.alpha, self.beta, self.vbeta, self.device = K, KS, alpha, beta, vbeta, device
        self.plan(0, 1, 1)

    __getitem__ = object.__getattribute__  # a["wk"], a["n"] = ...: the sums' earlier spelling (a dict)
    __setitem__ = object.__setattr__

    def plan(self, total_sweeps: int, post_samples: int, post_every: int) -> None:
        """Average the counts of the samples at sweeps total, total - e, …, total - (S-1)·e
        (e = post_every, S = post_samples capped at total / 4e)."""
        S, e = max(1, int(post_samples)), max(1, int(post_every))
        # at most the last quarter of the chain (burn-in first): a 200-sweep day averages the 50
        # samples of sweeps 151-200, a 30-sweep run 7, a run of < 8 sweeps none. ONI_POST_SPAN
        # (default 0.25) sets that fraction.
        span = float(os.environ.get("ONI_POST_SPAN", "0.25"))
        S = min(S, int(int(total_sweeps) * span) // e)
        at = [total_sweeps - j * e for j in range(S) if total_sweeps - j * e > 0]
        self.at = sorted(at) if S > 1 else []
        # the sums are allocated at the first sample (ensure), when the counts they bound exist
        self.n = 0
        self.wk = self.k = self.dk = None
        self.cache = None

    def ensure(self, nwk: torch.Tensor, nk: torch.Tensor, ndk: torch.Tensor, T_global: int) -> None:
        """Allocate the sample sums. S samples of an int32 count wrap an int32 sum once the count
        passes 2^31 / S (43M at S = 50: one topic's share of a config-4/5 corpus), so each table is
        int64 when S times its largest possible entry could pass 2^31 -- n_k: the global token
        count; n_wk: the largest global word count; n_dk: the longest document row -- and int32
        otherwise (the default day: half the bytes in k_apply's fused add). ONI_POST_WIDE=1 forces
        int64. ``nwk``, ``nk``, ``ndk``: the current count tables."""
        if not self.at or self.wk is not None:
            return
        S, K, dev = len(self.at), self.K, self.device
        force = os.environ.get("ONI_POST_WIDE", "0") == "1"
        wk_max = int(nwk[:, :K].sum(1, dtype=torch.int64).max()) if nwk.shape[0] else 0
        dk_max = int(ndk[:, :K].sum(1, dtype=torch.int64).max()) if ndk.shape[0] else 0

        def dt(bound: int):
            return torch.int64 if force or bound * S > INT32_COUNT_MAX else torch.int32
        self.wk = torch.zeros(nwk.shape, dtype=dt(wk_max), device=dev)
        self.k = torch.zeros(nk.shape, dtype=dt(max(T_global, int(nk[:K].max()))), device=dev)
        self.dk = torch.zeros(ndk.shape, dtype=dt(dk_max), device=dev)

    def acc(self, ndk_next: torch.Tensor) -> tuple:
        """``acc`` of ops.gibbs_apply: the sums gain n_wk, n_k and the doc rows ``ndk_next`` in its launch."""
        return (self.wk, self.k, self.dk, ndk_next)

    def accumulate(self, nwk: torch.Tensor, nk: torch.Tensor, ndk: torch.Tensor, T_global: int) -> None:
        """Add the current counts to the sample sums: samples taken every post_every > 1 sweeps,
        outside the graphs (contiguous windows add inside k_apply)."""
        self.ensure(nwk, nk, ndk, T_global)
        self.wk += nwk
        self.k += nk
        self.dk += ndk

    def state(self) -> dict | None:
        """The accumulated samples (for a checkpoint; the K real topics only, so the state does
        not depend on the kernel tiling's padding), or None outside an averaging window."""
        if self.n == 0:
            return None
        K = self.K
        return {"n": int(self.n), "wk": self.wk[:, :K].cpu().to(torch.int64), "k": self.k[:K].cpu().to(torch.int64),
                "dk": self.dk[:, :K].cpu().to(torch.int64)}

    def load_state(self, st: dict) -> None:
        """Restore :meth:`state` into the allocated sums (same documents and vocabulary)."""
        K = self.K
        for k in ("wk", "k", "dk"):
            s = getattr(self, k)
            want = (s.shape[0], K) if s.dim() == 2 else (K,)
            v = st[k]
            # states saved before the K-column format hold the KS-wide tiling-padded tables (the
            # padding topics are never used): their first K columns are the same sums
            if tuple(v.shape[:-1]) == want[:-1] and v.shape[-1] == self.KS and self.KS != K:
                v = v[..., :K]
            if tuple(v.shape) != want:
                raise ValueError(f"averaging state {k} shape {tuple(st[k].shape)} != {want}")
            s.zero_()
            s[..., :K].copy_(v.to(s.device))
        self.n = int(st["n"])
        self.cache = None

    def estimate(self, sweeps_done: int):
        """(θ, φ) from the accumulated samples, once every planned sample is in; else None."""
        if self.n == 0 or self.n != len(self.at) or sweeps_done != self.at[-1]:
            return None
        if self.cache is None:
            S, K = float(self.n), self.K
            th = theta_rows(self.dk, K, S * self.alpha, S * K * self.alpha)
            if self.device.type == "cuda":
                ph = ops.phi_rows(self.wk, self.k, K, S * self.beta, float(np.float32(S) * np.float32(self.vbeta)))
            else:
                den = self.k.to(torch.float32) + np.float32(S) * self.vbeta
                ph = (self.wk.to(torch.float32) + S * self.beta) / den
                ph[:, K:] = 0
                ph = ph.contiguous()
            self.cache = (th, ph)
        return self.cache
