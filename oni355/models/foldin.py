"""Fold-in inference: θ of new documents against a saved model's frozen word table (`lda inf`).

The Gibbs counterpart of lda-c's ``lda inf``: the documents' topics are sampled
from (n_dk^¬t + α)·φ_wk with φ fixed, so nothing couples two documents -- no n_wk, no Δ buffers,
no posterior word sums, no all-reduce. Every chunk of a single-chunk document runs all its sweeps
in one launch (k_foldin keeps the counts in registers); documents over several chunks are swept
one sweep per launch with their rows ping-ponged between two buffers, as in training.
θ is the average of the rows over the last ``avg_last`` sweeps (the posterior-average estimate the
training side uses, :meth:`oni355.models.gibbs.GibbsLDA.plan_average`).
"""
from __future__ import annotations

import torch

from .. import ops
from ..ref import foldin_spec
from ..utils.obs import traced
from .average import theta_rows, theta_rows_prior
from .corpus import Corpus


class FoldIn:
    """Device (or CPU-oracle) state of one fold-in run over ``corpus`` (word ids index ``table``:
    f32 [V + 1, KS] from :meth:`oni355.models.saved.SavedModel.table`, row V = unseen words).
    ``fuse=False`` launches every sweep on its own (the A/B of bench/foldin.py; same draws).
    ``prior``: f32 [D, KS] per-document Dirichlet rows (ops.prior_rows) that take α's place on the
    doc side of the draws and of θ; None is the flat prior α."""

    def __init__(self, corpus: Corpus, table: torch.Tensor, K: int, alpha: float, seed: int = 0x0D15EA5E,
                 fuse: bool = True, prior: torch.Tensor | None = None):
        c = corpus
        if table.dim() != 2 or table.dtype != torch.float32 or table.shape[0] != c.V:
            raise ValueError(f"the word table must be f32 [{c.V}, KS] (one row per corpus word id)")
        if table.shape[1] % c.G or table.shape[1] < K or (table.shape[1] // c.G) % 4:
            raise ValueError("the table's row width must be G*KP ≥ K with KP a multiple of 4")
        if table.device != c.tok_word.device:
            raise ValueError("corpus and word table live on different devices")
        if c.split is not None:
            raise NotImplementedError("fold-in scoring is single-GPU")
        self.c, self.table = c, table.contiguous()
        self.K, self.alpha, self.seed, self.fuse = int(K), float(alpha), int(seed), bool(fuse)
        self.G, self.KS = c.G, int(table.shape[1])
        self.KP = self.KS // self.G
        dev = self.device = c.tok_word.device
        if prior is not None:
            if prior.dtype != torch.float32 or tuple(prior.shape) != (max(c.D, 1), self.KS) or prior.device != dev:
                raise ValueError(f"the prior must be f32 [{max(c.D, 1)}, {self.KS}] on the corpus' device")
            prior = prior.contiguous()
        self.prior = prior
        self.tok_z = torch.zeros(c.sell_slots, dtype=torch.uint8, device=dev)
        self.ndk = torch.zeros(max(c.D, 1), self.KS, dtype=torch.int32, device=dev)
        self.ndk_sum = torch.zeros_like(self.ndk)
        # rows of the multi-chunk documents ping-pong between ndk and a second buffer
        self._alt = torch.zeros_like(self.ndk) if c.long_rows.numel() else None
        self.samples = 0
        self.sweeps_done = 0
        self.launches = {"init": 0, "sweep": 0, "multi_sweep": 0}

    def _state(self, src: torch.Tensor, dst: torch.Tensor) -> dict:
        st = dict(self.c.sell_state(self.tok_z), ndk_src=src, ndk_dst=dst, ndk_sum=self.ndk_sum, phi=self.table)
        if self.prior is not None:
            st["prior"] = self.prior
        return st

    def _pass(self, st: dict, init: bool, sweep_lo: int, n_sweeps: int, avg_from: int, select: int) -> None:
        ops.foldin_pass(st, self.G, self.KP, self.K, self.alpha, self.seed, init, sweep_lo, n_sweeps, avg_from,
                        self.c.chunk_len, select=select)

    @traced("oni:foldin.run")
    def run(self, sweeps: int = 30, avg_last: int = 10) -> "FoldIn":
        """Init pass + ``sweeps`` sweeps; ``ndk_sum`` := Σ of the rows after the last ``avg_last``."""
        c = self.c
        self.ndk.zero_()
        self.ndk_sum.zero_()
        self.launches = {"init": 0, "sweep": 0, "multi_sweep": 0}
        avg_from, self.samples = foldin_spec.window(sweeps, avg_last)
        if c.n_slices == 0:
            return self
        self._pass(self._state(self.ndk, self.ndk), True, 0, 1, 0, foldin_spec.SELECT_ALL)
        self.launches["init"] += 1
        if sweeps <= 0:
            self.ndk_sum.copy_(self.ndk)
            return self
        # single-chunk documents: every sweep in one launch, rows in place
        st = self._state(self.ndk, self.ndk)
        if self.fuse:
            self._pass(st, False, 1, sweeps, avg_from, foldin_spec.SELECT_SINGLE)
            self.launches["sweep"] += 1
        else:
            for s in range(1, sweeps + 1):
                self._pass(st, False, s, 1, avg_from, foldin_spec.SELECT_SINGLE)
                self.launches["sweep"] += 1
        # multi-chunk documents: the chunks' Δ meet between sweeps
        if self._alt is not None:
            lr = c.long_rows
            lrl = lr.long()
            cur, oth = self.ndk, self._alt
            for s in range(1, sweeps + 1):
                ops.copy_rows(cur, oth, lr, self.KS)
                self._pass(self._state(cur, oth), False, s, 1, avg_from, foldin_spec.SELECT_MULTI)
                self.launches["multi_sweep"] += 1
                cur, oth = oth, cur
                if s >= avg_from:
                    self.ndk_sum[lrl] += cur[lrl]
            if cur is not self.ndk:
                ops.copy_rows(cur, self.ndk, lr, self.KS)
        self.sweeps_done = sweeps
        return self

    def theta(self) -> torch.Tensor:
        """θ = (Σn_dk + S·α)/(Σn_d + S·K·α) over the S window samples, KS-padded with zeros; with a
        prior, (Σn_dk + S·pr_dk)/(Σn_d + S·Σ_k pr_dk)."""
        S, K = float(max(self.samples, 1)), self.K
        if self.prior is not None:
            return theta_rows_prior(self.ndk_sum, self.prior, K, S)
        return theta_rows(self.ndk_sum, K, S * self.alpha, S * K * self.alpha)

    def phi(self) -> torch.Tensor:
        return self.table
