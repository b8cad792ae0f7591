"""Variational-EM training on the device: the reference engine's own estimator (lda-c ``lda est``,
smoothed, fixed α and β) as a second, seed-free train method beside the collapsed-Gibbs sampler.

One EM iteration is four ops over the corpus' distinct (doc, word, count) pairs: the E-step
(``ops.vfold``, the kernel ``--infer-method vb`` scores with), the responsibilities
(``ops.vem_resp``), the sufficient statistics (``ops.vem_wsum``, a segmented sum over the
word-major pair list) and the new table (``ops.vem_table``). :mod:`oni355.ref.vem_spec` is the
specification. Nothing is sampled: the same day gives the same model and the same result list,
whatever the seed, and scoring the training day against the saved model with ``method="vb"``,
``iters=var_iters`` and no prior reproduces :meth:`VarLDA.theta`.

Not done here: α estimation (lda-c's Newton step), the ELBO, warm-starting γ between EM iterations.
"""
from __future__ import annotations

import math

import torch

from .. import ops
from ..ref import vem_spec
from ..utils import fault
from ..utils.obs import traced
from .corpus import Corpus
from .gibbs import GibbsConfig, tiling_for

EM_ITERS = 30   # not tuned: docs/vem.md has the likelihood trace
VAR_ITERS = 20  # lda-c's shipped var max iter, as --infer-iters


class VarLDA:
    """The surface the pipelines and ``SavedModel.from_run`` read from ``GibbsLDA``, without topic
    assignments, count tables or Δ buffers: θ, the table and the word-major pair order are all it
    holds."""

    def __init__(self, corpus: Corpus, K: int, alpha: float | None = None, beta: float | None = None, comm=None):
        if (comm is not None and comm.dist) or corpus.split is not None:
            raise NotImplementedError("vem training is single-GPU")
        cfg = GibbsConfig(K=int(K), alpha=alpha, beta=beta)
        self.c, self.K = corpus, int(K)
        self.alpha, self.beta = cfg.resolved_alpha(), cfg.resolved_beta()
        G, KP = tiling_for(self.K, "dense")  # the row width score_* builds a saved model's table with
        self.KS, self.V, self.device = G * KP, int(corpus.V), corpus.pair_word.device
        if self.V < 1:
            raise ValueError("vem training needs at least one word")
        c = corpus
        self._pairs = (c.pair_word.contiguous(), c.pair_cnt.contiguous(), c.doc_pair_ptr.contiguous())
        self._pair_doc = c.pair_doc.contiguous()
        self._wm = ops.vem_word_major(self._pairs[0], self._pair_doc, self.V)
        ss0 = torch.zeros(self.V, self.KS, dtype=torch.float32, device=self.device)
        ss0[:, :self.K] = vem_spec.init_u(self.V, self.K, device=self.device) + 1.0 / self.V
        self.table, self.ss_k = ops.vem_table(ss0, self.K, self.beta)
        self._theta = None
        self.var_iters = VAR_ITERS
        self.sweeps_done = 0  # EM iterations done
        self.likelihoods: list = []

    def _estep(self, want_gamma: bool):
        return ops.vfold(*self._pairs, self.table, self.K, self.alpha, None, self.var_iters, want_gamma=want_gamma)

    @traced("oni:vem.run")
    def run(self, em_iters: int = EM_ITERS, var_iters: int = VAR_ITERS, eval_every: int = 0, log=None) -> "VarLDA":
        """``em_iters`` rounds of E-step, responsibilities, statistics, table, then one final E-step
        against the final table. ``eval_every`` > 0 records the plug-in likelihood of every
        ``eval_every``-th iteration's E-step (θ and the table it ran against)."""
        if em_iters < 0 or var_iters < 0:
            raise ValueError("em_iters and var_iters must be ≥ 0")
        self.var_iters = int(var_iters)
        ptr, wm_doc, wm_word, wm_pos = self._wm
        for it in range(int(em_iters)):
            theta, gamma = self._estep(True)
            if eval_every > 0 and self.sweeps_done % eval_every == 0:
                self._theta = theta
                ll = self.record_likelihood()
                if log:
                    log(f"em iteration {self.sweeps_done} loglik {ll:.6e}")
            e, q = ops.vem_resp(gamma, self.table, self._pair_doc, self._pairs[0], self._pairs[1], self.K, wm_pos)
            ss = ops.vem_wsum(e, q, self.table, ptr, wm_doc, wm_word, self.V, self.K)
            self.table, self.ss_k = ops.vem_table(ss, self.K, self.beta)
            self.sweeps_done += 1
        self._theta = self._estep(False)
        return self

    def theta(self) -> torch.Tensor:
        """θ f32 [D, KS] of the last E-step, zero past K."""
        if self._theta is None:
            self._theta = self._estep(False)
        return self._theta

    def phi(self) -> torch.Tensor:
        """f32 [V, KS]: the table's first V rows."""
        return self.table[: self.V]

    def phi_oov(self) -> torch.Tensor:
        """f32 [K]: the table's row of a word the day never saw, β/(ss_k + Vβ)."""
        return self.table[self.V, : self.K]

    def log_likelihood(self) -> float:
        """The plug-in log-likelihood Σ count · log(θ_d·φ_w) of ops.doc_fit under θ and the table."""
        c = self.c
        fit = ops.doc_fit(self.theta(), self.table, self._pair_doc, self._pairs[0], self._pairs[1], c.D, self.V)
        return float(fit.tot[0])

    def record_likelihood(self) -> float:
        ll = self.log_likelihood()
        if not math.isfinite(ll):
            raise fault.NumericalFault(f"non-finite log-likelihood {ll} after EM iteration {self.sweeps_done}")
        self.likelihoods.append((self.sweeps_done, ll))
        return ll

    def close(self) -> None:
        self._wm = None
