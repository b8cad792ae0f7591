"""Variational-EM training on the device: the reference engine's own estimator (lda-c ``lda est``,
smoothed, fixed β) as a second, seed-free train method beside the collapsed-Gibbs sampler.

One EM iteration is four ops over the corpus' distinct (doc, word, count) pairs: the E-step
(``ops.vfold``, the kernel ``--infer-method vb`` scores with), the responsibilities
(``ops.vem_resp``), the sufficient statistics (``ops.vem_wsum``, a segmented sum over the
word-major pair list) and the new table (``ops.vem_table``). :mod:`oni355.ref.vem_spec` is the
specification. Nothing is sampled: the same day gives the same model and the same result list,
whatever the seed, and scoring the training day against the saved model with ``method="vb"``,
``iters=var_iters`` and no prior reproduces :meth:`VarLDA.theta`.

Two options, both off by default, add a fifth op after the E-step, ``ops.vem_bound`` (the
variational bound lda-c writes to likelihood.dat, and the α sufficient statistic), and read its two
totals back: ``em_tol`` stops EM on the bound's relative change, ``estimate_alpha`` re-estimates
the symmetric α by lda-c's Newton step after every table update.

Two more, also off by default, move the E-step to ``ops.vfold_exit``: ``var_tol`` > 0 stops a
document's E-step once Σ|γ_new − γ_old| ≤ var_tol · Σγ (lda-c's ``var converged``, as a γ-change
rule, not lda-c's likelihood-change rule), ``warm_start`` starts every EM iteration's E-step from the
previous iteration's γ. The final E-step (θ's) always starts cold, so scoring the training day with
``tol=var_tol`` still reproduces θ.

Not done here: vector α.
"""
from __future__ import annotations

import math

import numpy as np
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
        self._gamma = None  # γ of the E-step θ came from, kept when the bound is tracked
        self.var_iters = VAR_ITERS
        self.sweeps_done = 0  # EM iterations done
        self.likelihoods: list = []
        self.bounds: list = []  # (iteration, bound, conv, α the E-step ran with), one per tracked iteration
        self.em_tol, self.estimate_alpha, self.converged = 0.0, False, False
        self.var_tol, self.warm_start = 0.0, False
        self.var_iters_trace: list = []  # mean E-step updates per document, one per EM iteration of the exit path
        self._nit_sums: list = []        # the same as device scalars (Σ n_it), read back once per run

    def _estep(self, want_gamma: bool, gamma0=None):
        """(θ, γ) with ``want_gamma`` else θ. With ``var_tol`` and ``warm_start`` off this is ops.vfold,
        as it always was; otherwise ops.vfold_exit from ``gamma0`` (None: the cold start)."""
        if not (self.var_tol > 0 or self.warm_start):
            return ops.vfold(*self._pairs, self.table, self.K, self.alpha, None, self.var_iters, want_gamma=want_gamma)
        theta, gamma, n_it = ops.vfold_exit(*self._pairs, self.table, self.K, self.alpha, None, self.var_iters,
                                            self.var_tol, gamma0)
        self._nit_sums.append(n_it.sum())
        return (theta, gamma) if want_gamma else theta

    def _bound(self, gamma: torch.Tensor) -> tuple[float, float]:
        """(bound, α statistic) of an E-step's γ against the table and α it ran with: one launch
        sequence and one 16-byte read."""
        b = ops.vem_bound(gamma, self.table, self._pair_doc, self._pairs[0], self._pairs[1], self.K, self.alpha,
                          self._pairs[2])
        L, a_ss = b.tot.tolist()
        if not math.isfinite(L):
            raise fault.NumericalFault(f"non-finite variational bound {L} after EM iteration {self.sweeps_done}")
        return L, a_ss

    @traced("oni:vem.run")
    def run(self, em_iters: int = EM_ITERS, var_iters: int = VAR_ITERS, eval_every: int = 0, log=None,
            em_tol: float = 0.0, estimate_alpha: bool = False, var_tol: float = 0.0,
            warm_start: bool = False) -> "VarLDA":
        """``em_iters`` rounds of E-step, responsibilities, statistics, table, then one final E-step
        against the final table. ``eval_every`` > 0 records the plug-in likelihood of every
        ``eval_every``-th iteration's E-step (θ and the table it ran against).

        With ``em_tol`` > 0 or ``estimate_alpha`` every E-step is followed by ``ops.vem_bound`` and
        ``self.bounds`` gets (iteration, L, conv, α) with conv = (L_old − L)/L_old (1.0 for the
        first). ``estimate_alpha``: after the table update α ← ``vem_spec.alpha_newton``, rounded
        to float32 (what the E-step kernel and a saved model carry). ``em_tol`` > 0: ``em_iters``
        is the maximum; EM stops after the M-step of an iteration that is at least the third of
        this call and has 0 ≤ conv ≤ em_tol (lda-c's loop, without its doubling of the E-step
        iterations on a negative conv). With both off nothing of this runs.

        ``var_tol`` > 0 or ``warm_start``: the E-steps run ``ops.vfold_exit(max_iters=var_iters,
        tol=var_tol)``, inside the EM loop from the previous iteration's γ when ``warm_start`` (the
        first from the cold start); the final E-step always starts cold. ``var_iters_trace`` gets the
        mean number of updates per document of every EM iteration's E-step, read back once at the end."""
        if em_iters < 0 or var_iters < 0:
            raise ValueError("em_iters and var_iters must be ≥ 0")
        if not em_tol >= 0:
            raise ValueError("em_tol must be ≥ 0")
        if not (var_tol >= 0 and math.isfinite(var_tol)):
            raise ValueError("var_tol must be finite and ≥ 0")
        self.var_tol, self.warm_start = float(var_tol), bool(warm_start)
        self._nit_sums, prev = [], None
        self.var_iters = int(var_iters)
        self.em_tol, self.estimate_alpha, self.converged = float(em_tol), bool(estimate_alpha), False
        track = self.em_tol > 0 or self.estimate_alpha
        ptr, wm_doc, wm_word, wm_pos = self._wm
        L_old = 0.0
        for it in range(int(em_iters)):
            theta, gamma = self._estep(True, prev)
            if self.warm_start:
                prev = gamma
            if eval_every > 0 and self.sweeps_done % eval_every == 0:
                self._theta = theta
                ll = self.record_likelihood()
                if log:
                    log(f"em iteration {self.sweeps_done} loglik {ll:.6e}")
            conv = 1.0
            if track:
                L, a_ss = self._bound(gamma)
                conv = 1.0 if L_old == 0 else (L_old - L) / L_old
                L_old = L
                self.bounds.append((self.sweeps_done, L, conv, self.alpha))
                if log:
                    log(f"em iteration {self.sweeps_done} bound {L:.10e} conv {conv:.3e} alpha {self.alpha:.6g}")
            e, q = ops.vem_resp(gamma, self.table, self._pair_doc, self._pairs[0], self._pairs[1], self.K, wm_pos)
            ss = ops.vem_wsum(e, q, self.table, ptr, wm_doc, wm_word, self.V, self.K)
            self.table, self.ss_k = ops.vem_table(ss, self.K, self.beta)
            if self.estimate_alpha:
                self.alpha = float(np.float32(vem_spec.alpha_newton(a_ss, int(gamma.shape[0]), self.K)))
            self.sweeps_done += 1
            if self.em_tol > 0 and it + 1 >= 3 and 0 <= conv <= self.em_tol:
                self.converged = True
                break
        if track:
            self._theta, self._gamma = self._estep(True)
        else:
            self._theta, self._gamma = self._estep(False), None
        if self._nit_sums:  # the EM loop's E-steps, not the final one: one read for all of them
            sums = torch.stack(self._nit_sums[:-1]).tolist() if len(self._nit_sums) > 1 else []
            self.var_iters_trace += [s / max(1, int(self.c.D)) for s in sums]
            self._nit_sums = []
        return self

    def theta(self) -> torch.Tensor:
        """θ f32 [D, KS] of the last E-step, zero past K."""
        if self._theta is None:
            self._theta = self._estep(False)
        return self._theta

    def bound(self) -> float:
        """The variational bound of the final E-step (θ's) against the final table and α."""
        if self._gamma is None:
            self._theta, self._gamma = self._estep(True)
        return self._bound(self._gamma)[0]

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
