"""Batch CVB0 training on the device: collapsed variational Bayes, zeroth order (Asuncion et al.
2009), the deterministic mean-field counterpart of the collapsed Gibbs sampler, as a third train
method. Like vem it has no seed; unlike vem an iteration holds no digamma, no exp and no inner
loop.

The state is a responsibility row per distinct (doc, word) pair, r f32 [P, KS], and the expected
counts it sums to. One iteration is two ops: ``ops.cvb0_update`` (every row from the OLD counts with
the pair's own share taken out, in place, and the new document counts in the same pass) and the
word counts, the segmented sum over the word-major pair list ``ops.vem_wsum`` already is (r as the
"documents", the counts as q, a table of ones); ``ops.vem_table`` gives n_k and, at the end, the
table a saved model carries. :mod:`oni355.ref.cvb0_spec` is the specification.

θ comes from the counts, (n_dk + α)/(N_d + Kα), not from a fold-in: scoring the training day against
the saved model is close to θ, not bitwise θ.

Not done here: a convergence exit, α estimation, more than one GPU, checkpoints.
"""
from __future__ import annotations

import math

import torch

from .. import ops
from ..utils import fault
from ..utils.obs import traced
from .corpus import Corpus
from .gibbs import GibbsConfig, tiling_for

CVB_ITERS = 100  # not tuned: docs/cvb0.md has the likelihood trace


class CvbLDA:
    """The surface the pipelines and ``SavedModel.from_run`` read from ``VarLDA``."""

    train_method = "cvb0"

    def __init__(self, corpus: Corpus, K: int, alpha: float | None = None, beta: float | None = None, comm=None):
        if (comm is not None and comm.dist) or corpus.split is not None:
            raise NotImplementedError("cvb0 training is single-GPU")
        cfg = GibbsConfig(K=int(K), alpha=alpha, beta=beta)
        self.c, self.K = corpus, int(K)
        self.alpha, self.beta = cfg.resolved_alpha(), cfg.resolved_beta()
        G, KP = tiling_for(self.K, "dense")  # the row width score_* builds a saved model's table with
        self.KS, self.V, self.device = G * KP, int(corpus.V), corpus.pair_word.device
        if self.V < 1:
            raise ValueError("cvb0 training needs at least one word")
        c = corpus
        self._pairs = (c.pair_doc.contiguous(), c.pair_word.contiguous(), c.pair_cnt.contiguous())
        self._ptr = c.doc_pair_ptr.contiguous()
        self._doc_len = c.doc_lengths().contiguous()
        self._wm = ops.cvb0_word_major(self._pairs[1], self._pairs[2], self.V)
        self._ones = torch.ones(self.V + 1, self.KS, dtype=torch.float32, device=self.device)
        self._r = ops.cvb0_init(self._pairs[1], self.V, self.K, self.KS)
        # the first document counts: an update's own sum needs the word counts first, so this one
        # sum goes through the same segmented-sum op, keyed by document (its own table of ones, dropped after)
        D = int(c.D)
        ident = torch.arange(self._r.shape[0], dtype=torch.int32, device=self.device)
        self.n_dk = ops.vem_wsum(self._r, self._pairs[2].to(torch.float32),
                                 torch.ones(D + 1, self.KS, dtype=torch.float32, device=self.device), self._ptr, ident,
                                 self._pairs[0], D, self.K) if D else self._r.new_zeros(0, self.KS)
        self._recount_words()
        self._theta = None
        self.sweeps_done = 0  # iterations done
        self.likelihoods: list = []

    def _recount_words(self) -> None:
        """n_wk, n_k and the table from the current r."""
        ptr, wm_src, wm_word, wm_cnt = self._wm
        self.n_wk = ops.vem_wsum(self._r, wm_cnt, self._ones, ptr, wm_src, wm_word, self.V, self.K)
        self.table, self.n_k = ops.vem_table(self.n_wk, self.K, self.beta)

    @traced("oni:cvb0.run")
    def run(self, iters: int = CVB_ITERS, eval_every: int = 0, log=None) -> "CvbLDA":
        """``iters`` Jacobi steps. ``eval_every`` > 0 records the plug-in likelihood of the state
        every ``eval_every``-th step starts from."""
        if iters < 0:
            raise ValueError("iters must be ≥ 0")
        for _ in range(int(iters)):
            if eval_every > 0 and self.sweeps_done % eval_every == 0:
                ll = self.record_likelihood()
                if log:
                    log(f"cvb0 iteration {self.sweeps_done} loglik {ll:.6e}")
            self.n_dk = ops.cvb0_update(self._r, self.n_dk, self.n_wk, self.n_k, *self._pairs, self._ptr, self.K,
                                        self.alpha, self.beta, self.V)
            self._recount_words()
            self._theta = None
            self.sweeps_done += 1
        return self

    def theta(self) -> torch.Tensor:
        """θ f32 [D, KS] of the current counts, zero past K."""
        if self._theta is None:
            self._theta = ops.cvb0_theta(self.n_dk, self._doc_len, self.K, self.alpha)
        return self._theta

    def phi(self) -> torch.Tensor:
        """f32 [V, KS]: the table's first V rows."""
        return self.table[: self.V]

    def phi_oov(self) -> torch.Tensor:
        """f32 [K]: the table's row of a word the day never saw, β/(n_k + Vβ)."""
        return self.table[self.V, : self.K]

    def log_likelihood(self) -> float:
        """The plug-in log-likelihood Σ count · log(θ_d·φ_w) of ops.doc_fit under θ and the table."""
        fit = ops.doc_fit(self.theta(), self.table, *self._pairs, self.c.D, self.V)
        return float(fit.tot[0])

    def record_likelihood(self) -> float:
        ll = self.log_likelihood()
        if not math.isfinite(ll):
            raise fault.NumericalFault(f"non-finite log-likelihood {ll} after cvb0 iteration {self.sweeps_done}")
        self.likelihoods.append((self.sweeps_done, ll))
        return ll

    def close(self) -> None:
        self._wm = self._r = self._ones = None
