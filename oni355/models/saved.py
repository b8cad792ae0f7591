"""A trained model kept on disk: what `lda inf` (:mod:`oni355.models.foldin`) scores against.

One ``.npz`` (no pickle) holding the word table φ of a finished training run, the vocabulary it is
indexed by, the row of a never-seen word, the feature cuts the words were made with and a small
provenance record. lda-c's ``final.beta`` + ``final.other`` play this role for the VEM engine.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field

import numpy as np
import torch

FORMAT = 1
_ARRAYS = ("vocab", "phi", "phi_oov", "cuts_time", "cuts_ibyt", "cuts_ipkt")


def oov_row(model) -> np.ndarray:
    """φ of a word with zero count under the estimate ``model.phi()`` returns: β/(n_k + Vβ) from
    the averaged sums with their S-scaling (PosteriorAverage.estimate / k_phi_rows: (0 + S·β)/(Σn_k + S·Vβ))
    once the window is complete, else from the current n_k (the q table's expression). f32 [K]."""
    K = model.K
    f32 = np.float32
    if model._averaged() is not None:
        a = model._avg
        S = float(a.n)
        num = f32(0) + f32(S * model.beta)
        den = a.k[:K].cpu().numpy().astype(f32) + f32(f32(S) * f32(model.vbeta))
    else:
        num = f32(0) + f32(model.beta)
        den = model.nk_cur[:K].cpu().numpy().astype(f32) + f32(model.vbeta)
    return (num / den).astype(f32)


@dataclass
class SavedModel:
    source: str
    K: int
    alpha: float
    beta: float
    vocab: np.ndarray      # int64 [V] sorted word keys (row i of phi)
    phi: np.ndarray        # f32 [V, K]
    phi_oov: np.ndarray    # f32 [K] row of a word the model never saw
    cuts: dict             # feature cuts as raw key arrays (flow: time / ibyt / ipkt, uint32)
    provenance: dict = field(default_factory=dict)

    @property
    def V(self) -> int:
        return int(self.vocab.shape[0])

    def __post_init__(self):
        self.vocab = np.ascontiguousarray(self.vocab, dtype=np.int64)
        self.phi = np.ascontiguousarray(self.phi, dtype=np.float32)
        self.phi_oov = np.ascontiguousarray(self.phi_oov, dtype=np.float32)
        self.cuts = {k: np.ascontiguousarray(v, dtype=np.uint32) for k, v in self.cuts.items()}
        if self.phi.shape != (self.V, self.K) or self.phi_oov.shape != (self.K,):
            raise ValueError(f"phi must be [V={self.V}, K={self.K}] and phi_oov [K]")
        if self.V > 1 and not bool((self.vocab[1:] > self.vocab[:-1]).all()):
            raise ValueError("vocab must be strictly ascending word keys")

    @classmethod
    def from_run(cls, run, cuts, source: str, cfg: dict | None = None) -> "SavedModel":
        """The model of a finished training run (``run``: pipeline.common.LdaRun; ``cuts``: the
        day's FlowCuts; ``cfg``: provenance such as the training day)."""
        from ..utils import provenance as prov
        m = run.model
        if run.route is not None or run.extra_models:
            raise NotImplementedError("models are saved from single-GPU, single-chain runs")
        K = m.K
        prv = {"sweeps": int(m.sweeps_done), "seed": int(m.cfg.seed), "tree_hash": prov.tree_hash("hip"),
               "averaged": m._averaged() is not None}
        prv.update(cfg or {})
        return cls(source=source, K=K, alpha=float(m.alpha), beta=float(m.beta),
                   vocab=run.vocab.cpu().numpy(), phi=m.phi()[:, :K].cpu().numpy(), phi_oov=oov_row(m),
                   cuts={"time": cuts.time, "ibyt": cuts.ibyt, "ipkt": cuts.ipkt}, provenance=prv)

    def save(self, path: str) -> str:
        meta = {"format": FORMAT, "source": self.source, "K": int(self.K), "alpha": float(self.alpha),
                "beta": float(self.beta), "provenance": self.provenance}
        if not path.endswith(".npz"):
            path += ".npz"
        with open(path, "wb") as f:
            np.savez(f, meta=np.array([json.dumps(meta, sort_keys=True)]), vocab=self.vocab, phi=self.phi,
                     phi_oov=self.phi_oov, **{f"cuts_{k}": v for k, v in self.cuts.items()})
        return path

    @classmethod
    def load(cls, path: str) -> "SavedModel":
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("meta", *_ARRAYS) if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a saved oni355 model (missing {missing})")
            meta = json.loads(str(z["meta"][0]))
            if meta.get("format") != FORMAT:
                raise ValueError(f"{path}: model format {meta.get('format')} (this build reads {FORMAT})")
            arr = {k: z[k] for k in _ARRAYS}
        return cls(source=meta["source"], K=int(meta["K"]), alpha=float(meta["alpha"]), beta=float(meta["beta"]),
                   vocab=arr["vocab"], phi=arr["phi"], phi_oov=arr["phi_oov"],
                   cuts={k[5:]: arr[k] for k in _ARRAYS if k.startswith("cuts_")}, provenance=meta.get("provenance", {}))

    def table(self, G: int, KP: int, device) -> torch.Tensor:
        """The sampler / score table: f32 [V + 1, G·KP], columns ≥ K zero, row V = ``phi_oov``."""
        KS = G * KP
        if KS < self.K:
            raise ValueError("G*KP must cover the model's K topics")
        t = np.zeros((self.V + 1, KS), dtype=np.float32)
        t[: self.V, : self.K] = self.phi
        t[self.V, : self.K] = self.phi_oov
        return torch.from_numpy(t).to(device)
