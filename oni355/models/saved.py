"""A trained model kept on disk: what `lda inf` (:mod:`oni355.models.foldin`) scores against.

One ``.npz`` (no pickle) holding the word table φ of a finished training run, the vocabulary it is
indexed by, the row of a never-seen word, the feature cuts the words were made with and a small
provenance record. lda-c's ``final.beta`` + ``final.other`` play this role for the VEM engine.
Optionally it also keeps the training day's document profiles (``doc_keys``, ``doc_theta``,
``doc_tokens``; lda-c's ``final.gamma``), which fold-in can use as per-IP topic priors.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field, replace

import numpy as np
import torch

from ..ref.foldin_spec import V6_KEY_BASE  # keys from here up are per-day IPv6 ids: never saved

FORMAT = 1
_BASE_ARRAYS = ("vocab", "phi", "phi_oov")
# the cut lists every source's words are made with (the BINNED names of pipeline/dns.py, proxy.py)
CUT_NAMES = {"flow": ("time", "ibyt", "ipkt"),
             "dns": ("frame_len", "time", "sub_len", "sub_ent", "periods"),
             "proxy": ("time", "ua_freq", "uri_ent", "uri_len")}
# a proxy model's user-agent frequency table (pipeline.proxy.featurize): both or none elsewhere
_UA_ARRAYS = ("ua_keys", "ua_counts")
# the optional document profiles: all three or none. An older build's loader ignores them.
_DOC_ARRAYS = ("doc_keys", "doc_theta", "doc_tokens")


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


def _cut_array(name: str, v) -> np.ndarray:
    """One cut list as saved: the integer values ``common.binned_cuts`` / ``FlowCuts`` return, kept
    exactly. They are u32 order keys (of f32 features) or raw counts: uint32 where every value fits
    (every cut of this code base does; flow cuts therefore stay uint32), else int64."""
    a = np.asarray(v)
    if a.dtype.kind not in "iu":
        raise ValueError(f"cuts[{name!r}] must be integers (raw order keys), got {a.dtype}")
    a = a.reshape(-1)
    if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
        return np.ascontiguousarray(a, dtype=np.int64)
    return np.ascontiguousarray(a, dtype=np.uint32)


def model_source(path: str) -> str:
    """The source (``flow``, ``dns``, ``proxy``) a saved model file was trained on; reads only the
    file's meta record."""
    with np.load(path, allow_pickle=False) as z:
        if "meta" not in z.files:
            raise ValueError("not a saved oni355 model (missing ['meta'])")
        return str(json.loads(str(z["meta"][0])).get("source"))


def _host(t) -> np.ndarray:
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def top_digest(domains) -> tuple[int, str]:
    """(entries, digest) of a top-domain list as :func:`oni355.pipeline.dns.top_set` reads it
    (stripped, lower case, empty lines dropped, order kept); (0, "") without a list."""
    import hashlib
    names = [d.strip().lower() for d in (domains or []) if d.strip()]
    if not names:
        return 0, ""
    return len(names), hashlib.sha256("\n".join(names).encode()).hexdigest()[:16]


@dataclass
class SavedModel:
    source: str
    K: int
    alpha: float
    beta: float
    vocab: np.ndarray      # int64 [V] sorted word keys (row i of phi)
    phi: np.ndarray        # f32 [V, K]
    phi_oov: np.ndarray    # f32 [K] row of a word the model never saw
    cuts: dict             # feature cuts as raw key arrays, by name (:data:`CUT_NAMES` of the source)
    provenance: dict = field(default_factory=dict)
    # the training day's document profiles (all three or none)
    doc_keys: np.ndarray | None = None     # int64 [Dm] strictly ascending document (IP) keys
    doc_theta: np.ndarray | None = None    # f32 [Dm, K] θ of each document at the end of training
    doc_tokens: np.ndarray | None = None   # int64 [Dm] training tokens of each document
    # a proxy model's user-agent frequency table of the training day (both; no other source has one)
    ua_keys: np.ndarray | None = None      # int64 [U] strictly ascending (signed) user-agent hashes
    ua_counts: np.ndarray | None = None    # int64 [U] events of the training day with that user agent

    @property
    def V(self) -> int:
        return int(self.vocab.shape[0])

    @property
    def has_docs(self) -> bool:
        return self.doc_keys is not None

    def without_docs(self) -> "SavedModel":
        """The same model without its document profiles."""
        return replace(self, doc_keys=None, doc_theta=None, doc_tokens=None)

    def __post_init__(self):
        self.vocab = np.ascontiguousarray(self.vocab, dtype=np.int64)
        self.phi = np.ascontiguousarray(self.phi, dtype=np.float32)
        self.phi_oov = np.ascontiguousarray(self.phi_oov, dtype=np.float32)
        self.cuts = {k: _cut_array(k, v) for k, v in self.cuts.items()}
        missing = [k for k in CUT_NAMES.get(self.source, ()) if k not in self.cuts]
        if missing:
            raise ValueError(f"a {self.source} model needs the cuts {missing}")
        ua = [getattr(self, k) is not None for k in _UA_ARRAYS]
        if any(ua) != (self.source == "proxy") or any(ua) != all(ua):
            raise ValueError("ua_keys and ua_counts come together, with a proxy model and no other")
        if all(ua):
            self.ua_keys = np.ascontiguousarray(self.ua_keys, dtype=np.int64)
            self.ua_counts = np.ascontiguousarray(self.ua_counts, dtype=np.int64)
            if self.ua_keys.ndim != 1 or self.ua_counts.shape != self.ua_keys.shape:
                raise ValueError("ua_keys must be [U] and ua_counts [U]")
            if self.ua_keys.shape[0] > 1 and not bool((self.ua_keys[1:] > self.ua_keys[:-1]).all()):
                raise ValueError("ua_keys must be strictly ascending (signed) user-agent hashes")
        if self.phi.shape != (self.V, self.K) or self.phi_oov.shape != (self.K,):
            raise ValueError(f"phi must be [V={self.V}, K={self.K}] and phi_oov [K]")
        if self.V > 1 and not bool((self.vocab[1:] > self.vocab[:-1]).all()):
            raise ValueError("vocab must be strictly ascending word keys")
        given = [getattr(self, k) is not None for k in _DOC_ARRAYS]
        if any(given) and not all(given):
            raise ValueError("doc_keys, doc_theta and doc_tokens come together or not at all")
        if all(given):
            self.doc_keys = np.ascontiguousarray(self.doc_keys, dtype=np.int64)
            self.doc_theta = np.ascontiguousarray(self.doc_theta, dtype=np.float32)
            self.doc_tokens = np.ascontiguousarray(self.doc_tokens, dtype=np.int64)
            Dm = self.doc_keys.shape[0] if self.doc_keys.ndim == 1 else -1
            if Dm < 0 or self.doc_theta.shape != (Dm, self.K) or self.doc_tokens.shape != (Dm,):
                raise ValueError(f"doc_keys must be [Dm], doc_theta [Dm, K={self.K}] and doc_tokens [Dm]")
            if Dm > 1 and not bool((self.doc_keys[1:] > self.doc_keys[:-1]).all()):
                raise ValueError("doc_keys must be strictly ascending document keys")

    @classmethod
    def from_run(cls, run, cuts, source: str, cfg: dict | None = None, docs: bool = True,
                 ua_table: tuple | None = None) -> "SavedModel":
        """The model of a finished training run (``run``: pipeline.common.LdaRun; ``cuts``: the
        day's cuts as a name → values mapping, or a flow day's FlowCuts; ``cfg``: provenance such
        as the training day, the top-domain list's size and digest, the user domain). ``docs``:
        keep the day's document profiles (θ as scoring read it, and each document's token count),
        without the documents keyed by the day's IPv6 dictionary. ``ua_table``: a proxy day's
        (sorted user-agent hashes, counts) as ``pipeline.proxy.featurize`` returns it."""
        from ..utils import provenance as prov
        m = run.model
        if run.route is not None or run.extra_models:
            raise NotImplementedError("models are saved from single-GPU, single-chain runs")
        K = m.K
        prv = {"sweeps": int(m.sweeps_done), "seed": int(m.cfg.seed), "tree_hash": prov.tree_hash("hip"),
               "averaged": m._averaged() is not None}
        prv.update(cfg or {})
        prof = {}
        if docs:
            from ..pipeline import common
            dkeys, theta = common.gather_theta(run, None)
            dkeys = dkeys.cpu().numpy().astype(np.int64)
            keep = dkeys < V6_KEY_BASE
            prof = {"doc_keys": dkeys[keep], "doc_theta": theta[:, :K].cpu().numpy()[keep],
                    "doc_tokens": run.corpus.doc_lengths()[: dkeys.shape[0]].cpu().numpy().astype(np.int64)[keep]}
        if hasattr(cuts, "ibyt"):  # a flow day's FlowCuts
            cuts = {"time": cuts.time, "ibyt": cuts.ibyt, "ipkt": cuts.ipkt}
        else:
            cuts = {k: np.asarray(v) for k, v in cuts.items()}
        if ua_table is not None:
            prof.update(ua_keys=_host(ua_table[0]), ua_counts=_host(ua_table[1]))
        return cls(source=source, K=K, alpha=float(m.alpha), beta=float(m.beta),
                   vocab=run.vocab.cpu().numpy(), phi=m.phi()[:, :K].cpu().numpy(), phi_oov=oov_row(m),
                   cuts=cuts, provenance=prv, **prof)

    def save(self, path: str) -> str:
        meta = {"format": FORMAT, "source": self.source, "K": int(self.K), "alpha": float(self.alpha),
                "beta": float(self.beta), "provenance": self.provenance}
        if not path.endswith(".npz"):
            path += ".npz"
        docs = {k: getattr(self, k) for k in _DOC_ARRAYS} if self.has_docs else {}
        if self.ua_keys is not None:
            docs.update({k: getattr(self, k) for k in _UA_ARRAYS})
        with open(path, "wb") as f:
            np.savez(f, meta=np.array([json.dumps(meta, sort_keys=True)]), vocab=self.vocab, phi=self.phi,
                     phi_oov=self.phi_oov, **{f"cuts_{k}": v for k, v in self.cuts.items()}, **docs)
        return path

    @classmethod
    def load(cls, path: str) -> "SavedModel":
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("meta", *_BASE_ARRAYS) if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a saved oni355 model (missing {missing})")
            meta = json.loads(str(z["meta"][0]))
            if meta.get("format") != FORMAT:
                raise ValueError(f"{path}: model format {meta.get('format')} (this build reads {FORMAT})")
            source = meta["source"]
            if source not in CUT_NAMES:
                raise ValueError(f"{path}: a model of the unknown source {source!r}")
            need = [f"cuts_{k}" for k in CUT_NAMES[source]] + (list(_UA_ARRAYS) if source == "proxy" else [])
            missing = [k for k in need if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a saved {source} model (missing {missing})")
            arr = {k: z[k] for k in _BASE_ARRAYS}
            cuts = {k[5:]: z[k] for k in need if k.startswith("cuts_")}
            docs = {k: z[k] for k in _DOC_ARRAYS if k in z.files}
            if source == "proxy":
                docs.update({k: z[k] for k in _UA_ARRAYS})
        return cls(source=source, K=int(meta["K"]), alpha=float(meta["alpha"]), beta=float(meta["beta"]),
                   vocab=arr["vocab"], phi=arr["phi"], phi_oov=arr["phi_oov"],
                   cuts=cuts, provenance=meta.get("provenance", {}), **docs)

    def table(self, G: int, KP: int, device) -> torch.Tensor:
        """The sampler / score table: f32 [V + 1, G·KP], columns ≥ K zero, row V = ``phi_oov``."""
        KS = G * KP
        if KS < self.K:
            raise ValueError("G*KP must cover the model's K topics")
        t = np.zeros((self.V + 1, KS), dtype=np.float32)
        t[: self.V, : self.K] = self.phi
        t[self.V, : self.K] = self.phi_oov
        return torch.from_numpy(t).to(device)
