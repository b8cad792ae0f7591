"""The host-side schedule of GibbsLDA, pinned: every count mode, the auto switch, the dense and MH
samplers, posterior averaging (in-sweep and eager, int32 and int64 sums, saved and restored inside
the window), the packed and the lagged X01 of a forced 1-rank group, and a canonical-z resume, each
on a corpus of a few hundred tokens through the device-free path (CPU tensors, the NumPy oracle).

Each case's chain is recorded in tests/golden/gibbs_model_chain.json as SHA-256 of the bytes of
canonical_z(), n_wk, n_k, n_dk, theta() and phi(), next to change_log, the all-reduce count and
whether a packed payload exists. ``PYTHONPATH=. python tests/test_gibbs_model_golden_cpu.py``
rewrites the file from the code as it stands: only a change that means to alter the chain should.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oni355.models import gibbs as gm
from oni355.models.corpus import build_corpus
from oni355.models.gibbs import GibbsConfig, GibbsLDA
from oni355.parallel.comm import Comm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gibbs_model_chain.json")
CPU = torch.device("cpu")
D, V, L = 30, 40, 16
POST = {"ONI_POST_SPAN": "1"}  # a window of 3 samples inside 8 sweeps
# one forced rank: every word's count is its own; ≤ 3 travels as bytes, ≤ 12 as halves, the rest int32
PACK = {"ONI_FORCE_DIST": "1", "ONI_X01_PACK": "1", "ONI_X01_TINY_MAX": "3", "ONI_X01_LIGHT_MAX": "12"}
LAG = {**PACK, "ONI_X01_LAG": "1", "ONI_X01_LAG_FROM": "3"}


def _corpus(K, sampler):
    """30 documents of 3-20 tokens over 40 words (Zipf), document 0 with 70 tokens and documents 1
    and 2 with 40: at L = 16 these three span several chunks."""
    r = np.random.default_rng(17)
    lens = r.integers(3, 21, D)
    lens[:3] = (70, 40, 40)
    tdoc = np.repeat(np.arange(D), lens)
    tword = (r.zipf(1.4, tdoc.size) - 1) % V
    o = np.lexsort((tword, tdoc))
    keys = torch.arange(D, dtype=torch.int32) * 7 + 1
    c = build_corpus(torch.from_numpy(tdoc[o]), torch.from_numpy(tword[o]), D, V, keys, gm.tiling_for(K, sampler)[0],
                     L=L)
    assert 300 <= c.T <= 600 and int((c.doc_lengths() > L).sum()) >= 2
    return c


def _model(K=20, sampler="dense", dist=False, **cfg):
    comm = Comm(0, 1, CPU, forced=True) if dist else None
    m = GibbsLDA(_corpus(K, sampler), GibbsConfig(K=K, seed=21, sampler=sampler, **cfg), comm=comm)
    m.initialize()
    return m


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _record(m):
    K = m.K
    return {"z": _sha(m.canonical_z()), "nwk": _sha(m.nwk[:, :K]), "nk": _sha(m.nk_cur[:K]),
            "ndk": _sha(m.ndk_cur[:, :K]), "theta": _sha(m.theta()), "phi": _sha(m.phi()),
            "change_log": [[int(s), float(f)] for s, f in m.change_log],
            "allreduce_calls": int(m.timings["allreduce_calls"]), "x01_none": m._x01 is None}


def _same_chain(a, b):
    """Equal topics, counts and estimates (a resumed model's change_log starts at its resume)."""
    ra, rb = _record(a), _record(b)
    return all(ra[k] == rb[k] for k in ("z", "nwk", "nk", "ndk", "theta", "phi"))


def _chain(sweeps=6, **kw):
    m = _model(**kw)
    m.sweep(sweeps)
    return m


def _auto_crossing():
    m = _chain(count_mode="auto", auto_threshold=0.9)
    assert m._delta_on and m.change_log  # the threshold is crossed inside the 6 sweeps
    return m


def _averaged(post_every, **kw):
    m = _model(post_samples=3, post_every=post_every, **kw)
    m.plan_average(8)
    m.sweep(8)
    assert m._averaged() is not None
    return m


def _averaged_resumed():
    """7 of the 8 sweeps (two of the three samples), then the canonical z and the sample sums into a
    fresh model that draws the last one: the uninterrupted average."""
    a = _model(post_samples=3, post_every=1)
    a.plan_average(8)
    a.sweep(7)
    st = a.average_state()
    assert st is not None and st["n"] == 2
    b = _model(post_samples=3, post_every=1)
    b.plan_average(8)
    b.load_canonical_z(a.canonical_z(), 7)
    b.load_average_state(st)
    b.sweep(1)
    assert b._averaged() is not None
    assert _same_chain(b, _averaged(1))
    return b


def _packed(**kw):
    m = _model(dist=True, **kw)
    x = m._x01
    assert x is not None and min(int(x[k].numel()) for k in ("tiny", "light", "heavy")) > 0
    m.sweep(6)
    return m


def _lagged():
    m = _packed(x01_lag=True)
    assert m._lag_live
    return m


def _resumed():
    """Sweeps 1-3, the canonical z into a fresh model, sweeps 4-6: the uninterrupted chain."""
    a = _chain(sweeps=3)
    b = _model()
    b.load_canonical_z(a.canonical_z(), 3)
    b.sweep(3)
    assert _same_chain(b, _chain())
    return b


CASES = {
    **{f"mode_{cm}": ({}, lambda cm=cm: _chain(count_mode=cm)) for cm in ("recount", "atomic", "delta", "dual", "wdelta")},
    "auto_switch3": ({}, lambda: _chain(count_mode="auto", auto_switch=3)),
    "auto_threshold": ({}, _auto_crossing),
    "dense_k20": ({}, lambda: _chain(K=20)),
    "dense_k50": ({}, lambda: _chain(K=50)),
    "mh_alias_k20": ({"ONI_MH_WORD": "alias"}, lambda: _chain(sampler="mh")),
    "mh_cdf_k20": ({"ONI_MH_WORD": "cdf"}, lambda: _chain(sampler="mh")),
    "post_every1": (POST, lambda: _averaged(1)),
    "post_every2": (POST, lambda: _averaged(2)),
    "post_every1_wide": ({**POST, "ONI_POST_WIDE": "1"}, lambda: _averaged(1)),
    "post_resumed_mid_window": (POST, _averaged_resumed),
    "dist_x01_packed": (PACK, _packed),
    "dist_x01_lagged": (LAG, _lagged),
    "canonical_z_resume": ({}, _resumed),
}
# what a developer's shell may carry: every case starts from the defaults
CLEARED = ("ONI_COUNT_MODE", "ONI_AUTO_THRESHOLD", "ONI_AUTO_DELTA", "ONI_AUTO_EARLY", "ONI_SAMPLER", "ONI_INIT",
           "ONI_POST_SAMPLES", "ONI_POST_EVERY", "ONI_POST_SPAN", "ONI_POST_WIDE", "ONI_X01_LAG", "ONI_X01_LAG_FROM",
           "ONI_X01_PACK", "ONI_X01_PACK_MIN_BYTES", "ONI_X01_TINY_MAX", "ONI_X01_LIGHT_MAX", "ONI_FORCE_DIST",
           "ONI_COMM_REAL", "ONI_MH_WORD", "ONI_MH_DOC_MOVES", "ONI_APPLY_INPLACE", "ONI_EXACT_GUARD",
           "ONI_CHECK_INVARIANTS", "ONI_HEALTH_CHECK")


def _run(name):
    env, run = CASES[name]
    saved = dict(os.environ)
    try:
        for k in CLEARED:
            os.environ.pop(k, None)
        os.environ.update(env)
        return _record(run())
    finally:
        os.environ.clear()
        os.environ.update(saved)


@pytest.mark.parametrize("name", sorted(CASES))
def test_chain_matches_the_recorded_fingerprint(name):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(CASES)
    assert _run(name) == want[name]


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump({name: _run(name) for name in sorted(CASES)}, f, indent=1, sort_keys=True)
        f.write("\n")
