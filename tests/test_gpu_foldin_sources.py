"""score_dns and score_proxy on the GPU against the CPU path, bit for bit (rows, scores, words,
the window sums), and k_foldin over the DNS batch's corpus at K = 50 against ref/foldin_spec.py.

A model is trained (CPU, a few sweeps) on one synthetic day of 4000 events and scores another:
its first 700 events moved to one client, so that at chunk_len 16 that document spans 44 chunks;
some events carry a word the model never saw (the out-of-vocabulary row), some proxy events a user
agent absent from the model's table. Both runs with and without per-IP priors.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

from oni355.pipeline import dns, proxy
from oni355.ref import foldin_spec, spec
from oni355.store.columnar import StringColumn

pytestmark = pytest.mark.gpu

N = 4000
HEAVY = 700
CHUNK = 16
SEED = 0x5EED0042
K_OF = {"dns": 50, "proxy": 20}
KW = dict(maxresults=300, sweeps=3, avg_last=2, seed=SEED, chunk_len=CHUNK)
_CACHE: dict = {}


def _setup(src):
    """(model, batch columns, {prior_mass: CPU result}): trained and scored on the CPU once."""
    if src in _CACHE:
        return _CACHE[src]
    if src == "dns":
        from oni355.synth.dns import generate_dns
        day, other = generate_dns(N, seed=21, user_domain="intel"), generate_dns(N, seed=22, user_domain="intel")
        tr = dns.run_dns(dict(day.cols), K=K_OF[src], sweeps=6, maxresults=50, device="cpu", user_domain="intel")
        m = dns.model_from_result(tr, None, "intel")
        ipcol, oddcol = "ip_dst", "dns_qry_type"
    else:
        from oni355.synth.proxy import generate_proxy
        day, other = generate_proxy(N, seed=21), generate_proxy(N, seed=22)
        tr = proxy.run_proxy(dict(day.cols), K=K_OF[src], sweeps=6, maxresults=50, device="cpu")
        m = proxy.model_from_result(tr)
        ipcol, oddcol = "clientip", "respcode"
    cols = {k: (v if isinstance(v, StringColumn) else np.asarray(v).copy()) for k, v in other.cols.items()}
    cols[ipcol][:HEAVY] = cols[ipcol][0]
    cols[oddcol][5:N:97] = 251 if src == "dns" else 999  # words the model never saw
    if src == "proxy":
        ua = cols["useragent"].to_list()
        ua[3:N:211] = ["never-seen-agent"] * len(ua[3:N:211])
        cols["useragent"] = StringColumn.from_list(ua)
    cpu = {mass: _score(src, cols, m, "cpu", mass) for mass in (0.0, 5.0)}
    _CACHE[src] = (m, cols, cpu)
    return _CACHE[src]


def _score(src, cols, m, device, mass):
    if src == "dns":
        return dns.score_dns(dict(cols), m, device=device, prior_mass=mass, **KW)
    return proxy.score_proxy(dict(cols), m, device=device, prior_mass=mass, **KW)


@pytest.mark.parametrize("mass", [0.0, 5.0])
@pytest.mark.parametrize("src", ["dns", "proxy"])
def test_gpu_scoring_equals_the_cpu_path(gpu, src, mass):
    m, cols, cpu = _setup(src)
    rc = cpu[mass]
    rg = _score(src, cols, m, gpu, mass)
    assert rc.stats["n_oov_tokens"] == rg.stats["n_oov_tokens"] >= len(range(5, N, 97))
    assert rg.stats["long_docs"] >= 1 and rg.stats["L"] == CHUNK and rg.stats["mode"] == "infer"
    assert rg.lda.launches["multi_sweep"] == KW["sweeps"]
    assert len(rg.rows) == KW["maxresults"]
    assert np.array_equal(rc.rows, rg.rows)
    assert np.array_equal(rc.scores, rg.scores)
    assert np.array_equal(rc.words, rg.words)
    assert np.array_equal(rc.lda.ndk_sum.numpy(), rg.lda.ndk_sum.cpu().numpy())
    assert np.array_equal(rc.lda.theta().numpy(), rg.lda.theta().cpu().numpy())
    if mass:
        assert rc.stats["n_prior_docs"] == rg.stats["n_prior_docs"] > 0
        assert np.array_equal(rc.lda.prior.numpy(), rg.lda.prior.cpu().numpy())
        assert not np.array_equal(rg.lda.ndk_sum.cpu().numpy(), cpu[0.0].lda.ndk_sum.numpy())
    else:
        assert rg.lda.prior is None and "n_prior_docs" not in rg.stats


def test_foldin_over_the_dns_corpus_replays_the_oracle(gpu):
    """tok_z, ndk and ndk_sum of the device run over the corpus the GPU path built (K = 50: tiling
    (2, 28)) against foldin_spec.foldin_run on the same corpus."""
    m, cols, _ = _setup("dns")
    f = _score("dns", cols, m, gpu, 0.0).lda
    assert (f.G, f.KP, f.K) == (2, 28, 50)
    c = dataclasses.replace(f.c, **{fl.name: getattr(f.c, fl.name).cpu() for fl in dataclasses.fields(f.c)
                                    if isinstance(getattr(f.c, fl.name), torch.Tensor)})
    assert c.T == N and bool(c.chunk_multi.any()) and int((c.tok_word == m.V).sum()) > 0
    st = dict(tok_word=c.tok_word.numpy().view(np.uint32), tok_z=np.zeros(c.sell_slots, np.uint8),
              slice_off=c.slice_off.numpy(), chunk_doc=c.chunk_doc.numpy(), chunk_pos0=c.chunk_pos0.numpy(),
              chunk_key=c.chunk_key.numpy().view(np.uint32), chunk_multi=c.chunk_multi.numpy(),
              ndk_src=np.zeros((c.D, f.KS), np.int32), ndk_dst=np.zeros((c.D, f.KS), np.int32),
              phi=f.table.cpu().numpy())
    s0, s1 = spec.split_seed(SEED)
    want_sum, want_n = foldin_spec.foldin_run(st, f.G, f.KP, f.K, m.alpha, s0, s1, KW["sweeps"], KW["avg_last"],
                                              c.chunk_len.numpy())
    assert np.array_equal(f.tok_z.cpu().numpy(), st["tok_z"])
    assert np.array_equal(f.ndk.cpu().numpy(), want_n)
    assert np.array_equal(f.ndk_sum.cpu().numpy(), want_sum)
    assert int(want_n.sum()) == N and int(want_sum.sum()) == N * f.samples
