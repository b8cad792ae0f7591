"""Fold-in with per-IP topic priors from the saved model, on the CPU: the prior-row and θ oracles
(oni355/ref/foldin_spec.py), draws under a non-flat prior, the saved model's optional document
profiles, the bitwise off-switch of score_flow, the measured quality claim of docs/foldin.md and the
oni-ml options --infer-prior-mass / --no-model-docs."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch
from scipy import stats

from oni355 import ops
from oni355.models.average import theta_rows_prior
from oni355.models.corpus import build_corpus
from oni355.models.foldin import FoldIn
from oni355.models.saved import SavedModel
from oni355.ref import foldin_spec, spec

F32 = np.float32
P_MIN = 1e-4  # the significance level of tests/test_conditional.py
V6 = foldin_spec.V6_KEY_BASE


def small_prior_case():
    """A model of 6 documents (the last keyed by a per-day IPv6 id, which only a hand-made model can
    hold) and a batch of 9 keys: hits, misses, a key below the first and one above the last model
    key, token counts below and above the mass, and the IPv6 id itself."""
    K, KS, alpha, mass = 5, 8, 0.7, 50.0
    mkeys = np.array([10, 20, 30, 40, 50, V6 + 3], np.int64)
    tokens = np.array([3, 100, 7, 49, 51, 500], np.int64)
    theta = np.random.default_rng(6).dirichlet(np.full(K, 0.3), 6).astype(F32)
    batch = np.array([5, 10, 15, 20, 40, 50, 60, V6 + 3, V6 + 9], np.int64)
    return mkeys, theta, tokens, batch, K, KS, alpha, mass


def test_prior_rows_element_by_element():
    mkeys, theta, tokens, batch, K, KS, alpha, mass = small_prior_case()
    got = foldin_spec.prior_rows(mkeys, theta, tokens, batch, K, KS, alpha, mass)
    assert got.dtype == F32 and got.shape == (9, KS)
    row_of = {10: 0, 20: 1, 40: 3, 50: 4}  # the V6 key is in the model arrays and still gets α
    for i, key in enumerate(batch.tolist()):
        for j in range(KS):
            if key in row_of and j < K:
                r = row_of[key]
                m = min(F32(tokens[r]), F32(mass))
                want = spec.fma_f32(np.array([m], F32), theta[r, j:j + 1], np.array([F32(alpha)]))[0]
            else:
                want = F32(alpha)
            assert got[i, j] == want and np.isfinite(got[i, j]), (key, j)
    # the capped and the uncapped mass both occur
    assert F32(tokens[0]) < F32(mass) < F32(tokens[1])
    # the op's CPU path is the oracle
    t = ops.prior_rows(torch.from_numpy(mkeys), torch.from_numpy(theta), torch.from_numpy(tokens),
                       torch.from_numpy(batch), K, KS, alpha, mass)
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), got)
    # no model documents, no batch documents
    e = foldin_spec.prior_rows(mkeys[:0], theta[:0], tokens[:0], batch, K, KS, alpha, mass)
    assert np.array_equal(e, np.full((9, KS), F32(alpha)))
    assert foldin_spec.prior_rows(mkeys, theta, tokens, batch[:0], K, KS, alpha, mass).shape == (0, KS)
    from oni355.pipeline import flow
    assert flow.V6_KEY_BASE == V6


def _np_state(c, phi, KS):
    return dict(tok_word=c.tok_word.numpy().view(np.uint32), tok_z=np.zeros(c.sell_slots, np.uint8),
                slice_off=c.slice_off.numpy(), chunk_doc=c.chunk_doc.numpy(), chunk_pos0=c.chunk_pos0.numpy(),
                chunk_key=c.chunk_key.numpy().view(np.uint32), chunk_multi=c.chunk_multi.numpy(),
                ndk_src=np.zeros((c.D, KS), np.int32), ndk_dst=np.zeros((c.D, KS), np.int32), phi=phi)


@pytest.mark.parametrize("K", [7, 40])
def test_oracle_draws_follow_the_conditional_under_a_prior_row(K):
    """One document with a non-flat prior row, one token looked at (the first of the chunk), many
    seeds: p(k) ∝ (n_k^¬t + pr_k)·φ_wk."""
    G, KP = ops.choose_tiling(K)
    KS = G * KP
    r = np.random.default_rng(K)
    w = torch.tensor([0, 1, 1], dtype=torch.int32)
    c = build_corpus(torch.zeros(3, dtype=torch.int32), w, 1, 3, torch.tensor([12345], dtype=torch.int32), G, L=64)
    phi = np.zeros((3, KS), np.float32)
    phi[:, :K] = (r.random((3, K)) ** 3 + 1e-3).astype(np.float32)
    row = np.zeros(KS, np.int32)
    row[:K] = r.integers(0, 5, K)
    z0 = 2
    row[z0] += 1
    alpha = 0.3
    prior = np.full((1, KS), F32(alpha))
    prior[0, :K] = (F32(alpha) + F32(6.0) * r.dirichlet(np.full(K, 0.2)).astype(F32)).astype(F32)
    assert prior[0, :K].max() > 4 * prior[0, :K].min()  # far from flat
    st = _np_state(c, phi, KS)
    first = int(c.slice_off[0])  # chunk 0, step 0: word 0
    assert st["tok_word"][first] == 0
    n_seeds = 3000
    z = np.empty(n_seeds, np.int64)
    for s in range(n_seeds):
        st["tok_z"][:] = z0
        st["ndk_src"][0] = row
        foldin_spec.foldin_pass(st, G, KP, K, alpha, *spec.split_seed(1000 + s), False, 1, c.chunk_len.numpy(),
                                prior=prior)
        z[s] = st["tok_z"][first]
    n = row[:K].astype(np.float64)
    n[z0] -= 1
    p = (n + prior[0, :K].astype(np.float64)) * phi[0, :K].astype(np.float64)
    p /= p.sum()
    obs = np.bincount(z, minlength=K)[:K]
    exp = p * n_seeds
    rare = exp < 5
    o, e = np.append(obs[~rare], obs[rare].sum()), np.append(exp[~rare], exp[rare].sum())
    if e[-1] == 0:
        o, e = o[:-1], e[:-1]
    chi2, pv = stats.chisquare(o, e)
    assert pv > P_MIN, (chi2, pv)
    # and the flat conditional is rejected by the same draws: the prior row is what was used
    pf = (n + alpha) * phi[0, :K].astype(np.float64)
    ef = pf / pf.sum() * n_seeds
    keep = ef >= 5
    assert stats.chisquare(np.append(obs[keep], obs[~keep].sum() + 1e-9), np.append(ef[keep], ef[~keep].sum() + 1e-9))[1] < P_MIN


def test_an_all_alpha_prior_draws_what_no_prior_draws():
    K = 12
    G, KP = ops.choose_tiling(K)
    r = np.random.default_rng(5)
    lens = [14, 3, 6]  # doc 0: 3 chunks of at most 6
    tdoc = np.repeat(np.arange(3), lens)
    tword = r.integers(0, 9, tdoc.size)
    c = build_corpus(torch.from_numpy(tdoc).to(torch.int32), torch.from_numpy(tword).to(torch.int32), 3, 9,
                     torch.tensor([5, 6, 7], dtype=torch.int32), G, L=6)
    phi = np.zeros((9, KP), np.float32)
    phi[:, :K] = r.random((9, K)).astype(np.float32)
    a = FoldIn(c, torch.from_numpy(phi), K, 0.4, seed=11).run(4, 2)
    flat = torch.full((3, KP), 0.4, dtype=torch.float32)
    b = FoldIn(c, torch.from_numpy(phi), K, 0.4, seed=11, prior=flat).run(4, 2)
    for k in ("tok_z", "ndk", "ndk_sum"):
        assert torch.equal(getattr(a, k), getattr(b, k))
    assert a.launches == b.launches
    # a non-flat row changes the chain, and a multi-chunk document uses its row in every chunk
    bent = flat.clone()
    bent[0, 3] = 400.0
    d = FoldIn(c, torch.from_numpy(phi), K, 0.4, seed=11, prior=bent).run(4, 2)
    assert int(d.ndk[0, 3]) >= 12 and int(d.ndk[0].sum()) == 14
    assert torch.equal(d.ndk[1:], a.ndk[1:])  # documents do not couple
    with pytest.raises(ValueError, match="prior"):
        FoldIn(c, torch.from_numpy(phi), K, 0.4, prior=flat[:2])
    with pytest.raises(ValueError, match="prior"):
        FoldIn(c, torch.from_numpy(phi), K, 0.4, prior=flat.to(torch.float64))


@pytest.mark.parametrize("K,KS,dtype", [(5, 8, torch.int32), (20, 20, torch.int32), (50, 56, torch.int64)])
def test_theta_rows_prior_equals_its_oracle(K, KS, dtype):
    r = np.random.default_rng(K)
    D, S = 37, 3.0
    n = np.zeros((D, KS), np.int64)
    n[:, :K] = r.integers(0, 2000, (D, K))
    n[0] = 0  # an empty document: θ = pr / Σpr
    n[1, :K] = 2 ** 24 + 1  # a count f32 cannot hold
    prior = np.full((D, KS), F32(0.7))
    prior[:, :K] = (F32(0.7) + F32(37.5) * r.dirichlet(np.full(K, 0.3), D).astype(F32)).astype(F32)
    want = foldin_spec.theta_rows_prior(n.astype(np.int32 if dtype == torch.int32 else np.int64), prior, K, S)
    got = theta_rows_prior(torch.from_numpy(n).to(dtype), torch.from_numpy(prior), K, S)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert not want[:, K:].any() and np.all(want[:, :K] > 0)
    assert np.allclose(want[:, :K].sum(1), 1.0, atol=1e-5)
    # element by element, from the definition
    S32 = np.array([F32(S)])
    for d in (0, 1, 5):
        sp = F32(0)
        for j in range(K):
            sp = F32(sp + prior[d, j])
        den = spec.fma_f32(S32, np.array([sp]), np.array([F32(int(n[d, :K].sum()))]))[0]
        for j in range(K):
            num = spec.fma_f32(S32, prior[d, j:j + 1], np.array([F32(n[d, j])]))[0]
            assert want[d, j] == F32(num / den)


# ---- saved model, score_flow, CLI ---------------------------------------------------------------
@pytest.fixture(scope="module")
def day():
    from oni355.synth.flow import generate_flows
    return generate_flows(5000, seed=21)


def _train(day, seed, maxresults):
    from oni355.pipeline.flow import run_flow
    return run_flow(dict(day.cols), K=20, sweeps=12, tol=1.0, maxresults=maxresults, device="cpu", seed=seed)


@pytest.fixture(scope="module")
def trained(day):
    """One training per model seed, every event ranked (maxresults = n, tol = 1)."""
    return {seed: _train(day, seed, day.n) for seed in (101, 202, 303)}


def test_document_profiles_round_trip(day, trained, tmp_path):
    from oni355.pipeline import common
    res = trained[101]
    m = SavedModel.from_run(res.lda, res.cuts, "flow", {"day": "20160708"})
    assert m.has_docs
    dkeys, theta = common.gather_theta(res.lda, None)
    assert np.array_equal(m.doc_keys, dkeys.numpy()) and m.doc_keys.dtype == np.int64
    assert np.array_equal(m.doc_theta, theta[:, :20].numpy()) and m.doc_theta.dtype == np.float32
    assert np.array_equal(m.doc_tokens, res.lda.corpus.doc_lengths().numpy()) and m.doc_tokens.dtype == np.int64
    assert int(m.doc_tokens.sum()) == 2 * day.n
    m2 = SavedModel.load(m.save(str(tmp_path / "m.npz")))
    for k in ("doc_keys", "doc_theta", "doc_tokens", "vocab", "phi", "phi_oov"):
        a, b = getattr(m, k), getattr(m2, k)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    # docs=False round-trips as "no profiles"
    m0 = SavedModel.from_run(res.lda, res.cuts, "flow", docs=False)
    assert not m0.has_docs and m0.doc_theta is None
    m3 = SavedModel.load(m0.save(str(tmp_path / "m0.npz")))
    assert not m3.has_docs and m3.phi.tobytes() == m.phi.tobytes()
    with np.load(str(tmp_path / "m0.npz")) as z:
        assert not any(k.startswith("doc_") for k in z.files)
    # a file written without the three arrays (an older build's) loads
    with np.load(str(tmp_path / "m.npz")) as z:
        old = {k: z[k] for k in z.files if not k.startswith("doc_")}
    np.savez(str(tmp_path / "old.npz"), **old)
    m4 = SavedModel.load(str(tmp_path / "old.npz"))
    assert not m4.has_docs and m4.vocab.tobytes() == m.vocab.tobytes()
    assert not m.without_docs().has_docs and m.without_docs().phi is m.phi
    # keys of the per-day IPv6 dictionary are dropped when saving
    run6 = type("Run", (), {})()
    run6.__dict__.update(res.lda.__dict__)
    k6 = res.lda.doc_keys64.clone()
    k6[-2:] = torch.tensor([V6, V6 + 1])
    run6.doc_keys64 = k6
    m6 = SavedModel.from_run(run6, res.cuts, "flow")
    assert m6.doc_keys.shape[0] == k6.numel() - 2 and int(m6.doc_keys.max()) < V6
    assert np.array_equal(m6.doc_theta, m.doc_theta[:-2]) and np.array_equal(m6.doc_tokens, m.doc_tokens[:-2])


def test_document_profiles_are_validated(trained):
    res = trained[101]
    m = SavedModel.from_run(res.lda, res.cuts, "flow")
    base = dict(source="flow", K=m.K, alpha=m.alpha, beta=m.beta, vocab=m.vocab, phi=m.phi, phi_oov=m.phi_oov, cuts=m.cuts)
    ok = SavedModel(**base, doc_keys=m.doc_keys[:4], doc_theta=m.doc_theta[:4], doc_tokens=m.doc_tokens[:4])
    assert ok.has_docs
    bad = [dict(doc_keys=m.doc_keys[:4][::-1], doc_theta=m.doc_theta[:4], doc_tokens=m.doc_tokens[:4]),   # descending
           dict(doc_keys=m.doc_keys[[0, 1, 1, 2]], doc_theta=m.doc_theta[:4], doc_tokens=m.doc_tokens[:4]),  # repeated
           dict(doc_keys=m.doc_keys[:4], doc_theta=m.doc_theta[:3], doc_tokens=m.doc_tokens[:4]),
           dict(doc_keys=m.doc_keys[:4], doc_theta=m.doc_theta[:4, :19], doc_tokens=m.doc_tokens[:4]),
           dict(doc_keys=m.doc_keys[:4], doc_theta=m.doc_theta[:4], doc_tokens=m.doc_tokens[:5]),
           dict(doc_keys=m.doc_keys[:4].reshape(2, 2), doc_theta=m.doc_theta[:4], doc_tokens=m.doc_tokens[:4]),
           dict(doc_keys=m.doc_keys[:4], doc_theta=m.doc_theta[:4]),                                      # one missing
           dict(doc_tokens=m.doc_tokens[:4])]
    for kw in bad:
        with pytest.raises(ValueError, match="doc_"):
            SavedModel(**base, **kw)


def _same(a, b):
    return (np.array_equal(a.rows, b.rows) and np.array_equal(a.scores, b.scores)
            and np.array_equal(a.src_scores, b.src_scores) and np.array_equal(a.dst_scores, b.dst_scores))


def test_prior_mass_zero_is_bitwise_the_model_without_profiles(day, trained):
    from oni355.pipeline.flow import score_flow
    res = trained[101]
    m = SavedModel.from_run(res.lda, res.cuts, "flow")
    kw = dict(maxresults=200, device="cpu", sweeps=6, avg_last=3, seed=101)
    with_docs = score_flow(dict(day.cols), m, prior_mass=0, **kw)
    stripped = score_flow(dict(day.cols), m.without_docs(), **kw)
    assert _same(with_docs, stripped)
    assert np.array_equal(with_docs.lda.ndk_sum.numpy(), stripped.lda.ndk_sum.numpy())
    assert with_docs.lda.prior is None and "n_prior_docs" not in with_docs.stats and "prior_mass" not in with_docs.stats
    # with a mass the same call takes the prior path: every IP of the day is known to its own model
    on = score_flow(dict(day.cols), m, prior_mass=50, **kw)
    assert on.stats["n_prior_docs"] == on.stats["D"] == m.doc_keys.shape[0] and on.stats["prior_mass"] == 50.0
    assert on.lda.prior is not None and not _same(on, stripped)
    want = foldin_spec.prior_rows(m.doc_keys, m.doc_theta, m.doc_tokens, m.doc_keys, 20, 20, m.alpha, 50.0)
    assert np.array_equal(on.lda.prior.numpy(), want)
    assert np.array_equal(on.lda.theta().numpy(),
                          foldin_spec.theta_rows_prior(on.lda.ndk_sum.numpy(), want, 20, 3.0))
    with pytest.raises(ValueError, match="docs=True"):
        score_flow(dict(day.cols), m.without_docs(), prior_mass=50, **kw)
    with pytest.raises(ValueError, match="prior_mass"):
        score_flow(dict(day.cols), m, prior_mass=-1, **kw)


def test_unknown_ips_get_the_flat_row(day, trained):
    """A model that knows only every other IP: the others' prior rows are α, and their documents
    come out exactly as without any prior (documents do not couple)."""
    from oni355.pipeline.flow import score_flow
    res = trained[101]
    m = SavedModel.from_run(res.lda, res.cuts, "flow")
    half = SavedModel(source="flow", K=m.K, alpha=m.alpha, beta=m.beta, vocab=m.vocab, phi=m.phi, phi_oov=m.phi_oov,
                      cuts=m.cuts, doc_keys=m.doc_keys[::2], doc_theta=m.doc_theta[::2], doc_tokens=m.doc_tokens[::2])
    kw = dict(maxresults=50, device="cpu", sweeps=3, avg_last=2, seed=101)
    on = score_flow(dict(day.cols), half, prior_mass=20, **kw)
    off = score_flow(dict(day.cols), half, **kw)
    D = on.stats["D"]
    assert on.stats["n_prior_docs"] == (D + 1) // 2
    pr = on.lda.prior.numpy()
    assert np.all(pr[1::2] == F32(m.alpha)) and np.all(pr[::2, :20].max(1) > F32(m.alpha))
    assert np.array_equal(on.lda.ndk_sum.numpy()[1::2], off.lda.ndk_sum.numpy()[1::2])
    assert not np.array_equal(on.lda.ndk_sum.numpy()[::2], off.lda.ndk_sum.numpy()[::2])


# the mass docs/foldin.md recommends (its quality table, measured on this day)
RECOMMENDED_MASS = 5.0


def test_recommended_mass_is_no_worse_than_no_prior(day, trained):
    """docs/foldin.md, "Measured quality with a prior": every 5th flow of the day (each IP with about
    a fifth of its tokens) scored against the day's model; the yardstick is the training run's own
    ranking restricted to those rows, top 50. Mass 0 is fold-in without priors (the baseline, computed
    here); the mean overlap over the three model seeds at the recommended mass is not below it."""
    from oni355.pipeline.flow import score_flow
    STEP, TOP = 5, 50
    batch = {k: np.ascontiguousarray(v[::STEP]) for k, v in day.cols.items()}
    ov = {0.0: [], RECOMMENDED_MASS: []}
    for seed, res in trained.items():
        m = SavedModel.from_run(res.lda, res.cuts, "flow")
        rows = res.rows
        assert rows.shape[0] == day.n
        yard = set((rows[rows % STEP == 0][:TOP] // STEP).tolist())
        for mass in ov:
            r = score_flow(dict(batch), m, tol=1.0, maxresults=TOP, device="cpu", seed=seed, prior_mass=mass)
            ov[mass].append(len(yard & set(r.rows.tolist())) / TOP)
    print("top-50 overlap per seed", ov)
    assert np.mean(ov[RECOMMENDED_MASS]) >= np.mean(ov[0.0])


def test_cli_prior_mass(tmp_path):
    from oni355.cli import ml
    lp, md, md0 = str(tmp_path / "lp"), str(tmp_path / "models"), str(tmp_path / "models0")
    base = ["20160708", "flow", "1.0", "50", "--synthetic", "3000", "--device", "cpu", "--lpath", lp, "--quiet"]
    assert ml.main(base + ["--sweeps", "6", "--save-model", md]) == 0
    mp = os.path.join(md, "flow_model.npz")
    assert SavedModel.load(mp).has_docs
    res = os.path.join(lp, "flow", "20160708", "flow_results.csv")
    os.remove(res)
    assert ml.main(base + ["--model", mp, "--infer-sweeps", "4", "--infer-avg-last", "2", "--infer-prior-mass", "50"]) == 0
    assert os.path.getsize(res) > 0
    with open(os.path.join(lp, "flow", "20160708", "metrics.jsonl")) as f:
        last = json.loads(f.readlines()[-1])
    assert last["mode"] == "infer" and last["n_prior_docs"] > 0 and last["prior_mass"] == 50.0
    # without the flag: today's run, no prior keys in the metrics
    assert ml.main(base + ["--model", mp, "--infer-sweeps", "4", "--infer-avg-last", "2"]) == 0
    with open(os.path.join(lp, "flow", "20160708", "metrics.jsonl")) as f:
        last = json.loads(f.readlines()[-1])
    assert "n_prior_docs" not in last
    # a model saved without profiles: usable as before, refused with a mass
    assert ml.main(base + ["--sweeps", "6", "--save-model", md0, "--no-model-docs"]) == 0
    mp0 = os.path.join(md0, "flow_model.npz")
    assert not SavedModel.load(mp0).has_docs
    assert ml.main(base + ["--model", mp0, "--infer-sweeps", "2"]) == 0
    with pytest.raises(SystemExit) as e:
        ml.main(base + ["--model", mp0, "--infer-prior-mass", "50"])
    assert e.value.code not in (0, None) and "--no-model-docs" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        ml.main(base + ["--model", mp, "--infer-prior-mass", "-1"])
    assert "--infer-prior-mass" in str(e.value.code)
