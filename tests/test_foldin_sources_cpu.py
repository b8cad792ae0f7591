"""Fold-in scoring of DNS and proxy days on the CPU: the saved model of any source (cuts, the
proxy user-agent table, the top-list digest), score_dns / score_proxy end to end against the
training run, model-derived wording (unseen words, unseen user agents), per-IP priors and the
oni-ml --save-model / --model options for both sources."""
from __future__ import annotations

import csv
import json
import os

import numpy as np
import pytest
import torch

from oni355 import ops, schema
from oni355.models.foldin import FoldIn
from oni355.models.gibbs import tiling_for
from oni355.models.saved import CUT_NAMES, SavedModel, top_digest
from oni355.pipeline import dns, proxy
from oni355.store.columnar import StringColumn

N_TOP = 100
N_EVENTS = 5000
SWEEPS = 12
SEEDS = (101, 202, 303, 404, 505, 606)  # the seed pairs of tests/test_foldin_cpu.py: consecutive seeds
K_OF = {"dns": 50, "proxy": 20}
TOP = ["google.com", "intel.com", "example.org"]


def _generate(source, n, seed):
    if source == "dns":
        from oni355.synth.dns import generate_dns
        return generate_dns(n, seed=seed, user_domain="intel")
    from oni355.synth.proxy import generate_proxy
    return generate_proxy(n, seed=seed)


def _train(source, cols, seed):
    kw = dict(K=K_OF[source], sweeps=SWEEPS, maxresults=N_TOP, device="cpu", seed=seed, top_domains=TOP)
    if source == "dns":
        return dns.run_dns(dict(cols), user_domain="intel", **kw)
    return proxy.run_proxy(dict(cols), **kw)


def _model(source, res, **kw):
    if source == "dns":
        return dns.model_from_result(res, TOP, "intel", {"day": "20160708"}, **kw)
    return proxy.model_from_result(res, TOP, {"day": "20160708"}, **kw)


def _score(source, cols, model, **kw):
    kw.setdefault("device", "cpu")
    kw.setdefault("top_domains", TOP)
    fn = dns.score_dns if source == "dns" else proxy.score_proxy
    return fn(dict(cols), model, **kw)


_DAYS: dict = {}


@pytest.fixture(scope="module", params=["dns", "proxy"])
def trained(request):
    """(source, day, training run with seed 101, its saved model); one training per source."""
    src = request.param
    if src not in _DAYS:
        day = _generate(src, N_EVENTS, 21)
        res = _train(src, day.cols, SEEDS[0])
        _DAYS[src] = (src, day, res, _model(src, res))
    return _DAYS[src]


def _same(a, b):
    return np.array_equal(a.rows, b.rows) and np.array_equal(a.scores, b.scores) and np.array_equal(a.words, b.words)


def test_saved_model_round_trip(trained, tmp_path):
    src, _, res, m = trained
    p = m.save(str(tmp_path / f"{src}_model.npz"))
    m2 = SavedModel.load(p)
    assert (m2.source, m2.K, m2.alpha, m2.beta) == (src, K_OF[src], m.alpha, m.beta)
    for k in ("vocab", "phi", "phi_oov", "doc_keys", "doc_theta", "doc_tokens"):
        a, b = getattr(m, k), getattr(m2, k)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # the cuts are the integers the training day's featurizer returned, exactly
    assert tuple(m2.cuts) == CUT_NAMES[src]
    for k in CUT_NAMES[src]:
        assert m2.cuts[k].dtype == np.uint32 and m2.cuts[k].tolist() == res.stats["cuts"][k]
        assert m2.cuts[k].tobytes() == m.cuts[k].tobytes()
    n, dg = top_digest(TOP)
    assert n == 3 and len(dg) == 16
    assert m2.provenance["top_entries"] == 3 and m2.provenance["top_digest"] == dg
    assert top_digest([" Google.com", "intel.com\n", "", "example.org"]) == (n, dg) and top_digest(None) == (0, "")
    assert top_digest(TOP[::-1])[1] != dg
    assert m2.provenance["day"] == "20160708" and m2.provenance["sweeps"] == SWEEPS
    if src == "dns":
        assert m2.provenance["user_domain"] == "intel" and m2.ua_keys is None
    else:
        tk, tc = res.stats["ua_table"]
        assert m2.ua_keys.dtype == np.int64 and m2.ua_counts.dtype == np.int64
        assert np.array_equal(m2.ua_keys, tk.numpy()) and np.array_equal(m2.ua_counts, tc.numpy())
        assert np.all(np.diff(m2.ua_keys) > 0) and int(m2.ua_counts.sum()) == N_EVENTS
        # a proxy file without its user-agent table is refused by name
        with np.load(p) as z:
            arrays = {k: z[k] for k in z.files if k != "ua_keys"}
        bad = str(tmp_path / "no_ua.npz")
        np.savez(bad, **arrays)
        with pytest.raises(ValueError, match="ua_keys"):
            SavedModel.load(bad)
        base = dict(source="proxy", K=m.K, alpha=m.alpha, beta=m.beta, vocab=m.vocab, phi=m.phi, phi_oov=m.phi_oov,
                    cuts=m.cuts)
        with pytest.raises(ValueError, match="ua_keys"):
            SavedModel(**base, ua_keys=m.ua_keys[::-1].copy(), ua_counts=m.ua_counts)
        with pytest.raises(ValueError, match="ua_keys"):
            SavedModel(**base, ua_keys=m.ua_keys)
    # a file lacking one of the source's cut lists names it
    with np.load(p) as z:
        arrays = {k: z[k] for k in z.files if k != "cuts_time"}
    bad = str(tmp_path / "no_cut.npz")
    np.savez(bad, **arrays)
    with pytest.raises(ValueError, match="cuts_time"):
        SavedModel.load(bad)


def test_cut_values_outside_u32_are_kept_as_int64(tmp_path):
    cuts = {"time": np.array([1, 2**32 + 5]), "ibyt": np.array([3, 4], np.int64), "ipkt": np.array([-1, 7])}
    m = SavedModel(source="flow", K=2, alpha=0.5, beta=0.1, vocab=np.array([4, 9]), phi=np.full((2, 2), 0.5),
                   phi_oov=np.full(2, 0.5), cuts=cuts)
    m2 = SavedModel.load(m.save(str(tmp_path / "m.npz")))
    assert [m2.cuts[k].dtype for k in ("time", "ibyt", "ipkt")] == [np.int64, np.uint32, np.int64]
    for k, v in cuts.items():
        assert m2.cuts[k].tolist() == v.tolist()
    with pytest.raises(ValueError, match="integers"):
        SavedModel(source="flow", K=2, alpha=0.5, beta=0.1, vocab=np.array([4, 9]), phi=np.full((2, 2), 0.5),
                   phi_oov=np.full(2, 0.5), cuts={**cuts, "time": np.array([0.5])})


def test_a_flow_model_file_holds_what_it_held(tmp_path):
    from oni355.pipeline.flow import run_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(2000, seed=5)
    res = run_flow(dict(day.cols), K=20, sweeps=4, maxresults=10, device="cpu", seed=7)
    base = {"meta", "vocab", "phi", "phi_oov", "cuts_time", "cuts_ibyt", "cuts_ipkt"}
    for docs, names in ((True, base | {"doc_keys", "doc_theta", "doc_tokens"}), (False, base)):
        p = SavedModel.from_run(res.lda, res.cuts, "flow", {"day": "d"}, docs=docs).save(str(tmp_path / f"m{docs}.npz"))
        with np.load(p) as z:
            assert set(z.files) == names
            for k in ("time", "ibyt", "ipkt"):
                want = np.asarray(getattr(res.cuts, k))
                assert z[f"cuts_{k}"].dtype == np.uint32 and np.array_equal(z[f"cuts_{k}"], want)
            assert z["vocab"].dtype == np.int64 and np.array_equal(z["vocab"], res.lda.vocab.numpy())
            assert z["phi"].dtype == np.float32 and np.array_equal(z["phi"], res.lda.model.phi()[:, :20].numpy())
            meta = json.loads(str(z["meta"][0]))
        assert meta["format"] == 1 and meta["source"] == "flow"
        assert set(meta["provenance"]) == {"sweeps", "seed", "tree_hash", "averaged", "day"}


@pytest.fixture(scope="module")
def floors():
    """Top-100 overlap of two trainings of the day that differ only in their seed, per source, over
    the five consecutive seed pairs: the noise floor measured here, not a recorded one."""
    out = {}

    def floor(src):
        if src not in out:
            _, day, res, _ = _DAYS[src]
            tops = [set(res.rows.tolist())] + [set(_train(src, day.cols, s).rows.tolist()) for s in SEEDS[1:]]
            out[src] = [len(a & b) / N_TOP for a, b in zip(tops, tops[1:])]
        return out[src]
    return floor


def test_scoring_the_training_day_agrees_with_training(trained, floors, tmp_path):
    src, day, res, m = trained
    m = SavedModel.load(m.save(str(tmp_path / "m.npz")))
    r = _score(src, day.cols, m, maxresults=N_TOP, seed=SEEDS[0])
    assert r.stats["mode"] == "infer" and r.stats["n_oov_tokens"] == 0 and r.stats["loglik"] is None
    assert r.stats["model_top_mismatch"] is False and r.stats["model_day"] == "20160708"
    assert r.stats["foldin_launches"] > 0 and r.stats["events"] == N_EVENTS and r.timings["records_scored"] == N_EVENTS
    assert len(r.rows) == N_TOP and np.all(np.diff(r.scores) >= 0) and isinstance(r.lda, FoldIn)
    # the model's cuts and dictionaries word the training day exactly as training did
    trained_words = dict(zip(res.rows.tolist(), res.words.tolist()))
    assert all(trained_words[i] == w for i, w in zip(r.rows.tolist(), r.words.tolist()) if i in trained_words)
    from oni355.io import results as rio
    out = rio.write_rendered(str(tmp_path / "results.csv"), schema.result_columns(src),
                             rio.render_result(src, dict(day.cols), r, 0, None))
    header, rows = rio.read_csv(out)
    assert header == schema.result_columns(src) and len(rows) == N_TOP
    overlap = len(set(r.rows.tolist()) & set(res.rows.tolist())) / N_TOP
    floor = floors(src)
    print(src, "fold-in overlap", overlap, "floor", floor)
    assert overlap >= min(floor)


def test_refusals(trained):
    src, day, _, m = trained

    class _Comm:
        dist = True
    with pytest.raises(NotImplementedError, match="fold-in scoring is single-GPU"):
        _score(src, {}, None, comm=_Comm())
    other = SavedModel(source="flow", K=m.K, alpha=m.alpha, beta=m.beta, vocab=m.vocab, phi=m.phi, phi_oov=m.phi_oov,
                       cuts={"time": [1], "ibyt": [1], "ipkt": [1]})
    with pytest.raises(ValueError, match=f"flow model cannot score {src}"):
        _score(src, day.cols, other)
    with pytest.raises(ValueError, match="prior_mass"):
        _score(src, day.cols, m, prior_mass=-1)
    with pytest.raises(ValueError, match="docs=True"):
        _score(src, day.cols, m.without_docs(), prior_mass=5)


def _batch(day, n):
    return {k: (v.slice(0, n) if isinstance(v, StringColumn) else np.asarray(v)[:n].copy()) for k, v in day.cols.items()}


def test_an_unseen_word_is_scored_with_the_oov_row(trained):
    src, day, _, m = trained
    n, odd = 600, [3, 77, 410]
    cols = _batch(day, n)
    if src == "dns":
        cols["dns_qry_type"][odd] = 251  # a query type no event of the training day has
    else:
        cols["respcode"][odd] = 999
    logs = []
    r = _score(src, cols, m, tol=2.0, maxresults=n, sweeps=4, avg_last=2, feedback={"x": [1]}, log=logs.append)
    assert any("feedback is ignored" in x for x in logs) and len(logs) == 1
    assert r.stats["n_oov_tokens"] == len(odd) and len(r.rows) == n
    words = dict(zip(r.rows.tolist(), r.words.astype(np.int64).tolist()))
    assert all(words[i] not in set(m.vocab.tolist()) for i in odd)
    assert sum(w not in set(m.vocab.tolist()) for w in words.values()) == len(odd)
    # the event's score is θ of its document · the model's phi_oov (row V of the table), bitwise
    G, KP = tiling_for(m.K, "dense")
    table = m.table(G, KP, "cpu")
    assert np.array_equal(table[m.V, :m.K].numpy(), m.phi_oov)
    ips = np.asarray(cols["ip_dst" if src == "dns" else "clientip"]).astype(np.uint32).astype(np.int64)
    rowof = np.searchsorted(np.unique(ips), ips[odd])
    want = ops.pair_score(r.lda.theta(), table, torch.from_numpy(rowof.astype(np.int32)),
                          torch.full((len(odd),), m.V, dtype=torch.int32)).numpy()
    score = dict(zip(r.rows.tolist(), r.scores.tolist()))
    assert [score[i] for i in odd] == want.tolist()


def test_top_list_or_user_domain_mismatch_is_reported(trained):
    src, day, _, m = trained
    cols = _batch(day, 300)
    logs = []
    r = _score(src, cols, m, sweeps=2, avg_last=1, top_domains=["example.com"], log=logs.append)
    assert r.stats["model_top_mismatch"] is True and len(logs) == 1 and "top-domain list of 1 entries" in logs[0]
    if src == "dns":
        logs.clear()
        r = _score(src, cols, m, sweeps=2, avg_last=1, user_domain="other", log=logs.append)
        assert r.stats["model_top_mismatch"] is True and len(logs) == 1 and "user domain 'other'" in logs[0]


def test_an_unseen_user_agent_counts_zero():
    """The proxy words of a batch come from the model's user-agent table: the table's count of the
    row's user agent (clamped to 2^31 − 1), 0 for one the training day never saw -- the expression
    featurize(day=...) computed in torch before the lookup op, written out here."""
    src, day, _, m = _DAYS.get("proxy") or ("proxy", None, None, None)
    if day is None:
        day = _generate("proxy", N_EVENTS, 21)
        m = _model("proxy", _train("proxy", day.cols, SEEDS[0]))
    n, odd = 500, [0, 9, 250, 499]
    cols = _batch(day, n)
    ua = cols["useragent"].to_list()
    for i in odd:
        ua[i] = "never-seen-agent/%d" % i
    cols["useragent"] = StringColumn.from_list(ua)
    tk, tc = torch.from_numpy(m.ua_keys), torch.from_numpy(m.ua_counts)
    words, cuts, table = proxy.featurize(cols, "cpu", None, dns.top_set(TOP), day=(m.cuts, (tk, tc)))
    assert table[0] is tk and cuts is m.cuts
    d = proxy.host_arrays(cols)
    from oni355.ops import strings as sops
    uh, _, _ = sops.string_features(torch.from_numpy(d["useragent.off"]), torch.from_numpy(d["useragent.chars"]))
    pos = torch.searchsorted(tk, uh).clamp_(max=max(tk.numel() - 1, 0))
    hit = tk[pos] == uh
    want = torch.where(hit, tc[pos], 0).clamp(max=2**31 - 1).to(torch.int32).contiguous()
    assert not hit[odd].any() and int((~hit).sum()) == len(odd) and bool((want[odd] == 0).all())
    got, miss = ops.table_lookup(tk, uh.contiguous(), tc)
    assert got.dtype == torch.int32 and torch.equal(got, want) and int(miss) == len(odd)
    bins = ops.bin_keys(want, m.cuts["ua_freq"]).numpy()
    assert np.array_equal((words.numpy() >> 20) & 7, bins) and np.all(bins[odd] == 0)
    r = proxy.score_proxy(cols, m, tol=2.0, maxresults=n, sweeps=2, avg_last=1, top_domains=TOP)
    scored = dict(zip(r.rows.tolist(), r.words.astype(np.int64).tolist()))
    assert all(scored[i] == int(words[i]) for i in range(n))


def test_prior_mass_zero_is_bitwise_the_model_without_profiles(trained):
    src, day, _, m = trained
    cols = _batch(day, 1500)
    kw = dict(maxresults=200, sweeps=4, avg_last=2, seed=101)
    with_docs = _score(src, cols, m, prior_mass=0, **kw)
    stripped = _score(src, cols, m.without_docs(), **kw)
    assert _same(with_docs, stripped)
    assert np.array_equal(with_docs.lda.ndk_sum.numpy(), stripped.lda.ndk_sum.numpy())
    assert with_docs.lda.prior is None and "n_prior_docs" not in with_docs.stats
    on = _score(src, cols, m, prior_mass=5, **kw)
    assert on.stats["n_prior_docs"] == on.stats["D"] > 0 and on.stats["prior_mass"] == 5.0
    assert on.lda.prior is not None and not np.array_equal(on.lda.ndk_sum.numpy(), stripped.lda.ndk_sum.numpy())


@pytest.mark.parametrize("src", ["dns", "proxy"])
def test_cli_save_model_then_model(src, tmp_path):
    from oni355.cli import ml
    lp, md = str(tmp_path / "lp"), str(tmp_path / "models")
    base = ["20160708", src, "1.0", "50", "--synthetic", "3000", "--device", "cpu", "--lpath", lp, "--quiet",
            "--topics", "20"]
    assert ml.main(base + ["--sweeps", "6", "--save-model", md]) == 0
    mp = os.path.join(md, f"{src}_model.npz")
    assert os.path.exists(mp) and SavedModel.load(mp).source == src and SavedModel.load(mp).has_docs
    res = os.path.join(lp, src, "20160708", f"{src}_results.csv")
    os.remove(res)
    assert ml.main(base + ["--model", mp, "--infer-sweeps", "4", "--infer-avg-last", "2", "--infer-prior-mass", "5"]) == 0
    with open(res, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == schema.result_columns(src) and len(rows) == 51
    with open(os.path.join(lp, src, "20160708", "metrics.jsonl")) as f:
        last = json.loads(f.readlines()[-1])
    assert last["mode"] == "infer" and last["n_oov_tokens"] == 0 and last["model_day"] == "20160708"
    assert last["model_sweeps"] == 6 and last["model_top_mismatch"] is False and last["n_prior_docs"] > 0
    # a model of the other source is a usage error, as are the options that train or need several GPUs
    other = "proxy" if src == "dns" else "dns"
    with pytest.raises(SystemExit) as e:
        ml.main(["20160708", other, "--synthetic", "100", "--device", "cpu", "--lpath", lp, "--model", mp])
    assert f"a {src} model cannot score {other} events" in str(e.value.code)
    for extra, msg in ((["--gpus", "2"], "single-GPU"), (["--ckpt-dir", str(tmp_path / "ck")], "--ckpt-dir"),
                       (["--ldac-out", str(tmp_path / "ld")], "--ldac-out")):
        with pytest.raises(SystemExit) as e:
            ml.main(base + ["--model", mp] + extra)
        assert e.value.code not in (0, None) and msg in str(e.value.code)
    assert ml.main(base + ["--sweeps", "4", "--save-model", md, "--no-model-docs"]) == 0
    assert not SavedModel.load(mp).has_docs
