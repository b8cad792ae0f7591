"""Fold-in inference on the CPU: the oracle (oni355/ref/foldin_spec.py) draws from the exact
conditional, its deterministic semantics, multi-chunk documents, the saved model's round trip,
score_flow end to end and the oni-ml --save-model / --model options."""
from __future__ import annotations

import csv
import json
import os
import pickle

import numpy as np
import pytest
import torch
from scipy import stats

from oni355 import ops, schema
from oni355.models.corpus import build_corpus
from oni355.models.foldin import FoldIn
from oni355.models.saved import SavedModel
from oni355.ref import foldin_spec, spec

P_MIN = 1e-4  # the significance level of tests/test_conditional.py


def _np_state(c, phi, KS):
    return dict(tok_word=c.tok_word.numpy().view(np.uint32), tok_z=np.zeros(c.sell_slots, np.uint8),
                slice_off=c.slice_off.numpy(), chunk_doc=c.chunk_doc.numpy(), chunk_pos0=c.chunk_pos0.numpy(),
                chunk_key=c.chunk_key.numpy().view(np.uint32), chunk_multi=c.chunk_multi.numpy(),
                ndk_src=np.zeros((c.D, KS), np.int32), ndk_dst=np.zeros((c.D, KS), np.int32), phi=phi)


def _one_doc(words, G, L=64, V=None):
    w = torch.tensor(words, dtype=torch.int32)
    return build_corpus(torch.zeros(len(words), dtype=torch.int32), w, 1, V or int(max(words)) + 1,
                        torch.tensor([12345], dtype=torch.int32), G, L=L)


@pytest.mark.parametrize("K", [7, 40])
def test_oracle_draws_follow_the_exact_conditional(K):
    """One document, one token looked at (the first of the chunk, drawn from the sweep-start row
    with the token removed), many seeds: p(k) ∝ (n_k^¬t + α)·φ_wk."""
    G, KP = ops.choose_tiling(K)
    KS = G * KP
    r = np.random.default_rng(K)
    c = _one_doc([0, 1, 1], G, V=3)
    phi = np.zeros((3, KS), np.float32)
    phi[:, :K] = (r.random((3, K)) ** 3 + 1e-3).astype(np.float32)
    row = np.zeros(KS, np.int32)
    row[:K] = r.integers(0, 5, K)
    z0 = 2
    row[z0] += 1
    alpha = 0.3
    st = _np_state(c, phi, KS)
    first = int(c.slice_off[0])  # chunk 0, step 0: word 0
    assert st["tok_word"][first] == 0
    n_seeds = 3000
    z = np.empty(n_seeds, np.int64)
    for s in range(n_seeds):
        st["tok_z"][:] = z0
        st["ndk_src"][0] = row
        foldin_spec.foldin_pass(st, G, KP, K, alpha, *spec.split_seed(1000 + s), False, 1, c.chunk_len.numpy())
        z[s] = st["tok_z"][first]
    n = row[:K].astype(np.float64)
    n[z0] -= 1
    p = (n + alpha) * phi[0, :K].astype(np.float64)
    p /= p.sum()
    obs = np.bincount(z, minlength=K)[:K]
    exp = p * n_seeds
    rare = exp < 5
    o, e = np.append(obs[~rare], obs[rare].sum()), np.append(exp[~rare], exp[rare].sum())
    if e[-1] == 0:
        o, e = o[:-1], e[:-1]
    chi2, pv = stats.chisquare(o, e)
    assert pv > P_MIN, (chi2, pv)


def test_a_document_of_one_sided_words_lands_in_that_topic():
    K, G, KP = 2, 1, 4
    phi = np.zeros((2, 4), np.float32)
    phi[0, :2] = np.array([1 - 1e-6, 1e-6], np.float32) / np.float32(1.0)
    phi[1, :2] = 0.5
    c = _one_doc([0] * 64, G, V=2)
    f = FoldIn(c, torch.from_numpy(phi), K, 0.5, seed=7).run(10, 5)
    th = f.theta().numpy()
    assert int(th[0, :K].argmax()) == 0 and th[0, 0] > 0.95
    assert int(f.ndk[0].sum()) == 64 and int(f.ndk_sum[0].sum()) == 64 * 5


def test_an_oov_token_uses_row_V():
    """Word id V indexes the table's last row: with all of its weight on topic 1 there, every OOV
    token lands in topic 1, whatever the in-vocabulary rows say."""
    V, K, G, KP = 3, 2, 1, 4
    table = np.zeros((V + 1, 4), np.float32)
    table[:V, 0] = 1.0
    table[V, 1] = 1.0
    c = _one_doc([0, V, 1, V, 2, V], G, V=V + 1)
    f = FoldIn(c, torch.from_numpy(table), K, 0.5, seed=3).run(3, 1)
    live = c.tok_word != -1
    assert np.array_equal(f.tok_z[live].numpy(), (c.tok_word[live] == V).numpy().astype(np.uint8))


def test_init_pass_is_a_sweep_without_the_decrement():
    """3-token chunk by hand: token t is drawn from (n_so_far + α)·φ_w with the pinned fma chain."""
    K, G, KP, alpha = 3, 1, 4, 0.25
    phi = np.zeros((2, 4), np.float32)
    phi[:, :3] = np.array([[0.2, 0.5, 0.3], [0.6, 0.1, 0.3]], np.float32)
    c = _one_doc([0, 1, 1], G, V=2)
    st = _np_state(c, phi, 4)
    s0, s1 = spec.split_seed(99)
    foldin_spec.foldin_pass(st, G, KP, K, alpha, s0, s1, True, 0, c.chunk_len.numpy())
    n = np.zeros(4, np.int32)
    off = int(c.slice_off[0])
    for t, w in enumerate([0, 1, 1]):
        rr = spec.token_rand(np.array([t], np.uint32), np.array([12345], np.uint32), 0, 2, s0, s1)
        run, cum = np.float32(0), []
        for j in range(4):
            run = spec.fma_f32(np.array([np.float32(n[j]) + np.float32(alpha)]), phi[w, j:j + 1], np.array([run]))[0]
            cum.append(run)
        thr = spec.u01(rr)[0] * cum[-1]
        zn = min(sum(x <= thr for x in cum), K - 1)
        assert st["tok_z"][off + t * 64] == zn
        n[zn] += 1
    assert np.array_equal(st["ndk_dst"][0], n)
    # the same state through a sweep-style pass over zeroed rows with nothing to remove is not
    # expressible (a sweep removes a counted token); the init pass IS that code minus the decrement:
    # a second init pass from the same seed reproduces it bit for bit
    st2 = _np_state(c, phi, 4)
    foldin_spec.foldin_pass(st2, G, KP, K, alpha, s0, s1, True, 0, c.chunk_len.numpy())
    assert np.array_equal(st2["tok_z"], st["tok_z"])


def test_a_document_cut_into_three_chunks():
    K = 12
    G, KP = ops.choose_tiling(K)
    L = 6
    r = np.random.default_rng(5)
    lens = [2 * L + 2, 3, L]  # doc 0: 3 chunks
    tdoc = np.repeat(np.arange(3), lens)
    tword = r.integers(0, 9, tdoc.size)
    c = build_corpus(torch.from_numpy(tdoc).to(torch.int32), torch.from_numpy(tword).to(torch.int32), 3, 9,
                     torch.tensor([5, 6, 7], dtype=torch.int32), G, L=L)
    assert int(c.chunk_multi.sum()) == 3
    phi = np.zeros((9, KP), np.float32)
    phi[:, :K] = r.random((9, K)).astype(np.float32)
    f = FoldIn(c, torch.from_numpy(phi), K, 0.4, seed=11)
    sums = np.zeros((3, KP), np.int64)
    S = 64 // G
    for sweeps in range(1, 5):
        f.run(sweeps, 2)
        # n_dk after the sweep = the counts of the document's tokens over all of its chunks
        want = np.zeros((3, KP), np.int64)
        cd, cl, so = c.chunk_doc.numpy(), c.chunk_len.numpy(), c.slice_off.numpy()
        for i in np.nonzero(cd >= 0)[0]:
            z = f.tok_z.numpy()[so[i // S] + i % S + np.arange(cl[i]) * S]
            np.add.at(want[cd[i]], z, 1)
        assert np.array_equal(f.ndk.numpy(), want)
        assert f.launches == {"init": 1, "sweep": 1, "multi_sweep": sweeps}
    # the window sum = Σ of the rows after the last two sweeps (the chain is a pure function of the
    # seed: a run of 3 sweeps ends where the third sweep of a 4-sweep run does)
    f.run(3, 1)
    third = f.ndk.numpy().copy()
    f.run(4, 1)
    fourth = f.ndk.numpy().copy()
    f.run(4, 2)
    assert np.array_equal(f.ndk_sum.numpy(), third + fourth)
    # and the op's own path equals the plain oracle run
    st = _np_state(c, phi, KP)
    ws, wn = foldin_spec.foldin_run(st, G, KP, K, 0.4, *spec.split_seed(11), 4, 2, c.chunk_len.numpy())
    assert np.array_equal(ws, f.ndk_sum.numpy()) and np.array_equal(wn, f.ndk.numpy())
    assert np.array_equal(st["tok_z"], f.tok_z.numpy())


# ---- saved model, score_flow, CLI ---------------------------------------------------------------
N_TOP = 100
# top-100 overlap of two run_flow trainings of the day below (K = 20, 12 sweeps) that differ only in
# their seed, over the seed pairs (101,202) (202,303) (303,404) (404,505) (505,606): the noise
# floor fold-in scoring of that day must not fall under (docs/foldin.md)
FLOOR = [0.30, 0.24, 0.37, 0.21, 0.29]


@pytest.fixture(scope="module")
def trained():
    from oni355.pipeline.flow import run_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(5000, seed=21)
    res = run_flow(dict(day.cols), K=20, sweeps=12, maxresults=N_TOP, device="cpu", seed=101)
    return day, res


def test_saved_model_round_trip(trained, tmp_path):
    _, res = trained
    m = SavedModel.from_run(res.lda, res.cuts, "flow", {"day": "20160708"})
    p = m.save(str(tmp_path / "flow_model.npz"))
    m2 = SavedModel.load(p)
    for k in ("vocab", "phi", "phi_oov"):
        a, b = getattr(m, k), getattr(m2, k)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for k in ("time", "ibyt", "ipkt"):
        assert m.cuts[k].dtype == np.uint32 and m.cuts[k].tobytes() == m2.cuts[k].tobytes()
    assert (m2.source, m2.K, m2.alpha, m2.beta) == (m.source, m.K, m.alpha, m.beta)
    assert m2.provenance["day"] == "20160708" and m2.provenance["sweeps"] == 12 and m2.provenance["seed"] == 101
    # φ is the training run's estimate; phi_oov = β/(n_k + Vβ) from the same (S-scaled) sums
    lda = res.lda.model
    assert np.array_equal(m.phi, lda.phi()[:, :20].numpy())
    a = lda._avg
    assert lda._averaged() is not None and a["n"] >= 2
    S = np.float32(a["n"])
    den = a["k"][:20].numpy().astype(np.float32) + np.float32(S * np.float32(lda.vbeta))
    assert np.array_equal(m.phi_oov, (np.float32(float(S) * lda.beta) / den).astype(np.float32))
    assert np.allclose(m.phi_oov, lda.beta / (a["k"][:20].numpy() / float(S) + lda.V * lda.beta), rtol=1e-5)
    t = m2.table(1, 20, "cpu")
    assert t.shape == (m.V + 1, 20) and np.array_equal(t[m.V].numpy(), m.phi_oov)
    # no pickle: an npz holding an object array is refused
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, meta=np.array([{"format": 1}], dtype=object), vocab=m.vocab)
    with pytest.raises(ValueError):
        SavedModel.load(bad)
    with open(str(tmp_path / "bad.pkl"), "wb") as f:
        pickle.dump({"phi": 1}, f)
    with pytest.raises(Exception):
        SavedModel.load(str(tmp_path / "bad.pkl"))


def test_score_flow_end_to_end(trained, tmp_path):
    from oni355.io import results as rio
    from oni355.pipeline.flow import score_flow
    from oni355.synth.flow import generate_flows
    day, res = trained
    m = SavedModel.load(SavedModel.from_run(res.lda, res.cuts, "flow").save(str(tmp_path / "m.npz")))
    r = score_flow(dict(day.cols), m, maxresults=N_TOP, device="cpu", seed=101)
    assert r.stats["mode"] == "infer" and r.stats["n_oov_tokens"] == 0
    assert len(r.rows) == N_TOP and np.all(np.diff(r.scores) >= 0) and isinstance(r.lda, FoldIn)
    assert np.array_equal(r.scores, np.minimum(r.src_scores, r.dst_scores))
    out = rio.write_rendered(str(tmp_path / "flow_results.csv"), schema.result_columns("flow"),
                             rio.render_result("flow", dict(day.cols), r, 0, None))
    header, rows = rio.read_csv(out)
    assert header == schema.FLOW_RESULT_COLUMNS and len(rows) == N_TOP
    assert [float(x[-1]) for x in rows] == sorted(float(x[-1]) for x in rows)
    # quality: the same day scored against its own model agrees with the training run's top-N at
    # least as well as two trainings with different seeds agree with each other
    overlap = len(set(r.rows.tolist()) & set(res.rows.tolist())) / N_TOP
    print("fold-in overlap", overlap, "floor", FLOOR)
    assert overlap >= min(FLOOR)
    # another day: tokens are out of vocabulary exactly when their word is absent from the model
    other = generate_flows(5000, seed=22)
    r2 = score_flow(dict(other.cols), m, maxresults=N_TOP, device="cpu", sweeps=4, avg_last=2)
    d = {k: torch.from_numpy(np.asarray(v).view(np.int32) if np.asarray(v).dtype == np.uint32 else np.asarray(v))
         for k, v in other.cols.items() if k in ("trhour", "trminute", "trsec", "ibyt", "ipkt", "sport", "dport")}
    tk, bk, pk = spec.flow_keys(d["trhour"].numpy(), d["trminute"].numpy(), d["trsec"].numpy(),
                                d["ibyt"].numpy().astype(np.int64), d["ipkt"].numpy().astype(np.int64))
    sw, dw = spec.flow_wordify(d["sport"].numpy(), d["dport"].numpy(), tk, bk, pk, m.cuts["time"], m.cuts["ibyt"],
                               m.cuts["ipkt"])
    words = np.concatenate([sw, dw]).astype(np.int64)
    absent = np.setdiff1d(words, m.vocab)
    assert r2.stats["n_oov_tokens"] == int(np.isin(words, absent).sum())
    assert (r2.stats["n_oov_tokens"] > 0) == (absent.size > 0)


def test_score_flow_refuses_a_process_group():
    from oni355.pipeline.flow import score_flow

    class _Comm:
        dist = True
    with pytest.raises(NotImplementedError, match="fold-in scoring is single-GPU"):
        score_flow({}, None, comm=_Comm())


def test_cli_save_model_then_model(tmp_path, capsys):
    from oni355.cli import ml
    lp, md = str(tmp_path / "lp"), str(tmp_path / "models")
    base = ["20160708", "flow", "1.0", "50", "--synthetic", "6000", "--device", "cpu", "--lpath", lp, "--quiet"]
    assert ml.main(base + ["--sweeps", "8", "--save-model", md]) == 0
    mp = os.path.join(md, "flow_model.npz")
    assert os.path.exists(mp)
    res = os.path.join(lp, "flow", "20160708", "flow_results.csv")
    os.remove(res)
    assert ml.main(base + ["--model", mp, "--infer-sweeps", "6", "--infer-avg-last", "3"]) == 0
    with open(res, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == schema.FLOW_RESULT_COLUMNS and len(rows) == 51
    with open(os.path.join(lp, "flow", "20160708", "metrics.jsonl")) as f:
        last = json.loads(f.readlines()[-1])
    assert last["mode"] == "infer" and last["n_oov_tokens"] == 0 and last["model_day"] == "20160708"
    assert last["model_sweeps"] == 8
    for extra, msg in ((["--gpus", "2"], "single-GPU"), (["--ckpt-dir", str(tmp_path / "ck")], "--ckpt-dir"),
                       (["--ldac-out", str(tmp_path / "ld")], "--ldac-out")):
        with pytest.raises(SystemExit) as e:
            ml.main(base + ["--model", mp] + extra)
        assert e.value.code not in (0, None) and msg in str(e.value.code)
    for src in ("dns", "proxy"):
        with pytest.raises(SystemExit) as e:
            ml.main(["20160708", src, "--synthetic", "100", "--device", "cpu", "--lpath", lp, "--model", mp])
        assert "per-day dictionaries" in str(e.value.code)
