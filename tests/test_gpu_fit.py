"""ops.doc_fit on the device (csrc/kernels/fit.hip) against the fsum / long-double reference of
tests/fit_inputs.py, bit-identical across runs and grids; score_flow(fit=True) against the CPU path."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fit_inputs as fx
from oni355 import ops

pytestmark = pytest.mark.gpu

PAIRS = fx.pair_list()


def _run(gpu, th, tb, pairs=PAIRS, **kw):
    pd, pw, pc, D = pairs
    out = ops.doc_fit(*(torch.from_numpy(x).to(gpu) for x in (th, tb, pd, pw, pc)), D, fx.V, **kw)
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("KS", [4, 20, 56, 112])
def test_doc_fit_against_the_reference(gpu, KS):
    pd, pw, pc, D = PAIRS
    th, tb = fx.model(KS, D)
    out = _run(gpu, th, tb)
    fx.check(out, fx.reference(th, tb, pd, pw, pc, D), D)
    ps = ops.pair_score(*(torch.from_numpy(x).to(gpu) for x in (th, tb, pd, pw))).cpu().numpy()
    want = np.full(D, np.inf, np.float32)
    np.minimum.at(want, pd, ps)
    assert out[3].tobytes() == want.tobytes()
    # same bits from a second run and from a grid of 3 blocks (every block takes many rounds)
    for kw in ({}, {"grid": 3}):
        assert [x.tobytes() for x in _run(gpu, th, tb, **kw)] == [x.tobytes() for x in out]


def test_no_pairs(gpu):
    th, tb = fx.model(20, 300)
    e = np.zeros(0, np.int32)
    ll, tok, oov, mn, tot = _run(gpu, th, tb, (e, e, e, 300))
    assert not ll.any() and not tok.any() and not oov.any() and np.all(np.isposinf(mn)) and not tot.any()


def test_a_zero_table_row_gives_minus_inf(gpu):
    D = PAIRS[3]
    th, tb = fx.model(20, D)
    base = _run(gpu, th, tb)
    tb[fx.V - 1] = 0
    ll, _, _, mn, tot = _run(gpu, th, tb)
    others = np.arange(D) != fx.ZERO_DOC
    assert np.isneginf(ll[fx.ZERO_DOC]) and mn[fx.ZERO_DOC] == 0 and np.isneginf(tot[0])
    assert np.all(np.isfinite(ll[others])) and ll[others].tobytes() == base[0][others].tobytes()


def test_score_flow_fit_on_the_gpu_equals_the_cpu_path(gpu):
    from oni355.models.saved import SavedModel
    from oni355.pipeline.flow import run_flow, score_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(5000, seed=21)
    res = run_flow(dict(day.cols), K=20, sweeps=12, maxresults=100, device=gpu, seed=101)
    m = SavedModel.from_run(res.lda, res.cuts, "flow")
    g = score_flow(dict(day.cols), m, maxresults=100, device=gpu, seed=101, fit=True)
    c = score_flow(dict(day.cols), m, maxresults=100, device="cpu", seed=101, fit=True)
    assert g.timings["fit_dev_s"] > 0 and np.array_equal(g.rows, c.rows) and g.scores.tobytes() == c.scores.tobytes()
    gf, cf = g.fit, c.fit
    assert all(torch.equal(getattr(gf, k).cpu(), getattr(cf, k)) for k in ("doc_keys", "tokens", "oov_tokens"))
    assert gf.min_score.cpu().numpy().tobytes() == cf.min_score.numpy().tobytes()
    # the tolerance of fit_inputs.reference: all terms of a document have one sign, Σ c·|log s| = |ll|
    ll_g, ll_c = gf.loglik.cpu().numpy(), cf.loglik.numpy()
    npairs = np.diff(c.lda.c.doc_pair_ptr.numpy())
    tol = (4 + np.ceil(np.log2(np.maximum(npairs, 2)))) * 2.0**-52 * np.abs(ll_c)
    print("max |gpu - cpu| / tol:", float(np.max(np.abs(ll_g - ll_c) / tol)))
    assert np.all(np.abs(ll_g - ll_c) <= tol)
    assert abs(g.stats["batch_loglik"] - c.stats["batch_loglik"]) <= \
        (4 + np.ceil(np.log2(npairs.sum()))) * 2.0**-52 * abs(c.stats["batch_loglik"])
    assert (g.stats["batch_tokens"], g.stats["batch_oov_tokens"]) == (c.stats["batch_tokens"], c.stats["batch_oov_tokens"])
