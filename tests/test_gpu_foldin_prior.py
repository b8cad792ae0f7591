"""The PRIOR instantiations of k_foldin, k_prior_rows (csrc/kernels/foldin.hip) and
k_theta_rows_prior (csrc/kernels/day_tail.hip) against their oracles (oni355/ref/foldin_spec.py),
bit for bit, on the hand-built corpus of tests/test_gpu_foldin.py (its helpers are copied here):
≤ 4k tokens, about 340 documents, 64 words + the out-of-vocabulary row, chunk length 10, α = 0.7,
3-chunk documents sharing a slice with single-chunk ones, a 1-token document, dead lanes.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.models.corpus import build_corpus
from oni355.models.foldin import FoldIn
from oni355.ref import foldin_spec, spec

pytestmark = pytest.mark.gpu

V = 64          # model words; id V = out of vocabulary
L = 10          # chunk length: no multiple of 4
SEED = 0x5EED1234
ALPHA = 0.7     # n + α not exact in f32: the kernel must add at use, as the oracle does
TILINGS = {12: (1, 12), 20: (1, 20), 50: (2, 28), 100: (4, 28), 128: (8, 16)}
MULTI_DOCS = (3, 8)  # the two 3-chunk documents of _corpus
F32 = np.float32
V6 = foldin_spec.V6_KEY_BASE


@functools.lru_cache(maxsize=None)
def _corpus(G: int, multi: bool = True):
    """Docs 0-2 and 4-6 hold exactly L tokens, doc 3 (``multi``) 2L + 3 tokens in 3 chunks between
    them; doc 7 has one token; a second 3-chunk document and ~330 short ones follow. Every unit
    width leaves the last slice with dead lanes for this chunk count."""
    r = np.random.default_rng(77)
    lens = [L, L, L, 2 * L + 3 if multi else L, L, L, L, 1]
    lens += [3 * L if multi else L - 1]
    lens += r.integers(1, L + 1, 330).tolist()
    D = len(lens)
    tdoc = np.repeat(np.arange(D), lens)
    tword = (r.zipf(1.3, tdoc.size) - 1) % V
    tword[r.random(tdoc.size) < 0.06] = V  # OOV tokens
    tword[0] = V
    keys = torch.arange(D, dtype=torch.int32) * 2654435 + 17
    c = build_corpus(torch.from_numpy(tdoc).to(torch.int32), torch.from_numpy(tword).to(torch.int32), D, V + 1, keys,
                     G, L=L)
    assert c.T <= 4000 and (c.chunk_doc < 0).any() and bool(c.chunk_multi.any()) == multi
    assert int((c.chunk_len == L).sum()) >= 6 and int((c.doc_lengths() == 1).sum()) >= 1
    if multi:
        assert sorted(c.long_rows.tolist()) == list(MULTI_DOCS)
    return c


def _to(c, dev):
    return dataclasses.replace(c, **{f.name: getattr(c, f.name).to(dev) for f in dataclasses.fields(c)
                                     if isinstance(getattr(c, f.name), torch.Tensor)})


def _table(K: int, KS: int) -> np.ndarray:
    r = np.random.default_rng(K)
    t = np.zeros((V + 1, KS), np.float32)
    t[:, :K] = (r.random((V + 1, K)) ** 4 + 1e-7).astype(np.float32)
    t[:V, :K] /= t[:V, :K].sum(0, keepdims=True)
    t[V, :K] = np.float32(1e-4) / (1 + np.arange(K, dtype=np.float32))
    return t


def _prior(D: int, K: int, KS: int) -> np.ndarray:
    """Rows 0.7 + m·θ (not exact in f32) with m ∈ {1, 37.5, 1000} and θ from a seeded Dirichlet;
    about a third of the documents stay at α; both 3-chunk documents carry a non-flat row."""
    r = np.random.default_rng(1000 + K)
    th = r.dirichlet(np.full(K, 0.3), D).astype(F32)
    m = np.array([1.0, 37.5, 1000.0], F32)[r.integers(0, 3, D)]
    pr = np.full((D, KS), F32(ALPHA))
    pr[:, :K] = spec.fma_f32(np.broadcast_to(m[:, None], th.shape), th, np.full(th.shape, F32(ALPHA)))
    flat = r.random(D) < 1 / 3
    flat[list(MULTI_DOCS)] = False
    pr[flat] = F32(ALPHA)
    assert 0.2 < flat.mean() < 0.45 and all(pr[d, :K].max() > pr[d, :K].min() for d in MULTI_DOCS)
    return pr


@functools.lru_cache(maxsize=None)
def _oracle(G, KP, K, sweeps, avg_last, multi=True, prior="bent"):
    """(tok_z, ndk, ndk_sum, prior) of the oracle run, computed once per case and only read."""
    KS = G * KP
    c = _corpus(G, multi)
    pr = {"bent": _prior(c.D, K, KS), "flat": np.full((c.D, KS), F32(ALPHA)), None: None}[prior]
    st = dict(tok_word=c.tok_word.numpy().view(np.uint32), tok_z=np.zeros(c.sell_slots, np.uint8),
              slice_off=c.slice_off.numpy(), chunk_doc=c.chunk_doc.numpy(), chunk_pos0=c.chunk_pos0.numpy(),
              chunk_key=c.chunk_key.numpy().view(np.uint32), chunk_multi=c.chunk_multi.numpy(),
              ndk_src=np.zeros((c.D, KS), np.int32), ndk_dst=np.zeros((c.D, KS), np.int32), phi=_table(K, KS))
    s0, s1 = spec.split_seed(SEED)
    ndk_sum, ndk = foldin_spec.foldin_run(st, G, KP, K, ALPHA, s0, s1, sweeps, avg_last, c.chunk_len.numpy(), prior=pr)
    for a in (st["tok_z"], ndk, ndk_sum):
        a.setflags(write=False)
    return st["tok_z"], ndk, ndk_sum, pr


def _check(gpu, K, sweeps, avg_last, fuse=True, prior="bent"):
    G, KP = ops.choose_tiling(K)
    assert (G, KP) == TILINGS[K]
    c = _corpus(G)
    want_z, want_n, want_sum, pr = _oracle(G, KP, K, sweeps, avg_last, prior=prior)
    f = FoldIn(_to(c, gpu), torch.from_numpy(_table(K, G * KP)).to(gpu), K, ALPHA, SEED, fuse=fuse,
               prior=torch.from_numpy(pr).to(gpu)).run(sweeps, avg_last)
    assert np.array_equal(f.tok_z.cpu().numpy(), want_z)
    assert np.array_equal(f.ndk.cpu().numpy(), want_n)
    assert np.array_equal(f.ndk_sum.cpu().numpy(), want_sum)
    assert int(want_n.sum()) == c.T and int(want_sum.sum()) == c.T * f.samples
    return f


@pytest.mark.parametrize("sweeps,avg_last", [(1, 1), (5, 3)])
@pytest.mark.parametrize("K", sorted(TILINGS))
def test_device_replays_the_oracle_with_a_prior(gpu, K, sweeps, avg_last):
    f = _check(gpu, K, sweeps, avg_last)
    assert f.launches == {"init": 1, "sweep": 1, "multi_sweep": sweeps}
    G, KP = TILINGS[K]
    # the prior is what made these draws: the flat chain differs
    assert not np.array_equal(_oracle(G, KP, K, sweeps, avg_last, prior=None)[1], _oracle(G, KP, K, sweeps, avg_last)[1])
    # θ of the run: the device kernel against its oracle
    want = foldin_spec.theta_rows_prior(f.ndk_sum.cpu().numpy(), f.prior.cpu().numpy(), K, float(f.samples))
    assert np.array_equal(f.theta().cpu().numpy(), want)


@pytest.mark.parametrize("K", [20, 100])
def test_an_all_alpha_prior_is_the_flat_prior(gpu, K):
    """tok_z, ndk and ndk_sum only: the two θ expressions round differently by design."""
    G, KP = TILINGS[K]
    f = _check(gpu, K, 5, 3, prior="flat")
    c = _corpus(G)
    g = FoldIn(_to(c, gpu), torch.from_numpy(_table(K, G * KP)).to(gpu), K, ALPHA, SEED).run(5, 3)
    for k in ("tok_z", "ndk", "ndk_sum"):
        assert torch.equal(getattr(f, k), getattr(g, k))
    assert f.launches == g.launches
    want = _oracle(G, KP, K, 5, 3, prior=None)
    assert np.array_equal(g.tok_z.cpu().numpy(), want[0]) and np.array_equal(g.ndk_sum.cpu().numpy(), want[2])


@pytest.mark.parametrize("K", [20, 100])
def test_unfused_launches_draw_the_same_with_a_prior(gpu, K):
    f = _check(gpu, K, 5, 3, fuse=False)
    assert f.launches == {"init": 1, "sweep": 5, "multi_sweep": 5}


def test_init_only_with_a_prior(gpu):
    f = _check(gpu, 20, 0, 10)
    assert f.samples == 1 and f.launches == {"init": 1, "sweep": 0, "multi_sweep": 0}


@pytest.mark.parametrize("K", [20, 100])
def test_dead_units_read_no_prior_row(gpu, K):
    """A launch's dead units (chunks outside its selection -- a run launches ``select`` 1 and 2 --
    and padding chunks, whose document is −1) use no prior row: the prior table is a view behind
    sentinel rows of NaN (row −1 of the view is one), the doc tables behind sentinel rows of −7, and
    the results stay those of the oracle."""
    G, KP = TILINGS[K]
    KS = G * KP
    c = _corpus(G)
    want_z, want_n, want_sum, pr = _oracle(G, KP, K, 3, 2)
    big = torch.full((c.D + 2, KS), float("nan"), dtype=torch.float32, device=gpu)
    big[1:-1] = torch.from_numpy(pr).to(gpu)
    f = FoldIn(_to(c, gpu), torch.from_numpy(_table(K, KS)).to(gpu), K, ALPHA, SEED, prior=big[1:-1])
    assert f.prior.data_ptr() == big[1:-1].data_ptr()
    rows = [torch.full((c.D + 2, KS), -7, dtype=torch.int32, device=gpu) for _ in range(3)]
    f.ndk, f.ndk_sum, f._alt = (b[1:-1] for b in rows)
    f.run(3, 2)
    assert f.launches == {"init": 1, "sweep": 1, "multi_sweep": 3}
    for b in rows:
        assert bool((b[0] == -7).all()) and bool((b[-1] == -7).all())
    assert bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[-1]).all())
    assert np.array_equal(f.tok_z.cpu().numpy(), want_z)
    assert np.array_equal(f.ndk.cpu().numpy(), want_n)
    assert np.array_equal(f.ndk_sum.cpu().numpy(), want_sum)


def test_uninstantiated_tiling_with_a_prior_is_an_error(gpu):
    c = _to(_corpus(2, multi=False), gpu)
    KS = 24  # (2, 12): choose_tiling never returns it
    f = FoldIn(c, torch.zeros(V + 1, KS, device=gpu), 24, ALPHA, SEED,
               prior=torch.full((c.D, KS), ALPHA, dtype=torch.float32, device=gpu))
    with pytest.raises(RuntimeError, match="oni_foldin_launch"):
        f.run(1, 1)


def _small_prior_case():
    """tests/test_foldin_prior_cpu.py small_prior_case: 6 model documents, 9 batch keys."""
    K, KS, alpha, mass = 5, 8, 0.7, 50.0
    mkeys = np.array([10, 20, 30, 40, 50, V6 + 3], np.int64)
    tokens = np.array([3, 100, 7, 49, 51, 500], np.int64)
    theta = np.random.default_rng(6).dirichlet(np.full(K, 0.3), 6).astype(F32)
    batch = np.array([5, 10, 15, 20, 40, 50, 60, V6 + 3, V6 + 9], np.int64)
    return mkeys, theta, tokens, batch, K, KS, alpha, mass


def _big_prior_case():
    """340 batch documents against 500 model documents, [340, 56]: about half are known, token counts
    on both sides of the mass, keys up to and past the IPv6 base, K < KS."""
    r = np.random.default_rng(340)
    K, KS, alpha, mass = 50, 56, 0.7, 37.5
    mkeys = np.unique(np.concatenate([r.integers(0, 2 ** 32 - 1, 480), V6 + np.arange(20)])).astype(np.int64)
    Dm = mkeys.shape[0]
    tokens = r.integers(1, 80, Dm).astype(np.int64)
    tokens[0] = 2 ** 40  # f32(tokens) is taken before the min
    theta = r.dirichlet(np.full(K, 0.3), Dm).astype(F32)
    batch = np.unique(np.concatenate([r.choice(mkeys, 170, replace=False), r.integers(0, 2 ** 32 - 1, 170),
                                      mkeys[:1], mkeys[-1:], [0, 2 ** 32 - 1]]))[:340].astype(np.int64)
    return mkeys, theta, tokens, batch, K, KS, alpha, mass


@pytest.mark.parametrize("case", [_small_prior_case, _big_prior_case])
def test_prior_rows_kernel_equals_its_oracle(gpu, case):
    mkeys, theta, tokens, batch, K, KS, alpha, mass = case()
    want = foldin_spec.prior_rows(mkeys, theta, tokens, batch, K, KS, alpha, mass)
    known = (want[:, :K] != F32(alpha)).any(1)
    assert known.any() and (~known).any() and np.isfinite(want).all()
    assert np.all(want[batch >= V6] == F32(alpha)) and np.isin(batch[batch >= V6], mkeys).any()
    dev = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    got = ops.prior_rows(dev(mkeys), dev(theta), dev(tokens), dev(batch), K, KS, alpha, mass)
    assert got.dtype == torch.float32 and got.shape == (batch.shape[0], KS)
    assert np.array_equal(got.cpu().numpy(), want)
    # a model without documents: every row is α
    e = ops.prior_rows(dev(mkeys[:0]), dev(theta[:0]), dev(tokens[:0]), dev(batch), K, KS, alpha, mass)
    assert bool((e == F32(alpha)).all())


@pytest.mark.parametrize("D,K,KS,dtype", [(9, 5, 8, torch.int32), (340, 50, 56, torch.int32), (340, 20, 20, torch.int64)])
def test_theta_rows_prior_kernel_equals_its_oracle(gpu, D, K, KS, dtype):
    r = np.random.default_rng(D + K)
    n = np.zeros((D, KS), np.int64)
    n[:, :K] = r.integers(0, 3000, (D, K))
    n[0] = 0               # an empty document
    n[1, :K] = 2 ** 24 + 1  # a count f32 cannot hold
    pr = np.full((D, KS), F32(ALPHA))
    pr[:, :K] = (F32(ALPHA) + F32(37.5) * r.dirichlet(np.full(K, 0.3), D).astype(F32)).astype(F32)
    nt = torch.from_numpy(n).to(dtype)
    want = foldin_spec.theta_rows_prior(nt.numpy(), pr, K, 3.0)
    got = ops.theta_rows_prior(nt.to(gpu), torch.from_numpy(pr).to(gpu), K, 3.0)
    assert np.array_equal(got.cpu().numpy(), want) and not want[:, K:].any()


def test_score_flow_with_a_prior_gpu_matches_cpu(gpu, tmp_path):
    from oni355.models.saved import SavedModel
    from oni355.pipeline.flow import run_flow, score_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(5000, seed=21)
    tr = run_flow(dict(day.cols), K=20, sweeps=8, maxresults=100, device="cpu")
    m = SavedModel.load(SavedModel.from_run(tr.lda, tr.cuts, "flow").save(str(tmp_path / "m.npz")))
    assert m.has_docs
    other = generate_flows(5000, seed=22)  # a day with unseen words
    kw = dict(maxresults=200, sweeps=6, avg_last=3, prior_mass=50)
    rc = score_flow(dict(other.cols), m, device="cpu", **kw)
    rg = score_flow(dict(other.cols), m, device=gpu, **kw)
    assert rc.stats["n_prior_docs"] == rg.stats["n_prior_docs"] > 0 and rg.stats["prior_mass"] == 50.0
    assert np.array_equal(rc.lda.prior.numpy(), rg.lda.prior.cpu().numpy())
    assert np.array_equal(rc.lda.ndk_sum.numpy(), rg.lda.ndk_sum.cpu().numpy())
    assert np.array_equal(rc.lda.theta().numpy(), rg.lda.theta().cpu().numpy())
    assert np.array_equal(rc.rows, rg.rows)
    assert np.array_equal(rc.scores, rg.scores)
    assert np.array_equal(rc.src_scores, rg.src_scores) and np.array_equal(rc.dst_scores, rg.dst_scores)
