"""k_foldin (csrc/kernels/foldin.hip) against its oracle (oni355/ref/foldin_spec.py), bit for bit
on tok_z, ndk and ndk_sum, for the dense tilings (1,12), (1,20), (2,28), (4,28), (8,16), and for
(4,8) and (16,8) of the training samplers' table, which ops.choose_tiling never returns.

The corpus is hand-built (≤ 4k tokens, 64 words + the out-of-vocabulary row) with the shapes where
the kernel can go wrong: a 1-token document, chunks of exactly the chunk length, a chunk length
that is no multiple of 4, 3-chunk documents sharing a slice with single-chunk ones, a slice with
dead lanes, OOV tokens and K < KS padding.
"""
from __future__ import annotations

import dataclasses

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


def _corpus(G: int, multi: bool = True):
    """Docs 0-2 and 4-6 hold exactly L tokens, doc 3 (``multi``) 2L + 3 tokens in 3 chunks between
    them (stable length sort: its full chunks sit among theirs in the first slice); doc 7 has one
    token; a second 3-chunk document and ~330 short ones follow. 8-lane units (8 chunks a slice)
    leave the last slice with dead lanes for this chunk count; so do the other widths."""
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


def _oracle(c, table, G, KP, K, sweeps, avg_last):
    KS = G * KP
    st = dict(tok_word=c.tok_word.numpy().view(np.uint32), tok_z=np.zeros(c.sell_slots, np.uint8),
              slice_off=c.slice_off.numpy(), chunk_doc=c.chunk_doc.numpy(), chunk_pos0=c.chunk_pos0.numpy(),
              chunk_key=c.chunk_key.numpy().view(np.uint32), chunk_multi=c.chunk_multi.numpy(),
              ndk_src=np.zeros((c.D, KS), np.int32), ndk_dst=np.zeros((c.D, KS), np.int32), phi=table)
    s0, s1 = spec.split_seed(SEED)
    ndk_sum, ndk = foldin_spec.foldin_run(st, G, KP, K, ALPHA, s0, s1, sweeps, avg_last, c.chunk_len.numpy())
    return st["tok_z"], ndk, ndk_sum


def _check(gpu, K, sweeps, avg_last, fuse=True, multi=True, tiling=None):
    G, KP = tiling or ops.choose_tiling(K)
    assert tiling or (G, KP) == TILINGS[K]
    c = _corpus(G, multi)
    table = _table(K, G * KP)
    want_z, want_n, want_sum = _oracle(c, table, G, KP, K, sweeps, avg_last)
    f = FoldIn(_to(c, gpu), torch.from_numpy(table).to(gpu), K, ALPHA, SEED, fuse=fuse).run(sweeps, avg_last)
    assert np.array_equal(f.tok_z.cpu().numpy(), want_z)
    assert np.array_equal(f.ndk.cpu().numpy(), want_n)
    assert np.array_equal(f.ndk_sum.cpu().numpy(), want_sum)
    assert int(want_n.sum()) == c.T and int(want_sum.sum()) == c.T * f.samples
    return f


# n_sweeps 1, 2 and 5 fused; the window from the first, a middle and the last sweep
@pytest.mark.parametrize("sweeps,avg_last", [(1, 1), (2, 2), (5, 5), (5, 3), (5, 1)])
@pytest.mark.parametrize("K", sorted(TILINGS))
def test_device_replays_the_oracle(gpu, K, sweeps, avg_last):
    f = _check(gpu, K, sweeps, avg_last)
    assert f.launches == {"init": 1, "sweep": 1, "multi_sweep": sweeps}


# tilings of the training samplers' table that choose_tiling never returns (the widest units among
# them): the corpus is built for that G explicitly, K < KS
@pytest.mark.parametrize("G,KP,K", [(4, 8, 30), (16, 8, 120)])
def test_table_tilings_choose_tiling_never_picks(gpu, G, KP, K):
    assert all(ops.choose_tiling(k) != (G, KP) for k in range(1, 256))
    c = _corpus(G)
    start = c.chunk_pos0[c.chunk_doc >= 0]
    assert bool(c.chunk_multi.any()) and bool((start % 4 != 0).any())
    f = _check(gpu, K, 2, 2, tiling=(G, KP))
    assert f.launches == {"init": 1, "sweep": 1, "multi_sweep": 2}


@pytest.mark.parametrize("K", [20, 100])
def test_unfused_launches_draw_the_same(gpu, K):
    f = _check(gpu, K, 5, 3, fuse=False)
    assert f.launches["sweep"] == 5


@pytest.mark.parametrize("K", [12, 50])
def test_no_multi_chunk_document_takes_one_sweep_launch(gpu, K):
    f = _check(gpu, K, 5, 2, multi=False)
    assert f.launches == {"init": 1, "sweep": 1, "multi_sweep": 0}


@pytest.mark.parametrize("K", [20, 100])
def test_deselected_chunks_touch_no_row(gpu, K):
    """A launch's dead units (chunks outside its selection, padding chunks) read and write no doc
    row: the tables are views behind a sentinel row that must survive every launch."""
    G, KP = ops.choose_tiling(K)
    c = _corpus(G)
    f = FoldIn(_to(c, gpu), torch.from_numpy(_table(K, G * KP)).to(gpu), K, ALPHA, SEED)
    big = [torch.full((c.D + 2, G * KP), -7, dtype=torch.int32, device=gpu) for _ in range(3)]
    f.ndk, f.ndk_sum, f._alt = (b[1:-1] for b in big)
    f.run(3, 2)
    for b in big:
        assert bool((b[0] == -7).all()) and bool((b[-1] == -7).all())
    assert int(f.ndk.sum()) == c.T


def test_init_only(gpu):
    f = _check(gpu, 20, 0, 10)
    assert f.samples == 1


def test_uninstantiated_tiling_is_an_error(gpu):
    c = _to(_corpus(2, multi=False), gpu)
    KS = 24  # (2, 12): choose_tiling never returns it
    f = FoldIn(c, torch.zeros(V + 1, KS, device=gpu), 24, ALPHA, SEED)
    with pytest.raises(RuntimeError, match="oni_foldin_launch"):
        f.run(1, 1)


def test_score_flow_gpu_matches_cpu(gpu, tmp_path):
    from oni355.models.saved import SavedModel
    from oni355.pipeline.flow import run_flow, score_flow
    from oni355.synth.flow import generate_flows
    day = generate_flows(5000, seed=21)
    tr = run_flow(dict(day.cols), K=20, sweeps=8, maxresults=100, device="cpu")
    m = SavedModel.load(SavedModel.from_run(tr.lda, tr.cuts, "flow").save(str(tmp_path / "m.npz")))
    other = generate_flows(5000, seed=22)  # a day with unseen words
    rc = score_flow(dict(other.cols), m, maxresults=200, device="cpu", sweeps=6, avg_last=3)
    rg = score_flow(dict(other.cols), m, maxresults=200, device=gpu, sweeps=6, avg_last=3)
    assert rc.stats["n_oov_tokens"] == rg.stats["n_oov_tokens"] > 0
    assert np.array_equal(rc.rows, rg.rows)
    assert np.array_equal(rc.scores, rg.scores)
    assert np.array_equal(rc.src_scores, rg.src_scores) and np.array_equal(rc.dst_scores, rg.dst_scores)
    assert np.array_equal(rc.lda.ndk_sum.numpy(), rg.lda.ndk_sum.cpu().numpy())
