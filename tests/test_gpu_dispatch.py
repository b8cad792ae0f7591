"""Every branch of the dense samplers' selection ladder (select_gibbs, csrc/kernels/gibbs_sampler.h)
that a GibbsLDA configuration can reach, against the NumPy oracle, bit for bit.

Every case asks the launcher's own ladder which kernel it picks (GibbsLDA.sweep_kernels ->
ops.gibbs_which -> oni_gibbs_which: the same select_gibbs the launch goes through) and asserts the
family and the distinguishing template flags first, so a case that falls to another branch fails
instead of passing for the wrong reason. Then the device model is compared with the CPU model
(count_mode="atomic", the oracle spec.gibbs_pass) after initialize() and after every sweep() call
on tok_z, ndk_cur, nwk, nk_cur, q, qfix (and tok_zlag when lagged) with torch.equal: no tolerances.

Ladder branches (descriptors as ops.GibbsKernel) and the cases that run them; "bitwise" is
test_gpu_kernels.py::test_gibbs_bitwise_vs_oracle, "lagged" is
test_x01_lag.py::test_lagged_kernels_match_the_oracle_bitwise:

init      generic INIT, modes 0 / 1            every case (initialize()).
lag  G=1  x1 ALN LAG, modes 0 / 4              test_lag_with_guard[20-recount-64-*] (0); lagged[20-wdelta] (4).
lag  G>1  ldsg ALN LAG (G = 2, 4), 0 / 4       test_lag_with_guard[50-wdelta-64-*] (4); lagged[100-auto] (0, 4).
          ldsg LAG, not ALN, modes 0 / 4       test_lag_unaligned[50|100-recount|wdelta-33] (chunks that start
                                               inside a Philox group), [200-wdelta-64] (G = 16 has no ALN kernel),
                                               test_lag_with_guard[50-wdelta-66-*].
lag  rest generic, handed tok_zlag             test_lag_unaligned[20-wdelta-33]; test_lag_with_guard[20-delta-64-*],
                                               [20-wdelta-66-*], [50-delta-64-*] and test_lag_with_guard_in_graphs:
                                               the guard is present and NO twin follows (on the parent commit a
                                               guarded generic twin followed the unguarded generic kernel, so at
                                               flag 0 two samplers swept the same tokens).
G=1       x1 ALN PKQ (ONI_SAMPLER_AB=4)        test_sampler_ab_kernels[4-*].
          x1 ALN, no LUT (ONI_SAMPLER_AB=8)    test_sampler_ab_kernels[8-*].
          x1 ALN LUT (the default), 0 / 4      test_tilings[16|24|28-*]; bitwise (K = 4, 20, 32).
          x1 WPD AIR, modes 3 / 4 (AB=1)       test_sampler_ab_kernels[1-20-dual|wdelta].
          x1 AIR, not ALN, modes 0-4           test_unaligned_chunks[20-33-*] (all five), [20-3-*], [20-127-*],
                                               test_unaligned_chunks_in_graphs; with aligned chunks modes 1-3:
                                               bitwise[20-atomic|delta|dual], test_guard_beyond_wdelta[20-*].
G>1       ldsg OCC=4, modes 0 / 4 (AB=2)       test_sampler_ab_kernels[2-50|100-*].
          ldsg ALN (G = 2, 4), modes 0 / 4     test_tilings[33|45|56|57|96|112-*-0.5] (every (2, KP) and (4, KP)
                                               reachable by default), test_tilings_narrow[40|64-*].
          ldsg, not ALN, modes 0-4             test_unaligned_chunks[50-30|33-*], [100-33-*], [200-5-wdelta];
                                               aligned G = 8 / 16: test_tilings[113|129|255-*-0.5],
                                               test_tilings_narrow[90-*-0.5], [100-*]; aligned modes 1-3: bitwise,
                                               test_guard_beyond_wdelta[50-*].
fallback  generic, modes 0-4                   test_tilings[*-None] wherever 50/K is inexact in f32,
                                               test_unaligned_chunks[7-33-wdelta]; bitwise[7-*], [*+generic].
twin      generic TWIN behind a row kernel     test_guard_beyond_wdelta[*] (x1 / ldsg, modes 0-3, aligned and
                                               L = 66), test_lag_with_guard (where a LAG row kernel is picked);
                                               wdelta: test_gpu_kernels.py::test_exact_guard_picks_the_row_...
(G, KP)   (1,16) (1,24) (1,28) (2,20) (2,24) (2,28) (4,16) (4,24) (4,28) (8,16) (16,16): test_tilings;
          (4,12) (4,16) (8,12) (8,16): test_tilings_narrow; (1,4) (1,8) (1,12) (1,20) (1,32) (4,20): bitwise.

Not covered, with the reason:
 * k_gibbs_x1<KP, MODE, AIR = false> (with and without WPD): the ladder needs qpf = 3 without
   alpha_in_row; GibbsLDA turns qpf into 0 (generic) whenever n + α is not exact, so only a direct
   ops.gibbs_pass caller reaches them.
 * (4,8), (8,8) and (16,8) are instantiated, but no ops.choose_tiling result reaches them.
 * The ALN instantiations of k_gibbs_ldsg for G = 8 / 16 are compiled but excluded by the ladder's
   (G == 2 || G == 4) test.
The device-free properties of the ladder (one sampler per sweep for either flag value, over every
argument combination) are in tests/test_dispatch_query_cpu.py.
"""
import functools
import os

import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.models import gibbs as gm
from oni355.models.corpus import build_corpus
from oni355.models.gibbs import GibbsConfig, GibbsLDA

pytestmark = pytest.mark.gpu

MODES = {"recount": 0, "atomic": 1, "delta": 2, "dual": 3, "wdelta": 4}
GUARD_ALPHA = 0.5 + 2.0 ** -10  # n + α exact in f32 up to n = 16,381 only
CPU = torch.device("cpu")


def _tokens(kind, K):
    """"toy": the corpus of test_gibbs_bitwise_vs_oracle (300 documents, 400 words, one of 5000
    tokens). "long": the corpus of test_exact_guard_picks_the_row_kernel_per_sweep_bitwise (120
    documents, 300 words, one of 20,000 tokens: past the exact range of GUARD_ALPHA)."""
    r = np.random.default_rng(K)
    if kind == "toy":
        D, V, seed = 300, 400, K
        lens = r.zipf(1.6, D).clip(1, 3000)
        lens[0] = 5000
    else:
        D, V, seed = 120, 300, 7
        lens = r.zipf(1.6, D).clip(1, 500)
        lens[0] = 20_000
    tdoc = np.repeat(np.arange(D), lens)
    tword = (r.zipf(1.3, tdoc.size) - 1) % V
    keys = ((np.arange(D, dtype=np.int64) * 2654435761 + seed) % (2**31 - 1)).astype(np.int32)
    return torch.from_numpy(tdoc), torch.from_numpy(tword), torch.from_numpy(keys), D, V


def _corpus(kind, K, L, dev):
    tdoc, tword, keys, D, V = _tokens(kind, K)
    G, _ = ops.choose_tiling(K)
    return build_corpus(tdoc.to(dev), tword.to(dev), D, V, keys.to(dev), G, L=L)


def _fields(lag):
    return ("tok_z", "ndk_cur", "nwk", "nk_cur", "q", "qfix") + (("tok_zlag",) if lag else ())


@functools.lru_cache(maxsize=None)
def _oracle_run(kind, K, L, alpha, plan, lag_from, tiling):
    """The CPU model's state after initialize() and after every sweep(n) of ``plan``: computed once
    per chain, shared by the cases that differ only in what the device runs, never modified.
    (lag_from / tiling: the environment the caller has set, part of the key.)"""
    assert os.environ.get("ONI_TILING", "wide") == tiling
    assert lag_from is None or os.environ["ONI_X01_LAG_FROM"] == lag_from
    cc = _corpus(kind, K, L, CPU)
    lag = lag_from is not None
    mc = GibbsLDA(cc, GibbsConfig(K=K, alpha=alpha, seed=1234, use_graph=False, count_mode="atomic", sampler="dense",
                                  x01_lag=lag))
    snaps = []

    def snap():
        snaps.append({f: getattr(mc, f).clone() for f in _fields(lag and mc._lag_live)})
    mc.initialize()
    snap()
    for n in plan:
        mc.sweep(n)
        snap()
    mc.check_invariants()
    return dict(tok_word=cc.tok_word, chunk_doc=cc.chunk_doc, snaps=snaps, lag_live=mc._lag_live)


def _oracle(kind, K, L, alpha, plan, lag):
    return _oracle_run(kind, K, L, alpha, tuple(plan), os.environ["ONI_X01_LAG_FROM"] if lag else None,
                       os.environ.get("ONI_TILING", "wide"))


def _same(snap, m):
    for f, want in snap.items():
        assert torch.equal(want, getattr(m, f).cpu()), f


def _is(kernel, **want):
    got = {k: getattr(kernel, k) for k in want}
    assert got == want, kernel


def _model(cg, K, mode, *, alpha=None, graph=False, lag=False, **cfg):
    return GibbsLDA(cg, GibbsConfig(K=K, alpha=alpha, seed=1234, use_graph=graph, count_mode=mode, sampler="dense",
                                    x01_lag=lag, **cfg))


def _replay(gpu, mg, kind, K, L, *, alpha=None, plan=(1, 1, 1), lag=False, flag=None):
    """initialize() + the sweep() calls of ``plan`` on the device model, each compared with the
    oracle bit for bit (``flag``: the exactness guard's value after every call); then the count
    invariants."""
    ref = _oracle(kind, K, L, alpha, plan, lag)
    cg = mg.c
    assert torch.equal(ref["tok_word"], cg.tok_word.cpu()) and torch.equal(ref["chunk_doc"], cg.chunk_doc.cpu())
    mg.initialize()
    _same(ref["snaps"][0], mg)
    for n, snap in zip(plan, ref["snaps"][1:]):
        mg.sweep(n)
        if flag is not None:
            assert int(mg._guard["flag"].item()) == flag
        _same(snap, mg)
    if lag:
        assert mg._lag_live and ref["lag_live"] and "tok_zlag" in ref["snaps"][-1]
    T, Kk = cg.T, mg.K
    assert int(mg.nwk[:, :Kk].sum()) == T == int(mg.ndk_cur[:, :Kk].sum()) == int(mg.nk_cur[:Kk].sum())
    assert int(mg.nwk.min()) >= 0 and int(mg.ndk_cur.min()) >= 0 and int(mg.nk_cur.min()) >= 0
    mg.check_invariants()
    mg.close()


def _row_kernel(mg, mode, aligned, *, lag=False):
    """What the ladder must pick for a dense model whose n + α is exact (GibbsLDA._air), without
    ONI_SAMPLER_AB: the descriptor fields that tell its branches apart."""
    m = MODES[mode]
    if mg.G == 1:
        if lag:
            fast = aligned and m in (0, 4)
            return dict(family="x1", mode=m, air=True, aln=True, lag=True, lut=False) if fast else dict(
                family="generic", mode=m, lag=True)
        aln = aligned and m in (0, 4)
        return dict(family="x1", mode=m, air=True, wpd=False, aln=aln, lag=False, pkq=False, lut=aln)
    if lag and m not in (0, 4):
        return dict(family="generic", mode=m, lag=True)
    aln = aligned and mg.G in (2, 4) and m in (0, 4)
    return dict(family="ldsg", mode=m, occ=1, aln=aln, lag=lag)


# ------------------------------------------------------------------------------------------------
# 1. chunk lengths that are no multiple of 4: chunks start inside a 4-token Philox group
# ------------------------------------------------------------------------------------------------
_UNALIGNED = ([(20, 33, m) for m in MODES] + [(20, L, m) for L in (3, 127) for m in ("wdelta", "recount")]
              + [(50, L, m) for L in (30, 33) for m in ("recount", "wdelta", "delta")]
              + [(100, 33, m) for m in ("recount", "wdelta", "atomic")] + [(200, 5, "wdelta"), (7, 33, "wdelta")])
_RESIDUES = {3: {0, 1, 2, 3}, 5: {0, 1, 2, 3}, 33: {0, 1, 2, 3}, 127: {0, 1, 2, 3}, 30: {0, 2}}


def _assert_unaligned(mg, L):
    cg = mg.c
    assert not mg._pos_aligned
    res = set((cg.chunk_pos0[cg.chunk_doc >= 0] % 4).unique().tolist())
    assert res == _RESIDUES[L] and res != {0}, res


@pytest.mark.parametrize("K,L,mode", _UNALIGNED)
def test_unaligned_chunks(gpu, K, L, mode):
    """The kernels that pick their Philox word per token (k_gibbs_x1 without ALN: rng.pick(s);
    k_gibbs_ldsg without ALN: gbase / next_refresh / the shuffle by gi - gbase) on chunks that start
    at every residue of a 4-token Philox group: L = 3 puts every group across two chunks, L = 127
    is the longest odd chunk, L = 30 gives residues {0, 2} only."""
    mg = _model(_corpus("toy", K, L, gpu), K, mode)
    _assert_unaligned(mg, L)
    first, twin = mg.sweep_kernels(MODES[mode])
    assert twin is None
    if K == 7:  # α = 50/7 is not exact in f32: the generic kernel
        assert not gm._alpha_in_row_exact(mg.alpha, mg.c.max_doc_len()) and mg.qpf == 0
        _is(first, family="generic", mode=4, lag=False, twin=False)
    else:
        assert mg.qpf == (3 if mg.G == 1 else 2) and (mg.G, mg.KP) == {20: (1, 20), 50: (2, 28), 100: (4, 28),
                                                                        200: (16, 16)}[K]
        _is(first, **_row_kernel(mg, mode, False))
    _replay(gpu, mg, "toy", K, L)


def test_unaligned_chunks_in_graphs(gpu):
    """Unaligned one-lane chunks through the auto mode's recount -> wdelta switch, captured in
    graphs: the eager device model, the graph-replayed one and the oracle are one chain."""
    K, L, cfg = 20, 33, dict(auto_switch=2, auto_threshold=0.99)
    cg = _corpus("toy", K, L, gpu)
    a, b = _model(cg, K, "auto", **cfg), _model(cg, K, "auto", graph=True, **cfg)
    _assert_unaligned(b, L)
    for m in (0, 4):
        assert b.sweep_kernels(m)[1] is None
        _is(b.sweep_kernels(m)[0], family="x1", mode=m, air=True, aln=False, lut=False)
    a.initialize()
    a.sweep(7)
    _replay(gpu, b, "toy", K, L, plan=(2, 5))
    assert b.timings.get("graph_replays", 0) >= 1
    assert a._sweep_mode(a.sweeps_done) == 4 == b._sweep_mode(b.sweeps_done)
    for f in _fields(False):
        assert torch.equal(getattr(a, f), getattr(b, f)), f


# ------------------------------------------------------------------------------------------------
# 2. tilings
# ------------------------------------------------------------------------------------------------
_TILING = {16: (1, 16), 24: (1, 24), 28: (1, 28), 33: (2, 20), 45: (2, 24), 56: (2, 28), 57: (4, 16), 96: (4, 24),
           112: (4, 28), 113: (8, 16), 129: (16, 16), 255: (16, 16)}
_NARROW = {40: (4, 12), 64: (4, 16), 90: (8, 12), 100: (8, 16)}


def _tiling_case(gpu, K, mode, alpha, want):
    cg = _corpus("toy", K, 64, gpu)
    mg = _model(cg, K, mode, alpha=alpha)
    assert ops.choose_tiling(K) == want == (mg.G, mg.KP) and mg._pos_aligned
    exact = gm._alpha_in_row_exact(mg.alpha, cg.max_doc_len())
    first, twin = mg.sweep_kernels(MODES[mode])
    assert twin is None and mg._guard is None
    if exact:
        assert mg.qpf == (3 if mg.G == 1 else 2)
        _is(first, **_row_kernel(mg, mode, True))
    else:  # n + α not exact in f32: the generic kernel, as for K = 7 and 12 in test_gibbs_bitwise_vs_oracle
        assert alpha is None and mg.qpf == 0
        _is(first, family="generic", mode=MODES[mode], twin=False)
    _replay(gpu, mg, "toy", K, 64, alpha=alpha)
    return exact


@pytest.mark.parametrize("alpha", [None, 0.5])
@pytest.mark.parametrize("mode", ["wdelta", "recount"])
@pytest.mark.parametrize("K", sorted(_TILING))
def test_tilings(gpu, K, mode, alpha):
    """Every default (G, KP) no other test runs, and the K at which choose_tiling changes units
    (33, 56 | 57, 112 | 113, 129) or pads most against the cnt < K - 1 clamp (33, 255). α = 50/K
    (None) is exact in f32 for K = 16 only -- the other K run the generic kernel there, and the
    row-f32 kernels of their tiling with the exact α = 0.5."""
    exact = _tiling_case(gpu, K, mode, alpha, _TILING[K])
    assert exact == (alpha is not None or K == 16)


@pytest.mark.parametrize("K,mode,alpha", [(K, m, a) for K in sorted(_NARROW) for m in ("wdelta", "recount")
                                          for a in ((None, 0.5) if K == 90 else (None,))])
def test_tilings_narrow(gpu, monkeypatch, K, mode, alpha):
    """ONI_TILING=narrow: (4,12), (4,16), (8,12), (8,16). α = 50/K is exact but for K = 90, which
    runs the generic kernel there and k_gibbs_ldsg<8, 12> with α = 0.5."""
    monkeypatch.setenv("ONI_TILING", "narrow")
    exact = _tiling_case(gpu, K, mode, alpha, _NARROW[K])
    assert exact == (alpha is not None or K != 90)


# ------------------------------------------------------------------------------------------------
# 3. the dense ONI_SAMPLER_AB kernels (bench/sampler_ab.py): the same chain, or the A/B is void
# ------------------------------------------------------------------------------------------------
_AB = ([("1", 20, m) for m in ("dual", "wdelta")] + [("2", K, m) for K in (50, 100) for m in ("recount", "wdelta")]
       + [(ab, K, m) for ab in ("4", "8") for K in (20, 32) for m in ("recount", "wdelta")])


@pytest.mark.parametrize("ab,K,mode", _AB)
def test_sampler_ab_kernels(gpu, monkeypatch, ab, K, mode):
    """ONI_SAMPLER_AB bit 0: k_gibbs_x1 WPD (word-sorted slots loaded on change); bit 1:
    k_gibbs_ldsg OCC = 4; bit 2: k_gibbs_x1 PKQ (packed q'); bit 3: k_gibbs_x1 with the bfe count
    update (no LUT). The CPU oracle ignores the variable."""
    monkeypatch.setenv("ONI_SAMPLER_AB", ab)
    mg = _model(_corpus("toy", K, 64, gpu), K, mode)
    assert mg._air and mg._pos_aligned and mg.qpf == (3 if mg.G == 1 else 2)
    m = MODES[mode]
    first, twin = mg.sweep_kernels(m)
    assert twin is None
    _is(first, **{"1": dict(family="x1", mode=m, air=True, wpd=True, aln=False, pkq=False, lut=False),
                  "2": dict(family="ldsg", mode=m, occ=4, aln=False, lag=False),
                  "4": dict(family="x1", mode=m, air=True, wpd=False, aln=True, pkq=True, lut=False),
                  "8": dict(family="x1", mode=m, air=True, wpd=False, aln=True, pkq=False, lut=False)}[ab])
    _replay(gpu, mg, "toy", K, 64)


# ------------------------------------------------------------------------------------------------
# 4. the exactness guard beyond wdelta / L = 64
# ------------------------------------------------------------------------------------------------
_TWIN = dict(family="generic", twin=True, guard=False)
_GUARD = ([(K, 64, m) for K in (20, 50) for m in ("recount", "delta", "dual", "atomic")]
          + [(20, 66, "recount"), (50, 66, "delta")])


def _guard_model(gpu, monkeypatch, K, L, mode, force_generic, **kw):
    if force_generic:
        monkeypatch.setenv("ONI_EXACT_GUARD_LIMIT", "10")
    cg = _corpus("long", K, L, gpu)
    assert not gm._alpha_in_row_exact(GUARD_ALPHA, cg.max_doc_len())
    mg = _model(cg, K, mode, alpha=GUARD_ALPHA, **kw)
    assert mg._guard is not None and mg._air and mg.qpf == (3 if mg.G == 1 else 2)
    assert mg._guard["rows"].numel() == 1 or force_generic  # only the long document can leave the range
    assert mg._pos_aligned == (L % 4 == 0)
    return mg


@pytest.mark.parametrize("force_generic", [False, True])
@pytest.mark.parametrize("K,L,mode", _GUARD)
def test_guard_beyond_wdelta(gpu, monkeypatch, K, L, mode, force_generic):
    """The per-sweep choice between a row-f32 kernel and its guarded generic twin in the count modes
    and on the unaligned chunks whose first launch is another kernel (k_gibbs_x1<KP, 0..3>,
    k_gibbs_ldsg<G, KP, 0..3>, each with its own return at flag 0): the oracle's draws for either
    flag value (ONI_EXACT_GUARD_LIMIT forces 0)."""
    mg = _guard_model(gpu, monkeypatch, K, L, mode, force_generic)
    first, twin = mg.sweep_kernels(MODES[mode])
    _is(first, guard=True, twin=False, **_row_kernel(mg, mode, L % 4 == 0))
    _is(twin, mode=MODES[mode], lag=False, **_TWIN)
    _replay(gpu, mg, "long", K, L, alpha=GUARD_ALPHA, flag=0 if force_generic else 1)


# ------------------------------------------------------------------------------------------------
# 5. the lagged word side (tok_zlag) x the guard, x unaligned chunks
# ------------------------------------------------------------------------------------------------
_LAG_PLAN = (4, 3, 2)
_LAG_GUARD = [(20, "delta", 64), (20, "recount", 64), (20, "wdelta", 66), (50, "delta", 64), (50, "wdelta", 64),
              (50, "wdelta", 66)]


def _lag_guard_case(gpu, monkeypatch, K, mode, L, force_generic, graph):
    monkeypatch.setenv("ONI_X01_LAG_FROM", "3")
    mg = _guard_model(gpu, monkeypatch, K, L, mode, force_generic, lag=True, graph=graph)
    want = _row_kernel(mg, mode, L % 4 == 0, lag=True)
    first, twin = mg.sweep_kernels(MODES[mode], lag=True)
    _is(first, twin=False, **want)
    if want["family"] == "generic":
        # the ladder's own pick is the (unguarded) generic kernel: it runs alone, for either flag
        assert twin is None and not first.guard
    else:
        assert first.guard
        _is(twin, mode=MODES[mode], lag=True, **_TWIN)
    _replay(gpu, mg, "long", K, L, alpha=GUARD_ALPHA, plan=_LAG_PLAN, lag=True, flag=0 if force_generic else 1)
    return mg


@pytest.mark.parametrize("force_generic", [True, False])
@pytest.mark.parametrize("K,mode,L", _LAG_GUARD)
def test_lag_with_guard(gpu, monkeypatch, K, mode, L, force_generic):
    """Lagged sweeps of a corpus that needs the guard. Where no LAG row kernel matches (delta, or
    unaligned one-lane chunks) the first pick is the generic kernel, which does not read the flag:
    launching the guarded twin behind it as well swept the tokens twice at flag 0 ([20-delta-64],
    [20-wdelta-66] and [50-delta-64], forced)."""
    _lag_guard_case(gpu, monkeypatch, K, mode, L, force_generic, False)


def test_lag_with_guard_in_graphs(gpu, monkeypatch):
    mg = _lag_guard_case(gpu, monkeypatch, 20, "delta", 64, True, True)
    assert mg.timings.get("graph_replays", 0) >= 1


@pytest.mark.parametrize("K,mode,L", [(K, m, 33) for K in (50, 100) for m in ("recount", "wdelta")]
                         + [(20, "wdelta", 33), (200, "wdelta", 64)])
def test_lag_unaligned(gpu, monkeypatch, K, mode, L):
    """The lagged k_gibbs_ldsg without ALN (unaligned chunks; G = 16 at any L) and the generic
    kernel that unaligned one-lane chunks fall to under tok_zlag. World 1, no process group."""
    monkeypatch.setenv("ONI_X01_LAG_FROM", "3")
    mg = _model(_corpus("toy", K, L, gpu), K, mode, lag=True)
    if L % 4:
        _assert_unaligned(mg, L)
    assert mg._air and mg._guard is None
    first, twin = mg.sweep_kernels(MODES[mode], lag=True)
    assert twin is None
    want = _row_kernel(mg, mode, L % 4 == 0, lag=True)
    assert want["family"] == ("generic" if K == 20 else "ldsg") and not want.get("aln", False)
    _is(first, **want)
    _replay(gpu, mg, "toy", K, L, plan=_LAG_PLAN, lag=True)
