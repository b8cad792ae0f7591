"""The training tail's HIP kernels (csrc/kernels/day_tail.hip) against the oracles of
oni355.ref.spec: k_tail_partials / k_tail_final (likelihood sums, health counts), k_theta_rows and
k_phi_rows (bitwise), and the model-level health check and log-likelihood that rest on them.

The synthetic tables, the tolerance and the fault plants are those of tests/test_day_tail_cpu.py,
which also shows, with the oracle alone, that one dropped or doubled cell moves a sum by more than
100 tolerances at every shape used here.
"""
import math

import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.models import average
from oni355.ref import spec
from oni355.utils import fault
from test_day_tail_cpu import (PLANT_IDS, PLANTS, TAIL_SHAPES, _toy_model, model_loglik_oracle, plant, tail_case,
                               tail_oracle, tail_tol)

pytestmark = pytest.mark.gpu


def _dev_tables(c, gpu):
    return [torch.from_numpy(c[k]).to(gpu) for k in ("nwk", "q", "nk", "ndk")]


def _tail(c, tabs):
    return ops.tail_sums(*tabs, c["D"], c["K"], c["alpha"], c["beta"], c["vbeta"])


# ------------------------------------------------------------------------------------------------
# k_tail_partials / k_tail_final
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TAIL_SHAPES))
def test_tail_sums_match_the_oracle(gpu, name):
    """The four lgamma sums within (U + K + 32) · 2^-53 · Σ|term| of the correctly rounded sums of
    libm terms (U = 2), the health slots exactly zero although the padding columns and the doc rows
    past D hold negatives and NaN, slot 7 zero, and the same bits from a second call.

    Largest |got − want| / (2^-53 · Σ|term|) observed on an MI355X, per sum [n_wk, n_k, n_dk, n_d]
    (the bound is U + K + 32, at least 35):
        smallest        0.000  0.000  1.190  1.190   (bound 35)
        past_one_grid   0.000  0.000  1.986  0.000   (bound 41)
        docs_past_grid  1.892  1.386  1.513  1.824   (bound 54)
        widest_row      0.000  0.000  8.934  0.000   (bound 290)
        rows_past_D     0.000  1.941  1.331  0.000   (bound 54)
        nd_2_32         0.000  1.488  0.000  0.000   (bound 38)
    i.e. at most 1.892, 1.941, 8.934 and 1.824 per sum; the model-level log-likelihood (K = 7, 300
    documents) sat 0.025 tolerances from the oracle and 0.042 from the CPU model's.
    """
    c = tail_case(name)
    sums, health, mags = tail_oracle(name)
    tabs = _dev_tables(c, gpu)
    got_t = _tail(c, tabs)
    got = got_t.cpu().tolist()
    ratios = [abs(got[j] - sums[j]) / (2.0 ** -53 * mags[j]) for j in range(4)]
    print(f"tail_sums {name}: error ratios {['%.3f' % x for x in ratios]} (bound {2 + c['K'] + 32})")
    assert health == [0, 0, 0] and got[4:] == [0.0, 0.0, 0.0, 0.0]
    for j in range(4):
        assert abs(got[j] - sums[j]) <= tail_tol(c["K"], mags[j]), (name, j, got[j], sums[j], ratios[j])
    again = _tail(c, tabs)
    assert torch.equal(got_t.view(torch.int64), again.view(torch.int64))  # deterministic: same bits


def _spread(r, n, k, must):
    """``k`` distinct cells of range(n): those of ``must`` that exist, the rest random."""
    cells = {i for i in must if 0 <= i < n}
    pool = r.permutation(n)
    for i in pool:
        if len(cells) >= min(k, n):
            break
        cells.add(int(i))
    return sorted(cells)


@pytest.mark.parametrize("name", list(TAIL_SHAPES))
def test_tail_health_slots_count_the_planted_cells(gpu, name):
    """Slots 4-6 equal the number of planted cells exactly: NaN, +inf and −inf in q, negatives in
    n_wk, n_k and n_dk, at cell 0, the last cell and cells 131071 / 131072 (the last thread of the
    grid's first trip and the first of its second) of the flattened real part; the garbage the
    case keeps in the padding columns and past row D is not counted. (The lgamma sums of a table
    with negative counts are not compared: the oracle's tolerance is stated for counts ≥ 0.)"""
    c = tail_case(name)
    K, V, D = c["K"], c["V"], c["D"]
    r = np.random.default_rng(5)
    nwk, q, nk, ndk = (c[k].copy() for k in ("nwk", "q", "nk", "ndk"))
    edge = (0, 131071, 131072)
    cells_q = _spread(r, V * K, 9, edge + (V * K - 1,))
    for n_, i in enumerate(cells_q):  # the flattened index runs over the K real columns
        q[i // K, i % K] = (np.nan, np.inf, -np.inf)[n_ % 3]
    cells_w = _spread(r, V * K, 7, edge + (V * K - 1,))
    for i in cells_w:
        nwk[i // K, i % K] = -1 - int(r.integers(0, 2**31 - 1))
    cells_k = _spread(r, K, 2, (0, K - 1))
    nk[cells_k] = -4
    cells_d = _spread(r, D * K, 11, (0, D * K - 1, 131071 * K, 131072 * K, 131072 * K + K - 1))
    for i in cells_d:
        ndk[i // K, i % K] = -1
    want = [len(cells_q), len(cells_w) + len(cells_k), len(cells_d)]
    assert all(s[0] == 0 and s[-1] == n - 1 for s, n in ((cells_q, V * K), (cells_w, V * K), (cells_d, D * K)))
    assert [int((~np.isfinite(q[:, :K])).sum()), int((nwk[:, :K] < 0).sum() + (nk[:K] < 0).sum()),
            int((ndk[:D, :K] < 0).sum())] == want
    tabs = [torch.from_numpy(a).to(gpu) for a in (nwk, q, nk, ndk)]
    got = _tail(c, tabs).cpu().tolist()
    assert got[4:7] == [float(x) for x in want] and got[7] == 0.0, (name, got[4:], want)


def test_tail_sums_refuse_bad_widths(gpu):
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device=gpu)  # noqa: E731
    q = torch.ones(2, 8, device=gpu)
    with pytest.raises(RuntimeError, match="oni_tail_sums"):  # K > KS
        ops.tail_sums(z(2, 8), q, z(8), z(3, 8), 3, 9, 0.1, 0.1, 0.2)
    with pytest.raises(RuntimeError, match="oni_tail_sums"):  # KS > 256
        ops.tail_sums(z(2, 260), torch.ones(2, 260, device=gpu), z(260), z(3, 260), 3, 20, 0.1, 0.1, 0.2)


# ------------------------------------------------------------------------------------------------
# k_theta_rows / k_phi_rows, bit for bit
# ------------------------------------------------------------------------------------------------
ADD = 0.1
BIG_D = 2048 * 256 + 257  # a second trip of k_theta_rows' row loop (grid capped at 2048 blocks)


def _theta_counts(D, K, KS, dtype, seed):
    r = np.random.default_rng(seed)
    n = r.integers(0, 2**25 + 2**24, (D, KS)).astype(dtype)  # past 2^24: f32(n) rounds
    n[r.random((D, KS)) < 0.3] = 0
    if dtype == np.int64:
        n[D // 2, :K] = 2**40 + r.integers(1, 2**30, K)
    if K >= 3:
        n[D - 1, :K] = 2**30  # an int32 row sum would pass 2^31 and wrap
    n[:, K:] = np.array([-123456789, 2**31 - 1, -1, 77] * 64, dtype=dtype)[: KS - K]
    return n


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("K,KS", [(1, 4), (4, 4), (20, 20), (20, 24), (255, 256)])
@pytest.mark.parametrize("D", [1, 255, 256, 257])
def test_theta_rows_bitwise(gpu, D, K, KS, dtype):
    n = _theta_counts(D, K, KS, dtype, D * 1000 + KS + K)
    den_add = K * 0.1 + 1.0 / 3.0  # not an f32
    assert float(np.float32(den_add)) != den_add
    want = spec.theta_rows(n, K, ADD, den_add)
    got = ops.theta_rows(torch.from_numpy(n).to(gpu), K, ADD, den_add).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert not got[:, K:].any() and np.all(got[:, :K] > 0)


@pytest.mark.parametrize("K", [1, 4])
def test_theta_rows_second_loop_trip_bitwise_and_cpu_equal(gpu, K):
    """D = 2048·256 + 257 rows at KS = 4: blocks 0 and 1 take a second trip. Also what
    models/average.py claims: the CPU expression and the GPU kernel agree bit for bit."""
    n = _theta_counts(BIG_D, K, 4, np.int32, K)
    den_add = K * 0.1 + 1.0 / 3.0
    want = spec.theta_rows(n, K, ADD, den_add)
    t = torch.from_numpy(n)
    got = average.theta_rows(t.to(gpu), K, ADD, den_add).cpu()
    assert np.array_equal(_bits(got.numpy()), _bits(want))
    assert torch.equal(average.theta_rows(t, K, ADD, den_add).view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("dk", [np.int32, np.int64], ids=["nk32", "nk64"])
@pytest.mark.parametrize("dw", [np.int32, np.int64], ids=["nw32", "nw64"])
@pytest.mark.parametrize("V,K,KS", [(1, 3, 4), (4095, 255, 256), (4097, 255, 256), (777, 20, 24)])
def test_phi_rows_bitwise(gpu, V, K, KS, dw, dk):
    """All four (n_wk, n_k) count widths; V·KS = 4, 4096·256 − 256 (one short of the capped grid)
    and 4096·256 + 256 (a second trip of the grid-stride loop)."""
    r = np.random.default_rng(V + KS)
    nw = r.integers(0, 2**25 + 2**24, (V, KS)).astype(dw)
    nk = r.integers(2**24, 2**31 - 1, KS).astype(dk)
    if dw == np.int64:
        nw[V // 2, :K] = 2**40 + r.integers(1, 2**30, K)
    if dk == np.int64:
        nk[K - 1] = 2**41 + 987654321
    nw[:, K:], nk[K:] = -99, -5
    add, vb = ADD, V * 0.01 + 1.0 / 3.0
    want = spec.phi_rows(nw, nk, K, add, vb)
    got = ops.phi_rows(torch.from_numpy(nw).to(gpu), torch.from_numpy(nk).to(gpu), K, add, vb).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert not got[:, K:].any() and np.all(got[:, :K] > 0)


# ------------------------------------------------------------------------------------------------
# the model: check_health and log_likelihood on the device sums
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(gpu):
    """(GPU model, CPU model) after initialize() and one sweep: K = 7, KS = 8, 300 documents. A
    corpus built on one GPU has no split-document pieces (Corpus.split is None, so D == D_own):
    check_health's ``extra`` branch over the rows [D_own, D) cannot be reached here."""
    mg, mc = _toy_model(gpu, n_docs=300), _toy_model(torch.device("cpu"), n_docs=300)
    assert (mg.K, mg.KS) == (7, 8) and mg.c.split is None and mg.c.D == mg.c.D_own == 300
    return mg, mc


def _copy_state(mg, mc):
    """The CPU model takes the GPU model's count tables (what log_likelihood reads)."""
    mc.nwk.copy_(mg.nwk.cpu())
    mc.nk_cur.copy_(mg.nk_cur.cpu())
    mc.ndk_cur.copy_(mg.ndk_cur.cpu())


def test_model_health_and_log_likelihood(models):
    mg, mc = models
    mg.check_health()
    _copy_state(mg, mc)
    want, tol, health = model_loglik_oracle(mc)
    got, cpu = mg.log_likelihood(), mc.log_likelihood()
    print(f"log-likelihood: gpu − oracle = {(got - want) / tol:.4f} tol, gpu − cpu = {(got - cpu) / tol:.4f} tol")
    assert health == [0, 0, 0] and math.isfinite(got)
    assert abs(got - want) <= tol and abs(got - cpu) <= tol, (got, cpu, want, tol)


@pytest.mark.parametrize("last", [False, True], ids=["first", "last"])
@pytest.mark.parametrize("table,value", PLANTS, ids=PLANT_IDS)
def test_model_check_health_raises_on_a_planted_fault(models, table, value, last):
    mg = models[0]
    undo = plant(mg, table, value, last, padding=False)
    try:
        with pytest.raises(fault.NumericalFault):
            mg.check_health()
    finally:
        undo()
    mg.check_health()


@pytest.mark.parametrize("last", [False, True], ids=["first", "last"])
@pytest.mark.parametrize("table,value", PLANTS, ids=PLANT_IDS)
def test_model_check_health_ignores_the_padding_columns(models, table, value, last):
    mg = models[0]
    undo = plant(mg, table, value, last, padding=True)
    try:
        mg.check_health()
    finally:
        undo()


def test_model_check_health_raises_after_corrupt(gpu):
    m = _toy_model(gpu, n_docs=30)
    m.check_health()
    m._corrupt()
    with pytest.raises(fault.NumericalFault):
        m.check_health()


def test_no_stale_tail_sums_after_load_canonical_z(models):
    """_tail() caches by sweeps_done: a state loaded at the same sweep count must not be served the
    previous state's sums."""
    mg, mc = models
    before = mg.log_likelihood()  # fills the cache at this sweeps_done
    assert mg._tail_cache is not None and mg._tail_cache[0] == mg.sweeps_done
    z = mg.canonical_z().cpu()
    z2 = ((z.to(torch.int64) * 3 + torch.arange(z.numel()) % 5) % mg.K).to(torch.uint8)
    assert not torch.equal(z, z2)
    sd = mg.sweeps_done
    mg.load_canonical_z(z2, sd)
    mc.load_canonical_z(z2, sd)
    assert mg.sweeps_done == sd and torch.equal(mg.nwk.cpu(), mc.nwk) and torch.equal(mg.ndk_cur.cpu(), mc.ndk_cur)
    want, tol, _ = model_loglik_oracle(mc)
    got = mg.log_likelihood()
    assert abs(got - want) <= tol and abs(got - mc.log_likelihood()) <= tol
    assert abs(got - before) > 1000 * tol  # the new state's value, not the cached one
    mg.check_health()
