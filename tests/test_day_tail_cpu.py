"""The training tail on the CPU: the oracles of oni355.ref.spec (theta_rows, tail_sums) pinned to
the project's own CPU expressions, the sensitivity of the likelihood-sum tolerance, and
GibbsLDA.check_health on planted faults.

The synthetic tables (``tail_case``), the tolerance (``tail_tol``) and the fault plants
(``PLANTS`` / ``plant``) are shared with tests/test_gpu_day_tail.py, which runs the HIP kernels
(k_tail_partials / k_tail_final, csrc/kernels/day_tail.hip) against the same oracle.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oni355.models import average
from oni355.models.corpus import build_corpus
from oni355.models.gibbs import GibbsConfig, GibbsLDA, tiling_for
from oni355.ref import spec
from oni355.utils import fault

# ------------------------------------------------------------------------------------------------
# tolerance of the four lgamma sums: |got − want| ≤ (U + K + 32) · 2^-53 · Σ|term|
#   U = 2: a device lgamma term is within 2 ulp of libm's (tests/test_gpu_kernels.py);
#   K + 32: the additions one term passes through -- a thread's chain of at most K + 1 doc terms
#   (or ceil(VK / 131072) word terms), 6 butterfly steps and 4 waves in k_tail_partials, 8
#   lane-strided partials and 6 butterfly steps in k_tail_final -- each at most 2^-53 relative.
# ------------------------------------------------------------------------------------------------
U_LGAMMA = 2


def tail_tol(K: int, mag: float) -> float:
    return (U_LGAMMA + K + 32) * 2.0 ** -53 * mag


ALPHA, BETA = 0.37, 0.01  # lgamma(0 + α) = 0.88, lgamma(0 + β) = 4.6: an empty cell's term is not small

# name: (K, KS, V, D, spare doc rows past D)
TAIL_SHAPES = {
    "smallest": (1, 4, 1, 1, 0),
    "past_one_grid": (7, 8, 18725, 300, 0),       # V·K = 131075 = 512·256 + 3
    "docs_past_grid": (20, 20, 6553, 131073, 0),  # V·K = 131060 < 512·256 < D − 1
    "widest_row": (256, 256, 3, 5, 0),
    "rows_past_D": (20, 24, 50, 37, 6),           # ndk has 43 rows; rows ≥ 37 hold negatives
    "nd_2_32": (4, 4, 8, 8, 0),                   # doc row 5 = four counts of 2^30: n_d = 2^32
}


def _counts(r, shape):
    """int32 counts: about 30 % zeros, the rest in [3, 200] (n + β, n + α stay away from 1 and 2,
    where lgamma crosses zero and a dropped cell would move a sum by nothing)."""
    return np.where(r.random(shape) < 0.3, 0, r.integers(3, 201, shape)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def tail_case(name: str) -> dict:
    """Synthetic (n_wk, q, n_k, n_dk) of one shape, with non-zero garbage in the padding columns
    and (where the shape has them) in the doc rows past D. Built once; treat as read-only."""
    K, KS, V, D, spare = TAIL_SHAPES[name]
    r = np.random.default_rng(sorted(TAIL_SHAPES).index(name) + 11)
    nwk, nk, ndk = _counts(r, (V, KS)), _counts(r, KS), _counts(r, (D + spare, KS))
    q = (r.random((V, KS)) + 1e-3).astype(np.float32)
    if name == "nd_2_32":
        ndk[5, :] = 2**30
    # what must be ignored: negatives and non-finite q in the columns ≥ K and the rows ≥ D
    nwk[:, K:], nk[K:], ndk[:, K:], q[:, K:] = -7, -3, -5, np.nan
    ndk[D:, :] = -9
    return dict(name=name, K=K, KS=KS, V=V, D=D, nwk=nwk, q=q, nk=nk, ndk=ndk, alpha=ALPHA, beta=BETA,
                vbeta=float(np.float32(V * BETA)))


@functools.lru_cache(maxsize=None)
def tail_oracle(name: str):
    c = tail_case(name)
    return spec.tail_sums(c["nwk"], c["q"], c["nk"], c["ndk"], c["D"], c["K"], c["alpha"], c["beta"], c["vbeta"])


@pytest.mark.parametrize("name", list(TAIL_SHAPES))
def test_tail_tolerance_sees_any_single_dropped_cell(name):
    """The reference alone: leaving out (or counting twice) any one cell with a non-zero term moves
    its sum by |term|, which is more than 100 tolerances in every sum of every shape the GPU test
    uses -- so a kernel within the tolerance has counted every cell exactly once."""
    c = tail_case(name)
    terms = spec.tail_terms(c["nwk"], c["nk"], c["ndk"], c["D"], c["K"], c["alpha"], c["beta"], c["vbeta"])
    sums, health, mags = tail_oracle(name)
    assert health == [0, 0, 0]  # the garbage sits only where the oracle must not look
    assert [len(t) for t in terms] == [c["V"] * c["K"], c["K"], c["D"] * c["K"], c["D"]]
    for j, t in enumerate(terms):
        a = np.abs(np.array(t))
        assert mags[j] == math.fsum(a.tolist()) and sums[j] == math.fsum(t)
        smallest = float(a[a > 0].min())
        assert smallest > 100 * tail_tol(c["K"], mags[j]), (name, j, smallest, tail_tol(c["K"], mags[j]))
    if name == "nd_2_32":  # an int32 row sum would wrap to 0: lgamma(Kα) instead of lgamma(2^32 + Kα)
        assert terms[3][5] == math.lgamma(2.0**32 + c["K"] * c["alpha"]) > 9e10


# lgamma of the double nearest each argument, to 32 digits (mpmath.loggamma at 40 digits)
_LGAMMA_32 = {
    0.01: "4.5994798780420217015805059587552", 0.37: "0.87694681948487930233854517131452",
    0.5: "0.57236494292470008707171367567653", 3.01: "0.70239474497808262281198614613659",
    3.37: "1.0603952411280858439668492815876", 94.72: "334.98798794037736238165028616125",
    200.37: "859.89346437578426265584648723106", 2.0**30 + 0.37: "21254091712.86245268547505754923",
    2.0**32 + 1.48: "90970455824.882330250003117781453",
}


def test_tail_terms_are_libm_accurate():
    """libm's lgamma, the oracle's term, against 32-digit values on arguments the cases use: within
    4 ulp (one ulp ≤ 2^-52 relative), the largest lgamma error glibc documents for any platform
    it lists double results for."""
    from fractions import Fraction
    for x, digits in _LGAMMA_32.items():
        want = Fraction(digits)
        assert abs(Fraction(math.lgamma(x)) - want) <= 4 * Fraction(2) ** -52 * abs(want), x


# ------------------------------------------------------------------------------------------------
# oracle pins
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("D,K,KS", [(1, 1, 4), (257, 4, 4), (300, 20, 24), (33, 255, 256)])
def test_spec_theta_rows_is_the_cpu_expression_bitwise(D, K, KS, dtype):
    """models.average.theta_rows on CPU tensors == spec.theta_rows, bit for bit: counts past 2^24
    (f32(n) rounds), a row sum past 2^31, int64 counts past 2^40, garbage in the padding."""
    r = np.random.default_rng(D + K)
    n = r.integers(0, 2**25, (D, KS)).astype(dtype)
    n[0, :K] = 2**30 if dtype == np.int32 else 2**41 + 12345
    n[:, K:] = -123456789
    add, den_add = 0.1, K * 0.1 + 1.0 / 3.0
    want = spec.theta_rows(n, K, add, den_add)
    got = average.theta_rows(torch.from_numpy(n), K, add, den_add).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not want[:, K:].any() and np.all(want[:, :K] > 0)
    ref = (n[:, :K].astype(np.float64) + add) / (n[:, :K].astype(np.float64).sum(1, keepdims=True) + den_add)
    assert np.allclose(want[:, :K], ref, rtol=3e-7, atol=0)


def test_spec_phi_rows_against_float64():
    r = np.random.default_rng(4)
    nw, nk = r.integers(0, 2**25, (40, 24)), r.integers(2**25, 2**33, 24)
    nw[:, 20:], nk[20:] = -5, 0
    want = spec.phi_rows(nw, nk, 20, 0.5, 12.3)
    assert want.dtype == np.float32 and not want[:, 20:].any()
    assert np.allclose(want[:, :20], (nw[:, :20] + 0.5) / (nk[:20] + 12.3), rtol=3e-7, atol=0)


def _toy_model(dev, n_docs=100, V=60, K=7, seed=1234):
    """A _toy_tokens-style corpus (tests/test_gpu_kernels.py): Zipf document lengths and words."""
    r = np.random.default_rng(seed)
    lens = r.zipf(1.6, n_docs).clip(1, 400)
    tdoc = torch.from_numpy(np.repeat(np.arange(n_docs), lens))
    tword = torch.from_numpy((r.zipf(1.3, tdoc.numel()) - 1) % V)
    keys = torch.from_numpy(((np.arange(n_docs, dtype=np.int64) * 2654435761 + seed) % (2**31 - 1)).astype(np.int32))
    c = build_corpus(tdoc.to(dev), tword.to(dev), n_docs, V, keys.to(dev), tiling_for(K, "dense")[0], L=64)
    m = GibbsLDA(c, GibbsConfig(K=K, seed=seed, use_graph=False, sampler="dense"))
    m.initialize()
    m.sweep(1)
    return m


def model_loglik_oracle(m):
    """(log-likelihood, tolerance) of a model's current counts from spec.tail_sums: the four sums
    and the two constants combined by fsum; every one of the six enters the tolerance's Σ|term|."""
    K, a, b, V = m.K, m.alpha, m.beta, m.V
    sums, health, mags = spec.tail_sums(m.nwk.cpu().numpy(), m.q.cpu().numpy(), m.nk_cur.cpu().numpy(),
                                        m.ndk_cur.cpu().numpy(), m.c.D_own, K, a, b, m.vbeta)
    cw = K * (math.lgamma(V * b) - V * math.lgamma(b))
    cd = m.c.D_own * (math.lgamma(K * a) - K * math.lgamma(a))
    want = math.fsum([cw, sums[0], -sums[1], cd, sums[2], -sums[3]])
    return want, tail_tol(K, math.fsum(mags) + abs(cw) + abs(cd)), health


@pytest.fixture(scope="module")
def cpu_model():
    return _toy_model(torch.device("cpu"))


def test_spec_tail_sums_is_the_cpu_log_likelihood(cpu_model):
    """The torch.lgamma path of GibbsLDA.log_likelihood against the oracle's sums."""
    m = cpu_model
    assert (m.K, m.KS) == (7, 8) and m.c.D == m.c.D_own == 100
    want, tol, health = model_loglik_oracle(m)
    got = m.log_likelihood()
    assert health == [0, 0, 0]
    assert abs(got - want) <= tol, (got, want, abs(got - want) / tol)
    assert tol < 1e-9 * abs(want)


# ------------------------------------------------------------------------------------------------
# check_health on planted faults
# ------------------------------------------------------------------------------------------------
# (table, value): what a plant writes; every plant goes to the first and to the last cell
PLANTS = [("q", float("nan")), ("q", float("inf")), ("q", float("-inf")), ("nwk", -1), ("nk", -1), ("ndk", -1)]
PLANT_IDS = [f"{t}={v}" for t, v in PLANTS]


def plant(m, table: str, value, last: bool, padding: bool):
    """Write ``value`` into the first or last cell of a table's real part (columns < K, doc rows
    < D) or of its padding columns; drops the cached tail sums as every writer of the state does.
    Returns a function that puts the old value back."""
    K, KS = m.K, m.KS
    t = {"q": m.q, "nwk": m.nwk, "nk": m.nk_cur, "ndk": m.ndk_cur}[table]
    col = (KS - 1 if last else K) if padding else (K - 1 if last else 0)
    if table == "nk":
        cell = (col,)
    else:
        rows = m.c.D if table == "ndk" else t.shape[0]
        cell = (rows - 1 if last else 0, col)
    old = t[cell].clone()
    t[cell] = value
    m._tail_cache = None

    def undo():
        t[cell] = old
        m._tail_cache = None
    return undo


def test_check_health_passes_on_a_clean_model(cpu_model):
    cpu_model.check_health()


@pytest.mark.parametrize("last", [False, True], ids=["first", "last"])
@pytest.mark.parametrize("table,value", PLANTS, ids=PLANT_IDS)
def test_check_health_raises_on_a_planted_fault(cpu_model, table, value, last):
    undo = plant(cpu_model, table, value, last, padding=False)
    try:
        with pytest.raises(fault.NumericalFault):
            cpu_model.check_health()
    finally:
        undo()
    cpu_model.check_health()


@pytest.mark.parametrize("last", [False, True], ids=["first", "last"])
@pytest.mark.parametrize("table,value", PLANTS, ids=PLANT_IDS)
def test_check_health_ignores_the_padding_columns(cpu_model, table, value, last):
    undo = plant(cpu_model, table, value, last, padding=True)
    try:
        cpu_model.check_health()
    finally:
        undo()


def test_check_health_raises_after_corrupt():
    m = _toy_model(torch.device("cpu"), n_docs=30)
    m.check_health()
    m._corrupt()
    with pytest.raises(fault.NumericalFault):
        m.check_health()
