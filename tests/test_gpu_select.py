"""Scoring and top-N selection (csrc/kernels/score.hip, pipeline.common.top_n) at their edges:
k_select against a NumPy mask, k_event_min against np.where, every width of k_score against
spec.score, and the histogram → bmax → cap → tie-break logic of top_n against a stable sort by
(score, row id) -- the last on CPU tensors too.
"""
import numpy as np
import pytest
import torch

from oni355 import ops
from oni355.pipeline import common
from oni355.ref import spec

BIG_N = 2048 * 256 + 1  # one element into the second trip of the capped grids (2048 blocks of 256)
SMALL = [1, 63, 64, 65]  # around one 64-lane wave; BIG_N appears once per kernel
TOL = np.float32(0.5)
BMAX = 1500  # below tol's bucket (1528): the bucket cut binds before tol does


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def _bucket(x):
    return (spec.f32_key(x) >> np.uint32(21)).astype(np.int64)


def _specials(tol=TOL, bmax=BMAX):
    """Scores from explicit bit patterns: tol itself and its two neighbours, the last value of
    bucket bmax and the first of bmax + 1, ±0, negatives, NaNs of both signs, ±inf."""
    tb = int(np.float32(tol).view(np.uint32))
    edge_in = spec.key_f32(np.uint32(((bmax + 1) << 21) - 1))
    edge_out = spec.key_f32(np.uint32((bmax + 1) << 21))
    assert _bucket(edge_in) == bmax and _bucket(edge_out) == bmax + 1 and edge_in < edge_out
    pats = _f32([tb, tb - 1, tb + 1, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0xBF800000, 0xFF7FFFFF,
                 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0x7F7FFFFF])
    return np.concatenate([pats, [edge_in, edge_out]]).astype(np.float32)


def _mixed(n, seed):
    """The specials (as many as fit) among log-uniform positives and a few negatives, shuffled."""
    r = np.random.default_rng(seed)
    x = np.exp(r.uniform(np.log(1e-6), np.log(4.0), n)).astype(np.float32)
    x[r.random(n) < 0.05] *= -1
    sp = _specials()
    k = min(n, sp.size)
    x[r.choice(n, k, replace=False)] = sp[r.permutation(sp.size)[:k]]
    return x


def _select_case(case, n):
    """(scores, tol, bmax) of one k_select case."""
    r = np.random.default_rng(n)
    if case == "mixed":
        x = _mixed(n, n)
        if n == BIG_N:  # the only live lane of the last wave (the rest have i >= n) holds a kept score
            x[-1] = np.float32(0.001)
        return x, TOL, BMAX
    if case == "tol_binds":  # tol below the bucket cut: only `score < tol` decides
        return _mixed(n, n + 1), np.float32(1e-4), BMAX
    if case == "tol_inf":  # keeps every finite value and −inf, drops +inf and NaN
        return _mixed(n, n + 2), np.float32(np.inf), 2047
    if case == "all":
        x = r.uniform(-1.0, 0.004, n).astype(np.float32)
        return x, TOL, BMAX
    if case == "none":
        x = r.uniform(0.5, 2.0, n).astype(np.float32)
        x[::3] = np.nan
        x[:1] = TOL  # equal to tol: not below it
        return x, TOL, BMAX
    if case == "waves":  # full 64-lane waves kept next to empty ones
        x = np.where((np.arange(n) // 64) % 2 == 0, np.float32(0.001), np.float32(0.7)).astype(np.float32)
        return x, TOL, BMAX
    raise AssertionError(case)


def _select_mask(x, tol, bmax):
    with np.errstate(invalid="ignore"):
        return (x < tol) & (_bucket(x) <= bmax)


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", [(c, n) for c in ("mixed", "tol_binds", "tol_inf", "all", "none", "waves")
                                    for n in SMALL] + [("mixed", BIG_N)])
def test_select_below_matches_the_mask(gpu, case, n):
    x, tol, bmax = _select_case(case, n)
    m = _select_mask(x, tol, bmax)
    count = int(m.sum())
    if case == "all":
        assert count == n
    if case == "none":
        assert count == 0
    if case == "tol_inf":
        assert np.array_equal(m, np.isfinite(x) | (x == -np.inf))
    s = torch.from_numpy(x).to(gpu)
    for cap in sorted({n, count}):  # cap == n, and cap exactly the count
        idx, sc = ops.select_below(s, float(tol), bmax, cap=cap)
        idx = idx.cpu().numpy()
        assert idx.size == count and np.unique(idx).size == count
        assert np.array_equal(np.sort(idx), np.nonzero(m)[0])
        assert np.array_equal(_bits(sc), _bits(x[idx]))  # each pair is (i, score[i]), bit for bit
    if count:
        with pytest.raises(RuntimeError, match="overflow"):
            ops.select_below(s, float(tol), bmax, cap=count - 1)


def _pairs(n, P, two, seed):
    r = np.random.default_rng(seed)
    p = [r.integers(0, P, n).astype(np.int32) for _ in range(2 if two else 1)]
    for a in p:
        a[0], a[-1] = (0, P - 1) if n > 1 else (P - 1, P - 1)
    if two and n > 2:
        p[1][0], p[0][1], p[1][1] = P - 1, P - 1, 0
    return p


def _pair_scores(P, seed):
    """Pair scores holding every special; the NaNs meet finite values on either side of the min."""
    ps = _mixed(P, seed)
    ps[0], ps[P - 1] = np.float32(np.nan), np.float32(0.25)
    return ps


def _hist_of(sc, tol):
    with np.errstate(invalid="ignore"):
        return np.bincount(_bucket(sc[sc < tol]), minlength=2048)


@pytest.mark.gpu
@pytest.mark.parametrize("two,parts,n", [(t, p, n) for t in (False, True) for p in (False, True) for n in SMALL]
                         + [(True, True, BIG_N)])
def test_event_min_matches_where(gpu, two, parts, n):
    """score = ps[p1] or (ps[p2] < ps[p1] ? ps[p2] : ps[p1]) -- a NaN first endpoint survives, a NaN
    second one does not -- and the histogram of the scores under tol is ADDED to what hist holds;
    −0.0 and +0.0 land in buckets 1023 and 1024, a score equal to tol in none."""
    P = 1000
    ps = _pair_scores(P, n + 7)
    p = _pairs(n, P, two, n)
    s1 = ps[p[0]]
    s2 = ps[p[1]] if two else None
    with np.errstate(invalid="ignore"):
        want = np.where(s2 < s1, s2, s1) if two else s1
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    h0 = (np.arange(2048) % 7 + 1).astype(np.int32)
    hist = t(h0.copy())
    got, g1, g2 = ops.event_min(t(ps), t(p[0]), t(p[1]) if two else None, tol=float(TOL), want_parts=parts, hist=hist)
    assert np.array_equal(_bits(got), _bits(want))
    if parts:
        assert np.array_equal(_bits(g1), _bits(s1))
        assert (g2 is None) if not two else np.array_equal(_bits(g2), _bits(s2))
    else:
        assert g1 is None and g2 is None
    assert np.array_equal(hist.cpu().numpy() - h0, _hist_of(want, TOL))
    plain, _, _ = ops.event_min(t(ps), t(p[0]), t(p[1]) if two else None)  # no histogram at all
    assert np.array_equal(_bits(plain), _bits(want))
    if n == 65 and two:  # the inputs do reach what the docstring names
        assert np.isnan(want[0]) and not np.isnan(want[1]) and _bucket(np.float32(-0.0)) == 1023
        assert _bucket(np.float32(0.0)) == 1024 and _hist_of(np.array([TOL, -0.0, 0.0], np.float32), TOL).sum() == 2


def _score_inputs(KS, n, seed):
    r = np.random.default_rng(seed)
    D, V = 211, 157
    th = (r.random((D, KS)) / KS).astype(np.float32)
    ph = (r.random((V, KS)) ** 6).astype(np.float32)
    ids = [r.integers(0, m, n).astype(np.int32) for m in (D, V, D, V)]
    for a, m in zip(ids, (D, V, D, V)):
        a[0], a[-1] = m - 1, 0  # the first and the last row of each table
    return th, ph, ids


def _check_score(gpu, KS, n, two):
    th, ph, (d1, w1, d2, w2) = _score_inputs(KS, n, KS + n)
    want, s1, s2 = spec.score(th, ph, d1, w1, d2 if two else None, w2 if two else None)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    tol = float(np.median(want))
    h0 = (np.arange(2048) % 5).astype(np.int32)
    hist = t(h0.copy())
    args = (t(d2), t(w2)) if two else (None, None)
    got, g1, g2 = ops.score(t(th), t(ph), t(d1), t(w1), *args, tol=tol, want_parts=True, hist=hist)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(g1), _bits(s1))
    assert (g2 is None) if not two else np.array_equal(_bits(g2), _bits(s2))
    assert np.array_equal(hist.cpu().numpy() - h0, _hist_of(want, np.float32(tol)))
    assert 0 < int((want < tol).sum()) < n or n == 1
    bare, b1, b2 = ops.score(t(th), t(ph), t(d1), t(w1), *args)
    assert np.array_equal(_bits(bare), _bits(want)) and b1 is None and b2 is None


@pytest.mark.gpu
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("KS", [20, 24, 32, 52, 64, 100, 104, 128, 4, 8, 28, 256])
def test_score_every_width_bitwise(gpu, KS, two):
    """The eight specialised k_score<KS> and the dynamic k_score<0> (KS = 4, 8, 28, 256)."""
    _check_score(gpu, KS, 1000, two)


@pytest.mark.gpu
def test_score_second_loop_trip_bitwise(gpu):
    _check_score(gpu, 20, BIG_N, True)


@pytest.mark.gpu
def test_score_refuses_a_width_that_is_no_multiple_of_4(gpu):
    th, ph, (d1, w1, _, _) = _score_inputs(6, 10, 1)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    with pytest.raises(RuntimeError, match="oni_score"):
        ops.score(t(th), t(ph), t(d1), t(w1))


# ------------------------------------------------------------------------------------------------
# common.top_n: the same cases on CPU tensors and on the GPU
# ------------------------------------------------------------------------------------------------
TOP_TOL = 0.5


def _top_scores(case):
    """(scores, maxresults) of one top_n case; 5000 scores."""
    r = np.random.default_rng(42)
    n = 5000
    x = r.uniform(0.3, 0.9, n).astype(np.float32)  # about a third under tol, all above the planted values
    if case in ("ties", "offset", "order"):
        # 40 scores below the tied value, then 300 rows sharing it exactly: the cut at 100 falls
        # inside the tie, so rows 41-100 are the tied rows of lowest id
        rows = r.permutation(n)
        x[rows[:40]] = r.uniform(0.01, 0.02, 40).astype(np.float32)
        x[rows[40:340]] = np.float32(0.0625)
        return x, 100
    if case == "one_bucket":  # every candidate in bucket(0.25); distinct scores and some ties
        x = np.full(n, 0.75, np.float32)
        rows = r.permutation(n)[:700]
        x[rows] = (np.float32(0.25) + r.integers(0, 50, 700).astype(np.float32) * np.float32(2.0 ** -20))
        assert np.unique(spec.f32_key(x[rows]) >> np.uint32(21)).size == 1
        return x, 100
    if case == "few":  # maxresults above the candidate count
        x = np.full(n, 0.75, np.float32)
        x[r.permutation(n)[:37]] = r.uniform(0.0, 0.4, 37).astype(np.float32)
        return x, 100
    if case == "zero":
        return x, 0
    if case == "nobody":
        return np.maximum(x, np.float32(0.5)), 100  # some equal to tol: not under it
    raise AssertionError(case)


def _top_reference(x, tol, maxresults, row_offset=0, order=None):
    """Stable order by (score, row id) of the scores under tol, first maxresults."""
    pos = np.nonzero(x < np.float32(tol))[0]
    gid = (order[pos] if order is not None else pos) + row_offset
    o = np.lexsort((gid, x[pos]))[:max(maxresults, 0)]
    return gid[o].astype(np.int64), x[pos][o], pos[o]


@pytest.mark.parametrize("hist_from", ["none", "event_min"])
@pytest.mark.parametrize("case", ["ties", "offset", "order", "one_bucket", "few", "zero", "nobody"])
@pytest.mark.parametrize("dev", ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_top_n_is_the_stable_sort_by_score_then_row(request, dev, case, hist_from):
    device = torch.device("cpu") if dev == "cpu" else request.getfixturevalue("gpu")
    x, maxresults = _top_scores(case)
    n = x.size
    row_offset = 1_000_000_007 if case == "offset" else 0
    order_np = np.random.default_rng(1).permutation(n).astype(np.int64) if case == "order" else None
    score = torch.from_numpy(x).to(device)
    hist = None
    if hist_from == "event_min":  # the histogram the fused score pass hands to top_n
        hist = torch.zeros(2048, dtype=torch.int32, device=device)
        score = ops.event_min(score, torch.arange(n, dtype=torch.int32, device=device), tol=TOP_TOL, hist=hist)[0]
        assert np.array_equal(_bits(score), _bits(x))
    order = torch.from_numpy(order_np).to(device) if order_np is not None else None
    want_rows, want_sc, want_pos = _top_reference(x, TOP_TOL, maxresults, row_offset, order_np)
    out = common.top_n(score, TOP_TOL, maxresults, None, row_offset=row_offset, hist=hist, order=order,
                       return_pos=order is not None)
    rows, sc = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert rows.dtype == np.int64 and sc.dtype == np.float32
    assert np.array_equal(rows, want_rows) and np.array_equal(_bits(sc), _bits(want_sc))
    if order is not None:
        pos = out[2].cpu().numpy()
        assert np.array_equal(pos, want_pos) and np.array_equal(_bits(x[pos]), _bits(sc))
        assert np.array_equal(order_np[pos] + row_offset, rows)
    # the cases are what they claim to be
    under = int((x < np.float32(TOP_TOL)).sum())
    if case in ("ties", "offset", "order"):
        assert rows.size == 100 and np.all(sc[40:] == np.float32(0.0625)) and np.all(np.diff(rows[40:]) > 0)
        assert int((x == np.float32(0.0625)).sum()) == 300
    elif case == "one_bucket":
        assert rows.size == 100 and under == 700
    elif case == "few":
        assert rows.size == under == 37
    else:
        assert rows.size == 0 and (under == 0) == (case == "nobody")
