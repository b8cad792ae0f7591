"""The inputs of the featurize edge tests really are edge cases, the ops' CPU side equals the oracle
on them, and the oracle pieces added for them (spec.quantile_pick, strings_spec.category_codes) agree
with what they factor out (spec.quantile_cuts, the proxy host rules). No GPU."""
import numpy as np
import pytest
import torch

import featurize_edge_inputs as fx
from oni355 import ops
from oni355.ops import strings as sops
from oni355.pipeline import proxy as px
from oni355.ref import psl, spec
from oni355.ref import strings_spec as ss
from oni355.store.columnar import StringColumn

U32 = np.uint32


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U32).view(np.int32))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _has_ties_and_duplicates(keys, cuts):
    return bool((keys[:, None] == cuts[None, :]).any()) and len(np.unique(cuts)) < len(cuts)


# ------------------------------------------------------------------------------------------------
# keys and bins
# ------------------------------------------------------------------------------------------------
def test_f32_inputs_hold_every_special_value():
    bits = fx.f32_bits()
    x = bits.view(np.float32)
    assert bits.size == fx.F32_SPECIAL_BITS.size + 1000
    nan = np.isnan(x)
    assert (nan & (bits >> 31 == 0)).any() and (nan & (bits >> 31 == 1)).any()
    assert np.isposinf(x).any() and np.isneginf(x).any()
    assert {0x00000000, 0x80000000} <= set(bits.tolist())
    den = (bits & U32(0x7F800000) == 0) & (bits & U32(0x007FFFFF) != 0)
    assert (den & (bits >> 31 == 0)).any() and (den & (bits >> 31 == 1)).any()
    assert torch.equal(ops.f32_keys(_t(x)), _i32(spec.f32_key(x)))
    fin = np.isfinite(x)
    order = np.lexsort((bits[fin] >> 31 == 0, x[fin]))  # ascending, -0 before +0
    xs, ks = x[fin][order], spec.f32_key(x[fin])[order].astype(np.int64)
    assert (np.diff(ks) >= 0).all() and (np.diff(ks)[np.diff(xs) > 0] > 0).all()


def test_saturation_list_brackets_every_clamp():
    v = fx.I64_SATURATION.tolist()
    assert {0, 2**32 - 2, 2**32 - 1, 2**32, np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1} <= set(v)
    want = spec.i64_keys(fx.I64_SATURATION)
    assert want.tolist() == [min(max(x, 0), 2**32 - 1) for x in v]
    assert torch.equal(ops.i64_keys(_t(fx.I64_SATURATION)), _i32(want))


def test_day_seconds_cover_the_day_and_leave_it():
    d = fx.day_seconds()
    sod = d["hour"][:86400].astype(np.int64) * 3600 + d["minute"][:86400] * 60 + d["second"][:86400]
    assert np.array_equal(sod, np.arange(86400))
    for c in ("hour", "minute", "second"):
        assert {-1, 24, 60, 2**31 - 1} <= set(d[c][86400:].tolist())
    assert set(fx.I64_SATURATION.tolist()) <= set(d["ibyt"].tolist()) and set(d["ibyt"].tolist()) == set(d["ipkt"].tolist())
    # the proxy path's host table holds exactly the oracle's f32 times
    t = spec.flow_time(d["hour"][:86400], d["minute"][:86400], d["second"][:86400])
    assert np.array_equal(px._hour_table("cpu").numpy().view(U32), t.view(U32))
    got = ops.flow_keys(*(_t(d[c]) for c in ("hour", "minute", "second", "ibyt", "ipkt")))
    want = spec.flow_keys(d["hour"], d["minute"], d["second"], d["ibyt"], d["ipkt"])
    for g, w in zip(got, want):
        assert torch.equal(g, _i32(w))


def test_bin_inputs_tie_at_duplicate_cuts():
    cases = {name: (k, c) for name, k, c in fx.bin_cases()}
    assert _has_ties_and_duplicates(*cases["deciles"]) and _has_ties_and_duplicates(*cases["fifteen"])
    assert len(cases["no_cuts"][1]) == 0 and len(cases["fifteen"][1]) == 15
    for k, c in cases.values():
        got = ops.bin_keys(_i32(k), c).numpy()
        assert np.array_equal(got, spec.bin_keys(k, c))
        # a tie belongs to the lower bin: bin = #{cuts < key}
        assert np.array_equal(got, np.searchsorted(np.sort(c), k, side="left"))


def test_flow_word_inputs():
    sp, dp = fx.flow_ports(1)
    pairs = set(zip(sp.tolist(), dp.tolist()))
    assert {(a, b) for a in fx.PORTS for b in fx.PORTS} == pairs
    assert {0, 1, 1023, 1024, 1025, 65535} <= set(fx.PORTS) and min(fx.PORTS) < 0 and max(fx.PORTS) > 65535
    cases = {c[0]: c[1:] for c in fx.flow_word_cases()}
    _, _, t, b, p, tc, bc, pc = cases["ties"]
    assert all(_has_ties_and_duplicates(k, c) for k, c in ((t, tc), (b, bc), (p, pc)))
    assert [len(c) for c in cases["no_cuts"][5:]] == [0, 0, 0]
    assert [len(c) for c in cases["max_cuts"][5:]] == [15, 15, 2]  # 32 cuts: the kernel's cut table is full
    assert all(_has_ties_and_duplicates(k, c) for k, c in zip(cases["max_cuts"][2:5], cases["max_cuts"][5:]))
    for sp, dp, t, b, p, tc, bc, pc in cases.values():
        got = ops.flow_wordify(_t(sp), _t(dp), _i32(t), _i32(b), _i32(p), tc, bc, pc)
        want = spec.flow_wordify(sp, dp, t, b, p, tc, bc, pc)
        devc = _i32(np.concatenate([tc, bc, pc]))
        again = ops.flow_wordify(_t(sp), _t(dp), _i32(t), _i32(b), _i32(p), tc, bc, pc, dev_cuts=devc)
        for g, a, w in zip(got, again, want):
            assert torch.equal(g, _i32(w)) and torch.equal(a, g)


def _pack_cpu(kw, dev_cuts):
    cuts = kw["cuts"]
    extra = {}
    if dev_cuts:
        extra["dev_cuts"] = _i32(np.concatenate([np.asarray(c, U32) for c in cuts] + [np.zeros(0, U32)]))
        cuts = [range(len(c)) for c in cuts]
    return sops.pack_words([_i32(k) for k in kw["keys"]], cuts, kw["kshift"], [_t(r) for r in kw["raws"]], kw["rmask"],
                           kw["rshift"], raw8=None if kw["raw8"] is None else _t(kw["raw8"]), r8mask=kw["r8mask"],
                           r8shift=kw["r8shift"], **extra)


def test_pack_inputs_sit_at_the_kernel_limits():
    cases = dict(fx.pack_cases())
    assert all(_has_ties_and_duplicates(k, c) for k, c in zip(cases["ties"]["keys"], cases["ties"]["cuts"]))
    mx = cases["max"]
    assert len(mx["keys"]) == sops.K_MAX_BINNED and all(len(c) == sops.K_MAX_CUTS for c in mx["cuts"])
    assert len(mx["raws"]) == sops.K_MAX_RAW and mx["raw8"] is not None
    assert max(mx["kshift"] + mx["rshift"] + [mx["r8shift"]]) == 60
    assert all(_has_ties_and_duplicates(k, c) for k, c in zip(mx["keys"], mx["cuts"]))
    assert cases["no_keys"]["keys"] == [] and len(cases["no_keys"]["raws"]) > 0
    assert [len(c) > 0 for c in cases["zero_between"]["cuts"]] == [True, False, True]
    assert all(len(c) == 0 for c in cases["no_cuts"]["cuts"])
    assert all((r < 0).any() for r in cases["negative_raw"]["raws"])
    for name, kw in cases.items():
        want = ss.pack_words(**kw)
        for dev_cuts in (False, True):
            assert np.array_equal(_pack_cpu(kw, dev_cuts).numpy().view(np.uint64), want), (name, dev_cuts)
    # the lowest and the highest bin of a 15-cut component reach the top of the word
    assert {0, 15} <= set((ss.pack_words(**mx) >> np.uint64(56) & np.uint64(15)).tolist())


def test_stride_inputs_pass_the_grid():
    d = fx.stride_inputs()
    assert fx.N_STRIDE > 2048 * 256 and fx.N_STRIDE % 256 != 0 and fx.N_STRIDE % 64 != 0
    assert all(v.shape[0] == fx.N_STRIDE for k, v in d.items() if not k.endswith("cuts"))
    assert all(_has_ties_and_duplicates(d[k], d[c]) for k, c in (("bkey", "bcuts"), ("pkey", "pcuts")))
    assert (d["tkey"][:, None] == d["tcuts"][None, :]).any()
    assert fx.N_HIST_STRIDE // 4 > 2 * 2048 * 256 and fx.N_HIST_STRIDE % 4 != 0
    # rows of threads that loop twice (below 257, from 2048·256 on) and of threads that loop once
    bits, special = d["f32"].view(U32), set(fx.F32_SPECIAL_BITS.tolist())
    for rows in (slice(0, 257), slice(257, fx.GRID), slice(fx.GRID, None)):
        assert special <= set(bits[rows].tolist()) and set(fx.I64_SATURATION.tolist()) <= set(d["ibyt"][rows].tolist())
        assert (d["tkey"][rows] == 0x80000000).any()  # the time +0


# ------------------------------------------------------------------------------------------------
# radix select
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", [10, 11])
def test_radix_prefix_sets(nbits):
    sets = {name: fx.radix_prefixes(name, nbits) for name in fx.RADIX_PREFIX_SETS}
    shift, mask, pre, _ = sets["mask0"]
    assert mask == 0 and pre.tolist() == [0] and shift + nbits == 32
    for name in fx.RADIX_PREFIX_SETS[1:]:
        shift, mask, pre, miss = sets[name]
        assert mask == (0xFFFFFFFF << (shift + nbits)) & 0xFFFFFFFF and mask != 0
        assert all(int(p) & ~mask == 0 for p in pre) and int(miss) & ~mask == 0 and miss not in pre
    assert len(np.unique(sets["distinct"][2])) == len(sets["distinct"][2]) > 1
    d = sets["duplicated"][2]
    assert len(np.unique(d)) < len(d) and d[0] in d[1:]  # the first copy is not the only one
    assert len(np.unique(sets["sixteen"][2])) == 16  # P = 16: the largest LDS footprint the launcher takes
    u = sets["unmatched"][2]
    for pattern in fx.RADIX_PATTERNS:
        hi = fx.radix_keys(pattern, 70_001, nbits, "unmatched") & U32(sets["unmatched"][1])
        assert (hi == u[0]).any() and not (hi == u[1]).any()


@pytest.mark.parametrize("nbits", [10, 11])
def test_radix_key_patterns(nbits):
    n = 70_001
    shift, mask, pre, miss = fx.radix_prefixes("duplicated", nbits)
    B = 1 << nbits
    i = np.arange(n)

    def parts(pattern):
        k = fx.radix_keys(pattern, n, nbits, "duplicated")
        return np.isin(k & U32(mask), pre), (k >> U32(shift)) & U32(B - 1)
    m, dg = parts("all_equal")
    assert m.all() and len(np.unique(dg)) == 1  # every wave sits entirely on one bin
    m, dg = parts("two_bins")
    assert m.all() and np.array_equal(dg, np.where(i % 2 == 0, 0, B - 1))
    for pattern, lane in (("lane0_nomatch", i % 64), ("lane0_nomatch_vec", (i // 4) % 64)):
        m, dg = parts(pattern)
        assert np.array_equal(m, lane != 0) and len(np.unique(dg)) == 1  # the first active lane matches nothing
    for pattern, lane in (("lane63_only", i % 64), ("lane63_only_vec", (i // 4) % 64)):
        m, _ = parts(pattern)
        assert np.array_equal(m, lane == 63)
    m, dg = parts("random")
    assert m.any() and not m.all() and len(np.unique(dg[m])) > B // 2
    # a duplicated prefix gets the full count in every copy
    h = spec.radix_hist(fx.radix_keys("random", n, nbits, "duplicated"), shift, nbits, pre, mask)
    assert np.array_equal(h[0], h[2]) and np.array_equal(h[0], h[3]) and h[0].sum() > 0
    assert set(fx.RADIX_N) == {0, 1, 3, 4, 5, 255, 257, 70_001}


@pytest.mark.parametrize("nbits", [10, 11])
def test_radix_hist_cpu_side_is_the_spec(nbits):
    for prefset in fx.RADIX_PREFIX_SETS:
        shift, mask, pre, _ = fx.radix_prefixes(prefset, nbits)
        for n in (0, 5, 257):
            k = fx.radix_keys("random", n, nbits, prefset)
            got = ops.radix_hist(_i32(k), shift, nbits, pre, mask)
            assert got.dtype == np.int64 and got.shape == (len(pre), 1 << nbits)
            assert np.array_equal(got, spec.radix_hist(k, shift, nbits, pre, mask))


@pytest.mark.parametrize("B", [1024, 2048])
def test_pick_cases_reach_every_branch(B):
    hist, base, rank, labels = fx.pick_cases(B)
    per, shift = B // 64, (0 if B == 1024 else 10)
    pre0 = np.full(len(base), 0xFFE00000, U32)
    prefix, left = spec.quantile_pick(hist, base, B, shift, pre0, rank)
    assert np.array_equal(prefix & U32(0xFFE00000), pre0)  # the digit is OR-ed in below the old bits
    digit = dict(zip(labels, ((prefix >> U32(shift)) & U32(B - 1)).tolist()))
    left = dict(zip(labels, left.tolist()))
    assert digit["bin0"] == digit["bin0_last"] == 0 and left["bin0_last"] == 2
    assert digit["last_bin_of_lane0"] == per - 1 and digit["first_bin_of_lane1"] == per
    assert left["first_bin_of_lane1"] == 0
    small = hist[:B].astype(np.int64)
    total = int(small.sum())
    assert digit["last_element"] == B - 1 and left["last_element"] == small[B - 1] - 1
    # the cap: no cumulative count exceeds the rank -> digit B-1, rank -= cumsum[B-2]
    assert digit["rank_eq_total"] == digit["rank_above_total"] == B - 1
    assert left["rank_eq_total"] == small[B - 1] and left["rank_above_total"] == small[B - 1] + 5
    assert total - small[B - 1] == int(small[:B - 1].sum())
    big = hist[B:2 * B].astype(np.int64)
    assert big.max() == 3_000_000_000 >= 2**31 and int(rank.max()) >= 2**32 and int(big.sum()) >= 2**32
    assert [digit[k] for k in ("big_first", "big_rank_over_2^32", "big_third", "big_last")] == [5, per - 1, per, B - 1]
    assert left["big_rank_over_2^32"] == 2**32 + 1 - 3_000_000_000 and left["big_last"] == 2_999_999_999
    assert digit["big_rank_eq_total"] == digit["big_above"] == B - 1 and left["big_above"] == 2**35 - 9_000_000_000
    assert not hist[2 * B:].any() and digit["zero_hist"] == digit["zero_hist_rank7"] == B - 1
    assert left["zero_hist_rank7"] == 7
    assert len(base) > len(np.unique(base)) == 3  # several queries share each histogram
    # the op's CPU side works in place and equals the spec
    p_t, r_t = _i32(pre0), _t(rank.copy())
    assert ops.quantile_pick(_i32(hist), _t(base), B.bit_length() - 1, shift, p_t, r_t) is None
    assert np.array_equal(p_t.numpy().view(U32), prefix) and r_t.tolist() == list(left.values())


def _cuts_by_pick(keys, fracs):
    """The device pipeline's three passes on the oracle: one shared histogram in pass 1, then one per
    query (prefixes not de-duplicated), spec.quantile_pick between the passes."""
    nq = len(fracs)
    prefix = np.zeros(nq, U32)
    rank = spec.quantile_ranks(keys.size, fracs).astype(np.int64)
    for pi, (shift, nbits) in enumerate(((21, 11), (10, 11), (0, 10))):
        top = shift + nbits
        mask = 0 if top >= 32 else (0xFFFFFFFF << top) & 0xFFFFFFFF
        B = 1 << nbits
        h = spec.radix_hist(keys, shift, nbits, prefix[:1] if pi == 0 else prefix, mask)
        base = np.zeros(nq, np.int64) if pi == 0 else np.arange(nq) * B
        prefix, rank = spec.quantile_pick(h, base, B, shift, prefix, rank)
    return prefix


def test_quantile_columns_and_pick_chain():
    cols = fx.quantile_columns()
    assert len(np.unique(cols["constant"])) == 1 and len(np.unique(cols["two_valued"])) == 2
    assert set(cols["zero_and_max"].tolist()) == {0, 0xFFFFFFFF}
    assert all(cols[f"n{n}"].size == n < len(spec.QUINTILES) + 2 for n in (2, 3, 5))
    lp = cols["last_pass_only"]
    assert len(np.unique(lp >> U32(10))) == 1 and len(np.unique(spec.quantile_cuts(lp, spec.DECILES))) == 9
    for name, k in cols.items():
        for fr in (spec.DECILES, spec.QUINTILES):
            want = spec.quantile_cuts(k, fr)
            assert np.array_equal(_cuts_by_pick(k, fr), want), name
            assert np.array_equal(ops.quantile_cuts(_i32(k), fr), want)
            # the histogram route of the op (taken on the CPU with an all-reduce) uses spec.quantile_pick
            assert np.array_equal(ops.quantile_cuts(_i32(k), fr, allreduce=lambda h: h), want), name
        got = ops.quantile_cuts_multi([_i32(k), _i32(k)], [spec.DECILES, spec.QUINTILES], allreduce=lambda h: h)
        assert np.array_equal(got[0], spec.quantile_cuts(k, spec.DECILES))
        assert np.array_equal(got[1], spec.quantile_cuts(k, spec.QUINTILES))


# ------------------------------------------------------------------------------------------------
# strings
# ------------------------------------------------------------------------------------------------
def test_string_block_properties():
    blk = fx.string_block()
    off, ch = fx.column(list(blk))
    assert len(blk) <= 2000 and blk[0] == b"" and blk[-1] == b"" and ch.size % 4 != 0
    lens = {len(s) for s in blk}
    assert set(fx.STRING_LENGTHS) <= lens and set(fx.STRING_LENGTHS) == {0, 1, 3, 4, 5, 254, 255, 256, 257, 600}
    assert set(ch.tolist()) == set(range(256))
    assert all(any(len(s) == n and len(set(s)) == 1 for s in blk) for n in (1, 255, 256, 257, 600))
    assert {a % 4 for a in off[:-1].tolist()} == {0, 1, 2, 3}  # strings start at every byte of a word
    got = sops.string_features(_t(off), _t(ch))
    want = ss.string_features(off, ch)
    assert np.array_equal(got[0].numpy().view(np.uint64), want[0])
    assert np.array_equal(got[1].numpy(), want[1]) and np.array_equal(got[2].numpy().view(U32), want[2].view(U32))
    # tiling keeps every string and its features
    reps = fx.GRID // len(blk) + 1
    toff, tch = fx.tiled_column(blk, reps)
    assert toff.size - 1 == reps * len(blk) > 2048 * 256 and toff[-1] == tch.size
    j = len(blk) + 17
    assert bytes(tch[toff[j]:toff[j + 1]]) == blk[17] and np.array_equal(np.diff(toff), np.tile(np.diff(off), reps))


def test_long_subdomains_wrap_the_byte_counters():
    names = fx.domain_names()
    custom = psl.SuffixRules.parse(fx.CUSTOM_PSL)
    wrapped = 0
    for rules in (psl.default_rules(), custom):
        for nm in names:
            reg, _, _ = ss.split_domain(nm, rules)
            sub = nm[:reg - 1 if reg > 0 else 0]
            counts = np.bincount([ss.cbin(c) for c in ss._lower(sub)], minlength=64)
            wrapped += int(counts.max() >= 256)
    assert wrapped >= 8
    subs = {ss.split_domain(nm)[0] - 1 for nm in names}
    assert set(fx.LONG_SUBDOMAINS) == {255, 256, 257, 300} <= subs
    assert any(max(nm) >= 0x80 for nm in names if nm) and any(nm and set(nm) == {46} for nm in names)
    off, ch = fx.column(names)
    top = ss.HashSet([ss.fnv1a(b"example.com")])
    for rules, user in ((None, ""), (custom, "www")):
        got = sops.domain_features(_t(off), _t(ch), top, user, rules)
        want = ss.domain_features(off, ch, top, user, rules)
        for g, w in zip(got, want):
            assert np.array_equal(g.numpy().view(np.uint8), np.asarray(w).view(np.uint8))
        assert {0, 1, 2} >= set(want[1].tolist()) and want[1].max() == (2 if user else 1)


def test_probe_sets_wrap_past_the_last_slot():
    sets = fx.probe_sets()
    hs, q = sets["wrap"]
    assert hs.mask == 255 and np.count_nonzero(hs.table) == 243  # load 0.95
    assert hs.table[255] != 0 and hs.table[0] != 0
    paths = {int(h): fx.probe_path(hs, int(h)) for h in q.tolist()}
    wraps = lambda p: any(b < a for a, b in zip(p, p[1:]))  # noqa: E731
    present = [h for h in paths if h in hs]
    assert any(wraps(paths[h]) for h in present)  # a stored key found after the probe wrapped
    absent = [h for h in paths if h not in hs and h > 1]
    assert any(wraps(paths[h]) and hs.table[paths[h][-1]] == 0 for h in absent)  # a miss that ends at an empty slot
    assert any(len(paths[h]) == 1 for h in absent) and max(len(p) for p in paths.values()) > 8
    assert 0 not in hs and 1 not in hs
    hz, _ = sets["with_zero"]
    assert 0 in hz and 1 in hz and 1 in hz.table.tolist() and 0 not in [int(x) for x in hz.table if x]
    one, sq = sets["two_slots"]
    full, _ = sets["two_slots_full"]
    assert one.mask == full.mask == 1 and np.count_nonzero(one.table) == 1 and np.count_nonzero(full.table) == 2
    assert {fx.probe_home(h, 1) for h in sq.tolist() if int(h) not in full} == {0, 1}
    for hs, q in sets.values():
        got = sops.set_probe(_t(q.view(np.int64)), hs)
        assert got.dtype == torch.uint8 and got.tolist() == [int(int(h) in hs) for h in q.tolist()]


def _host_rule(fn, items):
    """The CPU pipeline's route: the column's bytes, decoded as it decodes them, through the host rule."""
    col = StringColumn.from_list(items)
    return [fn(col[i]) for i in range(len(col))]


@pytest.mark.parametrize("which", ["friendly", "adversarial"])
def test_category_codes_oracle_equals_host_rules(which):
    for vals, pats, fold, dflt, fn in ((fx.CATEGORY_METHODS, px.METHOD_PATTERNS, 1, 0, px.method_code),
                                       (fx.CATEGORY_CTYPES, px.CTYPE_PATTERNS, 2, 10, px.ctype_class)):
        items = vals if which == "friendly" else fx.CATEGORY_ADVERSARIAL
        got = ss.category_codes([fx._enc(s) for s in items], pats, fold, dflt).tolist()
        assert got == _host_rule(fn, items)
    if which == "adversarial":
        adv = fx.CATEGORY_ADVERSARIAL
        assert all(any(s.endswith(c) or s.startswith(c) for s in adv if isinstance(s, str))
                   for c in ("\x1c", "\x1d", "\x1e", "\x1f", "\x85", "\xa0"))
        assert {"ﬁle/x", "ſ", "İ", "straße", "ｇｅｔ"} <= set(adv) and any("\x00" in s for s in adv if isinstance(s, str))
        # the byte-wise ASCII rule: what Unicode would trim or fold is part of the value
        assert px.method_code("GET\x1f") == px.method_code("GET\xa0") == px.method_code("poſt") == 0
        assert px.ctype_class("text/html\xa0") == 1 and px.ctype_class("\xa0text/html") == 10
        assert px.method_code(" get\v\f") == 1 and px.ctype_class("\f TEXT/plain") == 2


def test_category_codes_oracle_rule():
    pats = fx.SYNTHETIC_PATTERNS
    assert len(pats) == 32 and max(len(p.encode()) for p, _, _ in pats) == 32
    code = lambda s, fold=2: int(ss.category_codes([s], pats, fold, 99)[0])  # noqa: E731
    assert code(b"abcd") == 1 and code(b"abcdx") == 1  # prefix listed first wins the equal-length exact one
    assert code(b"wxyz") == 3 and code(b"wxyzx") == 4  # exact listed first; the prefix still takes longer strings
    assert code(b"abcdef") == 8 and code(b"ABCDEF\v\f") == 8 and code(b"abcde") == 1 and code(b"abx") == 9
    assert code(b"z" * 32) == 5 and code(b"z" * 33) == 5 and code(b"z" * 31) == 99
    assert code(b"") == 6 and code(b" \t\n\r\v\f") == 6 and code(b"\x1f") == 99 and code(b"a") == 99
    assert code(b"never") == 99 and code(b"NEVER") == 99 and code(b"NEVER", 0) == 7
    assert code("ét".encode()) == 10 and code("Ét".encode()) == 99
    assert (ss.category_codes(fx.category_strings(pats), (), 0, 7) == 7).all()
    strs = fx.category_strings(pats)
    assert any(s.endswith(b"\v\f") and len(s) > 2 for s in strs) and any(max(s) >= 0x80 for s in strs if s)
    assert any(s and not s.strip(b" \t\n\r\v\f") for s in strs)
