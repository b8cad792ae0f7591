"""The featurize kernels (quantile.hip, wordify_flow.hip, pack_words.hip, strings.hip) against the
NumPy/Python oracle at their edges, bit for bit. The inputs come from featurize_edge_inputs.py;
test_featurize_edges_cpu.py proves each of them reaches the edge it is named for."""
import numpy as np
import pytest
import torch

import featurize_edge_inputs as fx
from oni355 import ops
from oni355.ops import strings as sops
from oni355.pipeline import proxy as px
from oni355.ref import psl, spec
from oni355.ref import strings_spec as ss

pytestmark = pytest.mark.gpu
U32 = np.uint32


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U32).view(np.int32)).to(dev)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _u32(t):
    return t.cpu().numpy().view(U32)


# ------------------------------------------------------------------------------------------------
# keys and bins
# ------------------------------------------------------------------------------------------------
def test_f32_keys_special_values(gpu):
    bits = fx.f32_bits()
    x = bits.view(np.float32)
    got = _u32(ops.f32_keys(_t(x, gpu)))
    assert np.array_equal(got, spec.f32_key(x))
    fin = np.isfinite(x)
    order = np.lexsort((bits[fin] >> 31 == 0, x[fin]))  # ascending, -0 before +0
    ks, xs = got[fin][order].astype(np.int64), x[fin][order]
    assert (np.diff(ks) >= 0).all() and (np.diff(ks)[np.diff(xs) > 0] > 0).all()


def test_i64_keys_saturation(gpu):
    v = fx.I64_SATURATION
    assert np.array_equal(_u32(ops.i64_keys(_t(v, gpu))), spec.i64_keys(v))


def test_flow_keys_every_second_of_the_day(gpu):
    d = fx.day_seconds()
    tk, bk, pk = ops.flow_keys(*(_t(d[c], gpu) for c in ("hour", "minute", "second", "ibyt", "ipkt")))
    assert np.array_equal(_u32(tk), spec.f32_key(spec.flow_time(d["hour"], d["minute"], d["second"])))
    assert np.array_equal(_u32(bk), spec.i64_keys(d["ibyt"])) and np.array_equal(_u32(pk), spec.i64_keys(d["ipkt"]))


@pytest.mark.parametrize("case", fx.bin_cases(), ids=lambda c: c[0])
def test_bin_keys_ties_and_limits(gpu, case):
    _, k, c = case
    assert np.array_equal(ops.bin_keys(_i32(k, gpu), c).cpu().numpy(), spec.bin_keys(k, c))


@pytest.mark.parametrize("case", fx.flow_word_cases(), ids=lambda c: c[0])
def test_flow_wordify_ports_ties_and_limits(gpu, case):
    _, sp, dp, t, b, p, tc, bc, pc = case
    want = spec.flow_wordify(sp, dp, t, b, p, tc, bc, pc)
    args = (_t(sp, gpu), _t(dp, gpu), _i32(t, gpu), _i32(b, gpu), _i32(p, gpu), tc, bc, pc)
    host = ops.flow_wordify(*args)
    dev = ops.flow_wordify(*args, dev_cuts=_i32(np.concatenate([tc, bc, pc]), gpu))
    for h, d, w in zip(host, dev, want):
        assert np.array_equal(_u32(h), w) and torch.equal(h, d)


def _pack_gpu(kw, gpu, dev_cuts):
    cuts, extra = kw["cuts"], {}
    if dev_cuts:
        extra["dev_cuts"] = _i32(np.concatenate([np.asarray(c, U32) for c in cuts] + [np.zeros(0, U32)]), gpu)
        cuts = [range(len(c)) for c in cuts]
    return sops.pack_words([_i32(k, gpu) for k in kw["keys"]], cuts, kw["kshift"], [_t(r, gpu) for r in kw["raws"]],
                           kw["rmask"], kw["rshift"], raw8=None if kw["raw8"] is None else _t(kw["raw8"], gpu),
                           r8mask=kw["r8mask"], r8shift=kw["r8shift"], **extra)


@pytest.mark.parametrize("case", fx.pack_cases(), ids=lambda c: c[0])
def test_pack_words_limits(gpu, case):
    kw = case[1]
    want = ss.pack_words(**kw)
    host, dev = _pack_gpu(kw, gpu, False), _pack_gpu(kw, gpu, True)
    assert np.array_equal(host.cpu().numpy().view(np.uint64), want) and torch.equal(host, dev)


def test_grid_stride_second_iteration(gpu):
    """2048·256 + 257 rows through every element-wise kernel: each runs its loop a second time."""
    d = fx.stride_inputs()
    assert np.array_equal(_u32(ops.f32_keys(_t(d["f32"], gpu))), spec.f32_key(d["f32"]))
    assert np.array_equal(_u32(ops.i64_keys(_t(d["ibyt"], gpu))), d["bkey"])
    keys = ops.flow_keys(*(_t(d[c], gpu) for c in ("hour", "minute", "second", "ibyt", "ipkt")))
    for g, c in zip(keys, ("tkey", "bkey", "pkey")):
        assert np.array_equal(_u32(g), d[c])
    assert np.array_equal(ops.bin_keys(keys[1], d["bcuts"]).cpu().numpy(), spec.bin_keys(d["bkey"], d["bcuts"]))
    cuts = (d["tcuts"], d["bcuts"], d["pcuts"])
    sw, dw = ops.flow_wordify(_t(d["sport"], gpu), _t(d["dport"], gpu), *keys, *cuts)
    wsw, wdw = spec.flow_wordify(d["sport"], d["dport"], d["tkey"], d["bkey"], d["pkey"], *cuts)
    assert np.array_equal(_u32(sw), wsw) and np.array_equal(_u32(dw), wdw)
    kw = dict(cuts=list(cuts), kshift=[40, 36, 33], rmask=[0xFFFFFFFF], rshift=[0], r8mask=0xFF, r8shift=44)
    got = sops.pack_words(list(keys), raws=[_t(d["raw"], gpu)], raw8=_t(d["raw8"], gpu),
                          dev_cuts=_i32(np.concatenate(cuts), gpu), **kw)
    want = ss.pack_words([d["tkey"], d["bkey"], d["pkey"]], raws=[d["raw"]], raw8=d["raw8"], **kw)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want)


def test_launchers_reject_oversized_tables(gpu):
    k = _i32(fx.tie_keys(64, 1), gpu)
    z = np.zeros(0, U32)
    with pytest.raises(RuntimeError, match="oni_flow_wordify"):
        ops.flow_wordify(k, k, k, k, k, np.zeros(15, U32), np.zeros(15, U32), np.zeros(3, U32))  # 33 cuts
    with pytest.raises(RuntimeError, match="oni_flow_wordify"):
        ops.flow_wordify(k, k, k, k, k, np.zeros(16, U32), z, z)
    with pytest.raises(RuntimeError, match="oni_radix_hist"):
        ops.radix_hist(k, 0, 10, np.zeros(17, U32), 0)  # P > 16
    with pytest.raises(RuntimeError, match="oni_radix_hist"):
        ops.radix_hist(k, 0, 10, z, 0)  # P < 1
    for nbits in (9, 12):
        with pytest.raises(RuntimeError, match="oni_radix_hist"):
            ops.radix_hist(k, 0, nbits, np.zeros(1, U32), 0)
    with pytest.raises(RuntimeError, match="oni_radix_hist"):
        ops.radix_hist(k, 0, 12, np.zeros(16, U32), 0)  # 256 KiB of bins: over the LDS limit
    e32, e64 = torch.zeros(0, dtype=torch.int32, device=gpu), torch.zeros(0, dtype=torch.int64, device=gpu)
    with pytest.raises(RuntimeError, match="oni_quantile_pick"):
        ops.quantile_pick(torch.zeros(2048, dtype=torch.int32, device=gpu), e32, 11, 0, e32, e64)  # nq < 1
    one32, one64 = torch.zeros(1, dtype=torch.int32, device=gpu), torch.zeros(1, dtype=torch.int64, device=gpu)
    with pytest.raises(RuntimeError, match="oni_quantile_pick"):
        ops.quantile_pick(torch.zeros(2048, dtype=torch.int32, device=gpu), one32, 5, 0, one32.clone(), one64)
    # a rejected launch leaves no error behind: the next launch is clean
    assert np.array_equal(ops.bin_keys(k, z).cpu().numpy(), np.zeros(64, np.uint8))


# ------------------------------------------------------------------------------------------------
# radix select
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefset", fx.RADIX_PREFIX_SETS)
@pytest.mark.parametrize("nbits", [10, 11])
def test_radix_hist_alignments_patterns_prefix_sets(gpu, nbits, prefset):
    """Every size x key pattern, from key pointers at element offsets 0 (the 16-byte loads) and
    1, 2, 3 (the scalar loop) of one allocation."""
    shift, mask, pre, _ = fx.radix_prefixes(prefset, nbits)
    for n in fx.RADIX_N:
        buf = torch.zeros(n + 3, dtype=torch.int32, device=gpu)
        for pattern in fx.RADIX_PATTERNS:
            k = fx.radix_keys(pattern, n, nbits, prefset)
            want = spec.radix_hist(k, shift, nbits, pre, mask)
            kd = _i32(k, gpu)
            for off in range(4):
                view = buf[off:off + n]
                view.copy_(kd)
                assert n == 0 or (view.data_ptr() % 16 == 0) == (off == 0)
                got = ops.radix_hist(view, shift, nbits, pre, mask)
                assert np.array_equal(got, want), (n, pattern, off)


@pytest.mark.parametrize("nbits", [10, 11])
def test_radix_hist_vector_loop_second_iteration(gpu, nbits):
    n = fx.N_HIST_STRIDE
    shift, mask, pre, _ = fx.radix_prefixes("duplicated", nbits)
    k = fx.radix_keys("random", n, nbits, "duplicated")
    got = ops.radix_hist(_i32(k, gpu), shift, nbits, pre, mask)
    assert np.array_equal(got, spec.radix_hist(k, shift, nbits, pre, mask))


@pytest.mark.parametrize("B", [1024, 2048])
def test_quantile_pick_hand_made_histograms(gpu, B):
    hist, base, rank, labels = fx.pick_cases(B)
    shift = 0 if B == 1024 else 10
    pre0 = np.full(len(base), 0xFFE00000, U32)
    wp, wr = spec.quantile_pick(hist, base, B, shift, pre0, rank)
    p_t, r_t = _i32(pre0, gpu), _t(rank, gpu)
    ops.quantile_pick(_i32(hist, gpu), _t(base, gpu), B.bit_length() - 1, shift, p_t, r_t)
    bad = [s for s, a, b, c, d in zip(labels, _u32(p_t), wp, r_t.cpu().numpy(), wr) if a != b or c != d]
    assert not bad


@pytest.mark.parametrize("name", list(fx.quantile_columns()))
def test_quantile_cuts_degenerate_columns(gpu, name):
    """Host-picked, batched and device-only cuts == the oracle, from an aligned pointer and from a
    slice at element offset 1."""
    k = fx.quantile_columns()[name]
    frs = [spec.DECILES, spec.QUINTILES]
    want = [spec.quantile_cuts(k, fr) for fr in frs]
    padded = _i32(np.concatenate([np.zeros(1, U32), k]), gpu)
    for kd in (_i32(k, gpu), padded[1:]):
        for fr, w in zip(frs, want):
            assert np.array_equal(ops.quantile_cuts(kd, fr), w)
        multi = ops.quantile_cuts_multi([kd, kd], frs)
        assert np.array_equal(multi[0], want[0]) and np.array_equal(multi[1], want[1])
        assert np.array_equal(_u32(ops.quantile_cuts_dev([kd, kd], frs)), np.concatenate(want))


# ------------------------------------------------------------------------------------------------
# strings
# ------------------------------------------------------------------------------------------------
def _same_features(got, want):
    assert np.array_equal(got[0].cpu().numpy().view(np.uint64), want[0])
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    assert np.array_equal(_u32(got[2]), want[2].view(U32))


@pytest.fixture(scope="module")
def block_features():
    off, ch = fx.column(list(fx.string_block()))
    return off, ch, ss.string_features(off, ch)


@pytest.mark.parametrize("pad", [0, 1, 4])
def test_string_features_word_and_byte_paths(gpu, block_features, pad):
    """``chars`` as uploaded, from a view at byte offset 1 (the byte-wise path) and at offset 4."""
    off, ch, want = block_features
    view = _t(np.concatenate([np.zeros(pad, np.uint8), ch]), gpu)[pad:]
    assert view.data_ptr() % 4 == pad % 4
    _same_features(sops.string_features(_t(off, gpu), view), want)


@pytest.mark.parametrize("pad", [0, 1])
def test_string_features_stride_loop(gpu, block_features, pad):
    blk = fx.string_block()
    reps = fx.GRID // len(blk) + 1
    off, ch = fx.tiled_column(blk, reps)
    view = _t(np.concatenate([np.zeros(pad, np.uint8), ch]), gpu)[pad:]
    _same_features(sops.string_features(_t(off, gpu), view), [np.tile(w, reps) for w in block_features[2]])


@pytest.mark.parametrize("rules", ["builtin", "custom"])
def test_domain_features_counter_wrap_high_bytes_dots(gpu, rules):
    names = fx.domain_names()
    off, ch = fx.column(names)
    r, user = (None, "") if rules == "builtin" else (psl.SuffixRules.parse(fx.CUSTOM_PSL), "www")
    top = ss.HashSet([ss.fnv1a(b"example.com")])
    want = ss.domain_features(off, ch, top, user, r)
    got = sops.domain_features(_t(off, gpu), _t(ch, gpu), top, user, r)
    for g, w, what in zip(got, want, ("reg_hash", "top", "sub_len", "sub_ent", "periods")):
        assert np.array_equal(g.cpu().numpy().view(np.uint8), np.asarray(w).view(np.uint8)), what


@pytest.mark.parametrize("name", ["wrap", "with_zero", "two_slots", "two_slots_full"])
def test_set_probe_wrapping_chain(gpu, name):
    hs, q = fx.probe_sets()[name]
    got = sops.set_probe(_t(q.view(np.int64), gpu), hs)
    assert got.dtype == torch.uint8 and got.cpu().tolist() == [int(int(h) in hs) for h in q.tolist()]


_CATEGORY_TABLES = {"method": (px.METHOD_PATTERNS, 1, 0), "ctype": (px.CTYPE_PATTERNS, 2, 10),
                    "synthetic": (fx.SYNTHETIC_PATTERNS, 2, 99), "synthetic_upper": (fx.SYNTHETIC_PATTERNS, 1, 99),
                    "synthetic_nofold": (fx.SYNTHETIC_PATTERNS, 0, 99), "empty": ((), 0, 7)}


@pytest.mark.parametrize("table", list(_CATEGORY_TABLES))
def test_category_codes_byte_rule(gpu, table):
    pats, fold, dflt = _CATEGORY_TABLES[table]
    strs = fx.category_strings(pats or fx.SYNTHETIC_PATTERNS)
    off, ch = fx.column(strs)
    want = ss.category_codes(strs, pats, fold, dflt)
    for pad in (0, 1):
        view = _t(np.concatenate([np.zeros(pad, np.uint8), ch]), gpu)[pad:]
        got = sops.category_codes(_t(off, gpu), view, pats, fold, dflt).cpu().numpy()
        bad = [(s, int(g), int(w)) for s, g, w in zip(strs, got, want) if g != w]
        assert not bad
