"""Inputs of the featurize-layer edge tests (quantile.hip, wordify_flow.hip, pack_words.hip,
strings.hip), built in one place for two test files: test_featurize_edges_cpu.py asserts, for every
builder, the property that makes its input an edge case (and that the ops' CPU side equals the
oracle on it); test_gpu_featurize_edges.py runs the kernels on the same inputs against the oracle.
"""
import functools

import numpy as np

from oni355.ref import spec
from oni355.ref import strings_spec as ss

GRID = 2048 * 256            # the most threads an element-wise kernel launches
N_STRIDE = GRID + 257        # second grid-stride iteration with a ragged end
N_HIST_STRIDE = 2 * GRID * 4 + 7  # k_radix_hist reads four keys per lane
U32, I32, I64 = np.uint32, np.int32, np.int64

# ------------------------------------------------------------------------------------------------
# order keys
# ------------------------------------------------------------------------------------------------
F32_SPECIAL_BITS = np.array([
    0x00000000, 0x80000000,  # +0, -0
    0x7F800000, 0xFF800000,  # +inf, -inf
    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF,  # quiet / signalling NaNs
    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,  # smallest / largest denormals
    0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF,  # FLT_MIN, FLT_MAX
    0x3F800000, 0xBF800000], dtype=U32)

I64_SATURATION = np.array([np.iinfo(I64).min, -1, 0, 1, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1,
                           np.iinfo(I64).max, 1500], dtype=I64)


def f32_bits() -> np.ndarray:
    """The special values plus 1 000 random bit patterns (u32; view as f32)."""
    r = np.random.default_rng(11)
    return np.concatenate([F32_SPECIAL_BITS, r.integers(0, 2**32, 1000, dtype=np.uint64).astype(U32)])


def day_seconds() -> dict:
    """Every (h, m, s) of a day, then out-of-range integers; ibyt / ipkt cycle the saturation list."""
    sod = np.arange(86400)
    odd = np.array([-1, 24, 60, 2**31 - 1])
    h = np.concatenate([sod // 3600, odd, odd[::-1], np.full(4, 23)]).astype(I32)
    m = np.concatenate([sod // 60 % 60, odd, np.full(4, 59), odd]).astype(I32)
    s = np.concatenate([sod % 60, odd, odd, odd[::-1]]).astype(I32)
    n = h.size
    return dict(hour=h, minute=m, second=s, ibyt=np.resize(I64_SATURATION, n),
                ipkt=np.resize(I64_SATURATION[::-1], n))


def tie_keys(n: int, seed: int, hi: int = 12) -> np.ndarray:
    """Keys from a small integer range, most of them 1 (like ipkt on a real day)."""
    r = np.random.default_rng(seed)
    return np.where(r.random(n) < 0.6, 1, r.integers(0, hi, n)).astype(U32)


SIXTEENTHS = [(i, 16) for i in range(1, 16)]  # 15 cuts: the most a cut table holds
THIRDS = [(1, 3), (2, 3)]


def tie_cuts(keys: np.ndarray, fracs) -> np.ndarray:
    """Cuts that are themselves keys of the column: ties at a cut and duplicate cuts."""
    return spec.quantile_cuts(keys, fracs)


def bin_cases() -> list:
    """(name, keys, cuts) for k_bin_keys."""
    k = tie_keys(1031, 1)
    return [("deciles", k, tie_cuts(k, spec.DECILES)), ("no_cuts", k, np.zeros(0, U32)),
            ("fifteen", k, tie_cuts(tie_keys(1031, 2, 40), SIXTEENTHS))]


PORTS = [0, 1, 1023, 1024, 1025, 65535, -1, -2**31, 65536, 2**31 - 1]


def flow_ports(reps: int = 13) -> tuple:
    """The full cross product of PORTS for (sport, dport), repeated."""
    sp, dp = np.meshgrid(np.array(PORTS, I64), np.array(PORTS, I64), indexing="ij")
    return np.tile(sp.reshape(-1), reps).astype(I32), np.tile(dp.reshape(-1), reps).astype(I32)


def flow_word_cases() -> list:
    """(name, sport, dport, tkey, bkey, pkey, tcuts, bcuts, pcuts) for k_flow_wordify."""
    sp, dp = flow_ports()
    n = sp.size
    t, b, p = tie_keys(n, 3), tie_keys(n, 4), tie_keys(n, 5, 6)
    t40, b40 = tie_keys(n, 6, 40), tie_keys(n, 7, 40)
    z = np.zeros(0, U32)
    return [("ties", sp, dp, t, b, p, tie_cuts(t, spec.DECILES), tie_cuts(b, spec.DECILES), tie_cuts(p, spec.QUINTILES)),
            ("no_cuts", sp, dp, t, b, p, z, z, z),
            ("max_cuts", sp, dp, t40, b40, p, tie_cuts(t40, SIXTEENTHS), tie_cuts(b40, SIXTEENTHS),
             tie_cuts(p, THIRDS))]


def pack_cases(n: int = 1031) -> list:
    """(name, kwargs of strings_spec.pack_words) at the limits of k_pack."""
    r = np.random.default_rng(21)
    k3 = [tie_keys(n, 30 + i) for i in range(3)]
    k8 = [tie_keys(n, 40 + i, 40) for i in range(8)]
    raw = lambda lo, hi: r.integers(lo, hi, n).astype(I32)  # noqa: E731
    top = r.integers(0, 256, n).astype(np.uint8)
    return [
        ("ties", dict(keys=k3, cuts=[tie_cuts(k3[0], spec.DECILES), tie_cuts(k3[1], spec.QUINTILES),
                                     tie_cuts(k3[2], spec.QUINTILES)], kshift=[33, 29, 26],
                      raws=[raw(0, 70000), raw(0, 16)], rmask=[0xFFFF, 0xF], rshift=[4, 0], raw8=top, r8mask=3,
                      r8shift=37)),
        ("max", dict(keys=k8, cuts=[tie_cuts(k, SIXTEENTHS) for k in k8], kshift=[0, 4, 8, 12, 16, 20, 24, 56],
                     raws=[raw(0, 2**31 - 1) for _ in range(4)], rmask=[0xFF, 0xFF, 0xFF, 0xF],
                     rshift=[28, 36, 44, 52], raw8=top, r8mask=0xF, r8shift=60)),
        ("no_keys", dict(keys=[], cuts=[], kshift=[], raws=[raw(0, 1024), raw(0, 16)], rmask=[0x3FF, 0xF],
                         rshift=[8, 40], raw8=top, r8mask=0xFF, r8shift=0)),
        ("zero_between", dict(keys=k3, cuts=[tie_cuts(k3[0], spec.DECILES), np.zeros(0, U32),
                                             tie_cuts(k3[2], spec.QUINTILES)], kshift=[8, 4, 0], raws=[], rmask=[],
                              rshift=[], raw8=None, r8mask=0, r8shift=0)),
        ("no_cuts", dict(keys=k3, cuts=[np.zeros(0, U32)] * 3, kshift=[8, 4, 0], raws=[raw(0, 16)], rmask=[0xF],
                         rshift=[12], raw8=None, r8mask=0, r8shift=0)),
        ("negative_raw", dict(keys=k3[:1], cuts=[tie_cuts(k3[0], spec.DECILES)], kshift=[60],
                              raws=[raw(-2**31, 0), raw(-70000, 70000)], rmask=[0xFFFFFFFF, 0xFFFF], rshift=[0, 32],
                              raw8=top, r8mask=1, r8shift=59)),
    ]


@functools.lru_cache(maxsize=None)
def stride_inputs() -> dict:
    """N_STRIDE rows for every element-wise kernel: treat as read-only."""
    n = N_STRIDE
    r = np.random.default_rng(31)
    d = dict(f32=r.integers(0, 2**32, n, dtype=np.uint64).astype(U32).view(np.float32),
             hour=r.integers(0, 24, n).astype(I32), minute=r.integers(0, 60, n).astype(I32),
             second=r.integers(0, 60, n).astype(I32),
             ibyt=np.where(r.random(n) < 0.3, 1500, r.integers(-5, 2**33, n)).astype(I64),
             ipkt=np.where(r.random(n) < 0.6, 1, r.integers(0, 12, n)).astype(I64),
             sport=r.choice(np.array(PORTS, I64), n).astype(I32), dport=r.choice(np.array(PORTS, I64), n).astype(I32),
             raw=r.integers(-2**31, 2**31, n).astype(I32), raw8=r.integers(0, 256, n).astype(np.uint8))
    # the threads that run the loop twice (rows below 257 and from GRID on) take the compiler's
    # unrolled loop body, the others its remainder: the special values go through both
    m = F32_SPECIAL_BITS.size
    for at in (0, 300, GRID, n - m):
        d["f32"].view(U32)[at:at + m] = F32_SPECIAL_BITS
        d["hour"][at:at + 2] = d["minute"][at:at + 2] = d["second"][at:at + 2] = 0  # time +0
        d["ibyt"][at:at + I64_SATURATION.size] = I64_SATURATION
        d["ipkt"][at:at + I64_SATURATION.size] = I64_SATURATION[::-1]
    d["tkey"], d["bkey"], d["pkey"] = spec.flow_keys(d["hour"], d["minute"], d["second"], d["ibyt"], d["ipkt"])
    d["tcuts"] = tie_cuts(d["tkey"], spec.DECILES)
    d["bcuts"] = tie_cuts(d["bkey"], spec.DECILES)
    d["pcuts"] = tie_cuts(d["pkey"], spec.QUINTILES)
    return d


# ------------------------------------------------------------------------------------------------
# radix select
# ------------------------------------------------------------------------------------------------
RADIX_N = [0, 1, 3, 4, 5, 255, 257, 70_001]
RADIX_PASSES = {11: 10, 10: 0}  # nbits -> shift of the masked passes under test (the mask-0 set uses the top bits)
RADIX_PREFIX_SETS = ["mask0", "distinct", "duplicated", "sixteen", "unmatched"]
RADIX_PATTERNS = ["random", "all_equal", "two_bins", "lane0_nomatch", "lane0_nomatch_vec", "lane63_only",
                  "lane63_only_vec"]


def radix_prefixes(name: str, nbits: int) -> tuple:
    """(shift, mask, prefixes u32, a prefix value no key of radix_keys carries under another set)."""
    if name == "mask0":
        return 32 - nbits, 0, np.zeros(1, U32), None
    shift = RADIX_PASSES[nbits]
    top = shift + nbits
    mask = (0xFFFFFFFF << top) & 0xFFFFFFFF
    val = lambda j: U32((j * 0x9E3779B1) & mask)  # noqa: E731
    pre = {"distinct": [val(1), val(2), val(3)],
           "duplicated": [val(1), val(2), val(1), val(1), val(2)],
           "sixteen": [val(j) for j in range(1, 17)],
           "unmatched": [val(1), val(40)]}[name]
    return shift, mask, np.array(pre, U32), val(50)


def radix_keys(pattern: str, n: int, nbits: int, prefset: str) -> np.ndarray:
    """n keys for one k_radix_hist launch. ``lane`` is the wave lane that counts key i: i % 64 in the
    scalar loop, (i // 4) % 64 in the 16-byte-load loop (the ``_vec`` patterns)."""
    shift, mask, pre, miss = radix_prefixes(prefset, nbits)
    live = pre[:1] if prefset == "unmatched" else pre  # that set's second prefix is carried by no key
    r = np.random.default_rng(n * 31 + nbits)
    B = 1 << nbits
    low = r.integers(0, 1 << shift, n, dtype=np.uint64).astype(U32) if shift else np.zeros(n, U32)
    i = np.arange(n)
    lane = (i // 4) % 64 if pattern.endswith("_vec") else i % 64
    hit, other = live[0], (live[0] if miss is None else miss)
    if pattern == "random":
        pool = np.unique(live) if miss is None else np.concatenate([np.unique(live), [miss]])
        hi = pool[r.integers(0, len(pool), n)]
        digit = np.where(r.random(n) < 0.5, 7, r.integers(0, B, n))
    elif pattern == "all_equal":
        hi, digit, low = np.full(n, hit), np.full(n, B - 1), np.zeros(n, U32)
    elif pattern == "two_bins":
        hi, digit = np.full(n, hit), np.where(i % 2 == 0, 0, B - 1)
    elif pattern.startswith("lane0_nomatch"):
        hi, digit = np.where(lane == 0, other, hit), np.full(n, 5)
    else:  # lane63_only
        hi, digit = np.where(lane == 63, hit, other), np.full(n, 5)
    return (hi.astype(U32) | (digit.astype(U32) << U32(shift)) | low).astype(U32)


def pick_cases(B: int) -> tuple:
    """(hist u32 of three histograms, base int32, rank int64, labels) for k_quantile_pick: a small
    histogram, one with bins of 3·10⁹, an all-zero one; several queries share each base."""
    per = B // 64
    r = np.random.default_rng(B)
    small = r.integers(0, 6, B).astype(np.int64)
    small[r.random(B) < 0.3] = 0
    small[[0, per - 1, per, B - 1]] = [3, 2, 4, 1]
    c = np.cumsum(small)
    big = np.zeros(B, np.int64)
    big[[5, per - 1, per, B - 1]] = 3_000_000_000
    q = [(0, 0, "bin0"), (0, 2, "bin0_last"), (0, c[per - 1] - 1, "last_bin_of_lane0"),
         (0, c[per - 1], "first_bin_of_lane1"), (0, c[B // 2], "middle"), (0, c[-1] - 1, "last_element"),
         (0, c[-1], "rank_eq_total"), (0, c[-1] + 5, "rank_above_total"),
         (B, 0, "big_first"), (B, 2**32 + 1, "big_rank_over_2^32"), (B, 7_000_000_000, "big_third"),
         (B, 11_999_999_999, "big_last"), (B, 12_000_000_000, "big_rank_eq_total"), (B, 2**35, "big_above"),
         (2 * B, 0, "zero_hist"), (2 * B, 7, "zero_hist_rank7")]
    hist = np.concatenate([small, big, np.zeros(B, np.int64)]).astype(U32)
    return hist, np.array([b for b, _, _ in q], I32), np.array([k for _, k, _ in q], I64), [s for _, _, s in q]


def quantile_columns() -> dict:
    """name -> u32 key column for the three quantile_cuts entry points."""
    r = np.random.default_rng(41)
    cols = {"constant": np.full(1001, 0x80001234, U32),
            "two_valued": np.where(np.arange(1000) % 10 < 3, 5, 0xF0000000).astype(U32),
            "zero_and_max": np.where(np.arange(1000) < 300, 0, 0xFFFFFFFF).astype(U32),
            "last_pass_only": (U32(0x12345400) | r.integers(0, 1024, 5000).astype(U32)).astype(U32)}
    for n in (2, 3, 5):
        cols[f"n{n}"] = r.integers(0, 2**32, n, dtype=np.uint64).astype(U32)
    return cols


# ------------------------------------------------------------------------------------------------
# strings
# ------------------------------------------------------------------------------------------------
def column(strings: list) -> tuple:
    """(offsets int64 [N+1], chars uint8) of a list of byte strings."""
    off = np.zeros(len(strings) + 1, I64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return off, np.frombuffer(b"".join(strings), np.uint8).copy()


STRING_LENGTHS = [0, 1, 3, 4, 5, 254, 255, 256, 257, 600]


@functools.lru_cache(maxsize=None)
def string_block() -> tuple:
    """Under 2 000 byte strings for k_string_features (a tuple: read-only)."""
    r = np.random.default_rng(51)
    host = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-_./%", np.uint8)
    out = [b""]
    out += [bytes(r.choice(host, n)) for n in STRING_LENGTHS]
    out += [bytes(r.integers(0, 256, n, dtype=np.uint8)) for n in STRING_LENGTHS]
    out += [b"a" * n for n in STRING_LENGTHS[1:]] + [b"Z" * 300, b"\xff" * 256]
    out += [bytes(range(256)), bytes(range(255, -1, -1))] + [bytes([v]) for v in range(256)]
    out += [bytes(r.integers(0, 256, r.integers(0, 13), dtype=np.uint8)) for _ in range(1200)]
    if sum(len(s) for s in out) % 4 == 0:
        out.append(b"x")
    out.append(b"")
    return tuple(out)


def tiled_column(strings, reps: int) -> tuple:
    off, ch = column(list(strings))
    n, total = len(strings), int(off[-1])
    offs = (off[:-1][None, :] + (np.arange(reps, dtype=I64) * total)[:, None]).reshape(-1)
    return np.concatenate([offs, [reps * total]]).astype(I64), np.tile(ch, reps)


CUSTOM_PSL = "com\nexample.com\n*.dyn.example.com\n!keep.dyn.example.com\npvt.k12.ma.us\nus\n"
LONG_SUBDOMAINS = [255, 256, 257, 300]


def domain_names() -> list:
    out = []
    for n in LONG_SUBDOMAINS:
        out += [b"a" * n + b".example.com", (b"ab" * n)[:n] + b".example.co.uk", b"Q" * n + b".x.dyn.example.com"]
    out += [(b"a" * 50 + b".") * 6 + b"example.com", b"-" * 256 + b"." + b"a" * 256 + b".us"]
    out += [b"\xc3\xa9\xc3\xa9.example.com", b"\xff.\x80\x81.co.uk", bytes(range(128, 256)) + b".com",
            b"www.\xe4\xbe\x8b\xe3\x81\x88.jp", b"\x80", b"\xfe\xff."]
    out += [b".", b"..", b"...", b"." * 10, b"." * 300, b"", b"WWW.Example.COM", b"keep.dyn.example.com."]
    return out


def probe_home(h: int, mask: int) -> int:
    h = int(h) or 1
    return (h ^ (h >> 29)) & mask


def probe_path(hs, h: int) -> list:
    """The slots a probe for ``h`` visits, ending at its match or at the empty slot."""
    h = int(h) or 1
    i, path = probe_home(h, hs.mask), []
    for _ in range(hs.mask + 1):
        path.append(i)
        if int(hs.table[i]) in (h, 0):
            break
        i = (i + 1) & hs.mask
    return path


@functools.lru_cache(maxsize=None)
def probe_sets() -> dict:
    """name -> (HashSet, query hashes u64). ``wrap``: 243 hashes in 256 slots (load 0.95), eight of
    them homed in the last four slots, so their cluster runs past the end into slot 0."""
    r = np.random.default_rng(61)
    cand = r.integers(2, 2**64, 40_000, dtype=np.uint64)
    home = np.array([probe_home(h, 255) for h in cand.tolist()])
    tail, rest = cand[home >= 252], cand[home < 252]
    members = np.concatenate([tail[:8], rest[:235]])
    absent = np.concatenate([tail[8:40], rest[235:400]])
    wrap = ss.HashSet(members, load=0.95)
    q = np.concatenate([members, absent, np.array([0, 1], np.uint64)])
    with_zero = ss.HashSet(np.concatenate([members, np.zeros(1, np.uint64)]), load=0.95)
    a, b, c, d = (int(x) for x in rest[400:404])
    small_q = np.array([a, b, c, d, 0, 1, 2, 3], np.uint64)
    return {"wrap": (wrap, q), "with_zero": (with_zero, q), "two_slots": (ss.HashSet([a]), small_q),
            "two_slots_full": (ss.HashSet([a, b], load=0.95), small_q)}


# the strings on which str.strip() / str.upper() / str.lower() and the byte-wise ASCII rule differ
CATEGORY_ADVERSARIAL = [
    "GET\x1c", "GET\x1d", "GET\x1e", "GET\x1f", "\x1cGET", "\x1fPOST", "GET\x85", "\x85GET", "GET\xa0", "\xa0GET",
    "text/html\x1f", "\x1etext/html", "text/html\x85", "image/png\xa0", "\xa0-", "-\x1f", "\x1f", "\xa0", "\x85",
    "ﬁle/x", "ſ", "İ", "straße", "ｇｅｔ", "ＧＥＴ", "poſt", "poﬆ", "optıons", "İmage/png", "ımage/png",
    "GET\x00", "\x00GET", "GE\x00T", "text/\x00html", "text/html\x00", "\x00", " \x00 ",
    b"GET\xa0", b"\xa0GET", b"\x85text/html", b"text/html\xff", b"\xc2", b"image/\xe4\xbe"]
CATEGORY_METHODS = ["GET", " get ", "Post", "PUT\t", "head", "CONNECT", "options", "DELETE", "trace", "PATCH", "GETX",
                    "", "-", "OTHER", "g e t", "pOsT "]
CATEGORY_CTYPES = ["text/html", "TEXT/HTML; charset=utf-8", " text/plain", "image/png", "application/javascript",
                   "application/json", "application/octet-stream", "application/x-foo", "video/mp4", "audio/ogg",
                   "multipart/form-data", "", "-", " - ", "weird/type", "textual", "application", "IMAGE/"]

# 32 patterns (the table's limit), one of them 32 bytes (the pattern limit); prefix / exact pairs of
# equal length in both orders; an upper-case pattern that a lower-folded string can never equal
SYNTHETIC_PATTERNS = (("abcd", 1, 1), ("abcd", 0, 2), ("wxyz", 0, 3), ("wxyz", 1, 4), ("z" * 32, 1, 5), ("", 0, 6),
                      ("NEVER", 1, 7), ("abcdef", 0, 8), ("ab", 1, 9), ("ét", 1, 10)) + \
    tuple((f"p{j:02d}/", j % 2, 11 + j) for j in range(22))


def _enc(s) -> bytes:
    return s.encode() if isinstance(s, str) else bytes(s)


def category_strings(patterns=()) -> list:
    """Byte strings for k_category_codes under a pattern table."""
    out = [b"", b" ", b" \t\n\r\v\f", b"\v\f\v", b"a", b"A", b"\x80", b"\xff\xfe", b"G\xc9T"]
    out += [_enc(s) for s in CATEGORY_ADVERSARIAL + CATEGORY_METHODS + CATEGORY_CTYPES]
    for p, _, _ in patterns:
        p = p.encode()
        out += [p, p + b"\v\f", b"\f\v " + p + b"\r\n", p + b"x", p[:-1], p.upper(), p.lower(), p.swapcase() + b"/q",
                p + b"\x80", b"\xa0" + p, p + b" tail", p + p]
    return out
