"""Inputs, NumPy oracles and checks of the count-bookkeeping ops (ops.recount, ops.delta_recount,
ops.wdelta_recount / ops.wdelta_records, ops.gibbs_apply, ops.exact_guard, ops.copy_rows), shared by
tests/test_gpu_counts.py (the HIP kernels of csrc/kernels/gibbs.hip) and tests/test_counts_cpu.py
(the ops' CPU twins).

Every ``check_*`` builds its inputs from a seeded generator, asserts ON THE INPUTS that the branches
named in ``want`` are reached (so a changed constant cannot quietly empty a case), computes the
expected tables with plain NumPy in int64 (np.bincount / np.add.at; spec.gibbs_apply for q and
qfix), runs the op on ``device`` and compares everything bit for bit: no tolerance anywhere.
Tables the op accumulates into start from a non-zero pattern; tables it must overwrite start from
garbage.
"""
import functools

import numpy as np
import torch

from oni355 import ops
from oni355.ref import spec

I32, I64, U8 = np.int32, np.int64, np.uint8

# real topics of each padded width used here: K < KS wherever the width leaves room, so that the
# last padding column must keep its pre-fill
TOPICS = {4: 3, 8: 8, 12: 12, 16: 16, 20: 20, 24: 20, 28: 28, 32: 32, 52: 50, 256: 255}

RECOUNT_LARGE = 8 << 20  # oni_recount: `if (T < (int64_t(8) << 20))` -> k_recount<4>, else k_recount<16>


def to(a, device):
    """A tensor of its own on ``device``: never a view of the NumPy array (the oracle keeps that)."""
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(device)


def back(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    """Bitwise equality of two arrays of one dtype and shape (floats compared as their words)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        a, b = a.view(I32), b.view(I32)
    return bool(np.array_equal(a, b))


def prefill(shape, seed=0):
    """A non-zero int32 pattern (both signs) for tables a kernel adds into."""
    n = int(np.prod(shape))
    v = ((np.arange(n, dtype=I64) * 2654435761 + seed) % 13 - 6).astype(I32)
    v[v == 0] = 7
    return v.reshape(shape)


# what each T must reach, per kernel; recount_reached() is asserted against these
_P, _F = {"part_thread"}, {"full_thread"}
_WIDE = {"past_cap", "dense_run", "gap", "full_thread"}
# branches of k_recount<4> (tiles of 1024 tokens, 4 per thread) by T
K4_WANT = {1: _P, 3: _P, 15: _P | _F, 16: _F, 17: _P | _F, 1023: _P | _F, 1024: _F, 1025: _P | _F | {"two_tiles"},
           4096: _WIDE | {"one_row", "two_tiles"}, 4097: _WIDE | _P | {"one_row", "two_tiles"},
           4101: _WIDE | _P | {"one_row", "two_tiles"}, 8200: _WIDE | {"one_row", "two_tiles"}}
# branches of k_recount_reg (tiles of ops.RECOUNT_TILE tokens, 16 per thread) by T
REG_WANT = {1: _P, 15: _P, 16: _F, 17: _P | _F, 4096: _WIDE | {"word_change"},
            4097: _WIDE | _P | {"word_change", "two_tiles"},
            8200: _WIDE | _P | {"word_change", "two_tiles", "one_row"}}
APPLY_SHAPES = [(3, 4), (20, 20), (20, 24), (50, 52), (255, 256)]  # (K, KS)


# ------------------------------------------------------------------------------------------------
# 1. recount
# ------------------------------------------------------------------------------------------------
def recount_cap(KS):
    return max(1, ops.RECOUNT_CELLS // KS)


def recount_tile(T, KS, with_slots, stream=True):
    """Tokens per block of the kernel ops.recount picks: k_recount_reg works on ops.RECOUNT_TILE,
    k_recount<4> on 1024 and k_recount<16> on 4096 tokens; (tile, tokens per thread E)."""
    if not with_slots and KS <= 32 and stream:
        return ops.RECOUNT_TILE, 16
    return (1024, 4) if T < RECOUNT_LARGE else (4096, 16)


def recount_words(T, KS, tile):
    """Word-sorted ids of T tokens: word 0 owns more than two tiles (capped at half of a short T), a
    run of single-token words wider than the LDS cap follows, then three words whose ids lie more
    than the cap apart, then word V - 1. Returns (wsorted int32 [T], V)."""
    cap = recount_cap(KS)
    heavy = min(2 * tile + 5, T // 2)
    last = min(3, T - heavy)
    body = T - heavy - last
    singles = min(cap + 5, body)
    far = body - singles
    gap = 3 * cap + 7
    ids = [np.zeros(heavy, I64), np.arange(1, singles + 1, dtype=I64)]
    ids.append(singles + gap * (1 + (np.arange(far, dtype=I64) * 3) // max(far, 1)))
    top = max(int(a[-1]) for a in ids if a.size) if heavy + body else -1
    ids.append(np.full(last, top + gap + 1, I64))
    ws = np.concatenate(ids).astype(I32)
    assert ws.size == T and bool(np.all(np.diff(ws) >= 0))
    return ws, int(ws[-1]) + 1


def recount_reached(ws, tile, E, cap):
    """The kernel branches a word-sorted id array drives, by the kernels' own arithmetic."""
    T = ws.size
    starts = np.arange(0, T, tile)
    ends = np.minimum(starts + tile, T) - 1
    w_lo = ws[starts].astype(I64)
    span = ws[ends].astype(I64) - w_lo + 1
    rel = ws.astype(I64) - np.repeat(w_lo, ends - starts + 1)
    first = np.r_[True, ws[1:] != ws[:-1]]
    first[starts] = True
    distinct = np.add.reduceat(first.astype(I64), starts)
    step = np.r_[0, np.diff(ws.astype(I64))]
    step[starts] = 0
    inner = first.copy()  # a word change inside one thread's E contiguous tokens
    inner[::E] = False
    got = set()
    if bool((span == 1).any()):
        got.add("one_row")          # rows == 1: a tile inside one word
    if bool((rel >= cap).any()):
        got.add("past_cap")         # r >= rows: straight to a global atomic
    if bool((distinct > cap).any()):
        got.add("dense_run")        # more distinct words in a tile than LDS rows
    if bool((step > cap).any()):
        got.add("gap")              # ids more than the cap apart inside one tile
    if T >= E:
        got.add("full_thread")      # base + E <= hi: the vector loads
    if T % E:
        got.add("part_thread")      # base < hi < base + E (k_recount), n < E (k_recount_reg)
    if T > tile:
        got.add("two_tiles")
    if bool(inner.any()):
        got.add("word_change")      # k_recount_reg: flush(cur) before the last one
    return got


def recount_topics(r, n, K):
    z = r.integers(0, K, n).astype(U8)
    z[0], z[-1] = 0, K - 1
    return z


def recount_oracle(nwk0, ws, z, V, KS):
    cnt = np.bincount(ws.astype(I64) * KS + z.astype(I64), minlength=V * KS)
    return (nwk0.astype(I64).reshape(-1) + cnt).astype(I32).reshape(V, KS)


def run_recount(device, ws, V, KS, K, r, with_slots):
    """ops.recount on a pre-filled table against the bincount oracle."""
    T = ws.size
    if with_slots:
        n_slots = T + T // 3 + 7  # a slot array longer than T: the other slots are padding
        slot = r.permutation(n_slots)[:T].astype(I32)
        tok_z = r.integers(0, K, n_slots).astype(U8)  # padding slots hold topics nobody may count
        z = recount_topics(r, T, K)
        tok_z[slot] = z
        assert n_slots > T and np.unique(slot).size == T
    else:
        slot, z = None, recount_topics(r, T, K)
        tok_z = z
    assert int(z.max()) < K <= KS and (T < 2 or (int(z.min()) == 0 and int(z.max()) == K - 1))
    assert int(ws[-1]) == V - 1
    nwk0 = prefill((V, KS), seed=T)
    want = recount_oracle(nwk0, ws, z, V, KS)
    out = to(nwk0, device)
    ops.recount(to(ws, device), to(slot, device) if with_slots else None, to(tok_z, device), out, KS)
    got = back(out)
    assert same_bits(got, want), f"{int((got != want).sum())} of {want.size} cells differ"
    assert same_bits(got[:, K:], nwk0[:, K:])


def check_recount(device, T, KS, with_slots, want=(), stream=True):
    K = TOPICS[KS]
    tile, E = recount_tile(T, KS, with_slots, stream)
    ws, V = recount_words(T, KS, tile)
    reached = recount_reached(ws, tile, E, recount_cap(KS))
    assert set(want) <= reached, f"T={T} KS={KS}: {sorted(set(want) - reached)} not reached"
    run_recount(device, ws, V, KS, K, np.random.default_rng([T, KS, int(with_slots)]), with_slots)


@functools.lru_cache(maxsize=1)
def zipf_words(T, V):
    """Word-sorted ids of T tokens with Zipf(1) word frequencies over V words; read-only."""
    r = np.random.default_rng(T)
    p = 1.0 / np.arange(1, V + 1)
    cnt = r.multinomial(T, p / p.sum())
    if cnt[V - 1] == 0:
        cnt[V - 1], cnt[0] = 1, cnt[0] - 1
    ws = np.repeat(np.arange(V, dtype=I32), cnt)
    ws.setflags(write=False)
    return ws


def check_recount_large(device, KS, with_slots):
    """k_recount<16>: the smallest T that reaches it is the launcher's threshold."""
    T, V = RECOUNT_LARGE + 37, 50_000
    assert T >= (8 << 20)  # csrc/kernels/gibbs.hip, oni_recount: `if (T < (int64_t(8) << 20))`
    ws = zipf_words(T, V)
    tile, E = recount_tile(T, KS, with_slots)
    assert (tile, E) == (4096, 16) and not (not with_slots and KS <= 32)
    reached = recount_reached(ws, tile, E, recount_cap(KS))
    assert {"one_row", "past_cap", "dense_run", "full_thread", "part_thread", "two_tiles"} <= reached
    run_recount(device, ws, V, KS, TOPICS[KS], np.random.default_rng([KS, 16]), with_slots)


# ------------------------------------------------------------------------------------------------
# 2. delta recount
# ------------------------------------------------------------------------------------------------
def check_delta_recount(device, T, KS, G, stray=False):
    """``stray``: some UNMARKED tokens have z != z_prev; only the mask decides (device contract)."""
    r = np.random.default_rng([T, KS, G, int(stray)])
    K, S, tile, wmax = TOPICS[KS], 64 // G, ops.RECOUNT_TILE, recount_cap(KS)
    n_slots = -(-(T + T // 4 + 5) // S) * S
    assert n_slots % S == 0 and n_slots > T
    slots = np.sort(r.choice(n_slots, T, replace=False))
    V = 4 * wmax + 50
    tok_word = np.full(n_slots, -1, I32)  # PAD
    tok_word[slots] = r.integers(0, V, T)
    # the word-sorted index, as oni355/models/corpus.py builds it
    order = np.argsort(tok_word[slots], kind="stable")
    wsorted, wslot = tok_word[slots][order], slots[order].astype(I32)
    starts = np.arange(0, T, tile)
    tile_wlo = wsorted[starts]
    tile_whi = wsorted[np.minimum(starts + tile - 1, T - 1)]

    z = r.integers(0, K, n_slots).astype(U8)
    zp = z.copy()
    pad = np.setdiff1d(np.arange(n_slots), slots)
    zp[pad] = (z[pad] + 1) % K  # padding slots differ too: nobody may visit them
    pos = np.arange(T)
    cand = pos[pos // tile != 1]  # the second tile carries no marked token
    mpos = cand[r.random(cand.size) < 0.08]
    if mpos.size == 0:
        mpos = cand[:1]
    ms = wslot[mpos].astype(I64)
    moved = r.random(ms.size) < 0.85
    moved[0] = True
    if ms.size > 1:
        moved[-1] = False  # marked, but z == z_prev: nets to zero
    zp[ms[moved]] = (z[ms[moved]] + 1 + r.integers(0, K - 1, int(moved.sum()))) % K
    marked = np.zeros(n_slots, bool)
    marked[ms] = True
    unmarked = slots[~marked[slots]]
    if stray:
        st = unmarked[r.random(unmarked.size) < 0.05]
        zp[st] = (z[st] + 1) % K
        assert st.size > 0
    else:
        assert bool((z[unmarked] == zp[unmarked]).all())  # "marked" == what the CPU twin derives

    mask = np.zeros(n_slots // S, np.uint64)
    np.bitwise_or.at(mask, ms // S, np.uint64(1) << ((ms % S) * G).astype(np.uint64))
    if G > 1:  # noise on the bits of a unit's other lanes: only bit (slot % S) * G may be read
        nz = unmarked[r.random(unmarked.size) < 0.3].astype(I64)
        lane = 1 + r.integers(0, G - 1, nz.size)
        np.bitwise_or.at(mask, nz // S, np.uint64(1) << ((nz % S) * G + lane).astype(np.uint64))
    mask = mask.view(I64)

    # the branches these inputs reach
    w_m = tok_word[ms].astype(I64)
    t_m = mpos // tile
    rel = w_m - tile_wlo[t_m]
    rows = np.minimum(tile_whi.astype(I64) - tile_wlo + 1, wmax)
    assert ms.size >= 1 and bool((z[ms] != zp[ms]).any())
    if T >= 255:
        assert bool((tile_whi.astype(I64) - tile_wlo + 1 > wmax).any()), "no tile spans more than wmax words"
        assert bool((rel < rows[t_m]).any()) and bool((rel >= rows[t_m]).any()), "LDS and global side"
        assert bool((z[ms] == zp[ms]).any()), "no marked token with z == z_prev"
    if T > tile:
        assert starts.size >= 2 and not bool((t_m == 1).any()), "the second tile must stay unmarked"
    if T >= 4096:
        assert bool((ms % S == S - 1).any()) and bool((ms % S == 0).any()), "first and last bit of a mask word"

    d0 = prefill((V, KS), seed=G)
    want = d0.astype(I64)
    np.add.at(want, (w_m, z[ms].astype(I64)), 1)
    np.add.at(want, (w_m, zp[ms].astype(I64)), -1)
    zp_want = zp.copy()
    zp_want[ms] = z[ms]
    if stray:
        assert bool((zp_want[st] != z[st]).all())

    d, zt, zpt, mt = to(d0, device), to(z, device), to(zp, device), to(mask, device)
    ops.delta_recount(to(wslot, device), to(tile_wlo, device), to(tile_whi, device), mt, to(tok_word, device), zt, zpt,
                      d, KS, G)
    assert same_bits(back(d), want.astype(I32)), "Δn_wk"
    assert same_bits(back(zpt), zp_want), "tok_zprev"
    assert same_bits(back(zt), z) and same_bits(back(mt), mask), "tok_z / chg_mask must not change"


# ------------------------------------------------------------------------------------------------
# 3. word-bitmap delta recount
# ------------------------------------------------------------------------------------------------
def wdelta_words(T):
    """Three tokens per word; the last 40 % of the positions lie 66 000 ids further on, so the block
    that holds the jump has rows that do not fit 16 bits."""
    i = np.arange(T, dtype=I64)
    return (i // 3 + np.where(i >= (T * 3) // 5, 66_000, 0)).astype(I32)


def check_wdelta_recount(device, T, KS):
    r = np.random.default_rng([T, KS, 4])
    K, wmax, B = TOPICS[KS], recount_cap(KS), ops.WBITS_BLOCK
    ws = wdelta_words(T)
    V = int(ws[-1]) + 1
    nw = -(-T // 32)
    bits = np.zeros(nw + 1, np.uint32)  # one spare word past T: stays zero
    pcs = []
    for j in range(nw):
        valid = min(32, T - 32 * j)
        pc = (32, 0, 1, 4, 5, int(r.integers(0, 9)))[j % 6]
        if j == nw - 1:
            pc = max(pc, 1)  # the word that is only partly inside T carries a token
        pc = min(pc, valid)
        b = r.choice(valid, pc, replace=False)
        bits[j] = np.bitwise_or.reduce(np.uint32(1) << b.astype(np.uint32)) if pc else 0
        pcs.append(pc)
    assert T % 32 != 0 and bits[nw - 1] != 0 and int(bits[nw - 1]) >> (T - 32 * (nw - 1)) == 0
    pos = np.nonzero(np.unpackbits(bits.view(U8), bitorder="little")[:T])[0]
    assert pos.size == sum(pcs)

    # records: high half = the row in the block (0xFFFF: too far), low half = old | new << 8
    rel = ws.astype(I64) - np.repeat(ws[::B].astype(I64), B)[:T]
    high = np.minimum(rel, 0xFFFF)
    rec0 = ops.wdelta_records(to(ws, device))
    assert same_bits(back(rec0).view(np.uint32) >> 16, high.astype(np.uint32)), "wdelta_records"
    zo, zn = r.integers(0, K, T), r.integers(0, K, T)
    if pos.size > 1:
        zn[pos[1]] = zo[pos[1]]  # a marked token that stays: nets to zero
    rec = ((high << 16) | (zn << 8) | zo).astype(np.uint32).view(I32)

    starts = np.arange(0, T, B)
    ends = np.minimum(starts + B, T) - 1
    rows = np.minimum(ws[ends].astype(I64) - ws[starts] + 1, wmax)
    prow = rows[pos // B]
    if T >= 31:
        assert bool((rel[pos] >= 0xFFFF).any()), "no marked row re-read from wsorted"
        assert bool((rel[pos] < prow).any()), "no marked row in the LDS table"
    if T >= 33:
        assert 32 in pcs and 1 in pcs
    if T >= 8191:
        assert {0, 1, 4, 5, 32} <= set(pcs), "bitmap words of 0, 1, 4, 5 and 32 set bits"
        assert bool((ws[ends].astype(I64) - ws[starts] + 1 > 0xFFFF).any())
        assert bool(((rel[pos] >= prow) & (rel[pos] < 0xFFFF)).any()), "no marked row past wmax that fits 16 bits"

    d0 = prefill((V, KS), seed=T)
    want = d0.astype(I64)
    np.add.at(want, (ws[pos].astype(I64), zn[pos]), 1)
    np.add.at(want, (ws[pos].astype(I64), zo[pos]), -1)

    d, wb, rt = to(d0, device), to(bits.view(I32), device), to(rec, device)
    ops.wdelta_recount(wb, to(ws, device), rt, d, KS)
    assert same_bits(back(d), want.astype(I32)), "Δn_wk"
    assert not back(wb).any(), "the bitmap must be cleared"
    assert same_bits(back(rt), rec), "the records must not change"


# ------------------------------------------------------------------------------------------------
# 4. apply
# ------------------------------------------------------------------------------------------------
BIG1, BIG3 = 2**24 + 1, 2**24 + 3  # a tie and a round-up of the int -> f32 conversion
SENTINEL = 0x5A5A5A5A


def apply_inputs(V, K, KS, nk_rep, r):
    """(nwk, head, reps, nk_cur, nk_want): tables whose sum plants the edge values; nk_want[0] = 0,
    [1] = 1, [2] = 2^24 + 1 and [K - 1] = 2^24 + 3 where K > 3."""
    new = r.integers(5, 1000, (V, KS)).astype(I64)  # n_wk after the apply, padding columns too
    new[0, 2] = BIG1
    new[V - 1, K - 1 if K > 3 else 1] = BIG3
    head = r.integers(-5, 6, (V, KS)).astype(I64)
    head[0, 0] = -5
    nk_want = r.integers(2, 100_000, KS).astype(I64)
    nk_want[0], nk_want[1], nk_want[2] = 0, 1, BIG1
    if K > 3:
        nk_want[K - 1] = BIG3
    nk_cur = r.integers(1, 100_000, KS).astype(I64)
    nk_want[K:] = nk_cur[K:]  # padding columns: Δn_k is zero, n_k is copied through
    tot = nk_want - nk_cur
    reps = r.integers(-1000, 1001, (nk_rep, KS)).astype(I64)
    reps[:, K:] = 0
    reps[-1] += tot - reps.sum(0)
    assert bool((reps.sum(0) + nk_cur == nk_want).all()) and bool((head < 0).any())
    return (new - head).astype(I32), head.astype(I32), reps.astype(I32), nk_cur.astype(I32), nk_want.astype(I32)


def delta_buffer(head, reps, aux):
    return np.concatenate([head.reshape(-1), reps.reshape(-1), np.full(ops.DN_AUX, aux, I32)]).astype(I32)


def check_apply(device, K, KS, nk_rep, V, mode, bump=True):
    r = np.random.default_rng([K, KS, nk_rep, V])
    nwk0, head, reps, nk_cur, nk_want = apply_inputs(V, K, KS, nk_rep, r)
    beta, vbeta = 0.01, float(np.float32(V * 0.01))
    after = nwk0.astype(I64) + head
    if mode == "absolute":
        nwk_in, head_in = prefill((V, KS), seed=3) * 1000, after.astype(I32)  # garbage that must vanish
    elif mode == "inplace":
        nwk_in, head_in = after.astype(I32), np.full((V, KS), SENTINEL, I32)  # Δ head: never read
    else:
        nwk_in, head_in = nwk0, head
    dcur0 = delta_buffer(head_in, reps, 777)
    dother0 = np.full(dcur0.size, SENTINEL, I32)
    n_want, k_want, q_want, qf_want = spec.gibbs_apply(after.astype(I32), np.zeros((V, KS), I32),
                                                       reps.astype(I64).sum(0).astype(I32), nk_cur, K, beta, vbeta)
    assert same_bits(k_want, nk_want)
    # what these values pin, from the oracle's own tables
    assert same_bits(qf_want[:, 0], np.array([1, 0], np.float32)) and k_want[0] == 0  # an empty topic
    assert k_want[1] == 1 and qf_want[0, 1] != 1 and np.isfinite(qf_want[:, 1]).all()  # exactly one token
    assert same_bits(q_want[:, K:], np.zeros((V, KS - K), np.float32))
    assert same_bits(qf_want[:, K:], np.repeat(np.array([[1], [0]], np.float32), KS - K, 1))
    assert same_bits(k_want[K:], nk_cur[K:]) and (K == KS or bool(nk_cur[K:].all()))
    assert np.float32(BIG1) == 2**24 and np.float32(BIG3) == 2**24 + 4 and BIG1 in k_want and BIG1 in n_want

    t = dict(nwk=to(nwk_in, device), dcur=to(dcur0, device), dother=to(dother0, device), nk_cur=to(nk_cur, device),
             nk_next=to(np.full(KS, -99, I32), device), q=to(np.full((V, KS), np.nan, np.float32), device),
             qfix=to(np.full((2, KS), np.nan, np.float32), device), ctr=to(np.array([41], I32), device))
    ops.gibbs_apply(t["nwk"], t["dcur"], t["dother"], t["nk_cur"], t["nk_next"], t["q"], t["qfix"], V, K, KS, beta,
                    vbeta, t["ctr"], bump=bump, absolute=mode == "absolute", inplace=mode == "inplace")
    assert same_bits(back(t["nwk"]), n_want), "n_wk"
    assert same_bits(back(t["nk_next"]), k_want), "n_k"
    assert same_bits(back(t["q"]), q_want), "q"
    assert same_bits(back(t["qfix"]), qf_want), "qfix"
    do = back(t["dother"])
    if mode == "inplace":
        assert bool((do[: V * KS] == SENTINEL).all()), "in place: the Δ head of dother is not touched"
        assert not do[V * KS:].any(), "the replicas and the DN_AUX words of dother are zeroed"
    else:
        assert not do.any(), "dother (Δ head, replicas, DN_AUX words) is zeroed"
    assert int(back(t["ctr"])[0]) == (42 if bump else 41)
    assert same_bits(back(t["dcur"]), dcur0) and same_bits(back(t["nk_cur"]), nk_cur), "dcur / nk_cur are read-only"


def _apply_call(device, V, K, KS, r, nk_rep=2, **kw):
    """A delta apply on small random tables; returns the device tensors for the side under test."""
    nwk0, head, reps, nk_cur, _ = apply_inputs(V, K, KS, nk_rep, r)
    dcur = delta_buffer(head, reps, 1)
    t = dict(nwk=to(nwk0, device), dcur=to(dcur, device), dother=to(np.zeros_like(dcur), device),
             nk_cur=to(nk_cur, device), nk_next=to(np.zeros(KS, I32), device),
             q=to(np.zeros((V, KS), np.float32), device), qfix=to(np.zeros((2, KS), np.float32), device),
             ctr=to(np.zeros(1, I32), device))
    ops.gibbs_apply(t["nwk"], t["dcur"], t["dother"], t["nk_cur"], t["nk_next"], t["q"], t["qfix"], V, K, KS, 0.01,
                    float(np.float32(V * 0.01)), t["ctr"], **kw)
    want = spec.gibbs_apply(nwk0, head, reps.astype(I64).sum(0).astype(I32), nk_cur, K, 0.01,
                            float(np.float32(V * 0.01)))
    for name, w in zip(("nwk", "nk_next", "q", "qfix"), want):
        assert same_bits(back(t[name]), w), name
    return want


def check_apply_rows(device, case, KS=20):
    """The fused row copy (rdst[r] := rsrc[r])."""
    r = np.random.default_rng([KS, len(case)])
    V, K, D = 3, TOPICS[KS], 60
    src = r.integers(0, 10**6, (D, KS)).astype(I32)
    dst0 = r.integers(-10**6, 0, (D, KS)).astype(I32)
    rows = {"empty": np.zeros(0, I32), "subset": r.permutation(D)[:7].astype(I32),
            "many": r.permutation(D)[:40].astype(I32)}[case]
    if case == "subset":
        assert 0 < rows.size * KS and rows.size < D
    if case == "many":
        assert rows.size * KS > V * KS // 4 and rows.size * KS > 256  # the grid is sized by the rows
    want = dst0.copy()
    want[rows.astype(I64)] = src[rows.astype(I64)]
    st, dt = to(src, device), to(dst0, device)
    _apply_call(device, V, K, KS, r, rows_copy=(st, dt, to(rows, device)))
    assert same_bits(back(dt), want) and same_bits(back(st), src)


def check_apply_acc(device, wide, V=3, D=5, KS=24):
    """The posterior sums: bit 0 / 1 / 2 of ``wide`` makes wk / k / dk int64."""
    r = np.random.default_rng([wide, V, D])
    K = TOPICS[KS]
    dts = [np.int64 if wide >> b & 1 else np.int32 for b in range(3)]
    sums0 = [r.integers(1, 1000, s).astype(dt) for s, dt in zip(((V, KS), (KS,), (D, KS)), dts)]  # start non-zero
    ndk = r.integers(0, 5000, (D, KS)).astype(I32)
    ts = [to(s, device) for s in sums0]
    nt = to(ndk, device)
    n_want, k_want, _, _ = _apply_call(device, V, K, KS, r, acc=(ts[0], ts[1], ts[2], nt))
    for got, s0, add, dt, name in zip(ts, sums0, (n_want, k_want, ndk), dts, ("wk", "k", "dk")):
        assert got.dtype == (torch.int64 if dt is np.int64 else torch.int32)
        assert same_bits(back(got), (s0.astype(I64) + add.astype(I64)).astype(dt)), name
    assert same_bits(back(nt), ndk)


# ------------------------------------------------------------------------------------------------
# 5. exact guard, row copy
# ------------------------------------------------------------------------------------------------
GUARD_CASES = ("empty", "at_limit", "over_last", "over_first", "over_padding", "over_unlisted")
# (case, K, KS); there is no padding column at K == KS
GUARD_PARAMS = [(c, K, KS) for K, KS in ((20, 20), (50, 52)) for c in GUARD_CASES if c != "over_padding" or K < KS]


def check_exact_guard(device, case, K, KS):
    r = np.random.default_rng([K, KS])
    D, limit = 90, 16_000
    ndk = r.integers(0, limit, (D, KS)).astype(I32)
    rows = r.permutation(D)[:40].astype(I32)
    unlisted = np.setdiff1d(np.arange(D), rows)
    want = 1
    if case == "empty":
        rows = np.zeros(0, I32)
        ndk[:] = limit + 1
    elif case == "at_limit":
        ndk[rows[-1], K - 1] = limit
        ndk[rows[0], 0] = limit
    elif case == "over_last":  # the last element examined: a thread reaches it on a later stride
        ndk[rows[-1], K - 1] = limit + 1
        want = 0
        assert rows.size * K > 2 * 256 and (rows.size * K - 1) // 256 >= 2
    elif case == "over_first":
        ndk[rows[0], 0] = limit + 1
        want = 0
    elif case == "over_padding":
        assert KS > K
        ndk[:, K:] = limit + 1
    elif case == "over_unlisted":
        assert unlisted.size > 0
        ndk[unlisted] = limit + 1
    ref = 1 if rows.size == 0 else int(not (ndk[rows.astype(I64), :K].astype(I64) > limit).any())
    assert ref == want
    flag = to(np.array([1 - want], I32), device)  # pre-set to the opposite value
    nt = to(ndk, device)
    ops.exact_guard(nt, to(rows, device), K, limit, flag)
    assert int(back(flag)[0]) == want
    assert same_bits(back(nt), ndk)


def check_copy_rows(device, case, KS):
    r = np.random.default_rng([KS, len(case), 5])
    D = 37
    src = r.integers(0, 10**6, (D, KS)).astype(I32)
    dst0 = r.integers(-10**6, 0, (D, KS)).astype(I32)
    rows = {"empty": np.zeros(0, I32), "one": np.array([D - 1], I32), "all": r.permutation(D).astype(I32)}[case]
    want = dst0.copy()
    want[rows.astype(I64)] = src[rows.astype(I64)]
    st, dt = to(src, device), to(dst0, device)
    ops.copy_rows(st, dt, to(rows, device), KS)
    assert same_bits(back(dt), want), "rows not listed keep dst's contents"
    assert same_bits(back(st), src)
