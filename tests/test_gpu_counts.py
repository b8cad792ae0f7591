"""The kernels of csrc/kernels/gibbs.hip that turn a sweep's topic draws into tables, each driven
directly through its op and compared bit for bit with a NumPy oracle written in
tests/counts_inputs.py (np.bincount / np.add.at in int64; spec.gibbs_apply / spec.gibbs_qfix for q
and qfix). No tolerance anywhere. The same checks run on the ops' CPU twins in
tests/test_counts_cpu.py, so kernel == oracle == twin on the same inputs.

Every check asserts on its own inputs that the branch it names is reached (counts_inputs.
recount_reached and the asserts before each launch), and every table a kernel adds into starts from
a non-zero pattern.

Kernel / branch                                       test id
k_recount<4>   wslot, T < E / partial thread          test_recount_with_slots[1|3|1023|1025|4101-*]
               full 16-B loads only                   test_recount_with_slots[1024-*]
               rows == 1 (a tile inside one word)     test_recount_with_slots[4101-*]
               r >= rows (run of single-token words
               wider than the cap; gap in the ids)    test_recount_with_slots[4101-*]; KS = 256: cap of 8 rows
               null wslot (KS > 32)                   test_recount_sorted_topics[*-52|256]
               null wslot (STREAM_RECOUNT = False)    test_recount_without_streaming[*]
k_recount<16>  wslot / null wslot, T >= 8 Mi          test_recount_large[20-True], [52-False]
k_recount_reg  <4> <8> <12> <16> <20> <24> <28> <32>  test_recount_sorted_topics[*-4] ... [*-32]
               n < E tail                             test_recount_sorted_topics[1|15|17|4097|8200-*]
               full pass, flush on a word change      test_recount_sorted_topics[4096|4097|8200-*]
               second tile, rows == 1                 test_recount_sorted_topics[8200-*]
               KS <= 32, no multiple of 4: error      test_recount_stream_refuses_other_widths
k_delta_recount bit (slot & (S-1)) * G, G = 1..16     test_delta_recount[*-*-1|2|4|8|16]
               LDS / global split at wmax             test_delta_recount[255|4096|4097|9000-*]
               tok_zprev refresh, z == z_prev marked  test_delta_recount[*]
               tile_wlo / tile_whi, unmarked tile     test_delta_recount[4097|9000-*]
               the mask decides, not z != z_prev      test_delta_recount_only_marked_tokens_move[*]
k_wdelta_recount T no multiple of 32 / 8192           test_wdelta_recount[*]
               second round of the 4-bit loop         test_wdelta_recount[31|33|8191|8193|20011-*] (5, 31, 32 bits)
               r == 0xFFFF re-read of wsorted         test_wdelta_recount[31..20011-*]
               span past wmax                         test_wdelta_recount[8191|8193|20011-*]
               bitmap cleared, records untouched      test_wdelta_recount[*]
k_apply        delta / absolute / in place            test_apply[*-delta|absolute|inplace]
               nk_rep > 256 / KS groups; one group    test_apply[*-20-20-32|64-*] ...; test_apply[*-255-256-*]
               empty topic, one-token topic, 2^24 + 1 test_apply[*] (planted in every case)
               padding columns, dother, sweep_ctr     test_apply[*]
               second trip of the grid                test_apply_second_grid_trip
               fused row copy, grid sized by rows     test_apply_rows_copy[empty|subset|many]
               acc_wide 0..7                          test_apply_acc[0..7]
               D * KS / 4 the largest work size       test_apply_acc_sized_by_the_docs
               inplace with absolute                  test_apply_refuses_inplace_absolute
k_exact_guard  every case                             test_exact_guard[*]
k_copy_rows    empty / one / all rows                 test_copy_rows[*]
"""
import pytest
import torch

import counts_inputs as cx
from oni355 import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("KS", [4, 20, 52, 256])
@pytest.mark.parametrize("T", [1, 3, 1023, 1024, 1025, 4101])
def test_recount_with_slots(gpu, T, KS):
    cx.check_recount(gpu, T, KS, True, cx.K4_WANT[T])


@pytest.mark.parametrize("KS", [4, 8, 12, 16, 20, 24, 28, 32, 52, 256])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 4096, 4097, 8200])
def test_recount_sorted_topics(gpu, T, KS):
    assert ops.STREAM_RECOUNT
    cx.check_recount(gpu, T, KS, False, cx.REG_WANT[T] if KS <= 32 else cx.K4_WANT[T])


@pytest.mark.parametrize("T", [1, 15, 16, 17, 4096, 4097, 8200])
def test_recount_without_streaming(gpu, monkeypatch, T):
    monkeypatch.setattr(ops, "STREAM_RECOUNT", False)
    cx.check_recount(gpu, T, 20, False, cx.K4_WANT[T], stream=False)


@pytest.mark.parametrize("KS", [6, 30])
def test_recount_stream_refuses_other_widths(gpu, KS):
    """oni_recount_stream has no k_recount_reg<KS> for these: an error, not another kernel."""
    ws = torch.zeros(64, dtype=torch.int32, device=gpu)
    z = torch.zeros(64, dtype=torch.uint8, device=gpu)
    out = torch.zeros(1, KS, dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError, match="oni_recount_stream"):
        ops.recount(ws, None, z, out, KS)
    assert not bool(out.any())


@pytest.mark.parametrize("KS,with_slots", [(20, True), (52, False)])
def test_recount_large(gpu, KS, with_slots):
    cx.check_recount_large(gpu, KS, with_slots)


@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("KS", [20, 52, 256])
@pytest.mark.parametrize("T", [1, 255, 4096, 4097, 9000])
def test_delta_recount(gpu, T, KS, G):
    cx.check_delta_recount(gpu, T, KS, G)


@pytest.mark.parametrize("G", [1, 4])
def test_delta_recount_only_marked_tokens_move(gpu, G):
    """Unmarked tokens with z != z_prev touch neither Δn_wk nor tok_zprev (the CPU twin derives the
    change from z, so this contract is the kernel's alone)."""
    cx.check_delta_recount(gpu, 9000, 20, G, stray=True)


@pytest.mark.parametrize("KS", [20, 52])
@pytest.mark.parametrize("T", [1, 31, 33, 8191, 8193, 20011])
def test_wdelta_recount(gpu, T, KS):
    cx.check_wdelta_recount(gpu, T, KS)


@pytest.mark.parametrize("mode", ["delta", "absolute", "inplace"])
@pytest.mark.parametrize("nk_rep", [1, 2, 32, 64])
@pytest.mark.parametrize("K,KS", cx.APPLY_SHAPES)
@pytest.mark.parametrize("V", [1, 3, 205])
def test_apply(gpu, V, K, KS, nk_rep, mode):
    if nk_rep == 64 and KS >= 20:
        assert nk_rep > 256 // KS  # more replicas than replica groups: a group sums several
    if KS == 256:
        assert 256 // KS == 1
    cx.check_apply(gpu, K, KS, nk_rep, V, mode, bump=nk_rep in (1, 32))


def test_apply_second_grid_trip(gpu):
    V, KS = 105_001, 20
    assert V * KS // 4 > 2048 * 256  # oni::grid_for(work, 256, 2048): some threads take two vectors
    cx.check_apply(gpu, 20, KS, 32, V, "delta")


@pytest.mark.parametrize("case", ["empty", "subset", "many"])
def test_apply_rows_copy(gpu, case):
    cx.check_apply_rows(gpu, case)


@pytest.mark.parametrize("wide", range(8))
def test_apply_acc(gpu, wide):
    cx.check_apply_acc(gpu, wide)


def test_apply_acc_sized_by_the_docs(gpu):
    V, D, KS = 3, 300, 24
    assert D * KS // 4 > V * KS // 4 and D * KS // 4 > 256
    cx.check_apply_acc(gpu, 5, V=V, D=D, KS=KS)


def test_apply_refuses_inplace_absolute(gpu):
    t = torch.zeros(4 + 4 + ops.DN_AUX, dtype=torch.int32, device=gpu)
    f = torch.zeros(2, 4, dtype=torch.float32, device=gpu)
    with pytest.raises(ValueError, match="in place"):
        ops.gibbs_apply(t[:4].view(1, 4).clone(), t, t.clone(), t[:4].clone(), t[:4].clone(), f[:1].clone(), f, 1, 3, 4,
                        0.01, 0.01, t[:1].clone(), absolute=True, inplace=True)


@pytest.mark.parametrize("case,K,KS", cx.GUARD_PARAMS)
def test_exact_guard(gpu, case, K, KS):
    cx.check_exact_guard(gpu, case, K, KS)


@pytest.mark.parametrize("KS", [20, 52])
@pytest.mark.parametrize("case", ["empty", "one", "all"])
def test_copy_rows(gpu, case, KS):
    cx.check_copy_rows(gpu, case, KS)
