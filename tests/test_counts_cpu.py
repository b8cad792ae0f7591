"""The CPU twins of the count-bookkeeping ops against the same NumPy oracles, inputs and branch
asserts as tests/test_gpu_counts.py (tests/counts_inputs.py): whatever the kernels of
csrc/kernels/gibbs.hip are held to, the ops' CPU branches give bit for bit too.

Left to the device file: the 8 Mi-token k_recount<16> cases (the threshold is the launcher's), the
width the streaming launcher refuses, and the unmarked-token contract of k_delta_recount (the twin
derives "changed" from z != z_prev; the inputs here keep the two equal).
"""
import pytest
import torch

import counts_inputs as cx
from oni355 import ops

CPU = torch.device("cpu")


@pytest.mark.parametrize("KS", [4, 20, 52, 256])
@pytest.mark.parametrize("T", [1, 3, 1023, 1024, 1025, 4101])
def test_recount_with_slots(T, KS):
    cx.check_recount(CPU, T, KS, True, cx.K4_WANT[T])


@pytest.mark.parametrize("KS", [4, 8, 12, 16, 20, 24, 28, 32, 52, 256])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 4096, 4097, 8200])
def test_recount_sorted_topics(T, KS):
    assert ops.STREAM_RECOUNT
    cx.check_recount(CPU, T, KS, False, cx.REG_WANT[T] if KS <= 32 else cx.K4_WANT[T])


@pytest.mark.parametrize("T", [1, 15, 16, 17, 4096, 4097, 8200])
def test_recount_without_streaming(monkeypatch, T):
    monkeypatch.setattr(ops, "STREAM_RECOUNT", False)
    cx.check_recount(CPU, T, 20, False, cx.K4_WANT[T], stream=False)


@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("KS", [20, 52, 256])
@pytest.mark.parametrize("T", [1, 255, 4096, 4097, 9000])
def test_delta_recount(T, KS, G):
    cx.check_delta_recount(CPU, T, KS, G)


@pytest.mark.parametrize("KS", [20, 52])
@pytest.mark.parametrize("T", [1, 31, 33, 8191, 8193, 20011])
def test_wdelta_recount(T, KS):
    cx.check_wdelta_recount(CPU, T, KS)


@pytest.mark.parametrize("mode", ["delta", "absolute", "inplace"])
@pytest.mark.parametrize("nk_rep", [1, 2, 32, 64])
@pytest.mark.parametrize("K,KS", cx.APPLY_SHAPES)
@pytest.mark.parametrize("V", [1, 3, 205])
def test_apply(V, K, KS, nk_rep, mode):
    if nk_rep == 64 and KS >= 20:
        assert nk_rep > 256 // KS  # more replicas than replica groups: a group sums several
    if KS == 256:
        assert 256 // KS == 1
    cx.check_apply(CPU, K, KS, nk_rep, V, mode, bump=nk_rep in (1, 32))


def test_apply_second_grid_trip():
    V, KS = 105_001, 20
    assert V * KS // 4 > 2048 * 256  # oni::grid_for(work, 256, 2048): some threads take two vectors
    cx.check_apply(CPU, 20, KS, 32, V, "delta")


@pytest.mark.parametrize("case", ["empty", "subset", "many"])
def test_apply_rows_copy(case):
    cx.check_apply_rows(CPU, case)


@pytest.mark.parametrize("wide", range(8))
def test_apply_acc(wide):
    cx.check_apply_acc(CPU, wide)


def test_apply_acc_sized_by_the_docs():
    V, D, KS = 3, 300, 24
    assert D * KS // 4 > V * KS // 4 and D * KS // 4 > 256
    cx.check_apply_acc(CPU, 5, V=V, D=D, KS=KS)


def test_apply_refuses_inplace_absolute():
    t = torch.zeros(4 + 4 + ops.DN_AUX, dtype=torch.int32, device=CPU)
    f = torch.zeros(2, 4, dtype=torch.float32, device=CPU)
    with pytest.raises(ValueError, match="in place"):
        ops.gibbs_apply(t[:4].view(1, 4).clone(), t, t.clone(), t[:4].clone(), t[:4].clone(), f[:1].clone(), f, 1, 3, 4,
                        0.01, 0.01, t[:1].clone(), absolute=True, inplace=True)


@pytest.mark.parametrize("case,K,KS", cx.GUARD_PARAMS)
def test_exact_guard(case, K, KS):
    cx.check_exact_guard(CPU, case, K, KS)


@pytest.mark.parametrize("KS", [20, 52])
@pytest.mark.parametrize("case", ["empty", "one", "all"])
def test_copy_rows(case, KS):
    cx.check_copy_rows(CPU, case, KS)
