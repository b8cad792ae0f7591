"""One tiling table (ONI_TILINGS, csrc/kernels/gibbs_sampler.h) behind training and fold-in: every
(G, KP) ops.choose_tiling can return, and every pair of the table, is accepted by both launchers;
a pair outside it is refused by both. Asked without a device: oni_gibbs_which launches nothing, and
oni_foldin_launch returns before it touches HIP when the grid is empty (n_slices = 0)."""
import ctypes as C

import pytest

from oni355 import ops
from oni355.ops import _lib

# an independent copy of ONI_TILINGS: a tiling added to or taken from that table is edited here too
_TABLE = [(1, kp) for kp in range(4, 33, 4)] + [(2, 20), (2, 24), (2, 28)] + [(4, kp) for kp in range(8, 29, 4)] + [
    (8, 8), (8, 12), (8, 16), (16, 8), (16, 16)]
_HIP_INVALID_VALUE = 1


def _trains(G, KP):
    """oni_gibbs_which for the init pass and a sweep: both succeed or both refuse."""
    ok = []
    for init in (True, False):
        try:
            first, _ = ops.gibbs_which(G, KP, 0, 3 if G == 1 else 2, alpha_in_row=True, init=init)
            ok.append(first is not None and first.init == init)
        except RuntimeError as e:
            assert f"hipError {_HIP_INVALID_VALUE}" in str(e)
            ok.append(False)
    assert ok[0] == ok[1], (G, KP)
    return ok[0]


def _foldin_rc(G, KP, K, init):
    a = _lib.OniFoldin()
    a.n_slices, a.K, a.KS, a.sweep_lo, a.n_sweeps = 0, K, G * KP, 1, 1
    return _lib.lib().oni_foldin_launch(C.byref(a), G, KP, 1 if init else 0, None)


def _folds_in(G, KP, K):
    rc = [_foldin_rc(G, KP, K, init) for init in (True, False)]
    assert rc in ([0, 0], [_HIP_INVALID_VALUE] * 2), (G, KP, rc)
    return rc[0] == 0


@pytest.mark.parametrize("tiling", ["wide", "narrow"])
def test_every_chosen_tiling_trains_and_folds_in(monkeypatch, tiling):
    """The "mh" argument above K = 32 returns one-lane units wider than 32 topics: those run k_gibbs_mh through its
    own launcher (any KS), never the dense samplers or fold-in, and both of these refuse them."""
    monkeypatch.setenv("ONI_TILING", tiling)
    chosen = set()
    for K in range(1, 256):
        for sampler in (None, "mh"):
            G, KP = ops.choose_tiling(K, sampler)
            assert G * KP >= K
            dense = sampler is None or KP <= 32
            assert sampler is None or (G, KP) == (1, (K + 3) // 4 * 4)
            assert _folds_in(G, KP, K) == dense, (K, sampler, G, KP)
            if dense:
                chosen.add((G, KP))
            else:
                assert not _trains(G, KP), (K, sampler, G, KP)
    assert chosen <= set(_TABLE), chosen - set(_TABLE)
    for G, KP in chosen:
        assert _trains(G, KP), (G, KP)


def test_the_table_is_shared():
    for G, KP in _TABLE:
        assert _trains(G, KP), (G, KP)
        assert _folds_in(G, KP, G * KP if G * KP <= 255 else 255), (G, KP)
    for G, KP in ((2, 12), (16, 12), (2, 16), (8, 20), (3, 8), (1, 36), (1, 6)):
        assert not _trains(G, KP), (G, KP)
        assert not _folds_in(G, KP, min(G * KP, 255)), (G, KP)
