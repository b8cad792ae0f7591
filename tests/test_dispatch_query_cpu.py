"""The dense samplers' selection ladder, asked without a device (ops.gibbs_which -> oni_gibbs_which:
the select_gibbs the launch itself goes through, csrc/kernels/gibbs_sampler.h)."""
import itertools

import pytest

from oni355 import ops

_TILINGS = [(1, kp) for kp in range(4, 33, 4)] + [(2, 20), (2, 24), (2, 28)] + [(4, kp) for kp in range(8, 29, 4)] + [
    (8, 8), (8, 12), (8, 16), (16, 8), (16, 16)]


def _picks(ab):
    for (G, KP), mode, air, aligned, lag, guard in itertools.product(_TILINGS, range(5), (False, True), (False, True),
                                                                     (False, True), (False, True)):
        for qpf in (0, 3 if G == 1 else 2):
            first, twin = ops.gibbs_which(G, KP, mode, qpf, alpha_in_row=air, pos_aligned=aligned, lag=lag, guard=guard)
            yield (G, KP, mode, qpf, air, aligned, lag, guard, ab), first, twin


@pytest.mark.parametrize("ab", ["0", "1", "2", "4", "8"])
def test_one_sampler_runs_for_either_guard_flag(monkeypatch, ab):
    """For every instantiated tiling, count mode, sampler argument, flag combination and dense
    ONI_SAMPLER_AB bit: a guarded generic twin follows exactly the first picks that return when the
    guard's flag is 0 (the row-f32 kernels), so one sampler sweeps the tokens whatever the flag
    says -- never two (a twin behind the unguarded generic kernel), never none."""
    monkeypatch.setenv("ONI_SAMPLER_AB", ab)
    n_twins = 0
    for case, first, twin in _picks(ab):
        G, KP, mode, qpf, air, aligned, lag, guard, _ = case
        assert first is not None and first.mode == mode and not first.init and not first.twin, case
        assert first.guard == (first.family != "generic"), case
        assert first.family in (("generic", "x1") if G == 1 else ("generic", "ldsg")), case
        if qpf == 0 or (G > 1 and not air):
            assert first.family == "generic", case
        if first.family == "generic":
            assert first.lag == lag, case
        elif lag:
            assert first.lag and mode in (0, 4), case
        if guard:
            # flag 1: the first pick runs and a twin returns. Flag 0: the first pick runs unless it
            # reads the flag, and a twin runs
            assert (not first.guard) + (twin is not None) == 1, case
        else:
            assert twin is None, case
        if twin is not None:
            n_twins += 1
            got = (twin.family, twin.mode, twin.twin, twin.guard, twin.lag)
            assert got == ("generic", mode, True, False, lag), case
    assert n_twins > 0


def test_lagged_guard_cases_that_ran_two_samplers():
    """The three first picks behind which a guarded twin was launched although they do not read
    the flag (lag x guard: one-lane delta, one-lane unaligned wdelta, two-lane delta)."""
    for G, KP, mode, aligned in ((1, 20, 2, True), (1, 20, 4, False), (2, 28, 2, True)):
        first, twin = ops.gibbs_which(G, KP, mode, 3 if G == 1 else 2, alpha_in_row=True, pos_aligned=aligned, lag=True,
                                      guard=True)
        assert (first.family, first.guard, first.lag, twin) == ("generic", False, True, None)


def test_init_pass_and_bad_arguments():
    first, twin = ops.gibbs_which(4, 28, 0, 2, alpha_in_row=True, init=True)
    assert (first.family, first.init, first.mode, twin) == ("generic", True, 0, None)
    for G, KP in ((2, 16), (3, 20), (1, 36)):  # not instantiated
        with pytest.raises(RuntimeError):
            ops.gibbs_which(G, KP, 0, 0)
    with pytest.raises(RuntimeError):
        ops.gibbs_which(1, 20, 5, 3)
