"""CPU suite: the slot-group rule of a block (nep_kernels.hip block_split, through the host-only entry point
nep_debug_block_split).  A block of `na` iterating slots may run as two groups of ceil(na / 2) and floor(na / 2) slots
only where every x-pass launch of a group has the waves per workgroup (TW) of the launch over all na slots, plain and
certificate variant alike: TW fixes the order in which the column partials are added, i.e. the last bits of an LP.
No device calls: nothing here needs a GPU."""
import pytest

import iter_cases as ic

REFERENCE, FACILITY = 0, 1
# (functions, nodes, relaxation): the flagship replay's shape on either relaxation, and a shape whose tile still
# changes at 16 slots
SHAPES = ((256, 512, REFERENCE), (64, 24, REFERENCE), (256, 512, FACILITY))


def _rule(F, N, relaxation):
    """na -> (first group's slots or 0, plain TW, certificate TW) for na = 1 .. 64."""
    from core.engine.lp import debug_block_split
    return {na: debug_block_split(N, F, na, relaxation) for na in range(1, 65)}


@pytest.mark.parametrize("F,N,relaxation", SHAPES)
def test_split_only_where_both_halves_keep_the_tile(F, N, relaxation):
    got = _rule(F, N, relaxation)
    for na, (nA, tw_plain, tw_check) in got.items():
        assert tw_plain in (4, 8, 16) and tw_check in (4, 8, 16)
        if relaxation == REFERENCE:      # the launchers' tile is the one the test-suite's mirror computes
            assert (tw_plain, tw_check) == (ic.tile_waves(N, na, False, F), ic.tile_waves(N, na, True, F)), na
        a, b = (na + 1) // 2, na // 2
        same = b >= 1 and all(got[h][1:] == (tw_plain, tw_check) for h in (a, b))
        assert nA in (0, a), (na, nA)
        assert (nA == a) == same, (na, nA, got[a], got[b] if b else None)


def test_flagship_shape_splits_from_eight_slots_on():
    for relaxation in (REFERENCE, FACILITY):
        got = _rule(256, 512, relaxation)
        assert [na for na in got if got[na][0]] == list(range(8, 65)), relaxation
        assert all(got[na][0] == (na + 1) // 2 for na in range(8, 65))


def test_tile_change_refuses_the_split():
    """F = 64, N = 24: 16 slots run 4 waves per workgroup, 8 slots would run 8."""
    got = _rule(64, 24, REFERENCE)
    assert got[16][1:] == (4, 4) and got[8][1:] == (8, 8) and got[16][0] == 0
    assert got[32][0] == 16      # both halves at 4 waves


def test_bad_arguments():
    from core.engine.lp import EngineUnavailable, debug_block_split
    for args in ((24, 4, 0), (0, 4, 1), (24, 0, 1), (4096, 4, 1)):
        with pytest.raises(EngineUnavailable):
            debug_block_split(*args)
