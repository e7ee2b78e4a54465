"""CPU: the host side of the native placement search (nep_leaf_search; DESIGN.md §7 "Native search") and the lazy rule of
core.engine.heuristics.placement_search on the mirror model (tests/leaf_search_ref.py).

 1. nep_debug_leaf_apply_move — the move application that rebuilds the search's z and the verified neighbours' bytes —
    equals heuristics.apply_move byte for byte on every move of the full move and swap lists of the fixture placements
    and of leaf 0 of 72x12 / 96x8; the lists hold a DROP of a node's last placement, a SWAP whose source node closes, a
    CLOSE and variants without n; a record out of range is refused and writes nothing
 2. placement_search(verify="all") returns what the call without the argument returns
 3. placement_search(verify="lazy") from leaf 0 of 96x8 and 72x12: every accepted step lowers upper, the end point
    passes check_point, at least one move is accepted and fewer neighbours are verified than evaluated
"""
import numpy as np
import pytest

import leaf_ref
import leaf_search_ref as qref
from leaf_cases import check_point
from leaf_moves_cases import NAMES as _ALL, case

NAMES = [name for name in _ALL if name != "wide"]
_LISTS = {}


def _lists(name):
    """[(k, z, moves)] of a case: every fixture placement, leaf 0 of a generated instance"""
    if name not in _LISTS:
        g = case(name)
        ks = range(len(g.Z)) if name.startswith("fixture") else [0]
        _LISTS[name] = [(k, np.asarray(g.Z[k], np.float64), qref.full_moves(g.inst, g.Z[k])) for k in ks]
    return case(name), _LISTS[name]


@pytest.mark.parametrize("name", NAMES)
def test_apply_move_is_the_products(name):
    from core.engine.heuristics import apply_move
    from core.engine.lp import debug_leaf_apply_move
    g, lists = _lists(name)
    F, N, has_n = g.inst.F, g.inst.N, bool(g.inst.has_n)
    total = 0
    for k, z, moves in lists:
        for kind, f, j, src in moves:
            want = apply_move(z, F, N, has_n, kind, f, j, src)
            got = debug_leaf_apply_move(z, F, N, has_n, kind, f, j, src)
            assert got.tobytes() == want.tobytes(), (name, k, kind, f, j, src)
            total += 1
    print(name, "moves applied", total)
    assert total > 0


def test_the_lists_hold_every_kind_of_move():
    seen = set()
    for name in NAMES:
        g, lists = _lists(name)
        tag = "n" if g.inst.has_n else "no n"
        for k, z, moves in lists:
            cnt = g.inst.split(z)[0].sum(axis=0)
            for kind, f, j, src in moves:
                seen.add((tag, kind))
                if kind == 1 and cnt[j] == 1:
                    seen.add("drop of the last placement")
                if kind == 3 and cnt[src] == 1:
                    seen.add("swap whose source closes")
    assert {"drop of the last placement", "swap whose source closes"} <= seen, seen
    assert {("n", kind) for kind in (0, 1, 2, 3)} <= seen, seen
    assert any(s[0] == "no n" for s in seen if isinstance(s, tuple)), seen


def test_apply_move_refuses_a_record_out_of_range():
    from core.engine.lp import EngineUnavailable, debug_leaf_apply_move
    F, N = 3, 4
    z = np.zeros(F * N + N)
    for kind, f, j, src in ((4, 0, 0, None), (-1, 0, 0, None), (0, 3, 0, None), (0, -1, 0, None), (1, 0, 4, None),
                            (2, -1, -1, None), (3, 0, 1, 4), (3, 0, 1, None)):
        with pytest.raises(EngineUnavailable) as e:
            debug_leaf_apply_move(z, F, N, True, kind, f, j, src)
        assert "(-1)" in str(e.value) and "out of range" in str(e.value), str(e.value)
    # a CLOSE ignores fn; an in-place call is allowed
    got = debug_leaf_apply_move(np.ones(F * N + N), F, N, True, 2, -1, 2)
    assert got[:F * N].reshape(F, N)[:, 2].sum() == 0 and got[F * N + 2] == 0 and got.sum() == F * N + N - F - 1


_SEARCH = dict(rounds=16, width=16, warm=False)


def test_verify_all_is_the_default_search():
    from core.engine.heuristics import placement_search
    g = case("72x12")
    base = placement_search(qref.MirrorModel(g.inst), g.Z[0], max_passes=3, **_SEARCH)
    got = placement_search(qref.MirrorModel(g.inst), g.Z[0], max_passes=3, verify="all", **_SEARCH)
    assert base["accepted"] and got["accepted"] == base["accepted"]
    assert sorted(got) == sorted(base)
    for key in ("upper", "lower", "start_upper", "passes", "evaluated", "verified"):
        assert got[key] == base[key], key
    for key in ("z", "row", "dst", "val"):
        assert np.asarray(got[key]).tobytes() == np.asarray(base[key]).tobytes(), key
    assert 0 < base["verified"] <= base["evaluated"]
    with pytest.raises(ValueError):
        placement_search(qref.MirrorModel(g.inst), g.Z[0], verify="some", **_SEARCH)
    with pytest.raises(ValueError):
        placement_search(qref.MirrorModel(g.inst), g.Z[0], verify="lazy", **_SEARCH)


@pytest.mark.parametrize("name", ["96x8", "72x12"])
def test_lazy_search_on_the_mirror(name):
    from core.engine.heuristics import placement_search
    g = case(name)
    r = placement_search(qref.MirrorModel(g.inst), g.Z[0], verify="lazy", rounds=16, repair_every=4, width=16,
                         max_passes=6, warm=True)
    print(name, r["start_upper"], "->", r["upper"], "passes", r["passes"], "evaluated", r["evaluated"], "verified",
          r["verified"], r["accepted"])
    ups = [r["start_upper"]] + [a[4] for a in r["accepted"]]
    assert all(b < a for a, b in zip(ups, ups[1:]))
    assert ups[-1] == r["upper"]
    assert len(r["accepted"]) >= 1
    assert r["verified"] < r["evaluated"]
    assert not leaf_ref.rejects(g.inst, *g.inst.split(r["z"]))
    assert check_point(g.inst, r["z"], (r["row"], r["dst"], r["val"]), r["upper"]) == []
