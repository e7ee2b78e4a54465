"""CPU: the priced moves of a fixed placement (DESIGN.md §7 "Priced moves") — the numpy mirror tests/leaf_moves_ref.py
against leaf_ref's own Lagrangian, the library's host-only move list (nep_debug_leaf_move_list) against the mirror's,
and the product's placement_search (core/engine/heuristics.py) on the mirror model.

 1. on every non-rejected fixture placement, at the mirror's 16-round prices, every move of the full list changes
    L(C, y) — recomputed by leaf_ref.assign at the moved placement — by its delta within 1e-12 max(1, |L|) (the sums of
    <= 1e3 fp64 terms differ in order only), and no moved placement is rejected
 2. nep_debug_leaf_move_list on the mirror's table returns the mirror's list exactly (kinds, fn, node, order, delta to
    the bit), on the fixture and on two capacity-greedy leaves where memory screens adds out
 3. placement_search from a MIP optimum with one more node opened ends no worse than the optimum's own upper
 4. refusals of the host-only entry
"""
import math

import numpy as np
import pytest

import leaf_moves_ref as mref
import leaf_ref
from leaf_cases import groups, mirror
from leaf_heur_cases import greedy_group
from leaf_moves_cases import opened_start, optima as _optima

_CACHE = {}


def _full(inst):
    return 2 * inst.F * inst.N + inst.N


def _priced(g, k):
    """(y, table, lagr, moves) of placement k of a group at the mirror's 16-round prices, once per process"""
    key = (g.key, k)
    if key not in _CACHE:
        C, n = g.inst.split(g.Z[k])
        y = np.zeros(g.inst.N) if leaf_ref.rejects(g.inst, C, n) else \
            (mirror(g, k, 16) if hasattr(g, "cases") else leaf_ref.leaf_eval(g.inst, g.Z[k], rounds=16))["prices"]
        table, lagr = mref.price_table(g.inst, C, y, n)
        _CACHE[key] = (y, table, lagr, mref.move_list(g.inst, C, n, table, _full(g.inst)))
    return _CACHE[key]


GIDS = list(range(len(groups())))


@pytest.mark.parametrize("gi", GIDS)
def test_every_move_changes_the_bound_by_its_delta(gi):
    g = groups()[gi]
    inst = g.inst
    worst, kinds = 0.0, set()
    for k in range(len(g.Z)):
        C, n = inst.split(g.Z[k])
        y, table, lagr, moves = _priced(g, k)
        if leaf_ref.rejects(inst, C, n):
            assert moves == [] and lagr == math.inf and np.isinf(table).all()
            continue
        L0 = mref.lagrangian(inst, g.Z[k], y)
        assert abs(L0 - lagr) <= 1e-12 * max(1.0, abs(L0))
        assert (table[C < 0.5] <= 0.0).all() and (table[C > 0.5] >= 0.0).all()
        assert [m[3] for m in moves] == sorted(m[3] for m in moves)
        for kind, f, j, delta in moves:
            z2 = mref.apply_move(inst, g.Z[k], kind, f, j)
            assert not leaf_ref.rejects(inst, *inst.split(z2)), (k, kind, f, j)
            L = mref.lagrangian(inst, z2, y)
            err = abs(L - (lagr + delta)) / max(1.0, abs(L))
            worst = max(worst, err)
            assert err <= 1e-12, (k, kind, f, j, L, lagr, delta)
            kinds.add(kind)
    print(g.key, "worst relative error", worst, "kinds", sorted(kinds))


def _host_list(g, z, table, max_moves):
    from core.engine.lp import debug_leaf_move_list
    r = debug_leaf_move_list(g.data, g.variant, z, table, max_moves, alpha=g.alpha)
    return r, list(zip(r["kind"].tolist(), r["fn"].tolist(), r["node"].tolist(), r["delta"].tolist()))


@pytest.mark.parametrize("gi", GIDS)
def test_host_move_list_equals_the_mirror(gi):
    g = groups()[gi]
    for k in range(len(g.Z)):
        _, table, _, moves = _priced(g, k)
        r, got = _host_list(g, g.Z[k], table, _full(g.inst))
        assert r["n_moves"] == len(moves)
        assert got == moves, k          # (delta compared as Python floats: to the bit, up to the sign of zero)
        _, got = _host_list(g, g.Z[k], table, 5)
        assert got == moves[:5]


@pytest.mark.parametrize("shape,want", (((72, 12, 2, 0.5), 9), ((96, 8, 1, 1.0), 7)))
def test_host_move_list_screens_adds_by_memory(shape, want):
    g = greedy_group(*shape, closed=False)
    inst = g.inst
    C, n = inst.split(g.Z[0])
    _, table, _, moves = _priced(g, 0)
    screened = []
    assert mref.move_list(inst, C, n, table, _full(inst), screened) == moves
    print(shape, "adds screened out", len(screened))
    assert len(screened) == want >= 1
    listed = {(f, j) for kind, f, j, _ in moves if kind == mref.ADD}
    for f, j in screened:
        assert (f, j) not in listed
        assert leaf_ref.rejects(inst, *inst.split(mref.apply_move(inst, g.Z[0], mref.ADD, f, j))), (f, j)
    r, got = _host_list(g, g.Z[0], table, _full(inst))
    assert r["n_moves"] == len(moves) and got == moves
    closes = [m for m in moves if m[0] == mref.CLOSE]
    assert closes and all(m[1] == -1 for m in closes)


def test_the_fixture_has_six_optima_with_n():
    assert len(_optima()) == 6


@pytest.mark.parametrize("q", range(6))
def test_search_closes_an_opened_node(q):
    from core.engine.heuristics import placement_search
    gi, k = _optima()[q]
    g = groups()[gi]
    want = mirror(g, k, 32)["upper"]
    assert math.isfinite(want)
    z0, j = opened_start(g, k)
    res = placement_search(mref.MirrorModel(g.inst), z0, rounds=32, width=_full(g.inst), warm=False)
    print(g.key, "opened node", j, "start", res["start_upper"], "end", res["upper"], "optimum's upper", want,
          "passes", res["passes"], "evaluated", res["evaluated"], "accepted", res["accepted"])
    assert res["upper"] <= want + 1e-9
    assert res["start_upper"] > want + 1e-7
    assert res["accepted"] and res["upper"] == res["accepted"][-1][4] < res["start_upper"]
    assert not leaf_ref.rejects(g.inst, *g.inst.split(res["z"]))


def test_refusals():
    from core.engine import lp
    g = groups()[_optima()[0][0]]
    k = _optima()[0][1]
    inst = g.inst
    table = np.zeros((inst.F, inst.N))
    with pytest.raises(lp.EngineUnavailable) as e:
        lp.debug_leaf_move_list(g.data, g.variant, g.Z[k], table, -1, alpha=g.alpha)
    assert "(-1)" in str(e.value) and "max_moves" in str(e.value)
    z = g.Z[k].copy()
    z[int(np.flatnonzero(z == 1.0)[0])] = 0.5
    with pytest.raises(lp.EngineUnavailable) as e:
        lp.debug_leaf_move_list(g.data, g.variant, z, table, 4, alpha=g.alpha)
    assert "(-1)" in str(e.value) and "0 or 1" in str(e.value)
    with pytest.raises(lp.EngineUnavailable) as e:
        lp.debug_leaf_move_list(g.data, g.variant, g.Z[k], None, 4, alpha=g.alpha)
    assert "(-1)" in str(e.value) and "null" in str(e.value)
    for kw in (dict(relaxation=lp.RELAX_FACILITY), dict(step=lp.STEP2_DELETE, max_score=1.0)):
        with pytest.raises(lp.EngineUnavailable) as e:
            lp.debug_leaf_move_list(g.data, g.variant, g.Z[k], table, 4, alpha=g.alpha, **kw)
        assert "(-1)" in str(e.value) and "step-1 reference-relaxation models" in str(e.value), str(e.value)
    # the list of a placement the evaluator rejects is empty, and max_moves = 0 needs no move arrays
    z = g.Z[k].copy()
    z[:inst.N] = 0.0                        # function 0 without a destination
    assert lp.debug_leaf_move_list(g.data, g.variant, z, table, 4, alpha=g.alpha)["n_moves"] == 0
    lib = lp.load_library()
    cnt = np.zeros(1, np.int32)
    d = lp._desc(lp._arrays(g.data, inst.N, inst.F), inst.N, inst.F, lp.VARIANTS[g.variant], lp.STEP1, g.alpha, 1.3,
                 0.0, 0.0, g.data.node_budget)
    import ctypes
    assert lib.nep_debug_leaf_move_list(ctypes.byref(d), g.Z[k].ctypes.data, table.ctypes.data, 0, cnt.ctypes.data,
                                        None, None, None, None) == 0
    assert lib.nep_debug_leaf_move_list(ctypes.byref(d), g.Z[k].ctypes.data, table.ctypes.data, 4, cnt.ctypes.data,
                                        None, None, None, None) == -1
    assert lib.nep_leaf_moves(None, 1, None, None, 0, None, None, None, None, None, None, None) == -1
