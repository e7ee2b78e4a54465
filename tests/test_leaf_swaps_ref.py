"""CPU: the priced swaps of a fixed placement (DESIGN.md §7 "Priced swaps") — the numpy mirror tests/leaf_swaps_ref.py
against leaf_ref's own Lagrangian and against the single moves' table, the library's host-only selection and merge
(nep_debug_leaf_swap_list) against the mirror's, and the product's placement_search with swaps on the mirror model.
Instances: tests/leaf_moves_cases.py without "wide", prices after 16 mirror rounds.

 1. the 8 cheapest and 8 dearest swaps of every placement, applied and re-priced by leaf_moves_ref.lagrangian, change
    L(C, y) by their delta within 1e-12 max(1, |L|) (sums of <= 1e2 fp64 terms that differ in order only), and no
    resulting placement is rejected
 2. a swap is at least as good as the add followed by the function's best drop: best <= ADD's table entry + the node
    term of j' + the smallest finite DROP entry of f, within 1e-12
 3. nep_debug_leaf_swap_list equals swap_list on the same tables exactly, padding included, also where a function has
    fewer than per_fn admissible destinations
 4. placement_search(swaps=0) is the search without swaps; from the single moves' end point on 96x8, swaps=16 ends lower
 5. the case set holds every branch of the pricing (one coverage test)
"""
import math

import numpy as np
import pytest

import leaf_moves_ref as mref
import leaf_ref
import leaf_swaps_ref as sref
from leaf_cases import mirror
from leaf_moves_cases import NAMES as _ALL, case

NAMES = [name for name in _ALL if name != "wide"]
_CACHE = {}


def _priced(name, k):
    """(y, lagr, best, best_from) of placement k of a case at the mirror's 16-round prices, once per process; None for
    a rejected placement"""
    key = (name, k)
    if key not in _CACHE:
        g = case(name)
        C, n = g.inst.split(g.Z[k])
        if leaf_ref.rejects(g.inst, C, n):
            _CACHE[key] = None
        else:
            y = (mirror(g, k, 16) if hasattr(g, "cases") else leaf_ref.leaf_eval(g.inst, g.Z[k], rounds=16))["prices"]
            _CACHE[key] = (y, mref.lagrangian(g.inst, g.Z[k], y)) + sref.swap_tables(g.inst, C, y, n)
    return _CACHE[key]


def _placements(name):
    g = case(name)
    return [(k, _priced(name, k)) for k in range(len(g.Z)) if _priced(name, k) is not None]


def _node_term(inst, cnt, j):
    return inst.cost_n if inst.has_n and cnt[j] == 0 else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_cheapest_and_dearest_swaps_change_the_bound_by_their_delta(name):
    g = case(name)
    inst = g.inst
    worst, checked = 0.0, 0
    for k, (y, lagr, best, best_from) in _placements(name):
        full = sref.swap_list(best, best_from, inst.N, inst.F * inst.N)
        assert len(full) == int(np.isfinite(best).sum())
        assert [s[3] for s in full] == sorted(s[3] for s in full)
        C, n = inst.split(g.Z[k])
        for f, src, to, delta in full[:8] + full[-8:]:
            assert C[f, src] > 0.5 and not C[f, to] > 0.5
            assert delta == sref.swap_delta(inst, C, y, n, f, src, to)
            z2 = sref.apply_swap(inst, g.Z[k], f, src, to)
            assert not leaf_ref.rejects(inst, *inst.split(z2)), (k, f, src, to)
            L = mref.lagrangian(inst, z2, y)
            err = abs(L - (lagr + delta)) / max(1.0, abs(L))
            worst, checked = max(worst, err), checked + 1
            assert err <= 1e-12, (k, f, src, to, L, lagr, delta)
    print(name, "swaps checked", checked, "worst relative error", worst)
    assert checked


@pytest.mark.parametrize("name", NAMES)
def test_a_swap_is_no_worse_than_add_then_the_best_drop(name):
    g = case(name)
    inst = g.inst
    for k, (y, lagr, best, best_from) in _placements(name):
        C, n = inst.split(g.Z[k])
        table, _ = mref.price_table(inst, C, y, n)
        cnt = (C > 0.5).sum(axis=0)
        for f in range(inst.F):
            drops = table[f][(C[f] > 0.5) & np.isfinite(table[f])]
            if drops.size == 0:
                continue
            for j in np.flatnonzero(np.isfinite(best[f])).tolist():
                bound = table[f, j] + _node_term(inst, cnt, j) + drops.min()
                assert best[f, j] <= bound + 1e-12, (k, f, j, best[f, j], bound)


def _host(best, best_from, per_fn, max_moves):
    from core.engine.lp import debug_leaf_swap_list
    r = debug_leaf_swap_list(best, best_from, per_fn, max_moves)
    return r, list(zip(r["fn"].tolist(), r["from"].tolist(), r["to"].tolist(), r["delta"].tolist()))


@pytest.mark.parametrize("name", NAMES)
def test_host_swap_list_equals_the_mirror(name):
    inst = case(name).inst
    for k, (y, lagr, best, best_from) in _placements(name):
        for per_fn, mm in ((1, 64), (4, 64), (8, 8 * inst.F + 3), (4, 5), (8, 0)):
            want = sref.swap_list(best, best_from, per_fn, mm)
            r, got = _host(best, best_from, per_fn, mm)
            assert r["n_moves"] == len(want) and len(got) == mm
            assert got[:len(want)] == want, (k, per_fn, mm)     # (delta as Python floats: to the bit)
            assert all(t == (-1, -1, -1, math.inf) for t in got[len(want):])


def test_host_swap_list_where_a_function_has_fewer_than_per_fn():
    """10x5 at per_fn 8: functions with fewer than 8 admissible destinations give what they have"""
    name = next(n for n in NAMES if (case(n).inst.N, case(n).inst.F) == (10, 5))
    inst = case(name).inst
    short = 0
    for k, (y, lagr, best, best_from) in _placements(name):
        per = np.isfinite(best).sum(axis=1)
        short += int((per < 8).sum())
        want = sref.swap_list(best, best_from, 8, 64)
        assert len(want) == int(np.minimum(per, 8).sum())
        r, got = _host(best, best_from, 8, 64)
        assert r["n_moves"] == len(want) and got[:len(want)] == want
        assert all(t == (-1, -1, -1, math.inf) for t in got[len(want):])
    assert short


def test_host_swap_list_refusals():
    from core.engine import lp
    best, best_from = np.zeros((2, 3)), np.zeros((2, 3), np.int32)
    for per_fn, mm, word in ((0, 4, "per_fn"), (9, 4, "per_fn"), (4, -1, "max_moves")):
        with pytest.raises(lp.EngineUnavailable) as e:
            lp.debug_leaf_swap_list(best, best_from, per_fn, mm)
        assert "(-1)" in str(e.value) and word in str(e.value), str(e.value)
    lib = lp.load_library()
    cnt = np.zeros(1, np.int32)
    assert lib.nep_debug_leaf_swap_list(2, 3, None, best_from.ctypes.data, 4, 0, cnt.ctypes.data, None, None, None,
                                        None) == -1
    assert lib.nep_debug_leaf_swap_list(2, 3, best.ctypes.data, best_from.ctypes.data, 4, 4, cnt.ctypes.data, None,
                                        None, None, None) == -1
    assert lib.nep_leaf_swaps(None, 1, None, None, 4, 0, None, None, None, None, None, None, None, None) == -1


def test_apply_move_takes_a_swap():
    from core.engine.heuristics import apply_move
    z = np.array([1, 0, 0, 1, 1, 0, 1, 1, 0], np.float64)     # F = 2, N = 3, then n
    z2 = apply_move(z, 2, 3, True, 3, 0, 2, src=0)
    assert z2.tolist() == [0, 0, 1, 1, 1, 0, 1, 1, 1] and z.tolist() == [1, 0, 0, 1, 1, 0, 1, 1, 0]
    z3 = apply_move(z, 2, 3, True, 3, 1, 2, 1)                  # node 1 loses its last placement
    assert z3.tolist() == [1, 0, 0, 1, 0, 1, 1, 0, 1]
    assert apply_move(z[:6], 2, 3, False, 3, 1, 2, 1).tolist() == [1, 0, 0, 1, 0, 1]
    with pytest.raises(ValueError):
        apply_move(z, 2, 3, True, 3, 0, 2)
    with pytest.raises(ValueError):
        apply_move(z, 2, 3, True, 4, 0, 2)


_SEARCH = dict(rounds=16, width=16, warm=False)


def test_search_without_swaps_is_unchanged():
    """swaps = 0 never asks for swaps (leaf_moves_ref.MirrorModel has none to give) and returns the same search"""
    from core.engine.heuristics import placement_search
    g = case("72x12")
    base = placement_search(mref.MirrorModel(g.inst), g.Z[0], max_passes=4, **_SEARCH)
    got = placement_search(sref.MirrorModel(g.inst), g.Z[0], max_passes=4, swaps=0, **_SEARCH)
    print("72x12", base["start_upper"], "->", base["upper"], "passes", base["passes"], base["accepted"])
    assert base["accepted"] and all(len(a) == 5 and a[0] in (0, 1, 2) for a in base["accepted"])
    assert got["accepted"] == base["accepted"]
    for key in ("upper", "lower", "start_upper", "passes", "evaluated"):
        assert got[key] == base[key], key
    for key in ("z", "row", "dst", "val"):
        assert np.asarray(got[key]).tobytes() == np.asarray(base[key]).tobytes(), key


@pytest.mark.slow
def test_search_improves_with_swaps():
    """96x8: the single moves stop; swaps asked for beside them go on from that end point"""
    from core.engine.heuristics import placement_search
    g = case("96x8")
    model = sref.MirrorModel(g.inst)
    end = placement_search(model, g.Z[0], **_SEARCH)
    got = placement_search(model, end["z"], swaps=16, **_SEARCH)
    print("96x8", end["start_upper"], "->", end["upper"], "-> with swaps", got["upper"], "passes", got["passes"],
          got["accepted"])
    assert end["upper"] < end["start_upper"]
    assert got["start_upper"] == end["upper"]
    assert got["upper"] < end["upper"] - 1e-9 * max(1.0, abs(end["upper"]))
    assert any(a[0] == 3 and len(a) == 6 for a in got["accepted"])
    assert not leaf_ref.rejects(g.inst, *g.inst.split(got["z"]))


def test_the_cases_cover_the_pricing():
    seen = set()
    for name in NAMES:
        inst = case(name).inst
        for k, (y, lagr, best, best_from) in _placements(name):
            C, n = inst.split(case(name).Z[k])
            cnt, mem = sref._node_state(inst, C)
            for f in range(inst.F):
                op, src, w, m1, k1, m2 = sref._rows(inst, C, y, f)
                if op.size == 1:
                    seen.add("K = 1")
                if len(src) == 0:
                    seen.add("no loaded row")
                if len(src) and op.size > 1 and len(set(k1.tolist())) < op.size:
                    seen.add("an empty bucket")
                if (cnt[op] == 1).any():
                    seen.add("a single placement on the source, " + ("with n" if inst.has_n else "without n"))
                for j in np.flatnonzero(~(C[f] > 0.5)).tolist():
                    if not sref.admissible(inst, cnt, mem, f, j):
                        assert best[f, j] == math.inf and best_from[f, j] == -1
                        seen.add("a screened destination")
                    elif cnt[j] == 0:
                        seen.add("a node that opens")
    assert seen == {"K = 1", "no loaded row", "an empty bucket", "a single placement on the source, with n",
                    "a single placement on the source, without n", "a screened destination",
                    "a node that opens"}, seen
