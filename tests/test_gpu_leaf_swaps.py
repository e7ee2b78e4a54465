"""GPU: the priced swaps of fixed placements (nep_leaf_swaps, LPModel.leaf_swaps; DESIGN.md §7 "Priced swaps") against
the numpy mirror (tests/leaf_swaps_ref.py), on the instances of tests/leaf_moves_cases.py: every fixture group (10x5 ..
80x2), two capacity-greedy leaves with a closed variant each (72x12, 96x8) and "wide" 280x2 — more rows than threads,
K = 2 on the lane path, K = 100 on the wave path with a partial second chunk of the open list, N not a multiple of 64.
Prices: the device's own after 16 rounds.

  1. best equals the mirror's within 1e-11 max(1, |.|) (the project's tolerance for leaf_moves: the mirror rounds rho as
     the kernel does, the sums of <= 280 terms differ at most in their order), +inf exactly where the mirror's is;
     every best_from entry is validated by the mirror's delta of that very (f, from, to) within 1e-11 — not compared
     with the mirror's argmin, near-ties may differ; lagr is nep_leaf_moves' to the bit
  2. the returned list equals nep_debug_leaf_swap_list on the call's own tables exactly, for per_fn 1, 4 and 8; a list
     with a smaller max_moves is the head of the full one; a call without the tables returns the same list
  3. the identity through the evaluator: the 32 cheapest and 32 dearest swaps of the tables applied, one batched
     leaf_eval(Z', rounds=0, prices=y) gives lower within 1e-10 max(1, |.|) of lagr + delta, none INFEASIBLE
  4. two calls return the same bits; leaf_eval and leaf_moves before and after return the same bits; 70 placements in
     one call (the workspace holds 64) equal the single calls
  5. refusals
  6. placement_search on 96x8: from the single moves' end point, swaps = 16 ends strictly lower
"""
import math

import numpy as np
import pytest

import leaf_ref
import leaf_swaps_ref as sref
from leaf_cases import check_point, groups
from leaf_moves_cases import NAMES, case

pytestmark = pytest.mark.gpu
_RUNS = {}
_KEYS = ("n_moves", "fn", "from", "to", "delta", "lagr", "best", "best_from")


def _full(inst):
    return 8 * inst.F


def _run(name):
    """(group, model, 16-round evaluation, leaf_swaps result at per_fn 8 with the tables at its prices); the model
    stays open for the module"""
    if name not in _RUNS:
        from core.engine.lp import LPModel
        g = case(name)
        m = LPModel(g.data, g.variant, step=1, alpha=g.alpha, max_batch=1)
        r16 = m.leaf_eval(g.Z, rounds=16)
        sw = m.leaf_swaps(g.Z, prices=r16["prices"], per_fn=8, max_moves=_full(g.inst), table=True)
        _RUNS[name] = (g, m, r16, sw)
    return _RUNS[name]


def _live(g):
    return [k for k in range(len(g.Z)) if not leaf_ref.rejects(g.inst, *g.inst.split(g.Z[k]))]


@pytest.mark.parametrize("name", NAMES)
def test_tables_match_the_mirror(name):
    g, m, r16, sw = _run(name)
    inst = g.inst
    lagr = m.leaf_moves(g.Z, prices=r16["prices"], max_moves=0)["lagr"]
    assert sw["lagr"].tobytes() == lagr.tobytes()
    for k in range(len(g.Z)):
        C, n = inst.split(g.Z[k])
        best, best_from = sw["best"][k], sw["best_from"][k]
        if k not in _live(g):
            assert sw["n_moves"][k] == 0 and sw["lagr"][k] == math.inf
            assert np.isposinf(best).all() and (best_from == -1).all()
            continue
        y = r16["prices"][k]
        want, want_from = sref.swap_tables(inst, C, y, n)
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(best)) and np.isposinf(best[~fin]).all()
        assert np.array_equal(best_from >= 0, fin) and (best_from[~fin] == -1).all()
        err = np.abs(best[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
        worst = 0.0
        for f, j in zip(*np.nonzero(fin)):
            src = int(best_from[f, j])
            assert C[f, src] > 0.5
            d = sref.swap_delta(inst, C, y, n, int(f), src, int(j))
            worst = max(worst, abs(best[f, j] - d) / max(1.0, abs(d)))
        print(name, k, "finite entries", int(fin.sum()), "best max rel error", err.max() if err.size else 0.0,
              "sources' worst", worst, "sources unlike the mirror's", int((best_from != want_from).sum()),
              "open per function", C.sum(axis=1).astype(int).tolist()[:12])
        assert fin.any()
        assert (err <= 1e-11).all()
        assert worst <= 1e-11


def test_the_shapes_cover_both_row_paths():
    g = case("wide")
    inst = g.inst
    assert inst.N == 280 and inst.F == 2 and inst.N % 64
    assert max(inst.frow[f + 1] - inst.frow[f] for f in range(2)) > 256
    opens = [inst.split(z)[0].sum(axis=1).astype(int).tolist() for z in g.Z]
    assert opens == [[2, 2], [100, 100]] and 2 <= 16 < 64 < 100 < 128
    assert not any(leaf_ref.rejects(inst, *inst.split(z)) for z in g.Z)
    shapes = {(case(name).inst.N, case(name).inst.F) for name in NAMES}
    assert {(10, 5), (80, 2), (72, 12), (96, 8), (280, 2)} <= shapes


@pytest.mark.parametrize("name", NAMES)
def test_the_list_is_the_hosts(name):
    from core.engine.lp import debug_leaf_swap_list
    g, m, r16, sw = _run(name)
    mm = _full(g.inst)
    for per_fn in (1, 4, 8):
        r = sw if per_fn == 8 else m.leaf_swaps(g.Z, prices=r16["prices"], per_fn=per_fn, max_moves=mm, table=True)
        bare = m.leaf_swaps(g.Z, prices=r16["prices"], per_fn=per_fn, max_moves=mm)
        assert r["best"].tobytes() == sw["best"].tobytes() and r["best_from"].tobytes() == sw["best_from"].tobytes()
        for k in _live(g):
            h = debug_leaf_swap_list(r["best"][k], r["best_from"][k], per_fn, mm)
            cnt = int(r["n_moves"][k])
            assert h["n_moves"] == cnt > 0
            assert cnt == int(np.minimum(np.isfinite(r["best"][k]).sum(axis=1), per_fn).sum())
            for key in ("fn", "from", "to", "delta"):
                assert r[key][k].tobytes() == h[key].tobytes() == bare[key][k].tobytes(), (per_fn, k, key)
            assert (r["fn"][k, cnt:] == -1).all() and np.isposinf(r["delta"][k, cnt:]).all()
            assert (np.diff(r["delta"][k, :cnt]) >= 0.0).all()
        assert bare["n_moves"].tobytes() == r["n_moves"].tobytes() and "best" not in bare
    short = m.leaf_swaps(g.Z, prices=r16["prices"], per_fn=8, max_moves=7)
    for k in range(len(g.Z)):
        c = min(7, int(sw["n_moves"][k]))
        assert short["n_moves"][k] == c
        for key in ("fn", "from", "to", "delta"):
            assert short[key][k, :c].tobytes() == sw[key][k, :c].tobytes(), (k, key)


@pytest.mark.parametrize("name", NAMES)
def test_identity_through_the_evaluator(name):
    g, m, r16, sw = _run(name)
    inst = g.inst
    for k in _live(g):
        full = sref.swap_list(sw["best"][k], sw["best_from"][k], inst.N, inst.F * inst.N)
        pick = full[:32] + full[max(32, len(full) - 32):]
        Z2 = np.stack([sref.apply_swap(inst, g.Z[k], f, src, to) for f, src, to, _ in pick])
        r = m.leaf_eval(Z2, rounds=0, prices=np.tile(r16["prices"][k], (len(pick), 1)))
        want = sw["lagr"][k] + np.array([d for _, _, _, d in pick])
        err = np.abs(r["lower"] - want) / np.maximum(1.0, np.abs(want))
        print(name, k, "swaps", len(full), "checked", len(pick), "worst", err.max())
        assert (r["status"] != leaf_ref.INFEASIBLE).all()
        assert (err <= 1e-10).all()
    m.leaf_eval(g.Z, rounds=16)


def _congested():
    for gi, g in enumerate(groups()):
        for k, c in enumerate(g.cases):
            if (c["N"], c["seed"], c["placement"]) == (12, 1, "MIP optimum"):
                return gi, k
    raise AssertionError("fixture lacks the (12, 6, 1, 1.0) MIP optimum")


def test_two_calls_same_bits_and_the_evaluator_is_untouched():
    for name in (f"fixture{_congested()[0]}", "wide"):
        g, m, r16, sw = _run(name)
        mm = 2 * g.inst.F * g.inst.N + g.inst.N
        before = m.leaf_eval(g.Z, rounds=16)
        moves = m.leaf_moves(g.Z, prices=r16["prices"], max_moves=mm, table=True)
        again = m.leaf_swaps(g.Z, prices=r16["prices"], per_fn=8, max_moves=_full(g.inst), table=True)
        after = m.leaf_eval(g.Z, rounds=16)
        moves2 = m.leaf_moves(g.Z, prices=r16["prices"], max_moves=mm, table=True)
        for key in _KEYS:
            assert again[key].tobytes() == sw[key].tobytes(), (name, key)
        for key in ("lower", "upper", "status", "prices", "cpu"):
            assert before[key].tobytes() == after[key].tobytes() == r16[key].tobytes(), (name, key)
        for key in ("n_moves", "kind", "fn", "node", "delta", "lagr", "table"):
            assert moves[key].tobytes() == moves2[key].tobytes(), (name, key)
        # prices None are zeros; max_moves = 0 prices only
        zero = m.leaf_swaps(g.Z, max_moves=0, table=True)
        same = m.leaf_swaps(g.Z, prices=np.zeros((len(g.Z), g.inst.N)), max_moves=3, table=True)
        assert zero["best"].tobytes() == same["best"].tobytes() and zero["lagr"].tobytes() == same["lagr"].tobytes()
        assert zero["fn"].shape == (len(g.Z), 0)


def test_more_placements_than_a_chunk():
    """70 placements of the 12x6 instance (the workspace holds 64): each result equals the single call's bits"""
    gi, _ = _congested()
    g, m, r16, sw = _run(f"fixture{gi}")
    reps = 70 // len(g.Z) + 1
    Z = np.tile(g.Z, (reps, 1))[:70]
    P = np.tile(r16["prices"], (reps, 1))[:70]
    r = m.leaf_swaps(Z, prices=P, per_fn=8, max_moves=_full(g.inst), table=True)
    for key in _KEYS:
        want = np.tile(sw[key], (reps,) + (1,) * (sw[key].ndim - 1))[:70]
        assert r[key].tobytes() == want.tobytes(), key


def test_refusals():
    from core.engine.lp import EngineUnavailable, LPModel, RELAX_FACILITY, STEP2_DELETE
    gi, k = _congested()
    g, m, r16, _ = _run(f"fixture{gi}")
    fac = LPModel(g.data, g.variant, step=1, alpha=g.alpha, max_batch=1, relaxation=RELAX_FACILITY)
    st2 = LPModel(g.data, g.variant, step=STEP2_DELETE, alpha=g.alpha, max_score=1.0, max_batch=1)
    try:
        for other in (fac, st2):
            with pytest.raises(EngineUnavailable) as e:
                other.leaf_swaps(np.zeros((1, other.n_int)))
            assert "(-1)" in str(e.value) and "step-1 reference-relaxation models" in str(e.value), str(e.value)
    finally:
        fac.close()
        st2.close()
    one = g.Z[k:k + 1]
    z = one.copy()
    z[0, int(np.flatnonzero(z[0] == 1.0)[0])] = 0.5
    for call, word in ((lambda: m.leaf_swaps(z), "not 0 or 1"),
                       (lambda: m.leaf_swaps(one, prices=np.full((1, g.inst.N), -1.0)), "prices"),
                       (lambda: m.leaf_swaps(one, per_fn=0), "per_fn"),
                       (lambda: m.leaf_swaps(one, per_fn=9), "per_fn"),
                       (lambda: m.leaf_swaps(one, max_moves=-1), "max_moves")):
        with pytest.raises(EngineUnavailable) as e:
            call()
        assert "(-1)" in str(e.value) and word in str(e.value), str(e.value)
    cnt = np.zeros(1, np.int32)
    assert m._lib.nep_leaf_swaps(m._h, 1, one.ctypes.data, None, 4, 4, cnt.ctypes.data, None, None, None, None, None,
                                 None, None) == -1
    assert m._lib.nep_leaf_swaps(m._h, 1, one.ctypes.data, None, 4, 0, None, None, None, None, None, None, None,
                                 None) == -1
    assert m._lib.nep_leaf_swaps(m._h, 1, None, None, 4, 0, cnt.ctypes.data, None, None, None, None, None, None,
                                 None) == -1
    assert b"null argument" in m._lib.nep_last_error()


def test_search_with_swaps_goes_on_from_the_single_moves_end():
    from core.engine.heuristics import placement_search
    g, m, _, _ = _run("96x8")
    kw = dict(rounds=16, width=16, warm=False)
    end = placement_search(m, g.Z[0], **kw)
    got = placement_search(m, end["z"], swaps=16, **kw)
    print("96x8 device", end["start_upper"], "->", end["upper"], "passes", end["passes"], "-> with swaps", got["upper"],
          "passes", got["passes"], got["accepted"])
    assert end["upper"] < end["start_upper"]
    assert got["upper"] < end["upper"]
    assert any(a[0] == 3 and len(a) == 6 for a in got["accepted"])
    assert check_point(g.inst, got["z"], (got["row"], got["dst"], got["val"]), got["upper"]) == []
    assert not leaf_ref.rejects(g.inst, *g.inst.split(got["z"]))
    m.leaf_eval(g.Z, rounds=16)


def teardown_module(module):
    for v in _RUNS.values():
        v[1].close()
    _RUNS.clear()
