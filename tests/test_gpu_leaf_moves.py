"""GPU: the priced moves of fixed placements (nep_leaf_moves, LPModel.leaf_moves; DESIGN.md §7 "Priced moves") and the
placement search built on them (core/engine/heuristics.py placement_search), against the numpy mirror
(tests/leaf_moves_ref.py), on the instances of tests/leaf_moves_cases.py: every fixture group, two capacity-greedy
leaves with a closed variant each, and a 280x2 instance with more rows than threads and an open list beyond 64.  Between
them: K <= 16 and K > 16, N not a multiple of 64, functions without a loaded row.  Prices: the device's own after 16
rounds.

  5. table and lagr equal the mirror's within 1e-11 max(1, |.|) — the mirror rounds rho as the kernel does, so the sums
     of <= 280 terms differ at most in their order —, +inf exactly where the mirror has +inf
  6. the identity through the evaluator: the first 32 and last 32 moves of the full list applied, one batched
     leaf_eval(Z', rounds=0, prices=y) gives lower within 1e-10 max(1, |.|) of lagr + delta, none INFEASIBLE; lagr is
     leaf_eval(z, rounds=0, prices=y)'s lower within 1e-11
  7. the call's list is nep_debug_leaf_move_list's on the call's own table, exactly
  8. two calls return the same bits; a call while another slot iterates leaves that LP's result bit-identical; leaf_eval
     before and after a leaf_moves call returns the same bits
  9. more placements than the workspace's chunk in one call
 10. placement_search on the device model against the same call on the mirror model
 11. a step-1 solve with placement_search = 16 ends OPTIMAL at the objective of the solve without it
"""
import math

import numpy as np
import pytest

import leaf_moves_ref as mref
import leaf_ref
from leaf_cases import check_point, groups
from leaf_moves_cases import NAMES, case

pytestmark = pytest.mark.gpu
_RUNS = {}


def _full(inst):
    return 2 * inst.F * inst.N + inst.N


def _run(name):
    """(group, model, 16-round evaluation, full leaf_moves result with the table at its prices); the model stays open
    for the module"""
    if name not in _RUNS:
        from core.engine.lp import LPModel
        g = case(name)
        m = LPModel(g.data, g.variant, step=1, alpha=g.alpha, max_batch=1)
        r16 = m.leaf_eval(g.Z, rounds=16)
        mv = m.leaf_moves(g.Z, prices=r16["prices"], max_moves=_full(g.inst), table=True)
        _RUNS[name] = (g, m, r16, mv)
    return _RUNS[name]


def _close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(b)
    return bool(np.array_equal(fin, np.isfinite(a)) and np.array_equal(a[~fin], b[~fin]) and
                (np.abs(a[fin] - b[fin]) <= tol * np.maximum(1.0, np.abs(b[fin]))).all())


@pytest.mark.parametrize("name", NAMES)
def test_table_and_lagr_match_the_mirror(name):
    g, m, r16, mv = _run(name)
    inst = g.inst
    for k in range(len(g.Z)):
        C, n = inst.split(g.Z[k])
        table, lagr = mref.price_table(inst, C, r16["prices"][k], n)
        both = np.isfinite(table) & np.isfinite(mv["table"][k])
        err = np.abs(mv["table"][k][both] - table[both])
        print(name, k, "lagr", mv["lagr"][k], "mirror", lagr, "table max abs error", err.max() if err.size else 0.0,
              "open per function", C.sum(axis=1).astype(int).tolist()[:12])
        if leaf_ref.rejects(inst, C, n):
            assert mv["n_moves"][k] == 0 and mv["lagr"][k] == math.inf and np.isposinf(mv["table"][k]).all()
            continue
        assert _close(mv["table"][k], table, 1e-11)
        assert _close(mv["lagr"][k], lagr, 1e-11)


def test_the_shapes_cover_both_row_paths():
    seen = set()
    for name in NAMES:
        g = case(name)
        for z in g.Z:
            C, n = g.inst.split(z)
            if not leaf_ref.rejects(g.inst, C, n):
                seen |= {"K<=16" if c <= 16 else "K>16" for c in C.sum(axis=1)}
                if (g.inst.W.sum(axis=1) == 0.0).any():
                    seen.add("no loaded row")
        if g.inst.N % 64:
            seen.add("N not a multiple of 64")
    g = case("wide")
    assert g.inst.N >= 280 and g.inst.F == 2
    assert max(g.inst.frow[f + 1] - g.inst.frow[f] for f in range(2)) > 256
    assert g.inst.split(g.Z[1])[0].sum(axis=1).max() > 64
    assert not any(leaf_ref.rejects(g.inst, *g.inst.split(z)) for z in g.Z)
    assert seen == {"K<=16", "K>16", "no loaded row", "N not a multiple of 64"}, seen


@pytest.mark.parametrize("name", NAMES)
def test_identity_through_the_evaluator(name):
    g, m, r16, mv = _run(name)
    inst = g.inst
    r0 = m.leaf_eval(g.Z, rounds=0, prices=r16["prices"])
    for k in range(len(g.Z)):
        if leaf_ref.rejects(inst, *inst.split(g.Z[k])):
            continue
        assert abs(mv["lagr"][k] - r0["lower"][k]) <= 1e-11 * max(1.0, abs(r0["lower"][k]))
        cnt = int(mv["n_moves"][k])
        pick = sorted(set(range(min(32, cnt))) | set(range(max(0, cnt - 32), cnt)))
        if not pick:
            continue
        Z2 = np.stack([mref.apply_move(inst, g.Z[k], mv["kind"][k, q], mv["fn"][k, q], mv["node"][k, q])
                       for q in pick])
        r = m.leaf_eval(Z2, rounds=0, prices=np.tile(r16["prices"][k], (len(pick), 1)))
        want = mv["lagr"][k] + mv["delta"][k, pick]
        err = np.abs(r["lower"] - want) / np.maximum(1.0, np.abs(want))
        print(name, k, "moves", cnt, "checked", len(pick), "worst", err.max())
        assert (r["status"] != leaf_ref.INFEASIBLE).all()
        assert (err <= 1e-10).all()
    m.leaf_eval(g.Z, rounds=16)


@pytest.mark.parametrize("name", NAMES)
def test_the_list_is_the_hosts(name):
    from core.engine.lp import debug_leaf_move_list
    g, m, r16, mv = _run(name)
    for k in range(len(g.Z)):
        if leaf_ref.rejects(g.inst, *g.inst.split(g.Z[k])):
            continue
        h = debug_leaf_move_list(g.data, g.variant, g.Z[k], mv["table"][k], _full(g.inst), alpha=g.alpha)
        cnt = int(mv["n_moves"][k])
        assert h["n_moves"] == cnt > 0
        for key in ("kind", "fn", "node", "delta"):
            assert mv[key][k, :cnt].tobytes() == h[key].tobytes(), (k, key)
        assert (mv["kind"][k, cnt:] == -1).all() and np.isposinf(mv["delta"][k, cnt:]).all()
        assert (np.diff(mv["delta"][k, :cnt]) >= 0.0).all()
    # a shorter list is the head of the full one
    short = m.leaf_moves(g.Z, prices=r16["prices"], max_moves=7)
    for k in range(len(g.Z)):
        c = min(7, int(mv["n_moves"][k]))
        assert short["n_moves"][k] == c
        for key in ("kind", "fn", "node", "delta"):
            assert short[key][k, :c].tobytes() == mv[key][k, :c].tobytes(), (k, key)


def _congested():
    for gi, g in enumerate(groups()):
        for k, c in enumerate(g.cases):
            if (c["N"], c["seed"], c["placement"]) == (12, 1, "MIP optimum"):
                return gi, k
    raise AssertionError("fixture lacks the (12, 6, 1, 1.0) MIP optimum")


def test_two_calls_same_bits_and_the_evaluator_is_untouched():
    for name in (f"fixture{_congested()[0]}", "wide"):
        g, m, r16, mv = _run(name)
        before = m.leaf_eval(g.Z, rounds=16)
        again = m.leaf_moves(g.Z, prices=r16["prices"], max_moves=_full(g.inst), table=True)
        after = m.leaf_eval(g.Z, rounds=16)
        for key in ("n_moves", "kind", "fn", "node", "delta", "lagr", "table"):
            assert again[key].tobytes() == mv[key].tobytes(), (name, key)
        for key in ("lower", "upper", "status", "prices", "cpu"):
            assert before[key].tobytes() == after[key].tobytes() == r16[key].tobytes(), (name, key)
        # prices None are zeros; max_moves = 0 prices only
        zero = m.leaf_moves(g.Z, max_moves=0, table=True)
        same = m.leaf_moves(g.Z, prices=np.zeros((len(g.Z), g.inst.N)), max_moves=3, table=True)
        assert zero["table"].tobytes() == same["table"].tobytes() and zero["lagr"].tobytes() == same["lagr"].tobytes()
        assert zero["kind"].shape == (len(g.Z), 0)


def test_a_call_leaves_iterating_lps_alone():
    """two cold solves of the congested 12x6 leaf's LP, one with leaf_moves called between its blocks, the other without"""
    from core.engine.lp import LPModel
    gi, k = _congested()
    g = groups()[gi]
    out = []
    for call in (True, False):
        m = LPModel(g.data, g.variant, step=1, alpha=g.alpha, max_batch=2)
        try:
            m.submit([0], g.Z[k:k + 1], g.Z[k:k + 1], tol=5e-7, max_iters=2048)
            done, blocks = None, 0
            while m.active():
                if call and blocks % 4 == 0:
                    m.leaf_moves(g.Z, max_moves=16)
                r = m.advance(0)
                blocks += 1
                if len(r["slots"]):
                    done = r
            assert done is not None and blocks > 1
            z = m.solutions([0])[0]
            out.append((done["obj"].tobytes(), done["primal_obj"].tobytes(), done["iters"].tobytes(),
                        done["status"].tobytes(), z.tobytes()))
        finally:
            m.close()
    assert out[0] == out[1]


def test_more_placements_than_a_chunk():
    """70 placements of the 12x6 instance (the workspace holds 64): each result equals the single call's bits"""
    gi, _ = _congested()
    g, m, r16, mv = _run(f"fixture{gi}")
    reps = 70 // len(g.Z) + 1
    Z = np.tile(g.Z, (reps, 1))[:70]
    P = np.tile(r16["prices"], (reps, 1))[:70]
    r = m.leaf_moves(Z, prices=P, max_moves=_full(g.inst), table=True)
    for key in ("n_moves", "kind", "fn", "node", "delta", "lagr", "table"):
        want = np.tile(mv[key], (reps,) + (1,) * (mv[key].ndim - 1))[:70]
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
                other.leaf_moves(np.zeros((1, other.n_int)))
            assert "(-1)" in str(e.value) and "step-1 reference-relaxation models" in str(e.value), str(e.value)
    finally:
        fac.close()
        st2.close()
    z = g.Z[k:k + 1].copy()
    z[0, int(np.flatnonzero(z[0] == 1.0)[0])] = 0.5
    with pytest.raises(EngineUnavailable) as e:
        m.leaf_moves(z)
    assert "(-1)" in str(e.value) and "not 0 or 1" in str(e.value), str(e.value)
    with pytest.raises(EngineUnavailable) as e:
        m.leaf_moves(g.Z[k:k + 1], prices=np.full((1, g.inst.N), -1.0))
    assert "(-1)" in str(e.value)
    with pytest.raises(EngineUnavailable) as e:
        m.leaf_moves(g.Z[k:k + 1], max_moves=-1)
    assert "(-1)" in str(e.value) and "max_moves" in str(e.value)
    cnt = np.zeros(1, np.int32)
    assert m._lib.nep_leaf_moves(m._h, 1, g.Z[k:k + 1].ctypes.data, None, 4, cnt.ctypes.data, None, None, None, None,
                                 None, None) == -1
    assert m._lib.nep_leaf_moves(m._h, 1, g.Z[k:k + 1].ctypes.data, None, 0, None, None, None, None, None, None,
                                 None) == -1


def _search_pair(g, m, z0, **kw):
    from core.engine.heuristics import placement_search
    ref = placement_search(mref.MirrorModel(g.inst), z0, **kw)
    got = placement_search(m, z0, **kw)
    print(g.key, "device", got["start_upper"], "->", got["upper"], "passes", got["passes"], "evaluated",
          got["evaluated"], got["accepted"], "| mirror", ref["start_upper"], "->", ref["upper"], "passes",
          ref["passes"], ref["accepted"])
    return got, ref


@pytest.mark.parametrize("name", ("72x12", "96x8"))
def test_search_from_a_greedy_leaf(name):
    g, m, _, _ = _run(name)
    got, ref = _search_pair(g, m, g.Z[0], rounds=16, width=16, max_passes=4, warm=False, repair_every=None)
    assert got["upper"] <= ref["upper"] * (1.0 + 1e-8)
    assert got["upper"] < got["start_upper"]
    assert check_point(g.inst, got["z"], (got["row"], got["dst"], got["val"]), got["upper"]) == []
    assert not leaf_ref.rejects(g.inst, *g.inst.split(got["z"]))
    m.leaf_eval(g.Z, rounds=16)


def test_search_closes_an_opened_node():
    from leaf_cases import mirror
    from leaf_moves_cases import opened_start
    gi, k = _congested()
    g, m, _, _ = _run(f"fixture{gi}")
    want = mirror(g, k, 32)["upper"]
    z0, j = opened_start(g, k)
    got, ref = _search_pair(g, m, z0, rounds=32, width=_full(g.inst), warm=False)
    assert got["upper"] <= want + 1e-9 and got["start_upper"] > want + 1e-7
    assert check_point(g.inst, got["z"], (got["row"], got["dst"], got["val"]), got["upper"]) == []
    m.leaf_eval(g.Z, rounds=16)


def test_solver_option():
    from core.engine.lp import LPModel
    from core.solvers.neptune.neptune_step import NeptuneStep1CPUMinDelayAndUtilization
    gi, _ = _congested()
    g = groups()[gi]
    res, items = {}, {}
    for width in (0, 16):
        batch = 16
        st1 = NeptuneStep1CPUMinDelayAndUtilization(alpha=g.alpha, verbose=False, batch=batch)
        st1.placement_search = width
        st1.load_data(g.data)
        m = LPModel(g.data, g.variant, step=1, alpha=g.alpha, max_batch=batch + 2)
        bm = st1.bound_model(g.data, batch + 1)
        try:
            bnb = st1.branch_and_bound(m, bm, time_limit=60.0)
            inner = bnb.primal
            plain = st1.primal_heuristic(m.layout(), m.row_map())

            def recording(idx, val, z, flow, inner=inner, plain=plain, width=width):
                out = inner(idx, val, z, flow)
                if not len(idx):
                    items[width] = (len(plain(idx, val, z, flow)), out)
                return out
            bnb.primal = recording
            r = res[width] = bnb.solve()
        finally:
            m.close()
            bm.close()
        print(f"placement_search {width}: status {r.status} incumbent {r.objective} bound {r.bound} nodes {r.nodes} "
              f"leaves {r.leaves} lps {r.lps} seconds {r.seconds:.2f}")
    assert res[0].status == res[16].status == "OPTIMAL"
    assert abs(res[16].objective - res[0].objective) <= 1e-6 * max(1.0, abs(res[0].objective))
    n0, got0 = items[0]
    assert len(got0) == n0                               # off: the greedy's items alone
    n16, got16 = items[16]
    # the wrapper ran and its search moved: the mirror descends from this instance's greedy leaf 0 (0.26635 -> 0.23696),
    # so one item is appended, its point is verified and it is cheaper than every greedy point
    assert n16 == n0 and len(got16) == n16 + 1
    print("root items", n16, "->", len(got16))
    sol = got16[-1][2]
    assert sol is not None
    greedy = [it[2]["objective"] for it in got16[:n16] if it[2] is not None]
    print("search item objective", sol["objective"], "greedy objectives", greedy)
    assert check_point(g.inst, sol["z"], (sol["row"], sol["dst"], sol["val"]), sol["objective"]) == []
    assert greedy and sol["objective"] < min(greedy)
    assert np.array_equal(got16[-1][1], sol["z"])


def teardown_module(module):
    for key, v in list(_RUNS.items()):
        if key != "seen":
            v[1].close()
    _RUNS.clear()
