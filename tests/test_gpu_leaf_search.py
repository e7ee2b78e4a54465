"""GPU: the native placement search (nep_leaf_search, LPModel.leaf_search; DESIGN.md §7 "Native search") against the
Python descent (core.engine.heuristics.placement_search) on the same LPModel, on the instances of
tests/leaf_moves_cases.py: the 12x6 congested fixture, 72x12, 96x8 and "wide" 280x2 (N not a multiple of 4 or 64, more
rows than threads, K = 2 on the lane path and K = 100 on the wave path).

  1. expansion: nep_debug_leaf_expand over the full move and swap lists of every case equals apply_move's c as bytes,
     and its open-node count the sum of the applied n (a variant without n: the nodes with a placement); for one
     neighbour and for more neighbours than a chunk holds
  2. verify="all" is the Python search to the bit: z, upper, lower, the accepted list, passes, evaluated, verified and
     the routing entries — cold, with swaps, warm with the per-round repair, and with more neighbours than free slots
  3. verify="lazy" equals placement_search(verify="lazy") to the bit; the end point passes check_point; fewer
     neighbours are verified than evaluated
  4. two calls return the same bits; leaf_eval, leaf_moves and leaf_swaps before and after a search return the same bits
  5. refusals
"""
import ctypes

import numpy as np
import pytest

import leaf_ref
from leaf_cases import check_point, groups
from leaf_moves_cases import NAMES, case

pytestmark = pytest.mark.gpu
_MODELS = {}


def _congested():
    for gi, g in enumerate(groups()):
        for k, c in enumerate(g.cases):
            if (c["N"], c["seed"], c["placement"]) == (12, 1, "MIP optimum"):
                return f"fixture{gi}", k
    raise AssertionError("fixture lacks the (12, 6, 1, 1.0) MIP optimum")


def _model(name):
    if name not in _MODELS:
        from core.engine.lp import LPModel
        g = case(name)
        _MODELS[name] = (g, LPModel(g.data, g.variant, step=1, alpha=g.alpha, max_batch=1))
    return _MODELS[name]


def _device_lists(g, m, k):
    """every move and swap of placement k at the device's own 16-round prices: [(kind, fn, node, src or None)]"""
    inst = g.inst
    z = g.Z[k:k + 1]
    y = m.leaf_eval(z, rounds=16)["prices"]
    mv = m.leaf_moves(z, prices=y, max_moves=2 * inst.F * inst.N + inst.N)
    sw = m.leaf_swaps(z, prices=y, per_fn=8, max_moves=8 * inst.F)
    out = [(int(mv["kind"][0, q]), int(mv["fn"][0, q]), int(mv["node"][0, q]), None) for q in range(int(mv["n_moves"][0]))]
    out += [(3, int(sw["fn"][0, q]), int(sw["to"][0, q]), int(sw["from"][0, q])) for q in range(int(sw["n_moves"][0]))]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_expansion_is_apply_move(name):
    from core.engine.heuristics import apply_move
    g, m = _model(name)
    inst = g.inst
    F, N, has_n = inst.F, inst.N, bool(inst.has_n)
    cap = max(1, min(64, (64 << 20) // (F * N * 8)))
    total = 0
    for k in range(len(g.Z)):
        moves = _device_lists(g, m, k)
        if leaf_ref.rejects(inst, *inst.split(g.Z[k])):
            assert moves == []
            continue
        moves = (moves * ((cap + 6) // len(moves) + 1))[:max(len(moves), cap + 7)]   # (more than a chunk holds)
        assert len(moves) > cap, (name, k, len(moves))
        want = np.stack([apply_move(g.Z[k], F, N, has_n, kind, f, j, src) for kind, f, j, src in moves])
        wc = (want[:, :F * N] != 0).astype(np.uint8).reshape(-1, F, N)
        wn = want[:, F * N:].sum(axis=1) if has_n else wc.any(axis=1).sum(axis=1).astype(np.float64)
        cols = [np.array([mv[c] if mv[c] is not None else -1 for mv in moves], np.int32) for c in range(4)]
        got, nsum = m.debug_leaf_expand(g.Z[k], *cols)
        assert got.tobytes() == wc.tobytes(), (name, k)
        assert nsum.tobytes() == wn.tobytes(), (name, k)
        for q in (0, len(moves) - 1):                        # one neighbour: the first slot alone
            one, n1 = m.debug_leaf_expand(g.Z[k], *(c[q:q + 1] for c in cols))
            assert one.tobytes() == wc[q:q + 1].tobytes() and n1[0] == wn[q], (name, k, q)
        total += len(moves)
    print(name, "neighbours expanded", total, "kinds", sorted({mv[0] for mv in moves}))
    assert total > 0
    m.leaf_eval(g.Z, rounds=16)


def _same(got, want, keys=("z", "upper", "lower", "accepted", "passes", "evaluated", "verified", "start_upper", "row",
                           "dst", "val")):
    for key in keys:
        a, b = got[key], want[key]
        if isinstance(a, (list, int)) or a is None:
            assert a == b, (key, a, b)
        else:
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (key, a, b)


_SETS = {"cold": dict(rounds=16, width=16, warm=False),
         "swaps": dict(rounds=16, width=16, warm=False, swaps=16),
         "warm repair": dict(rounds=16, repair_every=4, width=16, swaps=16, warm=True)}
_CASES = [(name, key) for name in ("12x6", "72x12", "96x8", "wide", "wide100") for key in _SETS] + [("12x6", "chunks")]


def _start(name):
    """(group, model, start placement); "wide100": the wide instance from its 100 open nodes (the wave path)"""
    if name == "12x6":
        name, k = _congested()
    elif name == "wide100":
        name, k = "wide", 1
    else:
        k = 0
    g, m = _model(name)
    return g, m, g.Z[k]


def _kw(name, key):
    if key == "chunks":        # 80 neighbours asked for, 63 free slots
        return dict(rounds=16, width=48, swaps=32, per_fn=8, warm=False, max_passes=4)
    return dict(_SETS[key], max_passes=8 if name in ("72x12", "96x8") else 6)


@pytest.mark.parametrize("name,key", _CASES)
def test_verify_all_is_the_python_search(name, key):
    from core.engine.heuristics import placement_search
    g, m, z0 = _start(name)
    kw = _kw(name, key)
    want = placement_search(m, z0, **kw)
    got = m.leaf_search(z0, verify="all", **kw)
    print(name, key, want["start_upper"], "->", want["upper"], "passes", want["passes"], "evaluated", want["evaluated"],
          "verified", want["verified"], "accepted", len(want["accepted"]))
    _same(got, want)
    assert placement_search(m, z0, native=True, **kw)["accepted"] == want["accepted"]
    if key == "chunks":
        assert want["evaluated"] > 63 * want["passes"] >= 63
    if np.isfinite(got["upper"]):
        assert check_point(g.inst, got["z"], (got["row"], got["dst"], got["val"]), got["upper"]) == []


def test_more_neighbours_than_free_slots_from_every_start():
    """the 12x6 group's other placements as starts (the MIP optimum above accepts nothing): the chunked passes accept,
    under both rules, and equal the Python search"""
    from core.engine.heuristics import placement_search
    name, _ = _congested()
    g, m = _model(name)
    moved = {"all": 0, "lazy": 0}
    for k in range(len(g.Z)):
        if leaf_ref.rejects(g.inst, *g.inst.split(g.Z[k])):
            continue
        for verify in ("all", "lazy"):
            kw = dict(_kw("12x6", "chunks"), verify=verify, repair_every=4)
            want = placement_search(m, g.Z[k], **kw)
            got = m.leaf_search(g.Z[k], **kw)
            print(name, k, g.cases[k]["placement"], verify, want["start_upper"], "->", want["upper"], "passes",
                  want["passes"], "evaluated", want["evaluated"], "verified", want["verified"], want["accepted"])
            _same(got, want)
            moved[verify] += len(got["accepted"]) if got["evaluated"] > 63 * got["passes"] else 0
    assert moved["all"] > 0 and moved["lazy"] > 0, moved


def test_the_search_moves_somewhere():
    """the comparisons above are not between two searches that stand still"""
    for name in ("72x12", "96x8"):
        g, m, z0 = _start(name)
        r = m.leaf_search(z0, **_kw(name, "warm repair"))
        assert len(r["accepted"]) >= 2 and r["upper"] < r["start_upper"]


@pytest.mark.parametrize("name", ["12x6", "72x12", "96x8", "wide", "wide100"])
def test_verify_lazy_is_the_lazy_rule(name):
    from core.engine.heuristics import placement_search
    g, m, z0 = _start(name)
    for key in ("warm repair", "chunks"):
        if key == "chunks" and name != "12x6":
            continue
        kw = dict(_kw(name, key), repair_every=4)
        want = placement_search(m, z0, verify="lazy", **kw)
        got = m.leaf_search(z0, verify="lazy", **kw)
        print(name, key, want["start_upper"], "->", want["upper"], "passes", want["passes"], "evaluated",
              want["evaluated"], "verified", want["verified"], "accepted", len(want["accepted"]))
        _same(got, want)
        if np.isfinite(got["upper"]):
            assert check_point(g.inst, got["z"], (got["row"], got["dst"], got["val"]), got["upper"]) == []
        if got["evaluated"]:
            assert got["verified"] < got["evaluated"]


def test_two_calls_same_bits_and_the_evaluator_is_untouched():
    for name in ("12x6", "wide"):
        g, m, z0 = _start(name)
        inst = g.inst
        mm = 2 * inst.F * inst.N + inst.N
        before = m.leaf_eval(g.Z, rounds=16, repair_every=4)
        mv = m.leaf_moves(g.Z, prices=before["prices"], max_moves=mm, table=True)
        sw = m.leaf_swaps(g.Z, prices=before["prices"], per_fn=8, max_moves=8 * inst.F, table=True)
        for verify in ("all", "lazy"):
            kw = dict(_kw(name, "warm repair"), verify=verify)
            a = m.leaf_search(z0, **kw)
            b = m.leaf_search(z0, **kw)
            _same(a, b, keys=("z", "upper", "lower", "prices", "accepted", "passes", "evaluated", "verified",
                              "start_upper", "row", "dst", "val"))
        after = m.leaf_eval(g.Z, rounds=16, repair_every=4)
        mv2 = m.leaf_moves(g.Z, prices=before["prices"], max_moves=mm, table=True)
        sw2 = m.leaf_swaps(g.Z, prices=before["prices"], per_fn=8, max_moves=8 * inst.F, table=True)
        for r1, r2 in ((before, after), (mv, mv2), (sw, sw2)):
            for key in r1:
                assert r1[key].tobytes() == r2[key].tobytes(), (name, key)


def test_refusals():
    from core.engine.lp import EngineUnavailable, LPModel, LeafSearchOpts, RELAX_FACILITY, STEP2_DELETE
    g, m, z0 = _start("12x6")
    fac = LPModel(g.data, g.variant, step=1, alpha=g.alpha, max_batch=1, relaxation=RELAX_FACILITY)
    st2 = LPModel(g.data, g.variant, step=STEP2_DELETE, alpha=g.alpha, max_score=1.0, max_batch=1)
    try:
        for other in (fac, st2):
            with pytest.raises(EngineUnavailable) as e:
                other.leaf_search(np.zeros(other.n_int))
            assert "(-1)" in str(e.value) and "step-1 reference-relaxation models" in str(e.value), str(e.value)
    finally:
        fac.close()
        st2.close()
    z = z0.copy()
    z[int(np.flatnonzero(z == 1.0)[0])] = 0.5
    for call, word in ((lambda: m.leaf_search(z0, verify="lazy"), "repair_every"),
                       (lambda: m.leaf_search(z0, verify="lazy", repair_every=0), "repair_every"),
                       (lambda: m.leaf_search(z0, repair_every=-1), "repair_every"),
                       (lambda: m.leaf_search(z0, swaps=4, per_fn=0), "per_fn"),
                       (lambda: m.leaf_search(z0, swaps=4, per_fn=9), "per_fn"),
                       (lambda: m.leaf_search(z0, width=-1), "width"),
                       (lambda: m.leaf_search(z0, swaps=-1), "swaps"),
                       (lambda: m.leaf_search(z0, max_passes=-1), "max_passes"),
                       (lambda: m.leaf_search(z), "not 0 or 1")):
        with pytest.raises(EngineUnavailable) as e:
            call()
        assert "(-1)" in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        m.leaf_search(z0, verify="some")
    # NULL required pointers
    opts = LeafSearchOpts(16, 0, 4, 0, 4, 2, 0, 0, 0.0)
    zo, d3 = np.zeros(m.n_int), np.zeros(3)
    c32, c64 = np.zeros(2, np.int32), np.zeros(2, np.int64)
    arr32 = [np.zeros(2, np.int32) for _ in range(4)]
    arrd = [np.zeros(2) for _ in range(2)]
    full = [m._h, z0.ctypes.data, ctypes.byref(opts), zo.ctypes.data, d3.ctypes.data, d3.ctypes.data + 8, None,
            d3.ctypes.data + 16, c32.ctypes.data, c64.ctypes.data, c64.ctypes.data + 8, c32.ctypes.data + 4] + \
           [a.ctypes.data for a in arr32] + [a.ctypes.data for a in arrd]
    assert m._lib.nep_leaf_search(*full) == 0
    for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17):
        args = list(full)
        args[k] = None
        assert m._lib.nep_leaf_search(*args) == -1, k
        assert b"null argument" in m._lib.nep_last_error()
    m.leaf_eval(g.Z, rounds=16)


def teardown_module(module):
    for g, m in _MODELS.values():
        m.close()
    _MODELS.clear()
