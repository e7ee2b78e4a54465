"""CPU: the mirror of the fixed-placement evaluator's per-round repair (tests/leaf_heur_ref.py; nep_leaf_eval_ex,
DESIGN.md §7 "Fixed-placement evaluator") against the fixture's HiGHS leaf-LP values, and the host repair from given
loads (nep_debug_leaf_repair_from) against the mirror's.

 1. on every fixture placement at 32 rounds, repairing every round: upper <= the fixture's (round-0) upper, lower equals
    leaf_ref's at the same rounds, every point passes check_point and NeptuneStepBase.check_placement, and
    upper >= LP - 2e-6 max(1, |LP|)
 2. the three congested fixture placements end at the values measured when the feature was proposed (1e-9 relative);
    24x12 s2 "node closed" goes from NO_POINT to FEASIBLE
 3. nep_debug_leaf_repair_from equals the mirror's repair on every round of every fixture placement and of the 72x12 s2
    rho 0.5 capacity-greedy leaves 0 and 1: the same verdict, the same entries, the objective within 1e-9
 4. load = the flat row-order sums reproduces nep_debug_leaf_repair bit for bit
 5. the selection: repair_every = 4 repairs rounds 4, 8, ... and the last one; the earliest of equal rounds wins
"""
import math
import types

import numpy as np
import pytest

import leaf_heur_ref
import leaf_ref
from leaf_cases import check_point, groups, margin, mirror
from leaf_heur_cases import FIXTURE_ROUNDS, GENERATED_ROUNDS, fixture_case, greedy_group, mirror_ex

CASES = [(gi, k) for gi, g in enumerate(groups()) for k in range(len(g.cases))]


def _id(p):
    c = groups()[p[0]].cases[p[1]]
    return f"{c['N']}x{c['F']}s{c['seed']}-{c['variant']}-{c['placement'].replace(' ', '_')}"


def _passes_check_placement(g, z, entries):
    from core.solvers.neptune.neptune_step import NeptuneStepBase
    C, n = g.inst.split(z)
    if n is None:
        n = (C.sum(axis=0) > 0.5).astype(np.float64)
    return NeptuneStepBase.check_placement(types.SimpleNamespace(data=g.data), C, n, leaf_ref.dense_x(g.inst, entries))


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


@pytest.mark.parametrize("p", CASES, ids=_id)
def test_mirror_on_the_fixture(p):
    g, c = groups()[p[0]], groups()[p[0]].cases[p[1]]
    r = mirror_ex(g, p[1], FIXTURE_ROUNDS)
    base = leaf_ref.leaf_eval(g.inst, g.Z[p[1]], rounds=FIXTURE_ROUNDS)
    assert r["lower"] == base["lower"] and np.array_equal(r["prices"], base["prices"])
    assert r["upper"] <= base["upper"]
    if c["upper"] is not None:
        assert r["upper"] <= c["upper"]
    if c["status64"] == leaf_ref.INFEASIBLE:
        assert r["status"] == leaf_ref.INFEASIBLE and r["upper_round"] == -1
        return
    assert (r["upper_round"] >= 0) == math.isfinite(r["upper"]) == (r["entries"] is not None)
    if r["entries"] is not None:
        assert c["lp_value"] is not None, "a point at a placement HiGHS calls infeasible"
        assert r["upper"] >= c["lp_value"] - margin(c["lp_value"])
        assert check_point(g.inst, g.Z[p[1]], r["entries"], r["upper"]) == []
        assert _passes_check_placement(g, g.Z[p[1]], r["entries"])
        assert r["device_upper"] >= r["upper"] or r["upper_round"] == 0


@pytest.mark.parametrize("N,F,seed,placement,round0,want,rnd", [
    (24, 12, 2, "HiGHS 30 s incumbent", 0.19883813, 0.19883749289703848, 15),
    (24, 12, 2, "HiGHS 30 s incumbent, last open node closed", None, 0.20513919087979984, 11),
    (20, 10, 3, "MIP optimum, last open node closed", 0.2431388, 0.22942486596934672, 28)])
def test_congested_fixture_placements(N, F, seed, placement, round0, want, rnd):
    g, k = fixture_case(N, F, seed, placement)
    r0, r = mirror(g, k, FIXTURE_ROUNDS), mirror_ex(g, k, FIXTURE_ROUNDS)
    if round0 is None:
        assert r0["status"] == leaf_ref.NO_POINT and r["status"] == leaf_ref.FEASIBLE
    else:
        assert abs(r0["upper"] - round0) <= 1e-7
    assert _rel(r["upper"], want) <= 1e-9 and r["upper_round"] == rnd


def _every_round(g, k, rounds):
    C, n = g.inst.split(g.Z[k])
    if leaf_ref.rejects(g.inst, C, n):
        return []
    per = leaf_heur_ref.rounds_with_repair(g.inst, C, n, rounds, keep=True)[5]
    return [(rd, r) for rd, r in enumerate(per) if r is not None]


def _same_repair(g, z, r):
    from core.engine import lp
    found, upper, ent, cpu = lp.debug_leaf_repair(g.data, g.variant, z, r["asg"], alpha=g.alpha, load=r["load"])
    assert found == r["found"]
    if not found:
        assert upper == math.inf
        return
    assert _rel(upper, r["obj"]) <= 1e-9
    assert np.array_equal(ent[0], r["entries"][0]) and np.array_equal(ent[1], r["entries"][1])
    assert np.abs(ent[2] - r["entries"][2]).max() <= 1e-12
    assert np.abs(cpu - r["cpu"]).max() <= 1e-12 * max(1.0, r["cpu"].max())


@pytest.mark.parametrize("p", CASES, ids=_id)
def test_host_repair_from_loads_matches_the_mirror(p):
    g = groups()[p[0]]
    for rd, r in _every_round(g, p[1], FIXTURE_ROUNDS):
        assert r["moves"] < leaf_heur_ref.DEV_MOVES
        _same_repair(g, g.Z[p[1]], r)


@pytest.mark.parametrize("k", [0, 1])
def test_host_repair_from_loads_on_greedy_leaves(k):
    g = greedy_group(72, 12, 2, 0.5, closed=False)
    assert g.inst.R == 449
    rounds = _every_round(g, k, GENERATED_ROUNDS)
    assert len(rounds) == GENERATED_ROUNDS and max(r["moves"] for _, r in rounds) > 0
    for rd, r in rounds:
        _same_repair(g, g.Z[k], r)


@pytest.mark.parametrize("p", CASES, ids=_id)
def test_flat_loads_reproduce_the_plain_repair(p):
    from core.engine import lp
    g = groups()[p[0]]
    z = g.Z[p[1]]
    C, n = g.inst.split(z)
    if leaf_ref.rejects(g.inst, C, n):
        return
    asg, _, _ = leaf_ref.assign(g.inst, C, np.zeros(g.inst.N))
    flat = np.zeros(g.inst.N)
    for r in range(g.inst.R):
        f, i = int(g.inst.row_f[r]), int(g.inst.row_src[r])
        if i >= 0:
            flat[asg[r]] += g.inst.W[f, i] * g.inst.cpr[f, asg[r]]
    a = lp.debug_leaf_repair(g.data, g.variant, z, asg, alpha=g.alpha)
    b = lp.debug_leaf_repair(g.data, g.variant, z, asg, alpha=g.alpha, load=flat)
    assert a[0] == b[0] and a[1] == b[1]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[2], b[2])) and a[3].tobytes() == b[3].tobytes()
    m = leaf_heur_ref.repair(g.inst, C, n, asg, flat)
    m0 = leaf_ref.repair(g.inst, C, n, asg)
    assert m["found"] == m0[0] and m["obj"] == m0[1] and (m["ties"], m["nears"]) == m0[4]


def test_selection():
    g, k = fixture_case(24, 12, 2, "HiGHS 30 s incumbent")
    r4, r1 = mirror_ex(g, k, 30, every=4), mirror_ex(g, k, 30, every=1)
    assert [rd for rd, r in enumerate(r4["rounds"]) if r is not None] == [4, 8, 12, 16, 20, 24, 28, 30]
    assert all(r is not None for r in r1["rounds"][1:]) and r1["rounds"][0] is None
    objs = [r["obj"] if r is not None and r["found"] else math.inf for r in r1["rounds"]]
    assert r1["device_upper"] == min(objs)
    assert r1["upper_round"] in (0, objs.index(min(objs)))          # (the earliest round of the smallest objective)
    assert leaf_heur_ref.repaired(0, 0, 1) and not leaf_heur_ref.repaired(0, 4, 1)
    assert r4["lower"] == r1["lower"]
