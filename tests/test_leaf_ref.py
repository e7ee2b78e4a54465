"""CPU: the numpy mirror of the fixed-placement evaluator (tests/leaf_ref.py) against the HiGHS leaf-LP values of
tests/golden/leaf_eval.json, and the engine's host repair (csrc/nep_leaf_repair.cpp through nep_debug_leaf_repair)
against the mirror's.

 1. the mirror reproduces the fixture (lower at 0 and 64 rounds, upper, statuses): the fixture is current
 2. lower <= LP + 2e-6 max(1, |LP|) at every round (the margin tests/test_gpu_reduced_costs.py gives HiGHS);
    upper >= LP - the same margin; every returned point passes NeptuneStepBase.check_placement
 3. the uncongested placements end EXACT at round 0 (at least the fixture's four: (16, 8) and (24, 12)
    MinDelayAndUtilization, (16, 8) MinDelay and MinUtilization)
 4. the (12, 6, 1, 1.0) closed-node placement, whose routing is infeasible, has lower > 1.0 after 256 rounds
 5. the host repair matches the mirror's on every placement: same status, upper within 1e-9 relative, same entries
 6. a placement a row rejects, a fractional c and a facility descriptor at nep_debug_leaf_repair
"""
import ctypes
import math
import types

import numpy as np
import pytest

import leaf_ref
from leaf_cases import check_point, groups, margin, mirror

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


@pytest.mark.parametrize("p", CASES, ids=_id)
def test_mirror_reproduces_the_fixture(p):
    g, c = groups()[p[0]], groups()[p[0]].cases[p[1]]
    r0, r64 = mirror(g, p[1], 0), mirror(g, p[1], 64)
    fin = lambda v: v if math.isfinite(v) else None
    assert (int(r0["status"]), int(r64["status"])) == (c["status0"], c["status64"])
    for got, want in ((r0["lower"], c["lower0"]), (r64["lower"], c["lower64"]), (r64["upper"], c["upper"])):
        assert (fin(got) is None) == (want is None)
        if want is not None:
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize("p", CASES, ids=_id)
def test_mirror_brackets_the_leaf_lp(p):
    g, c = groups()[p[0]], groups()[p[0]].cases[p[1]]
    r = mirror(g, p[1], 64)
    if c["status64"] == leaf_ref.INFEASIBLE:
        assert c["lp_value"] is None and r["lower"] == math.inf
        return
    assert (np.diff(r["hist"]) >= 0.0).all()
    if c["lp_value"] is not None:
        assert r["hist"].max() <= c["lp_value"] + margin(c["lp_value"])
    if r["entries"] is not None:
        if c["lp_value"] is not None:
            assert r["upper"] >= c["lp_value"] - margin(c["lp_value"])
        assert c["lp_value"] is not None, "a point at a placement HiGHS calls infeasible"
        assert _passes_check_placement(g, g.Z[p[1]], r["entries"])
        assert check_point(g.inst, g.Z[p[1]], r["entries"], r["upper"]) == []


def test_uncongested_placements_are_exact_at_round_0():
    exact = []
    for gi, k in CASES:
        g, c = groups()[gi], groups()[gi].cases[k]
        if c["lower0"] is not None and c["lp_value"] is not None and \
                abs(c["lower0"] - c["lp_value"]) <= margin(c["lp_value"]) and c["upper"] is not None:
            r = mirror(g, k, 0)
            assert r["status"] == leaf_ref.EXACT, _id((gi, k))
            exact.append((c["N"], c["F"], c["variant"], c["placement"]))
    for want in ((16, 8, "MinDelayAndUtilization", "MIP optimum"), (24, 12, "MinDelayAndUtilization", "MIP optimum"),
                 (16, 8, "MinDelay", "MIP optimum"), (16, 8, "MinUtilization", "MIP optimum")):
        assert want in exact, want


def test_infeasible_routing_shows_as_a_runaway_bound():
    for gi, k in CASES:
        g, c = groups()[gi], groups()[gi].cases[k]
        if (c["N"], c["seed"], c["placement"]) == (12, 1, "MIP optimum, last open node closed"):
            assert c["lp_value"] is None and c["status64"] == leaf_ref.NO_POINT
            r = leaf_ref.leaf_eval(g.inst, g.Z[k], rounds=256)
            assert r["lower"] > 1.0 and r["status"] == leaf_ref.NO_POINT, r["lower"]
            return
    raise AssertionError("fixture lacks the (12, 6, 1, 1.0) closed-node placement")


@pytest.mark.parametrize("p", CASES, ids=_id)
def test_host_repair_matches_the_mirror(p):
    from core.engine import lp
    g, c = groups()[p[0]], groups()[p[0]].cases[p[1]]
    z = g.Z[p[1]]
    C, n = g.inst.split(z)
    if leaf_ref.rejects(g.inst, C, n):
        found, upper, ent, _ = lp.debug_leaf_repair(g.data, g.variant, z, np.zeros(g.inst.R, np.int32), alpha=g.alpha)
        assert not found and upper == math.inf and len(ent[0]) == 0
        return
    asg, _, _ = leaf_ref.assign(g.inst, C, np.zeros(g.inst.N))
    ok, obj, ent, cpu, _ = leaf_ref.repair(g.inst, C, n, asg)
    found, upper, ent2, cpu2 = lp.debug_leaf_repair(g.data, g.variant, z, asg, alpha=g.alpha)
    assert found == ok == (c["upper"] is not None)
    if not ok:
        assert upper == math.inf
        return
    assert abs(upper - obj) <= 1e-9 * max(1.0, abs(obj))
    assert np.array_equal(ent2[0], ent[0]) and np.array_equal(ent2[1], ent[1])
    assert np.abs(ent2[2] - ent[2]).max() <= 1e-12
    assert np.abs(cpu2 - cpu).max() <= 1e-12 * max(1.0, cpu.max())
    assert _passes_check_placement(g, z, ent2)


def test_host_repair_refusals():
    from core.engine import lp
    g = groups()[0]
    z = g.Z[0].copy()
    z[int(np.flatnonzero(z == 1.0)[0])] = 0.5
    with pytest.raises(lp.EngineUnavailable) as e:
        lp.debug_leaf_repair(g.data, g.variant, z, np.zeros(g.inst.R, np.int32), alpha=g.alpha)
    assert "(-1)" in str(e.value)
    # an assignment to a closed placement is no assignment of this leaf: no point, no fault
    C, _ = g.inst.split(g.Z[0])
    closed = int(np.flatnonzero(C[0] < 0.5)[0])
    found, upper, _, _ = lp.debug_leaf_repair(g.data, g.variant, g.Z[0], np.full(g.inst.R, closed, np.int32),
                                              alpha=g.alpha)
    assert not found and upper == math.inf
    lib = lp.load_library()
    k = lp._arrays(g.data, g.inst.N, g.inst.F)
    d = lp._desc(k, g.inst.N, g.inst.F, lp.VARIANTS[g.variant], lp.STEP1, g.alpha, 1.3, 0.0, 0.0, g.data.node_budget,
                 lp.RELAX_FACILITY)
    out = np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int64)
    asg = np.zeros(g.inst.R, np.int32)
    rc = lib.nep_debug_leaf_repair(ctypes.byref(d), g.Z[0].ctypes.data, asg.ctypes.data, out[0].ctypes.data,
                                   out[1].ctypes.data, 0, out[2].ctypes.data, None, None, None, None)
    assert rc == -1 and b"step-1 reference-relaxation" in lib.nep_last_error()
