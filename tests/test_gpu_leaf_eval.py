"""GPU: the fixed-placement evaluator (nep_leaf_eval / nep_leaf_routing_entries, LPModel.leaf_eval /
leaf_routing; DESIGN.md §7 "Fixed-placement evaluator") on every placement of tests/golden/leaf_eval.json, one batched
call per instance, against the numpy mirror (tests/leaf_ref.py) and the fixture's HiGHS leaf-LP values.

 1. round-0 `lower` equals the mirror's within 1e-11 relative (the fp64 summation order over <= 1e4 terms), the round-0
    loads read through `cpu` the mirror's within 1e-11
 2. at 64 rounds lower <= LP + 2e-6 max(1, |LP|) and lower >= the round-0 value; EXACT and INFEASIBLE statuses as in
    the fixture
 3. every placement the mirror found a point for returns one: its entries meet C1/C2, C4 and C5 in fp64, price at
    `upper`, and `upper` equals the mirror's within 1e-9 relative
 4. two identical calls return identical bits
 5. a cutoff below the LP value gives CUTOFF with lower >= cutoff
 6. prices_in = a call's prices_out reproduce that call's lower at round 0
 7. a facility model, a step-2 model, a fractional c, a negative price and a NULL output are refused
 8. a call while another slot iterates leaves that LP's result bit-identical to a run without the call
 9. more placements than the workspace's chunk; rows wider than a wave and an open list longer than 64
"""
import math

import numpy as np
import pytest

import leaf_ref
from leaf_cases import check_point, groups, margin, mirror

pytestmark = pytest.mark.gpu
_RUNS = {}


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def _run(gi):
    """(model, result at 0 rounds, result at 64 rounds, the 64-round call's routings) of fixture instance gi; the model
    stays open for the module"""
    if gi not in _RUNS:
        from core.engine.lp import LPModel
        g = groups()[gi]
        m = LPModel(g.data, g.variant, step=1, alpha=g.alpha, max_batch=1)
        r0 = m.leaf_eval(g.Z, rounds=0)
        r64 = m.leaf_eval(g.Z, rounds=64)
        pts = [m.leaf_routing(k) if math.isfinite(r64["upper"][k]) else None for k in range(len(g.Z))]
        _RUNS[gi] = (m, r0, r64, pts)
    return _RUNS[gi]


def _congested():
    """(gi, k) of the (12, 6, 1, 1.0) MIP optimum: its CPU rows bind (lower0 < LP)"""
    for gi, g in enumerate(groups()):
        for k, c in enumerate(g.cases):
            if (c["N"], c["seed"], c["placement"]) == (12, 1, "MIP optimum"):
                return gi, k
    raise AssertionError("fixture lacks the (12, 6, 1, 1.0) MIP optimum")


GIDS = list(range(len(groups())))


@pytest.mark.parametrize("gi", GIDS)
def test_round0_matches_the_mirror(gi):
    g = groups()[gi]
    _, r0, _, _ = _run(gi)
    for k, c in enumerate(g.cases):
        ref = mirror(g, k, 0)
        print(c["N"], c["F"], c["variant"], c["placement"], "lower0", r0["lower"][k], "fixture", c["lower0"])
        if c["lower0"] is None:
            assert r0["status"][k] == leaf_ref.INFEASIBLE and r0["lower"][k] == math.inf
            continue
        assert _rel(r0["lower"][k], c["lower0"]) <= 1e-11
        assert _rel(r0["lower"][k], ref["lower"]) <= 1e-11
        assert np.abs(r0["cpu"][k] - ref["cpu"]).max() <= 1e-11 * max(1.0, np.abs(ref["cpu"]).max())
        assert r0["status"][k] == ref["status"] == c["status0"]
    # the device's round-0 loads themselves (a call cut off at round 0 runs no repair, so `cpu` is leaf_node's sum)
    m = _run(gi)[0]
    rc = m.leaf_eval(g.Z, rounds=0, cutoff=-1e300)
    for k, c in enumerate(g.cases):
        if c["lower0"] is None:
            continue
        _, _, load = leaf_ref.assign(g.inst, *g.inst.split(g.Z[k])[:1], np.zeros(g.inst.N))
        assert rc["status"][k] == leaf_ref.CUTOFF
        assert np.abs(rc["cpu"][k] - load).max() <= 1e-11 * max(1.0, load.max())
    m.leaf_eval(g.Z, rounds=64)      # (the module's other tests read the last call's points)


@pytest.mark.parametrize("gi", GIDS)
def test_bound_after_64_rounds(gi):
    g = groups()[gi]
    _, r0, r64, _ = _run(gi)
    for k, c in enumerate(g.cases):
        print(c["N"], c["F"], c["variant"], c["placement"], "lower64", r64["lower"][k], "mirror", c["lower64"], "LP",
              c["lp_value"], "upper", r64["upper"][k], "status", r64["status"][k])
        if c["status64"] == leaf_ref.INFEASIBLE:
            assert r64["status"][k] == leaf_ref.INFEASIBLE
            assert r64["lower"][k] == math.inf and r64["upper"][k] == math.inf
            continue
        if c["lp_value"] is not None:
            assert r64["lower"][k] <= c["lp_value"] + margin(c["lp_value"])
        assert r64["lower"][k] >= r0["lower"][k]
        if c["status64"] == leaf_ref.EXACT:
            assert r64["status"][k] == leaf_ref.EXACT
        assert (r64["prices"][k] >= 0.0).all()


@pytest.mark.parametrize("gi", GIDS)
def test_points(gi):
    g = groups()[gi]
    _, _, r64, pts = _run(gi)
    for k, c in enumerate(g.cases):
        if c["upper"] is None:
            # (the chained-move case may be NO_POINT or better; whatever comes back must be a point)
            if pts[k] is not None:
                assert check_point(g.inst, g.Z[k], pts[k], r64["upper"][k]) == []
            continue
        assert pts[k] is not None, (c["placement"], r64["status"][k])
        assert _rel(r64["upper"][k], c["upper"]) <= 1e-9
        assert check_point(g.inst, g.Z[k], pts[k], r64["upper"][k]) == []
        if c["lp_value"] is not None:
            assert r64["upper"][k] >= c["lp_value"] - margin(c["lp_value"])
        row, dst, _ = pts[k]
        assert (np.diff(row.astype(np.int64) * g.inst.N + dst) > 0).all()     # row-major, ascending destination
        # the loads returned with a point are the point's
        x = leaf_ref.dense_x(g.inst, pts[k])
        cpu = np.einsum("fi,fj,fij->j", g.inst.W, g.inst.cpr, x)
        assert np.abs(r64["cpu"][k] - cpu).max() <= 1e-11 * max(1.0, cpu.max())


def test_two_calls_same_bits():
    gi, _ = _congested()
    g = groups()[gi]
    m, _, r64, _ = _run(gi)
    again = m.leaf_eval(g.Z, rounds=64)
    for key in ("lower", "upper", "status", "prices", "cpu"):
        assert again[key].tobytes() == r64[key].tobytes(), key


def test_cutoff():
    gi, k = _congested()
    g = groups()[gi]
    c = g.cases[k]
    m, r0, _, _ = _run(gi)
    cut = 0.5 * (c["lower0"] + c["lp_value"])       # above the round-0 bound, below the LP value
    r = m.leaf_eval(g.Z[k:k + 1], rounds=64, cutoff=cut)
    print("cutoff", cut, "lower", r["lower"][0], "status", r["status"][0])
    assert r["status"][0] == leaf_ref.CUTOFF and r["lower"][0] >= cut and r["upper"][0] == math.inf
    r = m.leaf_eval(g.Z[k:k + 1], rounds=64, cutoff=c["lower0"] - 1e-3)     # cut off at round 0
    assert r["status"][0] == leaf_ref.CUTOFF and r["lower"][0] == r0["lower"][k]


def test_prices_in_reproduce_the_bound():
    gi, k = _congested()
    g = groups()[gi]
    m, r0, r64, _ = _run(gi)
    assert r64["lower"][k] > r0["lower"][k] and r64["prices"][k].max() > 0.0
    r = m.leaf_eval(g.Z, rounds=0, prices=r64["prices"])
    assert r["lower"].tobytes() == r64["lower"].tobytes()
    assert np.array_equal(r["prices"], r64["prices"])


def test_refusals():
    from core.engine.lp import EngineUnavailable, LPModel, RELAX_FACILITY, STEP2_DELETE
    gi, k = _congested()
    g = groups()[gi]
    m = _run(gi)[0]
    fac = LPModel(g.data, g.variant, step=1, alpha=g.alpha, max_batch=1, relaxation=RELAX_FACILITY)
    st2 = LPModel(g.data, g.variant, step=STEP2_DELETE, alpha=g.alpha, max_score=1.0, max_batch=1)
    try:
        for other in (fac, st2):
            with pytest.raises(EngineUnavailable) as e:
                other.leaf_eval(np.zeros((1, other.n_int)))
            assert "(-1)" in str(e.value) and "step-1 reference-relaxation models" in str(e.value), str(e.value)
    finally:
        fac.close()
        st2.close()
    z = g.Z[k:k + 1].copy()
    z[0, int(np.flatnonzero(z[0] == 1.0)[0])] = 0.5
    with pytest.raises(EngineUnavailable) as e:
        m.leaf_eval(z)
    assert "(-1)" in str(e.value) and "not 0 or 1" in str(e.value), str(e.value)
    with pytest.raises(EngineUnavailable) as e:
        m.leaf_eval(g.Z[k:k + 1], prices=np.full((1, g.inst.N), -1.0))
    assert "(-1)" in str(e.value)
    assert m._lib.nep_leaf_eval(m._h, 1, g.Z[k:k + 1].ctypes.data, None, None, None, None, None, None, None) == -1
    with pytest.raises(EngineUnavailable) as e:
        m.leaf_routing(len(g.Z))
    assert "(-1)" in str(e.value)


def test_a_call_leaves_iterating_lps_alone():
    """two cold solves of the congested 12x6 leaf's LP (its CPU rows bind: it iterates for many blocks of 64), one with
    the evaluator called between its blocks, the other without"""
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
                    m.leaf_eval(g.Z, rounds=8)
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
    gi, k = _congested()
    g = groups()[gi]
    m, _, r64, _ = _run(gi)
    reps = 70 // len(g.Z) + 1
    Z = np.tile(g.Z, (reps, 1))[:70]
    r = m.leaf_eval(Z, rounds=64)
    for key in ("lower", "upper", "status", "prices", "cpu"):
        want = np.tile(r64[key], (reps,) + (1,) * (r64[key].ndim - 1))[:70]
        assert r[key].tobytes() == want.tobytes(), key
    row, dst, val = m.leaf_routing(len(g.Z) + k)            # placement k again, in the call's second round of Z
    row0, dst0, val0 = _run(gi)[3][k]
    assert np.array_equal(row, row0) and np.array_equal(dst, dst0) and np.array_equal(val, val0)
    m.leaf_eval(g.Z, rounds=64)                             # (the module's other tests read the last call's points)


def test_wide_rows_against_the_mirror():
    """150 nodes with half the cores, 90 % of the sources loaded: 137 and 142 rows per function (workgroups of 256
    threads, a wave per row) over 132 open destinations (three chunks of the open list, the last one partial), CPU rows
    that bind.  Round 0 and the repaired point equal the mirror's; the priced rounds raise the bound and keep it valid:
    never above the objective of the repaired point."""
    from core.engine.lp import LPModel
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    N, F = 150, 2
    p = synthetic_payload(N, F, seed=0, rho=0.9)
    p["node_cores"] = [max(1, c // 2) for c in p["node_cores"]]
    data = data_to_solver_input(p, with_db=False)
    inst = leaf_ref.Instance(data, "MinDelayAndUtilization", 0.5)
    assert max(inst.frow[f + 1] - inst.frow[f] for f in range(F)) > 128
    z = np.ones(F * N + N)
    z[:F * N].reshape(F, N)[:, 7::8] = 0.0
    z[F * N + 7::8] = 0.0
    assert not leaf_ref.rejects(inst, *inst.split(z))
    ref = leaf_ref.leaf_eval(inst, z, rounds=0)
    assert ref["status"] == leaf_ref.FEASIBLE and ref["ties"] == (0, 0)
    m = LPModel(data, "MinDelayAndUtilization", step=1, alpha=0.5, max_batch=1)
    try:
        r0 = m.leaf_eval(z[None, :], rounds=0)
        r16 = m.leaf_eval(z[None, :], rounds=16)
        print("wide: lower0", r0["lower"][0], "mirror", ref["lower"], "lower16", r16["lower"][0], "upper",
              r16["upper"][0], "mirror", ref["upper"], "status", r16["status"][0])
        assert _rel(r0["lower"][0], ref["lower"]) <= 1e-11
        assert r0["status"][0] == ref["status"]
        assert np.abs(r0["cpu"][0] - ref["cpu"]).max() <= 1e-11 * max(1.0, np.abs(ref["cpu"]).max())
        assert _rel(r16["upper"][0], ref["upper"]) <= 1e-9
        assert r0["lower"][0] < r16["lower"][0] <= ref["upper"] + 1e-9 * max(1.0, abs(ref["upper"]))
        assert check_point(inst, z, m.leaf_routing(0), r16["upper"][0]) == []
    finally:
        m.close()


def teardown_module(module):
    for m, *_ in _RUNS.values():
        m.close()
    _RUNS.clear()
