"""GPU: the fixed-placement evaluator's per-round repair on the device (nep_leaf_eval_ex, LPModel.leaf_eval(...,
repair_every=k); csrc/nep_leaf_heur.hip, DESIGN.md §7 "Fixed-placement evaluator") against the numpy mirror
(tests/leaf_heur_ref.py), one batched call per instance.

Shapes: the fixture groups at 32 rounds; at 16 rounds the capacity-greedy leaves 0 and 1 of synthetic 72x12 seed 2
rho 0.5 (449 rows, scans that cross a wave) and of 96x8 seed 1 rho 1 (no pooled rows, 120 rows on a node), each also
with its last open node closed; and "wide": synthetic 280x2 seed 2 rho 1 with the two largest nodes open for both
functions and every node's cores scaled so that those two hold 1.1 times the demand — 560 rows, 298 to 395 of them on
the one overloaded node (more than the workgroup's 256 threads) in 12 of its 16 rounds, no overloaded node in the other
four, a point in every round (checked with the mirror).

 a. repair_every = 0 returns nep_leaf_eval's lower, upper, status, prices, cpu and entries bit for bit
 b. repair_every = 1: lower and prices unchanged, upper <= (a)'s, every returned routing passes check_point at its price
 c. two calls return the same bits
 d. round_upper equals the mirror's per-round verdict and objective (1e-9 relative) on every (placement, round) whose
    mirror repair reports nears == 0; at least half of each fixture placement's rounds are compared
 e. device_upper agrees with the host-verified objective of round upper_round (1e-9) wherever the mirror flags no
    near-tie in that round; over all placements of the file at least 90 % agree
 f. repair_every = 4 repairs exactly rounds 4, 8, ... and the last one
 g. synthetic 12x6 seed 1 rho 1: the search with leaf_eval = 2 ends at the optimum leaf_eval = 0 finds
"""
import math

import numpy as np
import pytest

import leaf_ref
from leaf_cases import check_point, groups
from leaf_heur_cases import FIXTURE_ROUNDS, GENERATED_ROUNDS, Generated, greedy_group, mirror_ex

pytestmark = pytest.mark.gpu
_RUNS = {}
_AGREE = {}


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def _wide():
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    N, F, K = 280, 2, 2
    p = synthetic_payload(N, F, seed=2, rho=1.0)
    i0 = leaf_ref.Instance(data_to_solver_input(p, with_db=False), "MinDelayAndUtilization", 0.5)
    top = np.sort(np.argsort(-i0.cores, kind="stable")[:K])
    demand = sum(i0.W[f].sum() * i0.cpr[f, top].max() for f in range(F))
    scale = 1.1 * demand / i0.cores[top].sum()
    p["node_cores"] = [int(math.ceil(c * scale)) for c in p["node_cores"]]
    g = Generated()
    g.key, g.variant, g.alpha = ("wide", N, F), "MinDelayAndUtilization", 0.5
    g.data = data_to_solver_input(p, with_db=False)
    g.inst = leaf_ref.Instance(g.data, g.variant, g.alpha)
    C, n = np.zeros((F, N)), np.zeros(N)
    C[:, top], n[top] = 1.0, 1.0
    g.Z, g.names = np.concatenate([C.ravel(), n])[None, :], ["two largest nodes open"]
    return g


def _sets():
    """(name, group, rounds) of every instance of the file"""
    if "sets" not in _RUNS:
        out = [(f"fixture{gi}", g, FIXTURE_ROUNDS) for gi, g in enumerate(groups())]
        out.append(("72x12", greedy_group(72, 12, 2, 0.5), GENERATED_ROUNDS))
        out.append(("96x8", greedy_group(96, 8, 1, 1.0), GENERATED_ROUNDS))
        out.append(("wide", _wide(), GENERATED_ROUNDS))
        _RUNS["sets"] = out
    return _RUNS["sets"]


NAMES = [f"fixture{gi}" for gi in range(len(groups()))] + ["72x12", "96x8", "wide"]


def _run(name):
    """the calls of one instance: plain nep_leaf_eval, repair_every 0, 1 (twice) and 4, each with its routings"""
    if name not in _RUNS:
        from core.engine.lp import LPModel
        _, g, rounds = next(s for s in _sets() if s[0] == name)
        m = LPModel(g.data, g.variant, step=1, alpha=g.alpha, max_batch=1)
        try:
            out = {}
            for tag, kw in (("plain", {}), ("r0", dict(repair_every=0)), ("r1", dict(repair_every=1)),
                            ("again", dict(repair_every=1)), ("r4", dict(repair_every=4))):
                r = m.leaf_eval(g.Z, rounds=rounds, **kw)
                r["points"] = [m.leaf_routing(k) if math.isfinite(r["upper"][k]) else None for k in range(len(g.Z))]
                out[tag] = r
        finally:
            m.close()
        _RUNS[name] = (g, rounds, out)
    return _RUNS[name]


@pytest.mark.parametrize("name", NAMES)
def test_repair_every_0_is_the_plain_call(name):
    g, rounds, out = _run(name)
    a, b = out["plain"], out["r0"]
    for key in ("lower", "upper", "status", "prices", "cpu"):
        assert a[key].tobytes() == b[key].tobytes(), key
    for pa, pb in zip(a["points"], b["points"]):
        assert (pa is None) == (pb is None)
        if pa is not None:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(pa, pb))
    assert np.isinf(b["device_upper"]).all() and np.isinf(b["round_upper"]).all()
    assert (b["upper_round"] == np.where(np.isfinite(b["upper"]), 0, -1)).all()


@pytest.mark.parametrize("name", NAMES)
def test_repair_every_1_returns_verified_points(name):
    g, rounds, out = _run(name)
    a, b = out["plain"], out["r1"]
    assert a["lower"].tobytes() == b["lower"].tobytes() and a["prices"].tobytes() == b["prices"].tobytes()
    for k in range(len(g.Z)):
        print(name, k, "lower", b["lower"][k], "upper", a["upper"][k], "->", b["upper"][k], "round", b["upper_round"][k],
              "device", b["device_upper"][k], "status", a["status"][k], "->", b["status"][k])
        assert b["upper"][k] <= a["upper"][k]
        assert (b["points"][k] is not None) == math.isfinite(b["upper"][k]) == (b["upper_round"][k] >= 0)
        if b["points"][k] is not None:
            assert check_point(g.inst, g.Z[k], b["points"][k], b["upper"][k]) == []
            assert b["status"][k] in (leaf_ref.EXACT, leaf_ref.FEASIBLE)
            x = leaf_ref.dense_x(g.inst, b["points"][k])
            cpu = np.einsum("fi,fj,fij->j", g.inst.W, g.inst.cpr, x)
            assert np.abs(b["cpu"][k] - cpu).max() <= 1e-11 * max(1.0, cpu.max())
        elif a["status"][k] != leaf_ref.INFEASIBLE:
            assert b["status"][k] == a["status"][k]


@pytest.mark.parametrize("name", NAMES)
def test_two_calls_same_bits(name):
    _, _, out = _run(name)
    for key in ("lower", "upper", "status", "prices", "cpu", "upper_round", "device_upper", "round_upper"):
        assert out["r1"][key].tobytes() == out["again"][key].tobytes(), key


@pytest.mark.parametrize("name", NAMES)
def test_round_upper_matches_the_mirror(name):
    g, rounds, out = _run(name)
    r = out["r1"]
    for k in range(len(g.Z)):
        ref = mirror_ex(g, k, rounds)
        if ref["status"] == leaf_ref.INFEASIBLE:
            assert np.isinf(r["round_upper"][k]).all()
            continue
        compared = flagged = 0
        for rd, rr in enumerate(ref["rounds"]):
            if rr is None:
                assert r["round_upper"][k, rd] == math.inf, (k, rd)
                continue
            if rr["nears"] != 0:
                flagged += 1
                continue
            compared += 1
            want = rr["obj"] if rr["found"] else math.inf
            got = r["round_upper"][k, rd]
            assert (got == want) if math.isinf(want) else _rel(got, want) <= 1e-9, (k, rd, got, want, rr)
        repaired = compared + flagged
        print(name, k, "rounds repaired", repaired, "compared", compared)
        if name.startswith("fixture"):
            assert 2 * compared >= repaired
        if name == "wide":
            assert repaired == rounds and max(rr["moves"] for rr in ref["rounds"] if rr is not None) > 0


@pytest.mark.parametrize("name", NAMES)
def test_device_upper_against_the_verified_point(name):
    g, rounds, out = _run(name)
    r = out["r1"]
    agree = []
    for k in range(len(g.Z)):
        ref = mirror_ex(g, k, rounds)
        dev, up, rnd = r["device_upper"][k], r["upper"][k], int(r["upper_round"][k])
        if r["status"][k] in (leaf_ref.INFEASIBLE, leaf_ref.CUTOFF):
            continue
        if math.isinf(dev):
            ok = math.isinf(ref["device_upper"])
            sel = None
        else:
            finite = np.flatnonzero(np.isfinite(r["round_upper"][k]))
            sel = int(finite[np.argmin(r["round_upper"][k][finite])])      # (argmin: the earliest of equal rounds)
            assert r["round_upper"][k, sel] == dev
            if rnd > 0:
                assert rnd == sel
                ok = _rel(dev, up) <= 1e-9
            else:
                ok = rnd == 0 and up <= dev + 1e-9 * max(1.0, abs(dev))     # round 0's verified point is no dearer
        agree.append(ok)
        if not ok:
            flagged = [rd for rd, rr in enumerate(ref["rounds"]) if rr is not None and rr["nears"] != 0]
            print(name, k, "device_upper", dev, "round", sel, "upper", up, "upper_round", rnd, "flagged", flagged)
            assert sel in flagged if sel is not None else bool(flagged), (name, k)
    _AGREE[name] = agree
    if len(_AGREE) == len(NAMES):
        every = [a for v in _AGREE.values() for a in v]
        print("device_upper agrees on", sum(every), "of", len(every), "placements")
        assert sum(every) >= 0.9 * len(every)


@pytest.mark.parametrize("name", NAMES)
def test_repair_every_4(name):
    g, rounds, out = _run(name)
    r1, r4 = out["r1"], out["r4"]
    want = [rd for rd in range(rounds + 1) if (rd > 0 and rd % 4 == 0) or rd == rounds]
    assert r4["lower"].tobytes() == r1["lower"].tobytes()
    for k in range(len(g.Z)):
        off = [rd for rd in range(rounds + 1) if rd not in want]
        assert np.isinf(r4["round_upper"][k, off]).all()
        assert r4["round_upper"][k, want].tobytes() == r1["round_upper"][k, want].tobytes()
        if r4["points"][k] is not None:
            assert check_point(g.inst, g.Z[k], r4["points"][k], r4["upper"][k]) == []


def test_search_with_leaf_eval_2():
    from core.engine.lp import LPModel
    from core.solvers.neptune.neptune_step import NeptuneStep1CPUMinDelayAndUtilization
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    p = synthetic_payload(12, 6, seed=1, rho=1.0)
    alpha = p["solver"]["args"]["alpha"]
    data = data_to_solver_input(p, with_db=False)
    res = {}
    for leaf_eval in (0, 2):
        batch = 16
        st1 = NeptuneStep1CPUMinDelayAndUtilization(alpha=alpha, verbose=False, batch=batch)
        st1.leaf_eval = leaf_eval
        st1.load_data(data)
        m = LPModel(data, "MinDelayAndUtilization", step=1, alpha=alpha, max_batch=batch + 2)
        bm = st1.bound_model(data, batch + 1)
        try:
            r = res[leaf_eval] = st1.branch_and_bound(m, bm, time_limit=60.0).solve()
        finally:
            m.close()
            bm.close()
        print(f"leaf_eval {leaf_eval}: status {r.status} incumbent {r.objective} bound {r.bound} nodes {r.nodes} "
              f"leaves {r.leaves} lps {r.lps} source {r.incumbent_source} {r.leaf_stats} seconds {r.seconds:.2f}")
    assert res[0].native and res[2].native
    assert res[0].status == res[2].status == "OPTIMAL"
    assert abs(res[2].objective - res[0].objective) <= 1e-6 * max(1.0, abs(res[0].objective))
    assert res[0].leaf_stats["leaf_eval_calls"] == 0 and res[2].leaf_stats["leaf_eval_calls"] > 0
