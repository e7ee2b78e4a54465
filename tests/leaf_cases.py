"""The fixture of the fixed-placement evaluator (tests/golden/leaf_eval.json, tools/gen_leaf_golden.py) grouped by
instance, with the numpy mirror's instance view (tests/leaf_ref.py), for the CPU and GPU suites."""
import json
import os

import numpy as np

import leaf_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leaf_eval.json")
_CACHE = {}


class Group:
    """One instance and its fixture placements: data (core.utils Data), inst (leaf_ref.Instance), cases (fixture
    dicts), Z [n, n_int]."""


def margin(lp):
    """the margin tests/test_gpu_reduced_costs.py gives a HiGHS value"""
    return 2e-6 * max(1.0, abs(lp))


def groups():
    if "g" in _CACHE:
        return _CACHE["g"]
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    out = {}
    for c in cases:
        key = (c["N"], c["F"], c["seed"], c["rho"], c["variant"])
        if key not in out:
            g = out[key] = Group()
            p = synthetic_payload(c["N"], c["F"], seed=c["seed"], rho=c["rho"])
            g.key, g.variant, g.alpha = key, c["variant"], c["alpha"]
            g.data = data_to_solver_input(p, with_db=False)
            g.inst = leaf_ref.Instance(g.data, c["variant"], c["alpha"])
            g.cases, g.Z = [], []
        g = out[key]
        g.cases.append(c)
        g.Z.append(np.concatenate([np.ravel(c["c"]), c["n"] if c["n"] is not None else []]).astype(np.float64))
    for g in out.values():
        g.Z = np.asarray(g.Z)
    _CACHE["g"] = list(out.values())
    return _CACHE["g"]


def mirror(g, k, rounds):
    """the mirror's leaf_eval of placement k of a group, computed once per (group, placement, rounds)"""
    key = (g.key, k, rounds)
    if key not in _CACHE:
        _CACHE[key] = leaf_ref.leaf_eval(g.inst, g.Z[k], rounds=rounds)
    return _CACHE[key]


def check_point(inst, z, entries, upper):
    """C1/C2, C4 and C5 of the routing `entries` at the placement z in fp64, and its price: returns a list of
    complaints (empty: the point is feasible and priced at `upper`)."""
    C, n = inst.split(z)
    x = leaf_ref.dense_x(inst, entries)                      # [f, i, j]
    bad = []
    col = x.sum(axis=1)
    if (col[C < 0.5] > 0.0).any():
        bad.append("flow into a closed placement (C1)")
    if (col < C * (1.0 - inst.eps) - 1e-12).any():
        bad.append("a column floor missed (C2)")
    if np.abs(x.sum(axis=2) - 1.0).max() > 1e-12:
        bad.append("a source not routed once (C4)")
    cpu = np.einsum("fi,fj,fij->j", inst.W, inst.cpr, x)
    if (cpu > inst.cores).any():
        bad.append(f"CPU above cores (C5): {(cpu - inst.cores).max()}")
    obj = (inst.cost_n * float(n.sum()) if n is not None else 0.0) + \
        inst.kobj * float(np.einsum("fi,ij,fij->", inst.W, inst.D, x))
    if abs(obj - upper) > 1e-9 * max(1.0, abs(upper)):
        bad.append(f"priced at {obj}, reported {upper}")
    return bad
