"""Instances of the priced-moves suites (tests/test_gpu_leaf_moves.py): the fixture groups of tests/leaf_cases.py, the
capacity-greedy leaf 0 of two generated instances with its last open node closed as well (tests/leaf_heur_cases.py),
and "wide" — synthetic 280x2 seed 2 rho 1 with its cores scaled as tests/test_gpu_leaf_heur.py scales them, at two
placements: the two largest nodes open for both functions (280 loaded rows a function, more than the workgroup's 256
threads, a lane per row, 278 closed columns) and the 100 largest open (an open list beyond 64: a wave per row, two
chunks of the open list, the second partial)."""
import math

import numpy as np

import leaf_moves_ref
import leaf_ref
from leaf_cases import groups
from leaf_heur_cases import Generated, greedy_group

_CACHE = {}


def wide():
    if "wide" in _CACHE:
        return _CACHE["wide"]
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    N, F = 280, 2
    p = synthetic_payload(N, F, seed=2, rho=1.0)
    i0 = leaf_ref.Instance(data_to_solver_input(p, with_db=False), "MinDelayAndUtilization", 0.5)
    order = np.argsort(-i0.cores, kind="stable")
    top = np.sort(order[:2])
    demand = sum(i0.W[f].sum() * i0.cpr[f, top].max() for f in range(F))
    scale = 1.1 * demand / i0.cores[top].sum()
    p["node_cores"] = [int(math.ceil(c * scale)) for c in p["node_cores"]]
    g = Generated()
    g.key, g.variant, g.alpha = ("wide moves", N, F), "MinDelayAndUtilization", 0.5
    g.data = data_to_solver_input(p, with_db=False)
    g.inst = leaf_ref.Instance(g.data, g.variant, g.alpha)
    Z = []
    for K in (2, 100):
        C, n = np.zeros((F, N)), np.zeros(N)
        C[:, order[:K]], n[order[:K]] = 1.0, 1.0
        Z.append(np.concatenate([C.ravel(), n]))
    g.Z, g.names = np.asarray(Z), ["two largest nodes open", "100 largest nodes open"]
    _CACHE["wide"] = g
    return g


def _two(g):
    """leaf 0 and its closed variant of a greedy group"""
    h = Generated()
    h.key, h.variant, h.alpha, h.data, h.inst = g.key + ("moves",), g.variant, g.alpha, g.data, g.inst
    h.Z, h.names = g.Z[:2], g.names[:2]
    return h


NAMES = [f"fixture{gi}" for gi in range(len(groups()))] + ["72x12", "96x8", "wide"]


def case(name):
    if name not in _CACHE:
        if name.startswith("fixture"):
            _CACHE[name] = groups()[int(name[7:])]
        elif name == "wide":
            _CACHE[name] = wide()
        else:
            _CACHE[name] = _two(greedy_group(72, 12, 2, 0.5) if name == "72x12" else greedy_group(96, 8, 1, 1.0))
    return _CACHE[name]


def optima():
    """(group index, placement) of the fixture's MIP optima whose variant has n"""
    out = []
    for gi, g in enumerate(groups()):
        for k, c in enumerate(g.cases):
            if c["placement"] == "MIP optimum" and g.inst.has_n:
                out.append((gi, k))
    return out


def opened_start(g, k):
    """the placement k of a group with its first closed node opened at the first function the ADD screens pass"""
    inst = g.inst
    C, n = inst.split(g.Z[k])
    table = np.zeros((inst.F, inst.N))
    moves = leaf_moves_ref.move_list(inst, C, n, table, 2 * inst.F * inst.N + inst.N)
    adds = {(f, j) for kind, f, j, _ in moves if kind == leaf_moves_ref.ADD}
    for j in np.flatnonzero(n < 0.5).tolist():
        for f in range(inst.F):
            if (f, j) in adds:
                return leaf_moves_ref.apply_move(inst, g.Z[k], leaf_moves_ref.ADD, f, j), j
    raise AssertionError("no node can be opened")
