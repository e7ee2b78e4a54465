"""Cases of the fixed-placement evaluator's per-round repair (nep_leaf_eval_ex) for the CPU and GPU suites: the fixture
groups of tests/leaf_cases.py at 32 rounds and generated capacity-greedy leaves at 16, each with the mirror's result
(tests/leaf_heur_ref.py), computed once per process."""
import numpy as np

import leaf_heur_ref
import leaf_ref
from leaf_cases import groups

FIXTURE_ROUNDS, GENERATED_ROUNDS = 32, 16
_CACHE = {}


class Generated:
    """One generated instance and its placements: data, inst (leaf_ref.Instance), variant, alpha, Z [n, n_int], names."""


def greedy_group(N, F, seed, rho, closed=True):
    """capacity-greedy leaves 0 and 1 of synthetic (N, F, seed, rho), MinDelayAndUtilization at alpha 0.5, and (closed)
    each with its last open node closed"""
    key = ("greedy", N, F, seed, rho, closed)
    if key in _CACHE:
        return _CACHE[key]
    from core.engine.heuristics import capacity_greedy
    from core.solvers.neptune.neptune_step import NeptuneStep1CPUMinDelayAndUtilization
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    g = Generated()
    g.key, g.variant, g.alpha = key, "MinDelayAndUtilization", 0.5
    d = g.data = data_to_solver_input(synthetic_payload(N, F, seed=seed, rho=rho), with_db=False)
    g.inst = leaf_ref.Instance(d, g.variant, g.alpha)
    st1 = NeptuneStep1CPUMinDelayAndUtilization(alpha=0.5, verbose=False)
    st1.load_data(d)
    wts = st1.objective_weights()
    leaves = capacity_greedy(d.workload_matrix, d.node_delay_matrix, d.core_per_req_matrix, d.node_cores_matrix,
                             d.function_memory_matrix, d.node_memory_matrix, np.asarray(d.node_cores_matrix, float),
                             tries=4, node_cost=wts[0], delay_coef=wts[1], new_pen=1.0)
    Z, names = [], []
    for k, (C, n, _, _) in enumerate(leaves[:2]):
        C, n = np.asarray(C, np.float64).reshape(F, N), np.asarray(n, np.float64).reshape(N)
        Z.append(np.concatenate([C.ravel(), n]))
        names.append(f"leaf {k}")
        if closed:
            j = int(np.flatnonzero(n > 0.5)[-1])
            C2, n2 = C.copy(), n.copy()
            C2[:, j] = 0.0
            n2[j] = 0.0
            Z.append(np.concatenate([C2.ravel(), n2]))
            names.append(f"leaf {k}, last open node closed")
    g.Z, g.names = np.asarray(Z), names
    _CACHE[key] = g
    return g


def mirror_ex(g, k, rounds, every=1):
    """the mirror's leaf_eval_ex of placement k of a group (fixture or generated), once per (group, k, rounds, every)"""
    key = ("ex", g.key, k, rounds, every)
    if key not in _CACHE:
        _CACHE[key] = leaf_heur_ref.leaf_eval_ex(g.inst, g.Z[k], rounds=rounds, every=every)
    return _CACHE[key]


def fixture_case(N, F, seed, placement):
    """(group, index) of the MinDelayAndUtilization fixture placement named `placement` of instance (N, F, seed)"""
    for g in groups():
        for k, c in enumerate(g.cases):
            if (c["N"], c["F"], c["seed"], c["variant"], c["placement"]) == \
                    (N, F, seed, "MinDelayAndUtilization", placement):
                return g, k
    raise AssertionError(f"fixture lacks {(N, F, seed, placement)}")
