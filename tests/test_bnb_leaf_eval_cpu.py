"""The native tree's use of the fixed-placement evaluator (csrc/nep_bnb.cpp, nep_bnb_params.leaf_eval)
on CPU: the tree drives HiGHS node LPs through core/engine/lp.PyBnbEngine (as tests/test_bnb_rc_fixing_cpu.py does)
and its evaluator pair is answered by the numpy mirror (tests/leaf_ref.py).

 1. the pair present with leaf_eval = 0, and leaf_eval = 1 without a pair: node, leaf and LP counts equal the plain
    search's
 2. leaf_eval = 1 on two small goldens and on synthetic_payload(12, 6, 1, rho = 1.0) (congested: its CPU rows bind):
    the same optimal objective within the search gap, leaves evaluated, no more leaf LPs than the plain search
 3. where the evaluator's routing ends as the incumbent (incumbent_source 3), nep_bnb_incumbent_routing's point passes
    check_placement and prices at the reported incumbent; it does on at least one instance
"""
import types
import warnings

import numpy as np
import pytest

import leaf_ref
from golden_util import golden, payload
from gpu_cases import VARIANT
from oracle_lp import OracleLP, StreamingOracleLP

G = golden()
GOLDENS = [n for n in ("syn_6x4_s1_r0.3_NeptuneMinDelayAndUtilization", "syn_8x4_s3_r1.0_NeptuneMinUtilization") if n in G]
CASES = GOLDENS + ["synthetic_12x6_s1_r1.0"]


class _LeafMixin:
    """LPModel.leaf_eval / leaf_routing's contracts from the mirror; the routing in this model's literal (f, i) rows"""

    def __init__(self, data, variant, **kw):
        super().__init__(data, variant, **kw)
        self.inst = leaf_ref.Instance(data, variant, kw.get("alpha", 0.5))
        self.leaf_log = []

    def leaf_eval(self, z, rounds=32, cutoff=np.inf, prices=None):
        z = np.asarray(z, np.float64).reshape(-1, self.n_int)
        self._last = [leaf_ref.leaf_eval(self.inst, zk, rounds=rounds, cutoff=cutoff) for zk in z]
        self.leaf_log.append((len(z), float(cutoff), [int(r["status"]) for r in self._last]))
        return {k: np.array([r[k] for r in self._last]) for k in ("lower", "upper", "status")}

    def leaf_routing(self, k):
        inst, N = self.inst, self.N
        row, dst, val = [], [], []
        for r, j, v in zip(*self._last[k]["entries"]):
            f, i = int(inst.row_f[r]), int(inst.row_src[r])
            for src in ([i] if i >= 0 else np.flatnonzero(inst.W[f] == 0.0).tolist()):
                row.append(f * N + src)
                dst.append(int(j))
                val.append(float(v))
        order = np.lexsort((dst, row))
        return np.asarray(row, np.int32)[order], np.asarray(dst, np.int32)[order], np.asarray(val)[order]


class LeafOracleLP(_LeafMixin, OracleLP):
    pass


class LeafStreamingOracleLP(_LeafMixin, StreamingOracleLP):
    pass


def _payload(name):
    if name in G:
        return payload(name)
    from core.utils.synthetic import synthetic_payload
    return synthetic_payload(12, 6, seed=1, rho=1.0)


def _search(name, cls, **kw):
    from core.engine.bnb import BranchAndBound
    from core.utils import data_to_solver_input
    p = _payload(name)
    data = data_to_solver_input(p, workload_coeff=p.get("workload_coeff", 1), with_db=False)
    lp = cls(data, VARIANT[p["solver"]["type"]], step=1, max_batch=6, alpha=p["solver"].get("args", {}).get("alpha", 0.5))
    bb = BranchAndBound(lp, data.workload_matrix, data.function_memory_matrix, data.node_memory_matrix, batch=4,
                        node_limit=20000, native=True, **kw)
    return bb.solve(), lp, bb, data


def _leaf_lps(res):
    return sum(res.lp_status_kind["leaf"].values()) + sum(res.lp_status_kind["retry"].values())


@pytest.fixture(scope="module")
def runs():
    return {name: (_search(name, OracleLP), _search(name, LeafOracleLP, leaf_eval=True)) for name in CASES}


@pytest.mark.parametrize("name", GOLDENS)
def test_off_or_without_a_pair_is_the_plain_search(name):
    plain = _search(name, StreamingOracleLP)[0]
    off, lp_off, _, _ = _search(name, LeafStreamingOracleLP, leaf_eval=False)
    nopair = _search(name, StreamingOracleLP, leaf_eval=True)[0]
    for r in (off, nopair):
        assert r.native and (r.nodes, r.leaves, r.lps) == (plain.nodes, plain.leaves, plain.lps)
        assert r.status == plain.status and r.objective == plain.objective
        assert r.leaf_stats["leaf_eval_calls"] == 0 and r.incumbent_source != 3
    assert lp_off.leaf_log == []


@pytest.mark.parametrize("name", CASES)
def test_on_keeps_the_optimum_with_no_more_leaf_lps(name, runs):
    (off, _, bb, _), (on, lp, _, _) = runs[name]
    print(name, "off", (off.nodes, off.leaves, off.lps, _leaf_lps(off)), off.objective, f"{off.seconds:.2f}s", "on",
          (on.nodes, on.leaves, on.lps, _leaf_lps(on)), on.objective, on.leaf_stats, "source", on.incumbent_source)
    assert off.native and on.native and off.status == on.status == "OPTIMAL"
    assert abs(on.objective - off.objective) <= 2.0 * bb.gap * max(1.0, abs(off.objective))
    if name in G:
        ref = G[name]["models"][0]["mip_objective"]
        assert abs(on.objective - ref) <= 2.0 * bb.gap * max(1.0, abs(ref))
    ls = on.leaf_stats
    assert ls["leaf_eval_leaves"] > 0 and ls["leaf_eval_calls"] == len(lp.leaf_log)
    assert ls["leaf_eval_leaves"] == sum(n for n, _, _ in lp.leaf_log)
    assert _leaf_lps(on) <= _leaf_lps(off)
    assert off.leaf_stats["leaf_eval_calls"] == 0


def test_the_evaluators_routing_as_incumbent(runs):
    from core.solvers.neptune.neptune_step import NeptuneStepBase
    seen = 0
    for name in CASES:
        on, lp, _, data = runs[name][1]
        if on.leaf_stats["leaf_eval_incumbents"] > 0:
            seen += 1
        if on.incumbent_source != 3:
            continue
        inst = lp.inst
        C, n = inst.split(on.z)
        x = np.asarray(on.x, np.float64).transpose(1, 0, 2)          # [f, i, j]
        nn = n if n is not None else (C.sum(axis=0) > 0.5).astype(np.float64)
        assert NeptuneStepBase.check_placement(types.SimpleNamespace(data=data), C, nn, x), name
        obj = (inst.cost_n * float(n.sum()) if n is not None else 0.0) + \
            inst.kobj * float(np.einsum("fi,ij,fij->", inst.W, inst.D, x))
        assert abs(obj - on.objective) <= 1e-9 * max(1.0, abs(obj)), (name, obj, on.objective)
    assert seen > 0 and any(runs[name][1][0].incumbent_source == 3 for name in CASES)


def test_python_loop_ignores_the_option_with_one_warning():
    from core.engine.bnb import BranchAndBound
    from core.utils import data_to_solver_input
    p = payload(GOLDENS[0])
    data = data_to_solver_input(p, workload_coeff=p.get("workload_coeff", 1), with_db=False)

    def run(**kw):
        lp = OracleLP(data, VARIANT[p["solver"]["type"]], step=1, max_batch=6,
                      alpha=p["solver"].get("args", {}).get("alpha", 0.5))
        bb = BranchAndBound(lp, data.workload_matrix, data.function_memory_matrix, data.node_memory_matrix, batch=4,
                            node_limit=20000, native=False, **kw)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            a = bb.solve()
            b = bb.solve()
        return a, b, w
    a, b, w = run(leaf_eval=True)
    assert sum("leaf_eval" in str(x.message) for x in w) == 1
    assert a.status == b.status == "OPTIMAL" and not a.native and a.leaf_stats is None
