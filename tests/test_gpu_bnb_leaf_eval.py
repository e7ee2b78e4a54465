"""GPU: the fixed-placement evaluator in the product's step-1 search (NeptuneStepBase.leaf_eval /
BranchAndBound(leaf_eval=True): native tree, facility-relaxation branching nodes, reference-model leaves evaluated by
nep_leaf_eval before their LPs; DESIGN.md §7 "Fixed-placement evaluator").  synthetic_payload(16, 8, seed 0),
MinDelayAndUtilization step 1, once with the option off and once with it on:

  * both end OPTIMAL with equal objectives within 1e-6 relative;
  * the on-run resolved leaves EXACT (leaf_eval_exact > 0) and ran no more leaf LPs than the off-run;
  * its final routing meets every reference row (scale_util.check_step1_solution) at its reported objective."""
import numpy as np
import pytest

from scale_util import check_step1_solution

pytestmark = pytest.mark.gpu


def _dense_rows(x):
    xb = np.zeros((len(x.row_f), x.N))
    np.add.at(xb, (x.row, x.dst), x.val)
    return xb


def _leaf_lps(res):
    return sum(res.lp_status_kind["leaf"].values()) + sum(res.lp_status_kind["retry"].values())


def _search(data, alpha, leaf_eval):
    from core.engine.lp import LPModel
    from core.solvers.neptune.neptune_step import NeptuneStep1CPUMinDelayAndUtilization
    batch = 16
    st1 = NeptuneStep1CPUMinDelayAndUtilization(alpha=alpha, verbose=False, batch=batch)
    st1.leaf_eval = leaf_eval
    st1.load_data(data)
    m = LPModel(data, "MinDelayAndUtilization", step=1, alpha=alpha, max_batch=batch + 2)
    bm = st1.bound_model(data, batch + 1)
    try:
        return st1.branch_and_bound(m, bm, time_limit=60.0).solve()
    finally:
        m.close()
        bm.close()


def test_leaf_eval_in_the_16x8_search():
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    p = synthetic_payload(16, 8, seed=0)
    alpha = p["solver"]["args"]["alpha"]
    data = data_to_solver_input(p, with_db=False)
    off = _search(data, alpha, False)
    on = _search(data, alpha, True)
    for tag, r in (("off", off), ("on", on)):
        print(f"leaf_eval {tag}: status {r.status} incumbent {r.objective} bound {r.bound} nodes {r.nodes} leaves "
              f"{r.leaves} lps {r.lps} leaf lps {_leaf_lps(r)} source {r.incumbent_source} {r.leaf_stats} "
              f"seconds {r.seconds:.2f}")
    assert off.native and on.native
    assert off.status == on.status == "OPTIMAL"
    assert abs(on.objective - off.objective) <= 1e-6 * max(1.0, abs(off.objective))
    assert off.leaf_stats["leaf_eval_calls"] == 0
    assert on.leaf_stats["leaf_eval_exact"] > 0, on.leaf_stats
    assert _leaf_lps(on) <= _leaf_lps(off)
    viol, worst, obj = check_step1_solution(data, "MinDelayAndUtilization", alpha, _dense_rows(on.x), on.x.row_f,
                                            on.x.row_src, on.z)
    assert worst <= 1e-6 and viol["C4"] <= 1e-6, viol
    assert abs(obj - on.objective) <= 1e-6 * max(1.0, abs(on.objective)), (obj, on.objective)
