"""GPU: reduced-cost fixing in the product's step-1 search (BranchAndBound(rc_fixing=True): native tree, facility-relaxation
branching nodes, reference-model leaves; DESIGN.md §7 "Reduced-cost fixing").  synthetic_payload(48, 24, seed 0),
MinDelayAndUtilization step 1, 2000 nodes, pseudo-cost branching (rule 1), once with fixing off and once with it on:

  * both final bounds are <= 0.1331127 (1 + 1e-6) — HiGHS's proven optimum of this instance (DESIGN.md §7 "Closing the
    search"): a bound above it would be an invalid fixing;
  * the incumbent with fixing is <= the other's + 1e-9, or both are the optimum (within 1e-6, the suite's parity bar);
  * the tree asked for fixings and used some (rc_calls > 0, rc_fixed > 0);
  * the incumbent meets every reference row (scale_util.check_step1_solution) at its reported objective."""
import numpy as np
import pytest

from scale_util import check_step1_solution

pytestmark = pytest.mark.gpu
HIGHS_OPT = 0.1331127


def _dense_rows(x):
    xb = np.zeros((len(x.row_f), x.N))
    xb[x.row, x.dst] = x.val
    return xb


def _search(data, alpha, rc_fixing):
    from core.engine.lp import LPModel
    from core.solvers.neptune.neptune_step import NeptuneStep1CPUMinDelayAndUtilization
    batch = 32
    st1 = NeptuneStep1CPUMinDelayAndUtilization(alpha=alpha, verbose=False, batch=batch, lp_tol=1e-6, lp_max_iters=4096)
    st1.load_data(data)
    m = LPModel(data, "MinDelayAndUtilization", step=1, alpha=alpha, max_batch=batch + 2)
    bm = st1.bound_model(data, batch + 1)
    try:
        return st1.branch_and_bound(m, bm, time_limit=120.0, root_max_iters=400000, gap=1e-4, branching=1,
                                    node_limit=2000, rc_fixing=rc_fixing).solve()
    finally:
        m.close()
        bm.close()


def test_rc_fixing_in_the_48x24_search():
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    p = synthetic_payload(48, 24, seed=0)
    alpha = p["solver"]["args"]["alpha"]
    data = data_to_solver_input(p, with_db=False)
    off = _search(data, alpha, False)
    on = _search(data, alpha, True)
    for tag, r in (("off", off), ("on", on)):
        print(f"rc_fixing {tag}: status {r.status} incumbent {r.objective} bound {r.bound} nodes {r.nodes} leaves "
              f"{r.leaves} lps {r.lps} rc {r.rc} seconds {r.seconds:.2f}")
    assert off.native and on.native
    assert off.rc == {"rc_fixed": 0, "rc_calls": 0, "rc_children_pruned": 0, "rc_leaves_dropped": 0}
    for r in (off, on):
        assert r.objective is not None
        assert r.bound <= HIGHS_OPT * (1 + 1e-6), r.bound
    both_optimal = all(abs(r.objective - HIGHS_OPT) <= 1e-6 for r in (off, on))
    assert on.objective <= off.objective + 1e-9 or both_optimal, (on.objective, off.objective)
    assert on.rc["rc_calls"] > 0 and on.rc["rc_fixed"] > 0, on.rc
    viol, worst, obj = check_step1_solution(data, "MinDelayAndUtilization", alpha, _dense_rows(on.x), on.x.row_f,
                                            on.x.row_src, on.z)
    assert worst <= 1e-6 and viol["C4"] <= 1e-6, viol
    assert abs(obj - on.objective) <= 1e-6 * max(1.0, abs(on.objective)), (obj, on.objective)
