"""GPU: the reduced costs of c and n a facility-relaxation LP's bound was computed with (API 13:
nep_lp_get_reduced_costs / nep_lp_rc_fixings, LPModel.reduced_costs / rc_fixings; DESIGN.md §7 "Reduced-cost fixing").

Instances synthetic_payload(16, 8, 0) and (24, 12, 0), MinDelayAndUtilization, solved as tests/test_gpu_fac.py solves
them (tol 5e-7, root cold, children warm from the root).  Children: n[j] = 0 for a node open at the root, n[j] = 1 for
a node closed at the root, one c = 1, two c = 0.

 1. validity against HiGHS (oracle.solve on facility_relaxation(build_model(...))): for the 6 largest |rc| among c, the
    4 largest among n and the 2 smallest overall, and each end t of the variable's box, the HiGHS value of the node LP
    with z_k = t is >= bound + rc_k t - min(rc_k lb_k, rc_k ub_k) - 2e-6 max(1, |value|) (infeasible: +inf);
    bound <= obj + 1e-12; for certified LPs bound >= obj - 2e-6 max(1, |obj|)
 2. not vacuous: per instance some picked variable has |rc| >= 1e-5
 3. rc_fixings == the numpy filter of the dense read-out, indices and values exactly, at four cutoffs; count-only
    with capacity 0
 4. the n[j] = 0 child emits no fixed variable
 5. a copied slot returns the same rc and bound
 6. a reference-relaxation model and an iterating slot are refused
 7. reading reduced costs changes no iterate: two cold root solves agree bit for bit
"""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
VARIANT = "MinDelayAndUtilization"
SIZES = [(16, 8), (24, 12)]
NCHILD = 4
SPARE = NCHILD + 1     # slot the tests copy into / submit on; the root is slot NCHILD


def _solve(m, slots, lb, ub, warm, chunk=25000, retries=7):
    """tests/test_gpu_fac.py's solve: LPs at the iteration limit continue from their own state"""
    from core.engine.lp import LP_ITERATION_LIMIT
    slots = np.asarray(slots)
    r = m.solve(slots, lb, ub, tol=5e-7, max_iters=chunk, warm_start=warm)
    for _ in range(retries):
        redo = np.flatnonzero(r["status"] == LP_ITERATION_LIMIT)
        if redo.size == 0:
            break
        rr = m.solve(slots[redo], None if lb is None else lb[redo], None if ub is None else ub[redo], tol=5e-7,
                     max_iters=chunk, warm_start=True)
        for k in ("status", "obj", "primal_obj"):
            r[k][redo] = rr[k]
        r["iters"][redo] += rr["iters"]
    return r


def _box(m, slot):
    """the node box of z_int as the engine holds it (nep_debug_state)"""
    from core.engine.lp import _check, _ptr
    lb, ub = np.zeros(m.n_int), np.zeros(m.n_int)
    _check(m._lib, m._lib.nep_debug_state(m._h, int(slot), None, None, None, _ptr(lb), _ptr(ub)), "nep_debug_state")
    return lb, ub


class _Case:
    pass


_CASES = {}


def _case(N, F):
    """One instance, solved once: the model (kept open for the module), the root and its children, their read-outs."""
    if (N, F) in _CASES:
        return _CASES[(N, F)]
    from core.engine.lp import LPModel, RELAX_FACILITY
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    from oracle.formulation import build_model, facility_relaxation
    from oracle.inputs import data_to_solver_input as oracle_input
    c = _Case()
    p = synthetic_payload(N, F, seed=0)
    c.N, c.F, c.alpha = N, F, p["solver"]["args"]["alpha"]
    c.data = data_to_solver_input(p, with_db=False)
    od = oracle_input(p, with_db=False)
    c.ref = facility_relaxation(build_model(od, VARIANT, step=1, alpha=c.alpha), od)
    c.nx = N * N * F
    c.m = m = LPModel(c.data, VARIANT, step=1, alpha=c.alpha, max_batch=NCHILD + 4, relaxation=RELAX_FACILITY)
    root = NCHILD
    rr = _solve(m, [root], None, None, False)
    z = m.solutions([root])[0]
    FN = F * N
    nroot = z[FN:FN + N]
    rng = np.random.default_rng(N + F)
    j_open, j_closed = int(np.argmax(nroot)), int(np.argmin(nroot))
    two = rng.choice(FN, size=2, replace=False).tolist()
    c.fix = [([FN + j_open], [0.0]), ([FN + j_closed], [1.0]), ([int(rng.integers(FN))], [1.0]), (two, [0.0, 0.0])]
    c.root_n = (float(nroot[j_open]), float(nroot[j_closed]))
    lb = np.full((NCHILD, m.n_int), -np.inf)
    ub = np.full((NCHILD, m.n_int), np.inf)
    for b, (idx, val) in enumerate(c.fix):
        lb[b, idx] = ub[b, idx] = val
        m.copy_state(root, b)
    res = _solve(m, np.arange(NCHILD), lb, ub, True)
    # LP 0 = the root, LP b + 1 = child b
    c.slots = [root] + list(range(NCHILD))
    c.status = [int(rr["status"][0])] + [int(s) for s in res["status"]]
    c.obj = [float(rr["obj"][0])] + [float(o) for o in res["obj"]]
    c.iters = [int(rr["iters"][0])] + [int(i) for i in res["iters"]]
    c.user_box = [(None, None)] + [(lb[b], ub[b]) for b in range(NCHILD)]
    c.rc, c.bound, c.box = {}, {}, {}
    from core.engine.lp import LP_INFEASIBLE
    for q, s in enumerate(c.slots):
        if c.status[q] == LP_INFEASIBLE:
            continue
        rc, bd = m.reduced_costs([s])
        c.rc[q], c.bound[q], c.box[q] = rc[0], float(bd[0]), _box(m, s)
    _CASES[(N, F)] = c
    return c


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for c in _CASES.values():
        c.m.close()
    _CASES.clear()


def _picks(c, q):
    """6 largest |rc| among c, 4 largest among n, 2 smallest overall"""
    FN, N = c.F * c.N, c.N
    a = np.abs(c.rc[q])
    pc = np.argsort(-a[:FN], kind="stable")[:6]
    pn = FN + np.argsort(-a[FN:FN + N], kind="stable")[:4]
    ps = np.argsort(a, kind="stable")[:2]
    return [int(k) for k in np.concatenate([pc, pn, ps])]


def _highs(c, q, k=None, t=None):
    """HiGHS value of LP q of the case (its node box), optionally with z_k = t; +inf when infeasible"""
    from oracle.solve import solve
    rl, ru = c.ref["lb"].copy(), c.ref["ub"].copy()
    ulb, uub = c.user_box[q]
    if ulb is not None:
        fin = np.isfinite(ulb)
        rl[c.nx:][fin] = ulb[fin]
        ru[c.nx:][fin] = uub[fin]
    if k is not None:
        rl[c.nx + k] = ru[c.nx + k] = t
    _, val, _ = solve(c.ref, relax=True, lb=rl, ub=ru)
    return math.inf if val is None else val


@pytest.mark.parametrize("q", range(NCHILD + 1))
@pytest.mark.parametrize("N,F", SIZES)
def test_reduced_costs_are_valid_against_highs(N, F, q):
    from core.engine.lp import LP_INFEASIBLE, LP_OPTIMAL
    c = _case(N, F)
    if c.status[q] == LP_INFEASIBLE:
        assert _highs(c, q) == math.inf, "the engine proved a feasible LP infeasible"
        return
    rc, bound, (lb, ub), obj = c.rc[q], c.bound[q], c.box[q], c.obj[q]
    print(f"{N}x{F} LP {q}: status {c.status[q]} obj {obj:.10g} bound {bound:.10g} after {c.iters[q]} iterations; "
          f"|rc| > 1e-6: {int((np.abs(rc) > 1e-6).sum())} of {rc.size}, max {np.abs(rc).max():.3e}")
    assert bound <= obj + 1e-12, (bound, obj)
    if c.status[q] == LP_OPTIMAL:
        assert bound >= obj - 2e-6 * max(1.0, abs(obj)), (bound, obj)
    node = _highs(c, q)
    assert bound <= node + 2e-6 * max(1.0, abs(node)), (bound, node)
    for k in _picks(c, q):
        for t in sorted({float(lb[k]), float(ub[k])}):
            need = bound + rc[k] * t - min(rc[k] * lb[k], rc[k] * ub[k])
            # fixing z_k can only raise HiGHS's value: where the node LP's own value already meets the inequality
            # (the end the reduced cost does not price, and every |rc| within the tolerance) the restricted LP does
            # too, without solving it (a 24x12 LP takes HiGHS ~2 s)
            if node >= need - 2e-6 * max(1.0, abs(node)):
                print(f"   k {k} rc {rc[k]:+.6e} box [{lb[k]:g}, {ub[k]:g}] t {t:g}: HiGHS >= {node:.10g} >= {need:.10g}")
                continue
            val = _highs(c, q, k, t)
            print(f"   k {k} rc {rc[k]:+.6e} box [{lb[k]:g}, {ub[k]:g}] t {t:g}: HiGHS {val:.10g} >= {need:.10g}")
            if val < math.inf:
                assert val >= need - 2e-6 * max(1.0, abs(val)), (k, t, val, need, rc[k])


@pytest.mark.parametrize("N,F", SIZES)
def test_reduced_costs_are_not_vacuous(N, F):
    """Some picked variable carries a reduced cost of at least 1e-5: at the root, else in a child with a fixed n."""
    c = _case(N, F)
    best = {q: max(abs(c.rc[q][k]) for k in _picks(c, q)) for q in c.rc}
    print(f"{N}x{F}: largest picked |rc| per LP {best}")
    if not (best.get(0, 0.0) >= 1e-5 or max(best.get(1, 0.0), best.get(2, 0.0)) >= 1e-5):
        for q in c.rc:
            print(f"LP {q} |rc|:", np.abs(c.rc[q]).tolist())
        pytest.fail(f"no picked reduced cost reaches 1e-5 at the root or in the children with a fixed n: {best}")


def _numpy_fixings(rc, bound, lb, ub, cutoff):
    with np.errstate(invalid="ignore"):
        keep = (lb < ub) & (rc != 0.0) & (bound + np.abs(rc) * (ub - lb) > cutoff)
    idx = np.flatnonzero(keep).astype(np.int32)
    return idx, np.where(rc[idx] > 0, lb[idx], ub[idx])


@pytest.mark.parametrize("N,F", SIZES)
def test_rc_fixings_equal_the_numpy_filter(N, F):
    from core.engine.lp import _ptr
    c = _case(N, F)
    m = c.m
    for q in c.rc:
        rc, bound, (lb, ub) = c.rc[q], c.bound[q], c.box[q]
        nz = np.abs(rc[rc != 0.0])
        cutoffs = [bound + 1e-4, bound + (float(np.median(nz)) if nz.size else 0.0), math.inf, bound - 1.0]
        for cut in cutoffs:
            idx, val = m.rc_fixings(c.slots[q], cut)
            widx, wval = _numpy_fixings(rc, bound, lb, ub, cut)
            print(f"{N}x{F} LP {q} cutoff {cut:.10g}: {len(idx)} fixings")
            assert np.array_equal(idx, widx), (q, cut)
            assert np.array_equal(val, wval), (q, cut)
            assert np.all(np.diff(idx) > 0)
            # capacity 0: the count only, the outputs untouched
            n = ctypes.c_int64(-1)
            oi, ov = np.full(max(1, len(widx)), -7, np.int32), np.full(max(1, len(widx)), -7.0)
            assert m._lib.nep_lp_rc_fixings(m._h, c.slots[q], float(cut), 0, ctypes.byref(n), _ptr(oi), _ptr(ov)) == 0
            assert n.value == len(widx) and np.all(oi == -7) and np.all(ov == -7.0)
        assert len(m.rc_fixings(c.slots[q], math.inf)[0]) == 0
        free_priced = np.flatnonzero((lb < ub) & (rc != 0.0))
        assert np.array_equal(m.rc_fixings(c.slots[q], bound - 1.0)[0], free_priced)


@pytest.mark.parametrize("N,F", SIZES)
def test_fixed_variables_are_never_emitted(N, F):
    """the n[j] = 0 child: its closed node's n and c (presolve closes them) have lb == ub and never appear"""
    c = _case(N, F)
    q = 1
    if q not in c.rc:
        pytest.fail(f"the n[j] = 0 child of {N}x{F} is infeasible: no reduced costs to test (root n {c.root_n})")
    lb, ub = c.box[q]
    fixed = np.flatnonzero(lb == ub)
    j = c.fix[0][0][0]
    assert j in fixed, (j, fixed)
    print(f"{N}x{F} n[j] = 0 child: {fixed.size} fixed variables in the engine's box")
    for cut in (c.bound[q] - 1.0, c.bound[q] + 1e-4, -math.inf):
        idx, _ = c.m.rc_fixings(c.slots[q], cut)
        assert np.intersect1d(idx, fixed).size == 0, (cut, np.intersect1d(idx, fixed))


@pytest.mark.parametrize("N,F", SIZES)
def test_copied_slot_keeps_reduced_costs(N, F):
    c = _case(N, F)
    m = c.m
    for q in list(c.rc)[:3]:
        m.copy_state(c.slots[q], SPARE)
        rc, bd = m.reduced_costs([SPARE, c.slots[q]])
        assert np.array_equal(rc[0], c.rc[q]) and np.array_equal(rc[1], c.rc[q])
        assert bd[0] == bd[1] == c.bound[q]
    m.copy_states([c.slots[0], c.slots[1]], [SPARE, SPARE + 1])
    rc, bd = m.reduced_costs([SPARE, SPARE + 1])
    assert np.array_equal(rc[0], c.rc[0]) and bd[0] == c.bound[0]
    if 1 in c.rc:
        assert np.array_equal(rc[1], c.rc[1]) and bd[1] == c.bound[1]


def test_refusals():
    from core.engine.lp import EngineUnavailable, LPModel
    c = _case(16, 8)
    ref = LPModel(c.data, VARIANT, step=1, alpha=c.alpha, max_batch=1)
    try:
        ref.solve([0], tol=1e-6, max_iters=64)
        for call in (lambda: ref.reduced_costs([0]), lambda: ref.rc_fixings(0, 0.0)):
            with pytest.raises(EngineUnavailable) as e:
                call()
            assert "(-1)" in str(e.value) and "facility-relaxation models only" in str(e.value), str(e.value)
    finally:
        ref.close()
    m = c.m
    # a slot that never held an LP: no check yet
    with pytest.raises(EngineUnavailable) as e:
        m.reduced_costs([SPARE + 2])
    assert "(-4)" in str(e.value) and "no certificate check yet" in str(e.value), str(e.value)
    # a bad slot, a NULL output
    with pytest.raises(EngineUnavailable) as e:
        m.reduced_costs([m.max_batch])
    assert "(-1)" in str(e.value)
    assert m._lib.nep_lp_rc_fixings(m._h, 0, 0.0, 0, None, None, None) == -1
    assert m._lib.nep_lp_get_reduced_costs(m._h, 1, None, None, None) == -1
    # a submitted, unfinished slot
    st = m.submit([SPARE + 2], tol=5e-7, max_iters=25000)
    assert m.active() == 1, st
    try:
        for call in (lambda: m.reduced_costs([SPARE + 2]), lambda: m.rc_fixings(SPARE + 2, 0.0)):
            with pytest.raises(EngineUnavailable) as e:
                call()
            assert "(-4)" in str(e.value) and "iterating" in str(e.value), str(e.value)
    finally:
        while m.active():
            m.advance(1)
    rc, bd = m.reduced_costs([SPARE + 2])
    assert np.isfinite(bd[0])


def test_reading_reduced_costs_leaves_the_iterates_alone():
    """two cold solves of the 16x8 root: one read its reduced costs (and fixings) when it finished, the other never"""
    from core.engine.lp import LPModel, RELAX_FACILITY
    c = _case(16, 8)
    out = []
    for read in (True, False):
        m = LPModel(c.data, VARIANT, step=1, alpha=c.alpha, max_batch=2, relaxation=RELAX_FACILITY)
        try:
            r = m.solve([0], tol=5e-7, max_iters=25000)
            if read:
                rc, bd = m.reduced_costs([0])
                m.rc_fixings(0, float(bd[0]) + 1e-4)
                if c.iters[0] < 25000:   # (the module's root, solved in one run like this one, agrees too)
                    assert np.array_equal(rc[0], c.rc[0]) and bd[0] == c.bound[0]
            z = m.solutions([0])[0]
            out.append((r["obj"].tobytes(), r["primal_obj"].tobytes(), r["iters"].tobytes(), z.tobytes()))
        finally:
            m.close()
    assert out[0] == out[1]
