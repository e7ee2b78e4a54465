"""Chunk elision of the steady-state x pass (nep_kernels.hip "Chunk elision", NEP_XPASS_ELIDE): a model created with
NEP_XPASS_ELIDE=1 skips the memory traffic of 16-byte chunks of a routing row whose four destinations are all closed
and must give, bit for bit, what the full-width pass (NEP_XPASS_ELIDE=0, the reference here) gives: the routing
rows, the small primal, the duals, status, iterations, bound and primal objective.

Shapes: F = 4 functions and N = 24 (one chunk per lane, 6 lanes own one), 256 (one chunk per lane, all lanes),
260 (two chunks per lane, the second on one lane only) and 512.  Boxes: no fixing (full masks); a leaf-type box
(every c and n fixed) with 1-3 open destinations per function — a single one which is also the last, j = N - 1; two
inside one chunk; one on each side of the middle (j = 255 | 256 from N = 260 on); three spread out — started cold,
and the same box warm-started from the full-mask LP's final state, whose routing sits under the newly closed
destinations: there x must be exactly +0 after the run on both paths (the invariant the elision rests on).
One step-2 model (the smallest recorded one with more than one node) runs its root and recorded node boxes on both
paths.

Budget: 200 iterations checked every 48 at tolerance 1e-12: an LP that iterates runs its INIT pass, five certificate
passes, the FIRST pass behind each (the first one always carries a restart) and ~230 steady-state passes, 241
iterations in all (asserted: at least 96).  The 24-node root LP certifies at its first check; its leaf boxes iterate."""
import os

import numpy as np
import pytest

from gpu_cases import build_args, fixing_bounds, lp_cases

pytestmark = pytest.mark.gpu

F = 4
SHAPES = (24, 256, 260, 512)
RUN = dict(tol=1e-12, max_iters=200, check_every=48)
FULL, LEAF, WARM = 0, 1, 2      # slots


def open_destinations(N):
    """Open destinations of the leaf box, per function."""
    mid = min(255, N // 2 - 1)
    return [[N - 1],                    # a single one, the last destination
            [8, 9],                     # two inside one 16-byte chunk
            [mid, mid + 1],             # either side of the middle (j = 256 starts the second chunk of a lane)
            [0, N // 3, N - 1]]


def leaf_box(N, n_int, has_n=True):
    lb = np.zeros(n_int)
    ub = np.zeros(n_int)
    for f, js in enumerate(open_destinations(N)):
        for j in js:
            lb[f * N + j] = ub[f * N + j] = 1.0
            if has_n:
                lb[F * N + j] = ub[F * N + j] = 1.0
    return lb, ub


def instance(N):
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    # (workload densities at which the host presolve finds the leaf box feasible, with 11 to 31 routing rows per
    # function: at most 16 waves share them, so some waves take a second row)
    # (N = 24: the seed whose leaf box iterates; this generator's 24-node root LPs certify at their first check)
    p = synthetic_payload(N, F, seed=5 if N == 24 else 3, rho={24: 0.4, 512: 0.05}.get(N, 0.1))
    return data_to_solver_input(p, with_db=False), p["solver"]["args"]["alpha"]


def _state(m, slot, n_dual):
    x, rf, _ = m.rows(slot)
    z, _ = m.solution(slot, dense_x=False)
    st = m.debug_state(slot, n_dual)
    return {"x": x, "rf": rf, "z": z, "y": st["y"], "ub": st["ub"]}


def _with_elide(flag, make):
    old = os.environ.get("NEP_XPASS_ELIDE")
    os.environ["NEP_XPASS_ELIDE"] = flag     # (read once, when the model is created)
    try:
        return make()
    finally:
        if old is None:
            del os.environ["NEP_XPASS_ELIDE"]
        else:
            os.environ["NEP_XPASS_ELIDE"] = old


def _run_step1(N, flag):
    from core.engine.lp import LPModel, debug_build, LP_INFEASIBLE
    data, alpha = instance(N)
    n_dual = debug_build(data, "MinDelayAndUtilization", step=1, alpha=alpha)["n_dual"]
    m = _with_elide(flag, lambda: LPModel(data, "MinDelayAndUtilization", step=1, alpha=alpha, max_batch=3))
    try:
        llb, lub = leaf_box(N, m.n_int)
        lb = np.stack([np.full(m.n_int, -np.inf), llb])
        ub = np.stack([np.full(m.n_int, np.inf), lub])
        res = m.solve([FULL, LEAF], lb, ub, **RUN)
        assert (res["status"] != LP_INFEASIBLE).all(), res
        m.copy_state(FULL, WARM)       # full masks: stale routing under the destinations the leaf box closes
        stale = m.rows(WARM)[0]
        resw = m.solve([WARM], llb[None], lub[None], warm_start=True, **RUN)
        assert (resw["status"] != LP_INFEASIBLE).all(), resw
        out = {"res": {k: np.concatenate([res[k], resw[k]]) for k in res}, "stale": stale}
        for s in (FULL, LEAF, WARM):
            out[s] = _state(m, s, n_dual)
        return out
    finally:
        m.close()


@pytest.fixture(scope="module")
def runs():
    """N -> (full-width reference, elided), computed once per shape."""
    cache = {}

    def get(N):
        if N not in cache:
            cache[N] = (_run_step1(N, "0"), _run_step1(N, "1"))
        return cache[N]
    return get


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _assert_same(ref, got, slot):
    for k in ("x", "z", "y"):
        a, b = _bits(ref[slot][k]), _bits(got[slot][k])
        assert np.array_equal(a, b), (slot, k, int((a != b).sum()))
    for k in ("status", "iters", "obj", "primal_obj"):
        assert np.array_equal(_bits(ref["res"][k][slot:slot + 1]), _bits(got["res"][k][slot:slot + 1])), \
            (slot, k, ref["res"][k][slot], got["res"][k][slot])


def _closed(st, N):
    """[R, N] bool: destination j closed for the function of row r (c's upper bound 0 in the slot's node box)."""
    return (st["ub"][:F * N].reshape(F, N) <= 0.0)[st["rf"]]


@pytest.mark.parametrize("N", SHAPES)
def test_full_masks(runs, N):
    ref, got = runs(N)
    print("iters", ref["res"]["iters"], got["res"]["iters"], "status", ref["res"]["status"])
    if N > 24:   # (a certificate pass, a FIRST pass and steady-state passes ran; see instance() for N = 24)
        assert ref["res"]["iters"][FULL] >= 96
    _assert_same(ref, got, FULL)


@pytest.mark.parametrize("N", SHAPES)
def test_leaf_box_cold(runs, N):
    ref, got = runs(N)
    closed = _closed(got[LEAF], N)
    nopen = (~closed).sum(1)
    print("open destinations per row", np.unique(nopen), "iters", ref["res"]["iters"])
    assert nopen.min() >= 1 and nopen.max() <= 3 and closed.mean() > 0.5
    assert ref["res"]["iters"][LEAF] >= 96
    _assert_same(ref, got, LEAF)
    for r in (ref, got):
        assert np.array_equal(_bits(r[LEAF]["x"][closed]), np.zeros(int(closed.sum()), np.uint32))


@pytest.mark.parametrize("N", SHAPES)
def test_leaf_box_warm_from_full_masks(runs, N):
    ref, got = runs(N)
    closed = _closed(got[WARM], N)
    # the warm start did copy routing under destinations this box closes
    stale = int((got["stale"][closed] != 0).sum())
    print("stale nonzeros under closed destinations", stale, "iters", ref["res"]["iters"])
    assert stale > 0
    assert ref["res"]["iters"][WARM] >= 96
    _assert_same(ref, got, WARM)
    for r in (ref, got):   # exactly +0 (all bits clear) at every closed destination
        assert np.array_equal(_bits(r[WARM]["x"][closed]), np.zeros(int(closed.sum()), np.uint32))


def _step2_case():
    import gpu_cases
    # (the smallest recorded step-2 model with more than one node: the single-node ones certify at their first check)
    cases = [(gpu_cases.G[name]["models"][k]["n_vars"], name, k) for name, k in lp_cases()
             if k >= 1 and name.startswith("syn_")]
    return min(cases)[1:]


def _run_step2(flag):
    from core.engine.lp import LPModel, debug_build
    name, k = _step2_case()
    data, variant, step, kw = build_args(name, k)
    n_dual = debug_build(data, variant, step=step, **kw)["n_dual"]
    N, Fn = len(data.nodes), len(data.functions)
    nodes = None
    m = _with_elide(flag, lambda: LPModel(data, variant, step=step, max_batch=8, **kw))
    try:
        nodes = fixing_bounds(name, k, m.n_int, N * N * Fn)[:7]
        B = 1 + len(nodes)
        lb = np.full((B, m.n_int), -np.inf)
        ub = np.full((B, m.n_int), np.inf)
        for b, (l, u, _) in enumerate(nodes):
            lb[b + 1], ub[b + 1] = l, u
        res = m.solve(np.arange(B), lb, ub, **RUN)
        out = {"res": res}
        for s in range(B):
            out[s] = _state(m, s, n_dual)
        return out, B
    finally:
        m.close()


def test_step2_model():
    (ref, B), (got, _) = _run_step2("0"), _run_step2("1")
    print(_step2_case(), "boxes", B, "iters", ref["res"]["iters"], "status", ref["res"]["status"])
    assert step2_is_step2()
    assert ref["res"]["iters"].max() >= 96
    for s in range(B):
        _assert_same(ref, got, s)


def step2_is_step2():
    name, k = _step2_case()
    return build_args(name, k)[2] >= 2
