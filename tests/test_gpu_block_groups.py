"""Slot groups of a block (nep_host.cpp launch_block / launch_span, NEP_BLOCK_GROUPS): a model created with
NEP_BLOCK_GROUPS=2 iterates the slots of a block as two groups on two streams wherever the split rule
(nep_kernels.hip block_split, tests/test_block_split.py) allows, and must give, bit for bit, what the single chain
(NEP_BLOCK_GROUPS=1, the reference here) gives: status, iterations, bound, primal objective, the routing rows, the
small primal and the duals of every slot.

Shapes: F = 4 functions and N = 24 (one chunk per lane) and 260 (two chunks per lane), 12 slots: with 4 functions
every launch runs 16 waves per workgroup, so every block of two or more slots splits (asserted through the rule's
host-only entry point).  Boxes: twelve node boxes that each close a third of every function's destinations
and one more, a different one per box, so the LPs differ and all iterate at tolerance 1e-12.  One step-2 model (its scalar pass runs every
iteration, in both groups), one facility-relaxation model, and F = 64 with 16 slots, where the halves would change the
tile from 4 to 8 waves and the rule has to refuse the split."""
import os

import numpy as np
import pytest

from gpu_cases import build_args, fixing_bounds
from test_gpu_xpass_elide import F, _bits, _state, _step2_case, instance, open_destinations

pytestmark = pytest.mark.gpu

SLOTS = 12
VARIANT = "MinDelayAndUtilization"


# N = 24: the boxes of this family that iterate (two of the first fourteen certify at their first check, as this
# generator's 24-node root LP does); every other shape here iterates all of them
BOX_IDS_24 = (1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13)


def boxes(N, n_int, count, nf=F):
    """count node boxes [count, n_int] (lb, ub): every function loses the destinations j = 2 (mod 3) and one more,
    j = (b + 5 f) mod N for box number b, except those the elision test's leaf box keeps open."""
    lb = np.full((count, n_int), -np.inf)
    ub = np.full((count, n_int), np.inf)
    keep = open_destinations(N)
    ids = BOX_IDS_24[:count] if (N, nf) == (24, F) else range(count)
    for k, b in enumerate(ids):
        for f in range(nf):
            for j in range(N):
                if (j % 3 == 2 or j == (b + 5 * f) % N) and j not in keep[f % len(keep)]:
                    ub[k, f * N + j] = 0.0
    return lb, ub


def _with_groups(flag, make):
    old = os.environ.get("NEP_BLOCK_GROUPS")
    os.environ["NEP_BLOCK_GROUPS"] = flag     # (read once, when the model is created)
    try:
        return make()
    finally:
        if old is None:
            del os.environ["NEP_BLOCK_GROUPS"]
        else:
            os.environ["NEP_BLOCK_GROUPS"] = old


def _drain(m, res, trace):
    """advance until nothing iterates; res: slot -> (status, iters, obj, primal_obj); trace: slots still iterating
    after each call."""
    while m.active():
        r = m.advance(1)
        for k, s in enumerate(r["slots"]):
            res[int(s)] = tuple(r[key][k] for key in ("status", "iters", "obj", "primal_obj"))
        trace.append(m.active())


def _collect(m, res, n_dual, extra=None):
    slots = sorted(res)
    out = {"res": {key: np.array([res[s][i] for s in slots])
                   for i, key in enumerate(("status", "iters", "obj", "primal_obj"))}, "slots": slots}
    for s in slots:
        out[s] = _state(m, s, n_dual)
    st = m.stats()
    out["stats"] = {k: st[k] for k in ("x_pass_launches", "x_pass_sampled", "x_pass_lp_iters", "lp_iterations")}
    out.update(extra or {})
    return out


def _assert_same(ref, got):
    assert ref["slots"] == got["slots"]
    for key in ("status", "iters", "obj", "primal_obj"):
        a, b = _bits(ref["res"][key]), _bits(got["res"][key])
        assert np.array_equal(a, b), (key, ref["res"][key], got["res"][key])
    for k, s in enumerate(ref["slots"]):
        if ref["res"]["iters"][k] == 0:      # (refused by presolve: the slot was never initialised)
            continue
        for key in ("x", "z", "y"):
            a, b = _bits(ref[s][key]), _bits(got[s][key])
            assert np.array_equal(a, b), (s, key, int((a != b).sum()))
    # iterations and LP-iterations are counted alike on both paths; a sampled launch covers every iterating slot
    assert ref["stats"] == got["stats"], (ref["stats"], got["stats"])


def _model(flag, N, relaxation=0, nf=F, max_batch=SLOTS, seed=None):
    from core.engine.lp import LPModel, debug_build
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    if nf == F:
        data, alpha = instance(N)
    else:
        p = synthetic_payload(N, nf, seed=seed, rho=0.4)
        data, alpha = data_to_solver_input(p, with_db=False), p["solver"]["args"]["alpha"]
    n_dual = debug_build(data, VARIANT, step=1, alpha=alpha, relaxation=relaxation)["n_dual"]
    m = _with_groups(flag, lambda: LPModel(data, VARIANT, step=1, alpha=alpha, max_batch=max_batch,
                                           relaxation=relaxation))
    return m, n_dual


def _splits(N, nf, na, relaxation=0):
    from core.engine.lp import debug_block_split
    return debug_block_split(N, nf, na, relaxation)[0]


def _both(run, *args):
    return run("1", *args), run("2", *args)


# ---------------------------------------------------------------------------------------------------------------
def _run_budgets(flag, N):
    """Per-LP budgets of 1 .. 12 blocks of 16 iterations: one LP leaves after every block, so the slots iterating
    walk 12, 11, ..., 1 — odd counts, and a single slot, which cannot split, while the blocks before it did."""
    m, n_dual = _model(flag, N)
    try:
        lb, ub = boxes(N, m.n_int, SLOTS)
        st = m.submit(np.arange(SLOTS), lb, ub, tol=1e-12, check_every=16, max_iters=16 * (1 + np.arange(SLOTS)))
        res, trace = {}, []
        _drain(m, res, trace)
        return _collect(m, res, n_dual, {"submit": st, "trace": trace})
    finally:
        m.close()


@pytest.mark.parametrize("N", (24, 260))
def test_per_lp_budgets_walk_the_slot_count_down(N):
    from core.engine.lp import LP_ITERATION_LIMIT
    ref, got = _both(_run_budgets, N)
    print("iters", ref["res"]["iters"], "status", ref["res"]["status"], "iterating after each call", ref["trace"])
    assert (ref["submit"] == LP_ITERATION_LIMIT).all() and np.array_equal(ref["submit"], got["submit"])
    assert ref["trace"] == got["trace"]
    # every count from 12 down to 1 iterated a block of its own: both parities and the unsplit single slot
    assert len(set(ref["res"]["iters"].tolist())) == SLOTS and set(ref["trace"]) >= set(range(1, SLOTS - 1))
    assert all(_splits(N, F, na) == (na + 1) // 2 for na in range(2, SLOTS + 1)) and _splits(N, F, 1) == 0
    _assert_same(ref, got)


# ---------------------------------------------------------------------------------------------------------------
def _run_refill(flag, N):
    """Ten LPs, the first with a budget of one block: advance(1) returns with the next block of the other nine
    already in flight; two more boxes are submitted behind it and join at the block after."""
    m, n_dual = _model(flag, N)
    try:
        lb, ub = boxes(N, m.n_int, SLOTS)
        budget = np.full(10, 240)
        budget[0] = 16
        m.submit(np.arange(10), lb[:10], ub[:10], tol=1e-12, check_every=16, max_iters=budget)
        res, trace = {}, []
        r = m.advance(1)
        for k, s in enumerate(r["slots"]):
            res[int(s)] = tuple(r[key][k] for key in ("status", "iters", "obj", "primal_obj"))
        inflight = m.active()
        st = m.submit([10, 11], lb[10:], ub[10:], tol=1e-12, check_every=16, max_iters=np.array([112, 240]))
        _drain(m, res, trace)
        return _collect(m, res, n_dual, {"first": r["slots"].tolist(), "inflight": inflight, "submit": st})
    finally:
        m.close()


@pytest.mark.parametrize("N", (24, 260))
def test_refill_behind_the_block_in_flight(N):
    from core.engine.lp import LP_ITERATION_LIMIT
    ref, got = _both(_run_refill, N)
    print("first call", ref["first"], "in flight", ref["inflight"], "iters", ref["res"]["iters"])
    assert ref["first"] == got["first"] == [0] and ref["inflight"] == got["inflight"] == 9
    assert (ref["submit"] == LP_ITERATION_LIMIT).all() and ref["slots"] == list(range(SLOTS))
    _assert_same(ref, got)


# ---------------------------------------------------------------------------------------------------------------
def _run_batch(flag, N, check_every, max_iters, relaxation=0):
    m, n_dual = _model(flag, N, relaxation)
    try:
        lb, ub = boxes(N, m.n_int, SLOTS)
        r = m.solve(np.arange(SLOTS), lb, ub, tol=1e-12, check_every=check_every, max_iters=max_iters)
        res = {s: tuple(r[key][s] for key in ("status", "iters", "obj", "primal_obj")) for s in range(SLOTS)}
        return _collect(m, res, n_dual)
    finally:
        m.close()


@pytest.mark.parametrize("N", (24, 260))
def test_sampled_eager_blocks_and_stats(N):
    """check_every = 48 and 288 iterations: six blocks, of which the first and the fifth run eagerly with the sampled
    full-width launch between a join and a fork; the sampled launches cover all twelve slots in both modes."""
    ref, got = _both(_run_batch, N, 48, 288)
    print("iters", ref["res"]["iters"], "stats", ref["stats"], got["stats"])
    assert (ref["res"]["iters"] == ref["res"]["iters"][0]).all() and ref["res"]["iters"][0] >= 5 * 48
    for r in (ref, got):
        st = r["stats"]
        assert st["x_pass_sampled"] >= 2 and st["x_pass_lp_iters"] == st["x_pass_sampled"] * SLOTS
        assert st["lp_iterations"] == st["x_pass_launches"] * SLOTS
    _assert_same(ref, got)


@pytest.mark.parametrize("N", (24, 260))
def test_short_blocks(N):
    """check_every = 3: every iteration plain (no Halpern step), no sampled launch, certificate every third."""
    ref, got = _both(_run_batch, N, 3, 60)
    print("iters", ref["res"]["iters"], "stats", ref["stats"])
    assert ref["res"]["iters"].min() >= 60 and ref["stats"]["x_pass_sampled"] == 0
    _assert_same(ref, got)


def test_facility_relaxation_model():
    from core.engine.lp import RELAX_FACILITY
    ref, got = _both(_run_batch, 24, 48, 288, RELAX_FACILITY)
    print("iters", ref["res"]["iters"], "status", ref["res"]["status"])
    assert ref["res"]["iters"].max() >= 96
    assert _splits(24, F, SLOTS, RELAX_FACILITY) == SLOTS // 2
    _assert_same(ref, got)


# ---------------------------------------------------------------------------------------------------------------
def _run_step2(flag):
    from core.engine.lp import LPModel, debug_build
    name, k = _step2_case()
    data, variant, step, kw = build_args(name, k)
    n_dual = debug_build(data, variant, step=step, **kw)["n_dual"]
    N, Fn = len(data.nodes), len(data.functions)
    m = _with_groups(flag, lambda: LPModel(data, variant, step=step, max_batch=8, **kw))
    try:
        nodes = fixing_bounds(name, k, m.n_int, N * N * Fn)[:7]
        B = 1 + len(nodes)
        lb = np.full((B, m.n_int), -np.inf)
        ub = np.full((B, m.n_int), np.inf)
        for b, (l, u, _) in enumerate(nodes):
            lb[b + 1], ub[b + 1] = l, u
        r = m.solve(np.arange(B), lb, ub, tol=1e-12, check_every=48, max_iters=200)
        res = {s: tuple(r[key][s] for key in ("status", "iters", "obj", "primal_obj")) for s in range(B)}
        return _collect(m, res, n_dual, {"shape": (N, Fn, step)})
    finally:
        m.close()


def test_step2_model():
    ref, got = _both(_run_step2)
    N, Fn, step = ref["shape"]
    print(_step2_case(), ref["shape"], "iters", ref["res"]["iters"], "status", ref["res"]["status"])
    assert step >= 2 and ref["res"]["iters"].max() >= 96
    na = int((ref["res"]["iters"] >= 96).sum())      # the LPs that iterated blocks side by side
    assert na >= 2 and _splits(N, Fn, na) == (na + 1) // 2
    _assert_same(ref, got)


# ---------------------------------------------------------------------------------------------------------------
def _run_tile_change(flag):
    """F = 64, N = 24, 16 slots: 4 waves per workgroup, 8 for either half — the block stays whole."""
    m, n_dual = _model(flag, 24, nf=64, max_batch=16, seed=5)
    try:
        lb, ub = boxes(24, m.n_int, 16, nf=64)
        r = m.solve(np.arange(16), lb, ub, tol=1e-12, check_every=48, max_iters=100)
        res = {s: tuple(r[key][s] for key in ("status", "iters", "obj", "primal_obj")) for s in range(16)}
        return _collect(m, res, n_dual)
    finally:
        m.close()


def test_tile_change_keeps_the_block_whole():
    from core.engine.lp import LP_INFEASIBLE, debug_block_split
    assert debug_block_split(24, 64, 16) == (0, 4, 4) and debug_block_split(24, 64, 8)[1:] == (8, 8)
    ref, got = _both(_run_tile_change)
    print("iters", ref["res"]["iters"], "status", ref["res"]["status"])
    assert (ref["res"]["status"] != LP_INFEASIBLE).all() and ref["res"]["iters"].min() >= 96
    _assert_same(ref, got)
