"""The LP kernels (x_pass, node_pass, scalar_pass) against the fp64 numpy mirror (ref_pdhg.blocks), iterate by
iterate: the routing rows x, the small primal z and the duals y of an LP stopped at its certificate iterations
k = 1, 17, 33, 49, 65 (check_every = 16), and the certificate's objective, bound and residual there.

How a state is read.  nep_lp_get_rows / nep_lp_get_solution refuse an iterating slot, and nep_lp_advance enqueues
the next block before it returns, so a block boundary cannot be read in passing.  Instead every snapshot is its own
cold run with max_iters = k: the LP stops inside scalar_pass of the certificate iteration that brings its count to k,
its state is the plain PDHG step of that iteration, and the remaining launches of the block leave it alone.  Every
slot of a run has the same budget, so all of them iterate side by side until the last block (asserted: no slot ends
earlier, all end with LP_ITERATION_LIMIT at k) and the tile size never changes under a run.  One run of k = 65 is an
INIT pass, 5 certificate passes, 4 FIRST passes (the first three carry a restart, the fourth does not: asserted
from the mirror) and 56 steady passes; the model's blocks alternate between eager launches and the captured graph.

The mirror is made the same algorithm first (ref_pdhg.blocks): the engine's step size and initial weight
(diag eta / omega after the submit), the engine's presolved node box (nep_debug_presolve), the engine's restart
factor 0.9 (nep_host.cpp; the mirror's own default is PDLP's 0.8 — every decision here is the same under both), and
the engine's certificate (ref_pdhg.engine_certificate: repaired point, better of the plain and the repaired bound).
Asserted from the mirror alone, per run: no column deficit c_target - eps - S in (0, 2e-3] at any compared
certificate (the mirror has no pooled / loaded shift); every restart decision unchanged when fpr, prev_fpr and
last_fpr move by a relative 1e-3 either way; y1 + y2 and y5 nonzero, over the snapshots, at a destination of every
256-destination chunk index the width has, and in the last chunk (leaf box: among its open destinations); rows of
support 1, 2..16 and > 16 all occur over the two boxes of a shape; the engine's presolve finds every box feasible.

Tolerance: from the mirror, never from the kernels.  d = largest difference between the fp32-emulating mirror
(blocks(fp32=True): x, its anchor, x̂, the packed duals, tau, lambda and the plain iterations' column / CPU sums
rounded to float32) and the fp64 mirror (8 d: summation orders numpy does not reproduce).  x and the certificate's
three scalars: within max(8 d, 64 * 2^-24 * max(1, |value|)) of the fp64 mirror, d per array and snapshot.  z and y:
block by block (iter_cases.blocks_of: c, n; y1, y2, y3, y5, y6, y7; step 2 also the row sum's and the score row's
duals and the idle disruption rows) within max(8 d_B, 64 * 2^-24 * s_B), d_B and s_B = largest |value| taken over the
block — the duals here are small (the objective is normalised: |y5| <= 1e-3, |y6| <= 1e-8), so a bound with an
absolute floor of 4e-6 could not fail on them — and never looser than the bound of the whole array that stood here
before; a block the mirror holds at exactly 0 must be exactly 0 on the device.  test_iter_sensitivity.py (CPU) shows
from the mirror alone that a 1 % error in any other block fails this somewhere.  iter_cases.ABS_FLOOR_BLOCKS: blocks kept
at the whole array's bound, with the numbers and the reason (y1).  Exact checks: slots holding the same box in one launch are bit-identical in x, z, y; x is +0
(all bits clear) at every closed destination.

Cases (iter_cases.matrix): F = 4, MinDelayAndUtilization; N = 26, 258, 514, 1026 (one chunk past a lane boundary
plus padding; CPL 1, 2, 4, 8) with 1 slot (root box, and the leaf box alone), 128 and 256 slots (alternating root /
leaf; the first two and last two slots are compared); N = 254, 510, 1022 and the largest admitted N at 256 slots;
one step-2 (delete, reduced disruption block) model at N = 258, two slots.  x_pass variants run: every (CPL, TW,
kind) the launchers can dispatch (test_abi.py test_iterate_matrix_reaches_every_dispatchable_variant lists them;
not dispatchable, hence not run: CPL 8 at TW 16, certificate passes at TW 16 beyond NP = 496 and at TW 8 beyond
NP = 876, i.e. CPL 4 / CHECK / TW 16 and CPL 8 / CHECK / TW 8 and 16).
iter_cases.matrix_tight: the tight instance (function memories 16, 15, 14, 13; memory 14.5 on function 2's own node of
every chunk index and on the last node) with a third box, "n-up": the root box with n = 1 forced on those nodes.  C7
is violated at c = 0, so y7 moves from k = 1 (0.2 .. 3); the c there rise to ~0.25 each, past the node's memory, and y3
moves from k = 17 on (0.004 .. 0.13): asserted from the mirror, at a chosen node of every chunk index.  The n-up box
alone at the four widths, and 256 slots cycling root / leaf / n-up at N = 258 and 1026 (first and last three slots
compared).  The tight leaf box forces only the smallest function on the last node: with all four the box is
infeasible and the presolve says so.  (Memory 16 there moves y3 at N = 26 and 258 only, and only at k = 33: at the
wider instances the c peak at 15.6 .. 15.8 of memory.)
iter_cases.matrix_wide: F = 67 at N = 26, root and leaf: node_pass sums two functions per lane with one short lane,
scalar_pass strides twice over its F and F + JB partials.
Warm starts (test_warm_started_children_match_mirror, N = 26 .. 1026): a cold root LP of the tight instance stopped
at k = 33, nep_lp_copy_state into two slots, a warm submit of a leaf-box child (the parent routes under destinations it
closes) and an n-up child with the default weight band, compared at k = 1 .. 65 of the children with the mirror
started from its own parent record (ref_pdhg.blocks start=): x projected onto the child's mask, z clipped, y kept,
anchors and bookkeeping afresh, omega the parent's (asserted on diag after the submit) and at least twice it from
the first restart on.  The n-up child at N = 26 is compared at k <= 33 only: its certificate at k = 49 has a column
deficit the pooled / loaded shift serves.

Not covered: the padding columns j >= N of x are not readable through the C ABI (only their effect on the sums
is); the pooled / loaded shift (excluded by precondition), dual polishing, the full (unreduced) step-2 block, the
weight band's cap (lineages of 1024 iterations) and n as a free variable away from 0 (its cost keeps it at exactly
0 in the root boxes and within 4e-6 of it in the leaf boxes of these short runs) are not mirrored or not reached;
the facility kernels have their own mirror and file (ref_fac.py, test_gpu_fac_iterates.py).

Measured on an MI355X, over all 32 runs (each test prints its own table with -s: d_B, s_B, kernel = |kernel - fp64
mirror| and the bound, per block, slot and snapshot).  Largest over snapshots and slots [d_B, s_B, kernel], and the
largest kernel / bound of the block:
  c    [1.9e-07, 1.0,     1.7e-07]  0.18      y1   [4.0e-13, 1.2e-05, 4.2e-13]  (whole array's bound: ABS_FLOOR_BLOCKS)
  n    [8.9e-11, 1.0,     1.9e-10]  0.84      y2   [8.2e-11, 5.5e-04, 2.4e-10]  0.90
  y3   [1.3e-04, 4.2,     1.2e-04]  0.61      y5   [1.1e-08, 2.6e-03, 1.0e-08]  0.87
  y6   [1.0e-14, 2.1e-08, 3.1e-14]  0.88      y7   [2.4e-03, 1.2e+02, 2.2e-03]  0.61
  step 2: yS [1.5e-12, 1.1e-04, 3.6e-13] 0.01; the row sum's dual and the idle disruption rows exactly 0.
x [7.3e-04, 1.0, 6.9e-04], pobj 1.8e-07, lagr 2.3e-03, pres 6.6e-05: all largest in the warm n-up child at N = 258,
whose weight jumps 250x at its first restart (the kernel follows the fp32 emulation there: 1.50e-4 against 1.59e-4
off the fp64 mirror on the same entry at k = 17); the cold runs stay at x <= 5.7e-5 as before.  The closest calls
(0.84 .. 0.90 of the bound) are n, y2, y5, y6 at single snapshots of a leaf box where 8 d_B binds and the kernel
sits at 6 .. 7 d_B.  y1 missed its own bound at three snapshots of the widest instances (numbers and reason in
iter_cases.ABS_FLOOR_BLOCKS) and keeps the whole array's bound.
What the emulation had to learn, as at N = 254 before (a first emulation rounded only the result of the shifted
point and gave d = 9.9e-8 for x at N = 254, leaf box, k = 17, where the kernel is 3.9e-6 off on a two-entry row: the
terms of tau g there are ~10^2 and cancel, so they are evaluated in float32 one by one as x_pass does): the plain
iterations' threshold is now summed and divided in float32 (ref_pdhg._theta32) and their column sums are added row
by row in float32 (RefModel.colsum32).  With the memory of the n-up nodes at exactly function 2's (14) the tight
leaf box puts C3 on its bound, where the mirror's y3 is exactly 0 and the kernel's fused multiply-add leaves 3e-18:
the instance avoids the tie (14.5).
"""
import concurrent.futures as cf

import numpy as np
import pytest

import iter_cases as ic

pytestmark = pytest.mark.gpu
FLOOR = ic.FLOOR
RUN = dict(tol=1e-12, check_every=ic.CHECK_EVERY, polish_after=-1.0)
ABS_FLOOR_BLOCKS = ic.ABS_FLOOR_BLOCKS


def _id(run):
    N, step, ns, box, tight, nf = ic.normalise(run)
    return (f"N{N}-step{step}-slots{ns}" + ("" if box is None else f"-box{box}") +
            ("-tight" if tight else "") + ("" if nf == ic.F else f"-F{nf}"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


_MODELS = {}


def _ref_model(N, step, tight=False, nf=ic.F):
    """(instance, its mirror model), built once per shape."""
    from ref_pdhg import RefModel
    key = (N, step, tight, nf)
    if key not in _MODELS:
        data = ic.instance(N, step, tight=tight, n_functions=nf)
        _MODELS[key] = (data, RefModel(data, ic.VARIANT, step=step, **ic.model_kw(step)))
    return _MODELS[key]


_MIRROR = {}


def mirror(N, step, eta, omega, tight=False, nf=ic.F, need=(0, 1)):
    """(fp64 records, fp32-emulation records) per box in `need`, at the engine's eta / omega: computed once per
    instance and box."""
    from core.engine.lp import debug_presolve
    from ref_pdhg import RefModel, blocks
    key = (N, step, tight, nf)
    data, m0 = _ref_model(*key)
    if key not in _MIRROR:
        lb, ub = ic.boxes(N, m0.n_int, step, nf, tight=tight)
        okf, okn, bf, _ = debug_presolve(data, ic.VARIANT, lb, ub, step=step, **ic.model_kw(step))
        _MIRROR[key] = {"eta": (eta, omega), "box": bf, "ok": okf & okn, "m": m0, "recs": {}, "sup": set()}
    out = _MIRROR[key]
    assert out["eta"] == (eta, omega)                   # (one model per shape: the same step for every run)
    todo = [b for b in need if (b, False) not in out["recs"]]
    assert out["ok"][list(need)].all(), (key, out["ok"])    # the engine's presolve finds every compared box feasible
    bf = out["box"]

    def one(box, fp32):
        m = RefModel(data, ic.VARIANT, step=step, **ic.model_kw(step)) if step != 1 else m0   # (dred writes m.lo / hi)
        return [r for r in blocks(m, box=(bf[box, 0], bf[box, 1]), tol=1e-12, max_iters=ic.SNAPSHOTS[-1],
                                  check_every=ic.CHECK_EVERY, eta=eta, omega0=omega, rs_nec=0.9, fp32=fp32,
                                  engine=True)]
    if todo:
        with cf.ThreadPoolExecutor(4) as ex:
            futs = {(b, fp): ex.submit(one, b, fp) for b in todo for fp in (False, True)}
            out["recs"].update({k: f.result() for k, f in futs.items()})
        try:
            for b in todo:
                _preconditions(N, step, out, b, tight, nf)
        except AssertionError:                          # (a later run of this shape must not find these records)
            for b in todo:
                out["recs"].pop((b, False)), out["recs"].pop((b, True))
            raise
        if step == 1 and not tight and nf == ic.F and {0, 1} <= {b for b, _ in out["recs"]}:
            assert out["sup"] == {"1", "2-16", ">16"}, (N, out["sup"])   # row supports, over the two boxes of a shape
    return out


def _restart(fpr, last, prev, k_since, k, nec):
    return fpr <= 0.2 * last or (fpr <= nec * last and fpr > prev) or k_since >= 0.36 * k


def _robust(N, box, recs):
    """No column deficit the pooled / loaded shift would serve; every restart decision holds when its operands move
    by a relative 1e-3 either way."""
    for r in recs:
        dfc = r["cert"]["deficit"]
        assert not ((dfc > 0) & (dfc <= 2e-3)).any(), (N, box, r["k"])
        if r["status"] is None:
            for nec in (0.8, 0.9):
                for s in (-1e-3, 1e-3):
                    for t in (-1e-3, 1e-3):
                        for u in (-1e-3, 1e-3):
                            assert _restart(r["fpr"] * (1 + s), r["last_fpr"] * (1 + t), r["prev_fpr"] * (1 + u),
                                            r["k_since"], r["k"], nec) == r["restart"], (N, box, r["k"])
            assert abs(r["k_since"] - 0.36 * r["k"]) > 1e-3 * 0.36 * r["k"]
            for v in (r["dz"], r["dy"]):
                assert abs(v - 1e-10) > 1e-3 * 1e-10


def _preconditions(N, step, mir, box, tight, nf):
    m = mir["m"]
    FN = nf * N
    nq = (ic.padded(N) + 255) // 256
    recs = mir["recs"][box, False]
    assert [r["k"] for r in recs] == list(ic.SNAPSHOTS) and recs[-1]["status"] == 1
    kx_q, y5_q, y3_q, y7_q = set(), set(), set(), set()
    _robust(N, box, recs)
    for r in recs:
        y = r["y"]
        kx = (y[m.o1:m.o1 + FN] + y[m.o2:m.o2 + FN]).reshape(nf, N)
        kx_q |= set((np.nonzero(kx.any(axis=0))[0] >> 8).tolist())
        y5_q |= set((np.nonzero(y[m.o5:m.o5 + N])[0] >> 8).tolist())
        nup = np.array(ic.nup_nodes(N))
        y3_q |= set((nup[y[m.o3 + nup] != 0.0] >> 8).tolist())
        y7_q |= set((nup[y[m.o7 + nup] != 0.0] >> 8).tolist())
        sup = (r["x"] > 0).sum(axis=1)
        mir["sup"] |= {c for c, hit in (("1", (sup == 1).any()), ("2-16", ((sup > 1) & (sup <= 16)).any()),
                                        (">16", (sup > 16).any())) if hit}
    print(f"mirror N={N} step={step} tight={tight} F={nf} box={box}: restarts "
          f"{[r.get('restart') for r in recs[:-1]]} chunk indices with kx != 0 {sorted(kx_q)}, y5 != 0 "
          f"{sorted(y5_q)}, at an n-up node y3 != 0 {sorted(y3_q)}, y7 != 0 {sorted(y7_q)}")
    assert {r["restart"] for r in recs[:-1]} == {True, False}         # FIRST passes with and without a restart
    if step == 1:
        assert kx_q == set(range(nq)) and y5_q == set(range(nq)), (N, box, kx_q, y5_q)
    else:                                                          # the score row's dual moves (scalar_pass)
        assert m.dred and any(r["y"][m.oS] != 0.0 for r in recs), (N, box)
    if box == 2 and nf == ic.F:      # the n-up box: the memory and C7 duals move at a chosen node of every chunk index
        assert y3_q == set(range(nq)) and y7_q == set(range(nq)), (N, y3_q, y7_q)


def _engine_run(run):
    """Per snapshot k: {slot: state} of the compared slots, their boxes, and the engine's eta / omega."""
    from core.engine.lp import LPModel, LP_ITERATION_LIMIT
    N, step, ns, box, tight, nf = ic.normalise(run)
    data, m0 = _ref_model(N, step, tight, nf)
    lb2, ub2 = ic.boxes(N, m0.n_int, step, nf, tight=tight)
    which = ic.slot_boxes(run)
    nb = len(set(which.tolist()))
    picks = sorted((set(range(max(nb, 2))) | set(range(ns - max(nb, 2), ns))) & set(range(ns)))
    m = LPModel(data, ic.VARIANT, step=step, max_batch=ns, **ic.model_kw(step))
    out = {"which": which, "picks": picks, "snaps": {}}
    try:
        assert m.n_int == m0.n_int
        for k in ic.SNAPSHOTS:
            st = m.submit(np.arange(ns), lb2[which], ub2[which], max_iters=k, **RUN)
            assert (st == LP_ITERATION_LIMIT).all(), st
            d0 = m.diag(0)
            out.setdefault("eta", (d0["eta"], d0["omega"]))
            nblocks = (k - 1) // ic.CHECK_EVERY + 1
            for b in range(nblocks):
                assert m.active() == ns            # every slot still iterates before each block: the tile holds
                r = m.advance(0)
                assert len(r["slots"]) == (ns if b == nblocks - 1 else 0), (k, b, r)
            assert (r["status"] == LP_ITERATION_LIMIT).all() and (r["iters"] == k).all(), (k, r)
            snap = {}
            for s in picks:
                x, rf, _ = m.rows(s)
                z, _ = m.solution(s, dense_x=False)
                snap[s] = {"x": x, "rf": rf, "z": z, "y": m.debug_state(s, m0.n_dual)["y"], "diag": m.diag(s)}
            out["snaps"][k] = snap
    finally:
        m.close()
    return out


def _within(name, got, ref, emu, tag, worst):
    d = float(np.abs(emu - ref).max())
    err = np.abs(got - ref)
    bound = np.maximum(8.0 * d, FLOOR * np.maximum(1.0, np.abs(ref)))
    w = worst.setdefault(name, [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], d), max(w[1], float(np.abs(ref).max())), max(w[2], float(err.max()))
    print(f"  {tag} {name}: d {d:.3e} kernel {float(err.max()):.3e} bound {float(bound.max()):.3e}")
    bad = err > bound
    assert not bad.any(), (tag, name, int(bad.sum()), float(err.max()), d)


def _within_blocks(blocks, got, ref, emu, tag, worst):
    """ic.block_rows: every block within its own bound; prints d_B, s_B and the kernel's error before it asserts."""
    keep = [b for b in blocks if b[0] in ABS_FLOOR_BLOCKS]
    rows = ic.block_rows([b for b in blocks if b[0] not in ABS_FLOOR_BLOCKS], got, ref, emu)
    for name, d, s, err, ok in rows:
        w = worst.setdefault(name, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], d), max(w[1], s), max(w[2], err)
        print(f"  {tag} {name}: d_B {d:.3e} s_B {s:.3e} kernel {err:.3e} bound {max(8 * d, FLOOR * s):.3e}")
    if keep:
        sel = np.concatenate([np.arange(o, o + n) for _, o, n in keep])
        _within("+".join(b[0] for b in keep), got[sel], ref[sel], emu[sel], tag, worst)
    bad = [r for r in rows if not r[4]]
    assert not bad, (tag, bad)


def _check_state(st, ref, emu, m, ub, blocks, tag, worst, k):
    """One slot's state at a snapshot against the mirror's records of its box (upper bounds ub)."""
    closed = (ub[m.oc:m.oc + m.F * m.N].reshape(m.F, m.N) <= 0.0)[st["rf"]]
    assert not _bits(st["x"][closed]).any(), tag          # +0 at every closed destination
    _within("x", st["x"].astype(np.float64), ref["x"], emu["x"], tag, worst)
    _within_blocks(blocks["z"], st["z"], ref["z"], emu["z"], tag, worst)
    _within_blocks(blocks["y"], st["y"], ref["y"], emu["y"], tag, worst)
    for name, key in (("pobj", "pobj"), ("lagr", "lagr"), ("pres", "res")):
        _within(name, np.float64(st["diag"][name]), np.float64(ref["cert"][key]),
                np.float64(emu["cert"][key]), tag, worst)
    assert st["diag"]["k"] == k


def _report(name, worst):
    print(name, "worst over snapshots and slots [d, |mirror|, kernel]:",
          {k: [f"{v[0]:.2e}", f"{v[1]:.2e}", f"{v[2]:.2e}"] for k, v in worst.items()})


def _compare(run):
    N, step, ns, box, tight, nf = ic.normalise(run)
    print(_id(run), "x_pass variants", sorted(ic.variants(N, ns, nf)))
    eng = _engine_run(run)
    need = set(eng["which"].tolist()) | (set() if tight or nf != ic.F else {0, 1})
    mir = mirror(N, step, *eng["eta"], tight=tight, nf=nf, need=sorted(need))
    m = mir["m"]
    blocks = ic.blocks_of(m)
    worst = {}
    for ki, k in enumerate(ic.SNAPSHOTS):
        snap = eng["snaps"][k]
        by_box = {}
        for s in eng["picks"]:
            b = int(eng["which"][s])
            ref, emu = mir["recs"][b, False][ki], mir["recs"][b, True][ki]
            st = snap[s]
            tag = f"k={k} slot={s} box={b}"
            _check_state(st, ref, emu, m, mir["box"][b, 1], blocks, tag, worst, k)
            if b in by_box:                                       # same box, same launch: the same bits
                o = snap[by_box[b]]
                for q in ("x", "z", "y"):
                    assert np.array_equal(_bits(o[q]), _bits(st[q])), (tag, q)
            by_box.setdefault(b, s)
    _report(_id(run), worst)


@pytest.mark.parametrize("run", ic.matrix(), ids=_id)
def test_kernel_iterates_match_mirror(run):
    _compare(run)


@pytest.mark.parametrize("run", ic.matrix_tight(), ids=_id)
def test_kernel_iterates_match_mirror_tight(run):
    """The n-up box of the tight instance: the memory duals y3, the C7 duals y7 and the free c move."""
    _compare(run)


@pytest.mark.parametrize("run", ic.matrix_wide(), ids=_id)
def test_kernel_iterates_match_mirror_wide(run):
    """F = 67: node_pass sums two functions per lane with one short lane, scalar_pass strides twice over its
    partials (test_iter_sensitivity.py asserts the shape)."""
    _compare(run)


# ---------------------------------------------------------------------------------------------------------------
# warm starts: every B&B child is one
# ---------------------------------------------------------------------------------------------------------------
WARM_K = 33                 # the parent: a cold root LP of the tight instance stopped at its third certificate
WARM_CHILDREN = (1, 2)      # a leaf-type child (closes destinations the parent routes to) and the n-up child


def mirror_warm(N, eta, omega):
    """Per child box: (fp64 records, fp32-emulation records) of the LP warm-started from the mirror's own parent —
    the root LP's record at k = WARM_K of the same arithmetic — with the engine's default weight band."""
    from ref_pdhg import OMEGA_TRAINED, blocks
    mir = mirror(N, 1, eta, omega, tight=True, need=(0,))
    if "warm" in mir:
        return mir
    m, bf = mir["m"], mir["box"]
    assert mir["ok"][list(WARM_CHILDREN)].all()
    ki = ic.SNAPSHOTS.index(WARM_K)
    assert WARM_K + ic.SNAPSHOTS[-1] < OMEGA_TRAINED      # the cap of the weight band stays inactive
    par = mir["recs"][0, False][ki]
    # the parent routes under destinations the leaf child closes: mass > 0.1 in every full 256-destination chunk
    # index; the last one holds two destinations at these widths, both open in the leaf box at N = 258 and one
    # closed (for three functions) beyond, which then carries mass too
    closed = (bf[1, 1][m.oc:m.oc + m.F * N].reshape(m.F, N) <= 0.0)[m.row_f]
    mass = np.bincount(np.arange(N) >> 8, weights=(par["x"] * closed).sum(axis=0))
    nclosed = np.bincount(np.arange(N) >> 8, weights=closed.any(axis=0))
    assert (mass[:N // 256] > 0.1).all() and ((mass > 0) == (nclosed > 0)).all(), (N, mass, nclosed)

    def one(box, fp32):
        p = mir["recs"][0, fp32][ki]
        return [r for r in blocks(m, box=(bf[box, 0], bf[box, 1]), tol=1e-12, max_iters=ic.SNAPSHOTS[-1],
                                  check_every=ic.CHECK_EVERY, eta=eta, omega0=omega, rs_nec=0.9, fp32=fp32,
                                  engine=True, start=(p["x"], p["z"], p["y"], p["omega"]), lineage=WARM_K)]
    with cf.ThreadPoolExecutor(4) as ex:
        futs = {(b, fp): ex.submit(one, b, fp) for b in WARM_CHILDREN for fp in (False, True)}
        warm = {k: f.result() for k, f in futs.items()}
    mir["warm_snaps"] = {}
    for b in WARM_CHILDREN:
        recs = warm[b, False]
        assert [r["k"] for r in recs] == list(ic.SNAPSHOTS) and recs[-1]["status"] == 1
        # snapshots compared: those before the first certificate with a column deficit the pooled / loaded shift would
        # serve (the mirror has none; a run stopped earlier never meets it) — all five, except for the n-up child at
        # N = 26, whose certificate at k = 49 has one: there k = 1, 17, 33
        dfc = [bool(((r["cert"]["deficit"] > 0) & (r["cert"]["deficit"] <= 2e-3)).any()) for r in recs]
        n = dfc.index(True) if True in dfc else len(recs)
        assert n >= 3 and (n == len(recs) or (N, b) == (26, 2)), (N, b, dfc)
        _robust(N, b, recs[:n])
        mir["warm_snaps"][b] = ic.SNAPSHOTS[:n]
        print(f"mirror N={N} warm child box={b}: parent omega {par['omega']:.4e} restarts "
              f"{[r.get('restart') for r in recs[:-1]]} omega {[round(r['omega'] / par['omega'], 3) for r in recs]} x parent's")
    mir["warm"] = warm
    return mir


def _engine_warm(N):
    """Per snapshot k: the two children's states after k warm iterations from a parent stopped at WARM_K (the parent
    is run again for every snapshot, as every snapshot is its own run)."""
    from core.engine.lp import LPModel, LP_ITERATION_LIMIT
    data, m0 = _ref_model(N, 1, True, ic.F)
    lb, ub = ic.boxes(N, m0.n_int, 1, ic.F, tight=True)
    kids = list(WARM_CHILDREN)
    m = LPModel(data, ic.VARIANT, step=1, max_batch=3, **ic.model_kw(1))
    out = {"snaps": {}}

    def run(slots, boxes, k, warm):
        st = m.submit(slots, lb[boxes], ub[boxes], max_iters=k, warm_start=warm, **RUN)
        assert (st == LP_ITERATION_LIMIT).all(), st
        d = [m.diag(s) for s in slots]
        while m.active():
            r = m.advance(0)
        assert sorted(r["slots"].tolist()) == sorted(slots) and (r["iters"] == k).all(), r
        assert (r["status"] == LP_ITERATION_LIMIT).all(), r
        return d
    try:
        for k in ic.SNAPSHOTS:
            d0 = run([0], [0], WARM_K, False)[0]
            out.setdefault("eta", (d0["eta"], d0["omega"]))
            omega_p = m.diag(0)["omega"]
            for s in kids:
                m.copy_state(0, s)
            for d in run(kids, kids, k, True):
                assert d["omega"] == omega_p and d["eta"] == d0["eta"]   # the child goes on at the parent's weight
            snap = {}
            for s in kids:
                x, rf, _ = m.rows(s)
                z, _ = m.solution(s, dense_x=False)
                snap[s] = {"x": x, "rf": rf, "z": z, "y": m.debug_state(s, m0.n_dual)["y"], "diag": m.diag(s)}
            out["snaps"][k] = snap
            out["omega_p"] = omega_p
    finally:
        m.close()
    return out


@pytest.mark.parametrize("N", ic.EXTRA_CHUNK)
def test_warm_started_children_match_mirror(N):
    """nep_lp_copy_state + a warm submit (init_slot with warm = 1 and the INIT passes over a copied state): the
    children of a root LP stopped at k = 33, one with the leaf box and one with the n-up box, against the mirror
    started from its own parent record."""
    eng = _engine_warm(N)
    mir = mirror_warm(N, *eng["eta"])
    m = mir["m"]
    blocks = ic.blocks_of(m)
    par = mir["recs"][0, False][ic.SNAPSHOTS.index(WARM_K)]
    # the parent's final weight, which the children inherit: its restarts' updates, so of the order of d
    assert abs(eng["omega_p"] - par["omega"]) <= 1e-3 * par["omega"], (eng["omega_p"], par["omega"])
    worst = {}
    for b in WARM_CHILDREN:
        for ki, k in enumerate(mir["warm_snaps"][b]):
            _check_state(eng["snaps"][k][b], mir["warm"][b, False][ki], mir["warm"][b, True][ki], m, mir["box"][b, 1],
                         blocks, f"warm k={k} box={b}", worst, k)
    _report(f"N{N}-warm", worst)
