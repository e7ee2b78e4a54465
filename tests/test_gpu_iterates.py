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
support 1, 2..16 and > 16 all occur over the two boxes of a shape.

Tolerance: from the mirror, never from the kernels.  d = largest difference between the fp32-emulating mirror
(blocks(fp32=True): x, its anchor, x̂, the packed duals, tau, lambda and the plain iterations' column / CPU sums
rounded to float32) and the fp64 mirror, per array and snapshot; the kernel must be within max(8 d, 64 * 2^-24 *
max(1, |value|)) of the fp64 mirror (8: summation orders numpy does not reproduce).  Exact checks: slots holding
the same box in one launch are bit-identical in x, z, y; x is +0 (all bits clear) at every closed destination.

Cases (iter_cases.matrix): F = 4, MinDelayAndUtilization; N = 26, 258, 514, 1026 (one chunk past a lane boundary
plus padding; CPL 1, 2, 4, 8) with 1 slot (root box, and the leaf box alone), 128 and 256 slots (alternating root /
leaf; the first two and last two slots are compared); N = 254, 510, 1022 and the largest admitted N at 256 slots;
one step-2 (delete, reduced disruption block) model at N = 258, two slots.  x_pass variants run: every (CPL, TW,
kind) the launchers can dispatch (test_abi.py test_iterate_matrix_reaches_every_dispatchable_variant lists them;
not dispatchable, hence not run: CPL 8 at TW 16, certificate passes at TW 16 beyond NP = 496 and at TW 8 beyond
NP = 876, i.e. CPL 4 / CHECK / TW 16 and CPL 8 / CHECK / TW 8 and 16).

Not covered, by construction of these short cold runs: the memory duals y3 and the C7 duals y7 stay exactly 0 in
every case, as do (step 2) the score row's dual unless iter_cases.STEP2_KW makes it move; the padding columns
j >= N of x are not readable through the C ABI (only their effect on the sums is); the pooled / loaded shift, dual
polishing, warm starts and the full (unreduced) step-2 block are excluded by precondition or not mirrored; the
facility kernels have their own mirror and file (ref_fac.py, test_gpu_fac_iterates.py).

Measured on an MI355X (worst snapshot and slot per run; kernel = |kernel - fp64 mirror|; each test prints its own
table with -s).  Kernel, over all 21 runs: x 5e-9 .. 5.7e-5 (largest at N = 1416), z <= 2.2e-11, y <= 2.1e-10,
pobj <= 3.3e-9, lagr <= 2.8e-8, pres <= 2.8e-5; the same slot of a shape differs between 1, 128 and 256 slots only
through the tile's summation order (N = 258 leaf box x: 1.3e-5 / 1.2e-5 / 7.9e-6).  Mirror noise d for x: 5e-9
(N = 26 leaf) .. 2e-5 (N = 1416); the kernel sits at 0.2 .. 6 d.  A first emulation that rounded only the result
of the shifted point gave d = 9.9e-8 for x at N = 254, leaf box, k = 17, where the kernel is 3.9e-6 off on two
entries of a two-entry row (40 d, 2.6 % over the floor): the terms of tau g there are ~10^2 and cancel, so the
emulation now evaluates them in float32 one by one as x_pass does (d = 1.3e-6 there).  The duals here are small
(|y| <= 1e-2: the objective is normalised), so for y the floor, not 8 d, is the binding bound; the measured y
differences are nevertheless of the order of d (0.3 .. 7 d on the worst snapshots), far below the floor.
"""
import concurrent.futures as cf

import numpy as np
import pytest

import iter_cases as ic

pytestmark = pytest.mark.gpu
FLOOR = 64 * 2.0 ** -24
RUN = dict(tol=1e-12, check_every=ic.CHECK_EVERY, polish_after=-1.0)


def _id(run):
    N, step, ns, box = run
    return f"N{N}-step{step}-slots{ns}" + ("" if box is None else f"-box{box}")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


_MODELS = {}


def _ref_model(N, step):
    """(instance, its mirror model), built once per shape."""
    from ref_pdhg import RefModel
    if (N, step) not in _MODELS:
        data = ic.instance(N, step)
        _MODELS[N, step] = (data, RefModel(data, ic.VARIANT, step=step, **ic.model_kw(step)))
    return _MODELS[N, step]


_MIRROR = {}


def mirror(N, step, eta, omega):
    """(fp64 records, fp32-emulation records) per box, at the engine's eta / omega: computed once per (N, step)."""
    from core.engine.lp import debug_presolve
    from ref_pdhg import RefModel, blocks
    key = (N, step)
    if key in _MIRROR:
        assert _MIRROR[key]["eta"] == (eta, omega)      # (one model per shape: the same step for every run)
        return _MIRROR[key]
    data, m0 = _ref_model(N, step)
    lb, ub = ic.boxes(N, m0.n_int, step)
    okf, okn, bf, _ = debug_presolve(data, ic.VARIANT, lb, ub, step=step, **ic.model_kw(step))
    assert okf.all() and okn.all()

    def one(box, fp32):
        m = RefModel(data, ic.VARIANT, step=step, **ic.model_kw(step)) if step != 1 else m0   # (dred writes m.lo / hi)
        return [r for r in blocks(m, box=(bf[box, 0], bf[box, 1]), tol=1e-12, max_iters=ic.SNAPSHOTS[-1],
                                  check_every=ic.CHECK_EVERY, eta=eta, omega0=omega, rs_nec=0.9, fp32=fp32,
                                  engine=True)]
    with cf.ThreadPoolExecutor(4) as ex:
        futs = {(b, fp): ex.submit(one, b, fp) for b in (0, 1) for fp in (False, True)}
        recs = {k: f.result() for k, f in futs.items()}
    out = {"eta": (eta, omega), "box": bf, "m": m0, "recs": recs}
    _preconditions(N, step, out)
    _MIRROR[key] = out
    return out


def _restart(fpr, last, prev, k_since, k, nec):
    return fpr <= 0.2 * last or (fpr <= nec * last and fpr > prev) or k_since >= 0.36 * k


def _preconditions(N, step, mir):
    m = mir["m"]
    FN = ic.F * N
    nq = (ic.padded(N) + 255) // 256
    sup_classes = set()
    for box in (0, 1):
        recs = mir["recs"][box, False]
        assert [r["k"] for r in recs] == list(ic.SNAPSHOTS) and recs[-1]["status"] == 1
        kx_q, y5_q = set(), set()
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
            y = r["y"]
            kx = (y[m.o1:m.o1 + FN] + y[m.o2:m.o2 + FN]).reshape(ic.F, N)
            kx_q |= set((np.nonzero(kx.any(axis=0))[0] >> 8).tolist())
            y5_q |= set((np.nonzero(y[m.o5:m.o5 + N])[0] >> 8).tolist())
            sup = (r["x"] > 0).sum(axis=1)
            sup_classes |= {c for c, hit in (("1", (sup == 1).any()), ("2-16", ((sup > 1) & (sup <= 16)).any()),
                                             (">16", (sup > 16).any())) if hit}
        print(f"mirror N={N} step={step} box={box}: restarts {[r.get('restart') for r in recs[:-1]]} "
              f"chunk indices with kx != 0 {sorted(kx_q)}, y5 != 0 {sorted(y5_q)}")
        assert {r["restart"] for r in recs[:-1]} == {True, False}     # FIRST passes with and without a restart
        if step == 1:
            assert kx_q == set(range(nq)) and y5_q == set(range(nq)), (N, box, kx_q, y5_q)
        else:                                                          # the score row's dual moves (scalar_pass)
            assert m.dred and any(r["y"][m.oS] != 0.0 for r in recs), (N, box)
    assert sup_classes == {"1", "2-16", ">16"} or step != 1, (N, sup_classes)


def _engine_run(N, step, ns, box):
    """Per snapshot k: {slot: state} of the compared slots, their boxes, and the engine's eta / omega."""
    from core.engine.lp import LPModel, LP_ITERATION_LIMIT
    data, m0 = _ref_model(N, step)
    lb2, ub2 = ic.boxes(N, m0.n_int, step)
    which = np.array([box] if ns == 1 else [s % 2 for s in range(ns)])
    picks = sorted({0, 1, ns - 2, ns - 1} & set(range(ns)))
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
    w = worst.setdefault(name, [0.0, 0.0])
    w[0], w[1] = max(w[0], d), max(w[1], float(err.max()))
    print(f"  {tag} {name}: d {d:.3e} kernel {float(err.max()):.3e} bound {float(bound.max()):.3e}")
    bad = err > bound
    assert not bad.any(), (tag, name, int(bad.sum()), float(err.max()), d)


@pytest.mark.parametrize("run", ic.matrix(), ids=_id)
def test_kernel_iterates_match_mirror(run):
    N, step, ns, box = run
    print(_id(run), "x_pass variants", sorted(ic.variants(N, ns)))
    eng = _engine_run(N, step, ns, box)
    mir = mirror(N, step, *eng["eta"])
    m = mir["m"]
    FN = ic.F * N
    zsel = np.r_[m.oc:m.oc + FN, m.on:m.on + N]        # c and n (reduced step 2 does not iterate the rest)
    worst = {}
    for ki, k in enumerate(ic.SNAPSHOTS):
        snap = eng["snaps"][k]
        by_box = {}
        for s in eng["picks"]:
            b = int(eng["which"][s])
            ref, emu = mir["recs"][b, False][ki], mir["recs"][b, True][ki]
            st = snap[s]
            tag = f"k={k} slot={s} box={b}"
            closed = (mir["box"][b, 1][m.oc:m.oc + FN].reshape(ic.F, N) <= 0.0)[st["rf"]]
            assert not _bits(st["x"][closed]).any(), tag          # +0 at every closed destination
            _within("x", st["x"].astype(np.float64), ref["x"], emu["x"], tag, worst)
            _within("z", st["z"][zsel], ref["z"][zsel], emu["z"][zsel], tag, worst)
            _within("y", st["y"], ref["y"], emu["y"], tag, worst)
            for name, key in (("pobj", "pobj"), ("lagr", "lagr"), ("pres", "res")):
                _within(name, np.float64(st["diag"][name]), np.float64(ref["cert"][key]),
                        np.float64(emu["cert"][key]), tag, worst)
            assert st["diag"]["k"] == k
            if b in by_box:                                       # same box, same launch: the same bits
                o = snap[by_box[b]]
                for q in ("x", "z", "y"):
                    assert np.array_equal(_bits(o[q]), _bits(st[q])), (tag, q)
            by_box.setdefault(b, s)
    print(_id(run), "worst over snapshots and slots [d, kernel]:",
          {k: [f"{v[0]:.2e}", f"{v[1]:.2e}"] for k, v in worst.items()})
