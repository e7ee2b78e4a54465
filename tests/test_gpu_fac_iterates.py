"""The facility-relaxation kernels (fac_x_pass, fac_node_pass; scalar_pass's certificate and reduced-cost bookkeeping)
against the fp64 numpy mirror (ref_fac.blocks), iterate by iterate, as test_gpu_iterates.py does for the reference
kernels: the routing rows x, the x <= c duals lambda and their per-function sums lsum (nep_debug_fac_state), c and n, the
duals y = (y3, y5, mu) of an LP stopped at its certificate iterations k = 1, 17, 33, 49, 65 (check_every = 16), the
certificate's objective, bound and residual there (diag), and the reduced costs and bound nep_lp_get_reduced_costs
reports (the best certificate's up to k: the rc_cur / rc_best double buffer).

Protocol (test_gpu_iterates.py): every snapshot is its own cold run with max_iters = k; every slot of a run has the same
budget, no slot ends early (asserted), so the tile never changes under a run.  The mirror is made the same algorithm
first: the engine's step size and initial weight (diag eta / omega after the submit), the engine's node boxes
(nep_debug_state lb / ub), the engine's scaling (rho, gam, rownorm from nep_debug_build, rho_l as the device holds it) —
the scaling itself is an input here, not a subject.  Asserted from the mirror alone, per shape
(ref_fac.matrix_preconditions): FIRST passes with and without a restart; no restart decision within a relative 1e-3 of
flipping; lambda, mu, y3 and y5 nonzero in every 256-destination chunk index, the last included; anchors of support
1, 2..16 and > 16; the best bound both replaced and kept.

Tolerance: from the mirror, never from the kernels.  d = largest difference between the fp32-emulating mirror
(blocks(fp32=True)) and the fp64 mirror, per array and snapshot; the kernel must be within max(8 d, 64 * 2^-24 *
max(1, |value|)) of the fp64 mirror.  Exact checks: slots holding the same box in one launch are bit-identical in x,
lambda, z and y; x is +0 (all bits clear) at every closed destination; lambda, mu, y3 and y5 are <= 0 everywhere.

Cases (iter_cases.fac_matrix; instances iter_cases.fac_instance: function 0 has 38 routing rows — more than two passes of
a 16-wave tile, no multiple of 4 —, every other function 9): F = 4, N = 26, 258, 514, 1026 (one chunk past a lane
boundary, two padding columns, 10 or 2 nodes in fac_node_pass's last 16-node block; CPL 1, 2, 4, 8) with 1 slot (root
box, and the leaf box alone), 128 and 256 slots (alternating root / leaf; the first two and last two slots compared);
N = 254, 510, 1022, 1470 and 1472 (the largest admitted width, no padding) at 256 slots; N = 26 with F = 67 at 2
slots (fac_node_pass sums per = 2 functions per group, the last group short).  fac_x_pass variants run: every (CPL, TW,
kind) the launchers can dispatch (test_ref_fac.py lists the others).  A last test continues copied states:
nep_lp_copy_state / nep_lp_copy_states of a facility slot (lambda, lsum, the reduced-cost buffers travel) warm-started
beside their source end with the same bits.

Not covered: the facility presolve and the scaling (inputs here), dual polishing (facility LPs never polish), the
warm-start primal-weight band (floor / cap / reference weight: the copied-state test runs with them off),
MinUtilization, and the padding columns j >= N of x and lambda themselves (only their effect on the sums is seen).

Measured on an MI355X (worst snapshot and slot per run; kernel = |kernel - fp64 mirror|; each test prints its table
with -s).  Kernel, over the 22 runs: x 4.4e-7 .. 2.4e-6 (largest at N = 510), lambda 9e-10 .. 1.3e-8, lsum <= 1.8e-8,
c / n <= 1.0e-7, y <= 7.5e-9, pobj <= 3.9e-6, lagr <= 5.4e-7, rc <= 2.2e-8, bound <= 1.0e-8, pres 1.7e-6 .. 2.2e-4 (the
largest at F = 67, where the residual itself is ~1e3: the repaired n is a CPU sum over a 1/64 core).  Mirror noise d:
x 4.4e-7 .. 2.3e-6, lambda 8.6e-10 .. 1.2e-8, pres 4.2e-6 .. 1.5e-4; the kernel sits at 0.6 .. 1.8 d in x and lambda at
every width, tile and slot count, and a slot differs between 1, 128 and 256 slots only through the tile's summation
order (N = 258 x: 1.2e-6 / 8.8e-7 / 1.7e-6).  A first emulation took the simplex threshold from the fp64 projection and
rounded it; with it pres at N = 1470, 256 slots, k = 33, root box, had d = 9.9e-8 against a kernel 4.8e-6 off (48 d,
1.25 x the floor) while its neighbours k = 17 and 49 had d = 4.1e-6 and 1.9e-6: pres there is the CPU sum of one node
over its cores (amplification 22 per row, 6 rows), and a scalar's d is a single noise sample, which fell to 1.3e-8 in
that column of x against a typical 3e-7.  fac_x_pass ends its threshold as (sum - 1) / count with a float32 sum in the
wave's order, so the emulation now does the same (ref_fac.wave_sum_f32): d = 6.3e-7 there, the kernel at 7.6 d.  With
the deliberate error of dropping (1 - lam) * lanc from lambda's Halpern step in a scratch build, all 22 runs fail at
k = 17, slot 0, in x (1.7e-3 .. 2.2e-1 off against d <= 1e-6), lambda (1.8e-3 .. 4.8e-3 against d <= 7e-9) and the
certificate; k = 1 still passes (no Halpern step before it), as does the copied-state test (its copies are exact
either way).
"""
import concurrent.futures as cf

import numpy as np
import pytest

import iter_cases as ic

pytestmark = pytest.mark.gpu
FLOOR = 64 * 2.0 ** -24
RUN = dict(tol=1e-12, check_every=ic.CHECK_EVERY, polish_after=-1.0)


def _id(run):
    N, F, ns, box = run
    return f"N{N}-F{F}-slots{ns}" + ("" if box is None else f"-box{box}")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


_DATA = {}


def _data(N, F):
    if (N, F) not in _DATA:
        _DATA[N, F] = ic.fac_instance(N, F)
    return _DATA[N, F]


_MIRROR = {}


def mirror(N, F, eta, omega, rho_l, box):
    """(fp64 records, fp32-emulation records) per box at the engine's eta / omega / rho_l / boxes: once per shape."""
    from core.engine.lp import debug_build, RELAX_FACILITY
    from ref_fac import RefFac, blocks, matrix_preconditions
    key = (N, F)
    if key in _MIRROR:
        got = _MIRROR[key]
        assert got["eta"] == (eta, omega) and np.array_equal(got["rho_l"], rho_l) and np.array_equal(got["box"], box)
        return got
    data = _data(N, F)
    b = debug_build(data, ic.VARIANT, alpha=ic.ALPHA, relaxation=RELAX_FACILITY)
    m = RefFac(data, ic.VARIANT, ic.ALPHA, b["rho"], b["gam"], b["rownorm"], rho_l=rho_l.astype(np.float64))
    assert (b["R"], b["n_int"], b["n_dual"]) == (m.R, m.n_int, m.n_dual) and (rho_l > 0).all()

    def one(bx, fp32):
        return list(blocks(m, box=(box[bx, 0], box[bx, 1]), tol=1e-12, max_iters=ic.SNAPSHOTS[-1],
                           check_every=ic.CHECK_EVERY, eta=eta, omega0=omega, fp32=fp32, engine=True))
    with cf.ThreadPoolExecutor(4) as ex:
        futs = {(bx, fp): ex.submit(one, bx, fp) for bx in (0, 1) for fp in (False, True)}
        recs = {k: f.result() for k, f in futs.items()}
    matrix_preconditions(m, {bx: recs[bx, False] for bx in (0, 1)}, ic.SNAPSHOTS, tag=key)
    for bx in (0, 1):
        print(f"mirror N={N} F={F} box={bx}: restarts {[r['restart'] for r in recs[bx, False][:-1]]} "
              f"best bound {[round(r['best'], 6) for r in recs[bx, False]]}")
    _MIRROR[key] = {"eta": (eta, omega), "rho_l": rho_l, "box": box, "m": m, "recs": recs}
    return _MIRROR[key]


def _read(m, s, n_dual):
    x, rf, _ = m.rows(s)
    z, _ = m.solution(s, dense_x=False)
    st = m.debug_state(s, n_dual)
    fs = m.debug_fac_state(s)
    rc, bound = m.reduced_costs([s])
    return {"x": x, "rf": rf, "z": z, "y": st["y"], "lam": fs["lam"], "lsum": fs["lsum"], "diag": m.diag(s),
            "rc": rc[0], "bound": float(bound[0])}


def _engine_run(N, F, ns, box):
    """Per snapshot k: {slot: state} of the compared slots; their boxes as the engine holds them; eta / omega / rho_l."""
    from core.engine.lp import LPModel, LP_ITERATION_LIMIT, RELAX_FACILITY
    data = _data(N, F)
    n_int, n_dual = F * N + N, 2 * N + F * N
    lb2, ub2 = ic.boxes(N, n_int, 1, F)
    which = np.array([box] if ns == 1 else [s % 2 for s in range(ns)])
    picks = sorted({0, 1, ns - 2, ns - 1} & set(range(ns)))
    m = LPModel(data, ic.VARIANT, alpha=ic.ALPHA, max_batch=max(ns, 2), relaxation=RELAX_FACILITY)
    out = {"which": which, "picks": picks, "snaps": {}}
    try:
        assert m.n_int == n_int
        # the node boxes as the engine presolves them (a lone slot's run: the other box through the spare slot)
        st = m.submit([0, 1], lb2, ub2, max_iters=1, **RUN)
        assert (st == LP_ITERATION_LIMIT).all(), st
        while m.active():
            m.advance(0)
        ebox = np.array([[m.debug_state(s, n_dual)[q] for q in ("lb", "ub")] for s in (0, 1)])
        out["box"] = ebox
        out["rho_l"] = m.debug_fac_state(0)["rho_l"]
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
            out["snaps"][k] = {s: _read(m, s, n_dual) for s in picks}
            for s in picks:                        # the box of the run is the box the mirror gets
                stt = m.debug_state(s, n_dual)
                assert np.array_equal(stt["lb"], ebox[which[s], 0]) and np.array_equal(stt["ub"], ebox[which[s], 1])
    finally:
        m.close()
    return out


def _within(name, got, ref, emu, tag, worst, missed):
    got, ref, emu = (np.asarray(a, np.float64) for a in (got, ref, emu))
    d = float(np.abs(emu - ref).max())
    err = np.abs(got - ref)
    bound = np.maximum(8.0 * d, FLOOR * np.maximum(1.0, np.abs(ref)))
    w = worst.setdefault(name, [0.0, 0.0])
    w[0], w[1] = max(w[0], d), max(w[1], float(err.max()))
    print(f"  {tag} {name}: d {d:.3e} kernel {float(err.max()):.3e} bound {float(bound.max()):.3e}")
    bad = err > bound
    if bad.any():                                  # (collected: one failure names every array a snapshot misses)
        missed.append((tag, name, int(bad.sum()), float(err.max()), d))


@pytest.mark.parametrize("run", ic.fac_matrix(), ids=_id)
def test_fac_kernel_iterates_match_mirror(run):
    N, F, ns, box = run
    print(_id(run), "fac_x_pass variants", sorted(ic.fac_variants(N, ns, F)))
    eng = _engine_run(N, F, ns, box)
    mir = mirror(N, F, *eng["eta"], eng["rho_l"], eng["box"])
    FN = F * N
    worst = {}
    for ki, k in enumerate(ic.SNAPSHOTS):
        snap = eng["snaps"][k]
        by_box = {}
        for s in eng["picks"]:
            b = int(eng["which"][s])
            ref, emu = mir["recs"][b, False][ki], mir["recs"][b, True][ki]
            assert ref["k"] == k and emu["k"] == k
            st = snap[s]
            tag = f"k={k} slot={s} box={b}"
            closed = (eng["box"][b, 1][:FN].reshape(F, N) <= 0.0)[st["rf"]]
            assert not _bits(st["x"][closed]).any(), tag          # +0 at every closed destination
            assert (st["lam"] <= 0).all() and (st["y"] <= 0).all(), tag     # lambda, y3, y5, mu: duals of <= rows
            missed = []
            for name in ("x", "lam", "lsum", "z", "y"):
                e, r = emu[name], ref[name]
                _within(name, st[name], r, e, tag, worst, missed)
            for name, key in (("pobj", "pobj"), ("lagr", "lagr"), ("pres", "res")):
                _within(name, st["diag"][name], ref["cert"][key], emu["cert"][key], tag, worst, missed)
            _within("rc", st["rc"], ref["rc_best"], emu["rc_best"], tag, worst, missed)
            _within("bound", st["bound"], ref["best"], emu["best"], tag, worst, missed)
            assert not missed, missed
            assert st["diag"]["k"] == k
            if b in by_box:                                       # same box, same launch: the same bits
                o = snap[by_box[b]]
                for q in ("x", "lam", "z", "y"):
                    assert np.array_equal(_bits(o[q]), _bits(st[q])), (tag, q)
            by_box.setdefault(b, s)
    print(_id(run), "worst over snapshots and slots [d, kernel]:",
          {k: [f"{v[0]:.2e}", f"{v[1]:.2e}"] for k, v in worst.items()})


def test_copied_facility_state_continues_identically():
    """A copied facility slot is its source: slots 0 and 1 run cold on the leaf box to k = 33 (the same bits), slot 2
    takes slot 0 by nep_lp_copy_state and slot 3 takes slot 1 by nep_lp_copy_states, and slots 1, 2, 3 warm-started
    with the same box for 33 more iterations end with the same bits in x, lambda, lsum, z, y and diag — a segment left
    out of either copy (lambda, lsum, theta, the duals, Ctrl) would only slow a search down, and shows here."""
    from core.engine.lp import LPModel, LP_ITERATION_LIMIT, RELAX_FACILITY
    N, F, k = 258, ic.F, 33
    n_int, n_dual = F * N + N, 2 * N + F * N
    lb2, ub2 = ic.boxes(N, n_int, 1, F)
    m = LPModel(_data(N, F), ic.VARIANT, alpha=ic.ALPHA, max_batch=4, relaxation=RELAX_FACILITY)

    def state(s):
        st = _read(m, s, n_dual)
        return {q: st[q] for q in ("x", "lam", "lsum", "z", "y")} | {"diag": np.array(list(st["diag"].values()))}

    def run(slots, warm):
        lb, ub = np.repeat(lb2[1:2], len(slots), axis=0), np.repeat(ub2[1:2], len(slots), axis=0)
        st = m.submit(slots, lb, ub, max_iters=k, warm_start=warm, **RUN)
        assert (st == LP_ITERATION_LIMIT).all(), st
        while m.active():
            r = m.advance(0)
        assert sorted(r["slots"].tolist()) == sorted(slots) and (r["iters"] == k).all(), r
    try:
        run([0, 1], False)
        a, b = state(0), state(1)
        for q in a:
            assert np.array_equal(_bits(a[q]), _bits(b[q])), q
        assert a["lam"].any() and a["lsum"].any() and a["y"].any()      # (there is a state to lose)
        m.copy_state(0, 2)
        m.copy_states([1], [3])
        run([1, 2, 3], True)
        ref = state(1)
        assert not np.array_equal(_bits(ref["x"]), _bits(a["x"]))       # (the continuation moved on)
        for s in (2, 3):
            got = state(s)
            for q in ref:
                assert np.array_equal(_bits(ref[q]), _bits(got[q])), (s, q)
    finally:
        m.close()
