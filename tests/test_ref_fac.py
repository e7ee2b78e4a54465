"""CPU suite: what makes tests/ref_fac.py (the numpy mirror of the facility relaxation's iteration) a reference for
test_gpu_fac_iterates.py, and what that file's case matrix must exercise — nothing here needs a GPU.

 1. K and K^T of the mirror are adjoint on random vectors (1e-12 relative).
 2. The mirror run to tol 1e-7 certifies synthetic 16x8 and 24x12 (seed 0, MinDelayAndUtilization; the root box and
    two of test_gpu_fac.py's children) within the budget test_gpu_fac.py grants the engine (8 x 25k iterations), its
    value is within 1e-6 of HiGHS on oracle.formulation.facility_relaxation, EVERY certificate's bound along the way
    is <= HiGHS + 1e-9 max(1, |v|), and the certified repaired point satisfies the oracle model's rows and bounds.
 3. On the matrix of test_gpu_fac_iterates.py (iter_cases.fac_matrix), from the mirror alone
    (ref_fac.matrix_preconditions): FIRST passes with and without a restart, no restart decision within 1e-3 of
    flipping, every dual family nonzero in every 256-destination chunk, anchors of support 1 / 2..16 / > 16, the best
    bound both replaced and kept.  (Scaling from nep_debug_build; without a device the x <= c rows take the mirror's
    default scale and step — the GPU file asserts the same conditions again at the engine's.)
 4. iter_cases.fac_lds_bytes / fac_tile_waves are the engine's launch rule (nep_debug_block_split) on every run of the
    matrix, and the matrix launches every fac_x_pass<CPL, kind, TW> the launchers can dispatch for its function counts.
"""
import numpy as np
import pytest

import iter_cases as ic


def _mirror_model(data, variant, alpha):
    from core.engine.lp import debug_build, RELAX_FACILITY
    from ref_fac import RefFac
    b = debug_build(data, variant, alpha=alpha, relaxation=RELAX_FACILITY)
    m = RefFac(data, variant, alpha, b["rho"], b["gam"], b["rownorm"])
    assert (b["R"], b["n_int"], b["n_dual"]) == (m.R, m.n_int, m.n_dual)
    return m


@pytest.mark.parametrize("N,F", [(26, 4), (258, 4), (26, ic.FAC_WIDE_F)])
def test_operators_are_adjoint(N, F):
    m = _mirror_model(ic.fac_instance(N, F), ic.VARIANT, ic.ALPHA)
    rng = np.random.default_rng(N + F)
    for _ in range(3):
        x, z = rng.standard_normal((m.R, N)), rng.standard_normal(m.n_int)
        y, lam = rng.standard_normal(m.n_dual), rng.standard_normal((m.R, N))
        ky, kl = m.K(x, z)
        gx, gz = m.KT(y, lam)
        a, b = (ky * y).sum() + (kl * lam).sum(), (x * gx).sum() + (z * gz).sum()
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (a, b)


def _oracle_point(m, L, x, c, n, W):
    """The oracle model's variable vector of a mirror point: x[f, i, j] from the aggregated rows (a zero-workload
    source takes its function's pooled row), then c, then n."""
    F, N = m.F, m.N
    v = np.zeros(L.nvars)
    xf = np.zeros((F, N, N))
    pooled = {int(m.row_f[r]): r for r in range(m.R) if m.row_src[r] < 0}
    for r in range(m.R):
        if m.row_src[r] >= 0:
            xf[m.row_f[r], m.row_src[r]] = x[r]
    for f in range(F):
        for i in range(N):
            if W[f, i] == 0:
                xf[f, i] = x[pooled[f]]
    v[:L.nx] = xf.ravel()
    v[L.c0:L.c0 + F * N] = c.ravel()
    v[L.n0:L.n0 + N] = n
    return v


@pytest.mark.parametrize("N,F", [(16, 8), (24, 12)])
def test_mirror_matches_highs(N, F):
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    from oracle.formulation import build_model, facility_relaxation
    from oracle.inputs import data_to_solver_input as oracle_input
    from oracle.solve import solve as highs
    from ref_fac import blocks
    from test_gpu_fac import _fixings
    variant = "MinDelayAndUtilization"
    p = synthetic_payload(N, F, seed=0)
    alpha = p["solver"]["args"]["alpha"]
    data = data_to_solver_input(p, with_db=False)
    od = oracle_input(p, with_db=False)
    ref_model = facility_relaxation(build_model(od, variant, step=1, alpha=alpha), od)
    L = ref_model["layout"]
    m = _mirror_model(data, variant, alpha)
    fix = _fixings(F, N, np.random.default_rng(N + F), 4)
    A = ref_model["A"].tocsr()
    rn = np.maximum(1.0, abs(A).max(axis=1).toarray().ravel())
    nx = N * N * F
    W = np.asarray(data.workload_matrix)
    for b, (idx, val) in enumerate([([], [])] + fix[1:3]):      # root, an opened node, a placement fixed open
        lb, ub = np.full(m.n_int, -np.inf), np.full(m.n_int, np.inf)
        lb[idx] = ub[idx] = val
        rl, ru = ref_model["lb"].copy(), ref_model["ub"].copy()
        if idx:
            rl[nx + np.asarray(idx)] = ru[nx + np.asarray(idx)] = val
        st, ref, _ = highs(ref_model, relax=True, lb=rl, ub=ru)
        assert st == 0 and ref is not None
        last = None
        for rec in blocks(m, lb, ub, tol=1e-7, max_iters=8 * 25000, check_every=64, engine=True):
            assert rec["lag"] <= ref + 1e-9 * max(1.0, abs(ref)), (b, rec["k"], rec["lag"], ref)   # every bound valid
            last = rec
        print(f"{N}x{F} LP {b}: mirror {last['obj']:.10g} after {last['k']} iterations, HiGHS {ref:.10g}")
        assert last["status"] == 0, (b, last["k"], last["pobj"], last["best"], last["res"])
        assert abs(last["obj"] - ref) <= 1e-6, (b, last["obj"], ref)
        # the certified repaired point is feasible for the oracle's rows and bounds (residual over the row's norm)
        cert = last["cert"]
        assert cert["res"] <= 1e-7 and abs(cert["pobj"] - ref) <= 1e-6
        xn = last["xn"]
        v = _oracle_point(m, L, xn, cert["c"], cert["n"], W)
        act = A @ v
        viol = np.maximum(np.maximum(ref_model["lo"] - act, act - ref_model["hi"]), 0.0) / rn
        assert viol.max() <= 2e-7, (b, float(viol.max()), int(viol.argmax()))
        assert (v >= rl - 1e-9).all() and (v <= ru + 1e-9).all()
        assert abs(float(ref_model["c"] @ v) - cert["pobj"]) <= 1e-9


_SHAPES = sorted({(N, F) for N, F, ns, box in ic.fac_matrix()})


@pytest.mark.parametrize("N,F", _SHAPES)
def test_matrix_preconditions_hold_on_the_mirror(N, F):
    from ref_fac import blocks, matrix_preconditions
    m = _mirror_model(ic.fac_instance(N, F), ic.VARIANT, ic.ALPHA)
    lb, ub = ic.boxes(N, m.n_int, 1, F)
    recs = {box: list(blocks(m, lb[box], ub[box], tol=1e-12, max_iters=ic.SNAPSHOTS[-1], check_every=ic.CHECK_EVERY,
                             engine=True)) for box in (0, 1)}
    matrix_preconditions(m, recs, ic.SNAPSHOTS, tag=(N, F))


@pytest.mark.parametrize("N", [26, 258, 1026])
def test_fp32_emulation_is_float32_noise(N):
    """blocks(fp32=True) is the same iteration with float32 noise, not another algorithm: the same restart decisions,
    x within 1e-5 of the fp64 run and not equal to it; wave_sum_f32 adds what a float64 sum adds, in the wave's order
    (an entry in every 16-byte chunk a lane owns, exact on small integers, float32 rounding on the rest)."""
    from ref_fac import blocks, wave_sum_f32
    m = _mirror_model(ic.fac_instance(N), ic.VARIANT, ic.ALPHA)
    lb, ub = ic.boxes(N, m.n_int, 1, ic.F)
    kw = dict(tol=1e-12, max_iters=ic.SNAPSHOTS[-1], check_every=ic.CHECK_EVERY)
    for box in (0, 1):
        ref, emu = (list(blocks(m, lb[box], ub[box], fp32=fp, **kw)) for fp in (False, True))
        assert [r["restart"] for r in ref] == [r["restart"] for r in emu]
        for r, e in zip(ref[1:], emu[1:]):
            for name, hi in (("x", 1e-5), ("lam", 1e-6), ("z", 1e-5), ("y", 1e-6)):
                d = np.abs(r[name] - e[name]).max()
                assert d <= hi and (d > 0 or name != "x"), (N, box, r["k"], name, d)
            assert (e["x"] == e["x"].astype(np.float32)).all() and (e["lam"] == e["lam"].astype(np.float32)).all()
    rng = np.random.default_rng(N)
    ints = rng.integers(-8, 9, size=(3, N)).astype(np.float32)
    assert np.array_equal(wave_sum_f32(ints), ints.sum(axis=1))
    vals = rng.standard_normal((5, N)).astype(np.float32)
    exact = vals.astype(np.float64).sum(axis=1)
    got = wave_sum_f32(vals)
    assert got.dtype == np.float32 and np.abs(got - exact).max() <= N * 2.0 ** -24 * np.abs(vals).sum(axis=1).max()
    assert (got != exact).any()


def test_fac_launch_rule_and_variant_coverage():
    """iter_cases' twins are the engine's rule on every run of the matrix, and the matrix reaches every fac_x_pass
    variant the launchers can dispatch: all of CPL 1 / 2 / 4 / 8 x TW 4 / 8 / 16 x INIT / CHECK / FIRST / STEADY except
    every kind of CPL >= 4 at TW 16 (fac_tile_waves caps N > 512 at 8 waves) and the certificate pass of CPL 8 at TW 8
    (164 bytes per padded destination at 8 waves: past the LDS cap beyond NP = 896)."""
    from core.engine.lp import debug_block_split, RELAX_FACILITY
    assert ic.fac_max_nodes() == 1472 and ic.fac_lds_bytes(4, 1472, True) <= ic.LDS_CAP < ic.fac_lds_bytes(4, 1476, True)
    ran = set()
    for N, F, ns, box in ic.fac_matrix():
        split, tw_plain, tw_check = debug_block_split(N, F, ns, RELAX_FACILITY)
        assert (tw_plain, tw_check) == (ic.fac_tile_waves(N, ns, False, F), ic.fac_tile_waves(N, ns, True, F)), (N, F, ns)
        for chk in (False, True):
            assert ic.fac_lds_bytes(ic.fac_tile_waves(N, ns, chk, F), ic.padded(N), chk) <= ic.LDS_CAP
        ran |= ic.fac_variants(N, ns, F)
    # the twin against the engine beyond the matrix: every width class edge and slot counts around the tile steps
    for N in (1, 256, 257, 512, 513, 896, 897, 900, 1024, 1025, 1472):
        for F in (ic.F, ic.FAC_WIDE_F, 256):
            for ns in (1, 2, 7, 8, 15, 16, 17, 64, 127, 128, 129, 255, 256, 1024):
                got = debug_block_split(N, F, ns, RELAX_FACILITY)[1:]
                assert got == (ic.fac_tile_waves(N, ns, False, F), ic.fac_tile_waves(N, ns, True, F)), (N, F, ns)
    can = ic.fac_dispatchable()
    every = {(c, t, kd) for c in (1, 2, 4, 8) for t in (4, 8, 16) for kd in ic.KINDS}
    assert every - can == {(c, 16, kd) for c in (4, 8) for kd in ic.KINDS} | {(8, 8, "CHECK")}
    assert ran == can, sorted(can - ran)
