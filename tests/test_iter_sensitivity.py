"""CPU checks of the kernel-vs-mirror comparison of test_gpu_iterates.py: that its bounds can fail.

The GPU test holds every block B of z and y within max(8 d_B, 64 * 2^-24 * s_B) of the fp64 mirror (d_B: the fp32
emulation's distance from it, s_B: the block's largest magnitude; iter_cases.block_rows).  Such a bound notices a
relative error e in B only where s_B e exceeds it, so this file runs the mirror alone — its own step size, weight
and presolve — on every instance and box of those runs at N = 26 and 258 and asserts, per block, that at some
snapshot s_B > 100 max(8 d_B, 64 * 2^-24 * s_B): an error of 1 % in the block fails the GPU test.  The only blocks
for which that does not hold are exactly 0 in the mirror at every snapshot of that box; the GPU test then asserts
that the device holds exactly 0 there, and ZERO lists them so that the list cannot grow unnoticed.  Over the boxes,
every block of the step-1 model passes somewhere, at either width.  n is the thin one: as a free variable its cost
keeps it at exactly 0 in the root boxes of these short runs; it leaves 0 only in leaf boxes (by ~1e-5, still 10^7
d_B), and in the n-up box the chosen nodes' n sit on their bound 1 (a fixed value, compared to 4e-6).

Blocks in iter_cases.ABS_FLOOR_BLOCKS (y1: see there) keep the whole array's bound and are left out here.

Also here: two mutations of the mirror's records (y1 scaled by 1.01, y7 set to 0) fail block_rows against the
unmutated fp64 record (y1's only once it leaves ABS_FLOOR_BLOCKS); the new instance options leave the old instances and boxes bit-identical; the F = 67 run has
the node_pass / scalar_pass shape it is there for.
"""
import hashlib

import numpy as np
import pytest

import iter_cases as ic

WIDTHS = (26, 258)
# (N, tight instance, box) -> the blocks the mirror holds at exactly 0 at every snapshot: no relative error can show
# there, and the GPU test asserts an exact 0 on the device instead.  y3 / y7 move only in the n-up box; free n is
# held at 0 by its cost in the root boxes; y1 stays 0 where every c is fixed and no flow meets a closed placement.
ZERO = {
    (26, False, 0): {"n", "y3", "y7"},
    (26, False, 1): {"n", "y1", "y3", "y7"},
    (26, True, 0): {"n", "y3", "y7"},
    (26, True, 1): {"y3", "y7"},
    (26, True, 2): set(),
    (258, False, 0): {"n", "y3", "y7"},
    (258, False, 1): {"y1", "y3", "y7"},
    (258, True, 0): {"n", "y3", "y7"},
    (258, True, 1): {"y3", "y7"},
    (258, True, 2): set(),
}
STEP1_BLOCKS = {"c", "n", "y1", "y2", "y3", "y5", "y6", "y7"} - set(ic.ABS_FLOOR_BLOCKS)

_RECS = {}


def records(N, tight, box, nf=ic.F):
    """(model, fp64 records, fp32-emulation records) of one box, at the mirror's own eta / omega / presolve."""
    from ref_pdhg import RefModel, blocks
    key = (N, tight, box, nf)
    if key not in _RECS:
        mk = (N, tight, nf)
        if mk not in _RECS:
            _RECS[mk] = RefModel(ic.instance(N, tight=tight, n_functions=nf), ic.VARIANT, step=1, **ic.model_kw(1))
        m = _RECS[mk]
        lb, ub = ic.boxes(N, m.n_int, 1, nf, tight=tight)
        ok, lo, hi, _ = m.presolve(lb[box], ub[box])
        assert ok
        _RECS[key] = (m,) + tuple(
            list(blocks(m, box=(lo, hi), tol=1e-12, max_iters=ic.SNAPSHOTS[-1], check_every=ic.CHECK_EVERY,
                        rs_nec=0.9, fp32=fp32, engine=True)) for fp32 in (False, True))
    return _RECS[key]


def _sensitive(m, ref, emu):
    """Names of the blocks in which a 1 % error would fail block_rows at some snapshot, and the all-zero ones."""
    hit, zero = set(), None
    for r, e in zip(ref, emu):
        z0 = set()
        for arr, blocks in ic.blocks_of(m).items():
            for name, d, s, _, ok in ic.block_rows(blocks, r[arr], r[arr], e[arr]):
                assert ok
                if s > 100.0 * max(8.0 * d, ic.FLOOR * s):
                    hit.add(name)
                if s == 0.0:
                    z0.add(name)
        zero = z0 if zero is None else zero & z0
    return hit, zero


@pytest.mark.parametrize("N", WIDTHS)
def test_a_one_percent_error_fails_the_comparison_in_every_block(N):
    seen = set()
    for (width, tight, box), zero_expected in ZERO.items():
        if width != N:
            continue
        m, ref, emu = records(N, tight, box)
        hit, zero = _sensitive(m, ref, emu)
        print(f"N={N} tight={tight} box={box}: sensitive {sorted(hit)} exactly zero {sorted(zero)}")
        assert zero == zero_expected, (N, tight, box, zero)
        hit &= STEP1_BLOCKS
        assert hit == STEP1_BLOCKS - zero_expected, (N, tight, box, hit)
        seen |= hit
    assert seen == STEP1_BLOCKS


@pytest.mark.parametrize("N", WIDTHS)
def test_mutated_mirror_records_fail_the_comparison(N):
    m, ref, emu = records(N, True, 2)
    yb = ic.blocks_of(m)["y"]
    caught = {"y1": 0, "y7": 0}
    for r, e in zip(ref, emu):
        y = r["y"].copy()
        y[m.o1:m.o1 + m.F * m.N] *= 1.01
        bad = [row[0] for row in ic.block_rows(yb, y, r["y"], e["y"]) if not row[4]]
        assert set(bad) <= {"y1"}
        caught["y1"] += bad == ["y1"] and "y1" not in ic.ABS_FLOOR_BLOCKS
        y = r["y"].copy()
        y[m.o7:m.o7 + m.N] = 0.0
        bad = [row[0] for row in ic.block_rows(yb, y, r["y"], e["y"]) if not row[4]]
        assert set(bad) <= {"y7"}
        caught["y7"] += bad == ["y7"]
    # (y1 keeps the whole array's bound while it is in ABS_FLOOR_BLOCKS: its own bound would catch this mutation)
    assert caught["y7"] >= 1 and (caught["y1"] >= 1) == ("y1" not in ic.ABS_FLOOR_BLOCKS), caught


def test_nup_box_moves_the_memory_and_c7_duals_in_every_chunk_index():
    for N in WIDTHS:
        m, ref, _ = records(N, True, 2)
        nup = np.array(ic.nup_nodes(N))
        nq = set(range((ic.padded(N) + 255) // 256))
        assert set((nup >> 8).tolist()) == nq and N - 1 in nup
        mem = ic.instance(N, tight=True)
        assert (mem.node_memory_matrix[nup] >= mem.function_memory_matrix.min()).all()
        assert (mem.node_memory_matrix[nup] < 0.3 * mem.function_memory_matrix.sum()).all()
        for o in (m.o3, m.o7):
            moved = set()
            for r in ref:
                moved |= set((nup[r["y"][o + nup] != 0.0] >> 8).tolist())
            assert moved == nq, (N, o, moved)
        c = ref[-1]["z"][m.oc:m.oc + m.F * N].reshape(m.F, N)
        assert c[:, nup].max() > 0.1                      # the z comparison is about numbers of order 1


def _numeric(d):
    out = {}
    for k, v in sorted(vars(d).items()):
        v = np.asarray(v)
        if v.dtype.kind in "iuf":
            out[k] = v
    return out


def _digest(d):
    h = hashlib.sha256()
    for k, v in _numeric(d).items():
        h.update(f"{k} {v.dtype.str} {v.shape}".encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()[:16]


# sha256 over every numeric field of instance(N, step), taken before instance() had the tight / n_functions options
OLD_INSTANCES = {
    (26, 1): "88e14bafbf97b654",
    (26, 2): "3c5ffe2fe25b16e0",
    (258, 1): "7a0fb144dd487383",
    (258, 2): "b201507aad21f4d5",
    (514, 1): "9bda9ab4ae095932",
    (514, 2): "eee65a64fd0f0be8",
    (1026, 1): "1cac5dd18c1e987d",
    (1026, 2): "a3bbd22239ed5757",
}


def test_new_instance_options_leave_the_old_instances_alone():
    """instance() / boxes() without the new options return what they returned before those existed: every numeric
    field bit for bit (np.array_equal against the call that spells the defaults out, and the digest recorded from the
    earlier generator), the boxes entry by entry."""
    for N in ic.EXTRA_CHUNK:
        for step in (1, 2):
            a, b = _numeric(ic.instance(N, step)), _numeric(ic.instance(N, step, tight=False, n_functions=ic.F))
            assert len(a) >= 12 and a.keys() == b.keys()
            assert all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
            assert _digest(ic.instance(N, step)) == OLD_INSTANCES[N, step], (N, step, _digest(ic.instance(N, step)))
        # the boxes: two rows as before, and the first of the tight boxes is the same root box
        m_int = ic.F * N + N
        lb, ub = ic.boxes(N, m_int)
        assert lb.shape == ub.shape == (2, m_int)
        assert np.isneginf(lb[0]).all() and np.isposinf(ub[0]).all()
        want_ub = np.full(m_int, np.inf)
        want_ub[:ic.F * N] = 0.0
        want_lb = np.full(m_int, -np.inf)
        for f in range(ic.F):
            for j in ic.leaf_open(N, f):
                want_ub[f * N + j] = want_lb[f * N + j] = 1.0
        assert np.array_equal(lb[1], want_lb) and np.array_equal(ub[1], want_ub)
        lt, ut = ic.boxes(N, m_int, tight=True)
        assert np.array_equal(lt[0], lb[0]) and np.array_equal(ut[:2], ub)
        assert np.array_equal(ut[2], ub[0]) and (np.nonzero(lt[2] == 1.0)[0] - ic.F * N).tolist() == ic.nup_nodes(N)


def test_wide_run_has_the_shape_it_is_there_for():
    """F = 67: node_pass's 64 lanes per node sum per = 2 functions each, 33 lanes a full share and one lane a single
    function; scalar_pass strides over F = 67 and F + JB = 69 partials in steps of 64, so its second stride runs."""
    for run in ic.matrix_wide():
        N, step, ns, box, tight, nf = ic.normalise(run)
        per, full, short = ic.node_pass_groups(nf)
        assert (per, full, short) == (2, 33, 1) and full < 64
        JB = (N + 15) // 16
        assert nf > 64 and nf + JB > 64
        d = ic.instance(N, step, tight=tight, n_functions=nf)
        assert d.workload_matrix.shape == (nf, N) and d.function_memory_matrix.shape == (nf,)
        assert (np.count_nonzero(d.workload_matrix[4:], axis=1) == 8).all()      # functions 4.. as functions 1-3
        assert sorted(set(ic.slot_boxes(run).tolist())) == [0, 1]
    assert ic.node_pass_groups(ic.F) == (1, 4, 0)
