"""Reduced-cost fixing in the native tree search (csrc/nep_bnb.cpp, nep_bnb_params.rc_fixing, API 13) on CPU: the
tree drives HiGHS node LPs through the call table tests/test_bnb_native_cpu.py builds (core/engine/lp.PyBnbEngine),
and its optional rc_fixings call is answered from scipy.optimize.linprog's marginals of the same node LP — an exact
LP's reduced costs d and value L, for which every point of the node's box with z_k = t costs at least
L + d_k t - min(d_k lb_k, d_k ub_k).  With fixing on, the search must end OPTIMAL at the same objective in no more
nodes; switched off, or without the call, it must make today's search.

The on / off comparison runs on OracleLP, whose LPs finish in the round they were submitted in.  StreamingOracleLP —
the other model tests/test_bnb_native_cpu.py builds — makes an LP finish 1 to 3 rounds later by a crc32 of its node
box, so a fixing added to a child's box re-rolls when that child finishes: the order in which the two searches meet
their nodes then differs for a reason that is no property of the LPs, and their node counts with it.  Measured
(nodes, leaves, LPs), fixing off -> on, OracleLP: syn_6x4_s1_r0.3 MDU (40, 9, 135) -> (40, 13, 139), 54 variables
fixed; syn_8x4_s2_r0.1 MinDelay (1, 2, 5) -> the same, no call (no incumbent before the search ends); sim5
MinUtilization (324, 53, 1070) -> (320, 38, 1047), 12 fixed, 11 children and 36 leaves cut; syn_8x4_s3_r1.0
MinUtilization (23, 11, 77) -> (23, 11, 78), 1 fixed.  On StreamingOracleLP the same four read (39, 10, 130) -> (40,
15, 134), (3, 4, 7) -> the same, (324, 54, 1069) -> (320, 39, 1046), (21, 13, 71) -> the same: the 6x4 search without
fixing takes 39 or 40 nodes by the finishing order alone.  The searches that must reproduce today's counts run on
StreamingOracleLP, as tests/test_bnb_native_cpu.py's do."""
import math

import numpy as np
import pytest
from scipy.optimize import linprog

from golden_util import golden, payload
from gpu_cases import VARIANT
from oracle_lp import OracleLP, StreamingOracleLP

G = golden()
STEP1 = [n for n in ("syn_6x4_s1_r0.3_NeptuneMinDelayAndUtilization", "syn_8x4_s2_r0.1_NeptuneMinDelay",
                     "sim5_NeptuneMinUtilization", "syn_8x4_s3_r1.0_NeptuneMinUtilization") if n in G]
# (nodes, leaves, LPs) of the native search on the commit before rc_fixing existed
PARENT = {"syn_6x4_s1_r0.3_NeptuneMinDelayAndUtilization": (39, 10, 130), "syn_8x4_s2_r0.1_NeptuneMinDelay": (3, 4, 7),
          "sim5_NeptuneMinUtilization": (324, 54, 1069), "syn_8x4_s3_r1.0_NeptuneMinUtilization": (21, 13, 71)}


class _RcMixin:
    """Keeps each slot's node box and answers LPModel.rc_fixings' contract from HiGHS's marginals (linprog) of that
    node LP."""

    def submit(self, slots, lb=None, ub=None, **kw):
        if not hasattr(self, "_box"):
            self._box = {}
        for b, s in enumerate(np.asarray(slots).reshape(-1)):
            self._box[int(s)] = (None if lb is None else np.array(lb[b]), None if ub is None else np.array(ub[b]))
        return super().submit(slots, lb, ub, **kw)

    def copy_state(self, src, dst):
        super().copy_state(src, dst)
        if int(src) in getattr(self, "_box", {}):
            self._box[int(dst)] = self._box[int(src)]

    def node_lp(self, slot):
        """(L, d, lb, ub) of the slot's node LP: its value, the reduced costs of z_int, the node box of z_int"""
        m = self.m
        lbi, ubi = self._box[int(slot)]
        rl, ru = m["lb"].copy(), m["ub"].copy()
        if lbi is not None:
            fin = np.isfinite(lbi)
            rl[self.nx:][fin] = np.maximum(rl[self.nx:][fin], lbi[fin])
            fin = np.isfinite(ubi)
            ru[self.nx:][fin] = np.minimum(ru[self.nx:][fin], ubi[fin])
        A = m["A"].tocsr()
        lo, hi = np.asarray(m["lo"], float), np.asarray(m["hi"], float)
        eq = lo == hi
        up, dn = ~eq & np.isfinite(hi), ~eq & np.isfinite(lo)
        from scipy.sparse import vstack
        A_ub = vstack([A[up], -A[dn]]) if (up.any() or dn.any()) else None
        b_ub = np.concatenate([hi[up], -lo[dn]]) if A_ub is not None else None
        r = linprog(m["c"], A_ub=A_ub, b_ub=b_ub, A_eq=A[eq] if eq.any() else None, b_eq=lo[eq] if eq.any() else None,
                    bounds=np.column_stack([rl, ru]), method="highs")
        assert r.status == 0, r.message
        d = np.asarray(r.lower.marginals) + np.asarray(r.upper.marginals)
        return float(r.fun), d[self.nx:], rl[self.nx:], ru[self.nx:]

    def rc_fixings(self, slot, cutoff):
        L, d, lb, ub = self.node_lp(slot)
        # (HiGHS's duals carry ~1e-9 of noise: a margin of that size keeps the fixings valid)
        keep = (lb < ub) & (np.abs(d) > 1e-9) & (L + np.abs(d) * (ub - lb) > cutoff + 1e-9 * max(1.0, abs(cutoff)))
        idx = np.flatnonzero(keep).astype(np.int32)
        self.fix_log = getattr(self, "fix_log", []) + [(int(slot), float(cutoff), idx.copy())]
        return idx, np.where(d[idx] > 0, lb[idx], ub[idx])


class RcOracleLP(_RcMixin, StreamingOracleLP):
    pass


class RcPlainOracleLP(_RcMixin, OracleLP):
    pass


def _search(name, cls, **kw):
    from core.engine.bnb import BranchAndBound
    from core.utils import data_to_solver_input
    p = payload(name)
    data = data_to_solver_input(p, workload_coeff=p.get("workload_coeff", 1), with_db=False)
    lp = cls(data, VARIANT[p["solver"]["type"]], step=1, max_batch=6, alpha=p["solver"].get("args", {}).get("alpha", 0.5))
    res = BranchAndBound(lp, data.workload_matrix, data.function_memory_matrix, data.node_memory_matrix, batch=4,
                         node_limit=20000, native=True, **kw).solve()
    return res, lp


@pytest.fixture(scope="module")
def runs():
    """per instance: the search without the call, and with the call and fixing on (OracleLP: see the module's text)"""
    out = {}
    for name in STEP1:
        out[name] = (_search(name, OracleLP)[0],) + _search(name, RcPlainOracleLP, rc_fixing=True)
    return out


@pytest.mark.parametrize("name", STEP1)
def test_fixing_keeps_the_optimum_in_no_more_nodes(name, runs):
    off, on, lp = runs[name]
    rec = G[name]["models"][0]
    print(name, "off", (off.nodes, off.leaves, off.lps), off.rc, "on", (on.nodes, on.leaves, on.lps), on.rc)
    assert off.native and on.native
    assert off.rc == {"rc_fixed": 0, "rc_calls": 0, "rc_children_pruned": 0, "rc_leaves_dropped": 0}
    want = "OPTIMAL" if rec["status"] == 0 else "INFEASIBLE"
    assert off.status == on.status == want
    if rec["status"] == 0:
        assert abs(on.objective - rec["mip_objective"]) <= 1e-6 * max(1.0, abs(rec["mip_objective"]))
        assert abs(on.objective - off.objective) <= 1e-9 * max(1.0, abs(off.objective))
    assert on.nodes <= off.nodes
    # the tree asked once per branching node that branched with an incumbent known, and counted what it used
    assert on.rc["rc_calls"] == len(getattr(lp, "fix_log", []))
    assert on.rc["rc_fixed"] <= sum(len(i) for _, _, i in getattr(lp, "fix_log", []))


def test_some_instance_fixes_variables(runs):
    fixed = {name: r[1].rc["rc_fixed"] for name, r in runs.items()}
    print(fixed)
    # (sim5_NeptuneMinUtilization: the node count is the objective, so with the first incumbent every n whose
    # reduced cost is a whole node closes)
    assert max(fixed.values()) > 0, fixed


@pytest.mark.parametrize("name", STEP1)
def test_switched_off_or_without_the_call_the_search_is_todays(name):
    off = _search(name, StreamingOracleLP)[0]
    today = (off.nodes, off.leaves, off.lps, off.lp_status)
    assert today[:3] == PARENT[name]   # (the search before API 13, counted on its parent commit)
    # rc_fixing = 0 with the call in the table
    r0, lp0 = _search(name, RcOracleLP, rc_fixing=False)
    assert (r0.nodes, r0.leaves, r0.lps, r0.lp_status) == today
    assert not getattr(lp0, "fix_log", []) and r0.rc["rc_calls"] == 0
    # rc_fixing = 1 with a NULL call
    r1, _ = _search(name, StreamingOracleLP, rc_fixing=True)
    assert (r1.nodes, r1.leaves, r1.lps, r1.lp_status) == today
    assert r1.rc["rc_calls"] == 0 and r1.rc["rc_fixed"] == 0
    assert r0.objective == r1.objective == off.objective


def test_python_loop_ignores_rc_fixing_with_one_warning():
    import warnings
    from core.engine.bnb import BranchAndBound
    from core.utils import data_to_solver_input
    name = STEP1[0]
    p = payload(name)
    data = data_to_solver_input(p, workload_coeff=p.get("workload_coeff", 1), with_db=False)
    lp = StreamingOracleLP(data, VARIANT[p["solver"]["type"]], step=1, max_batch=6,
                           alpha=p["solver"].get("args", {}).get("alpha", 0.5))
    bb = BranchAndBound(lp, data.workload_matrix, data.function_memory_matrix, data.node_memory_matrix, batch=4,
                        node_limit=20000, native=False, rc_fixing=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = bb.solve()
        b = bb.solve()
    assert sum("rc_fixing" in str(x.message) for x in w) == 1
    assert a.status == b.status == "OPTIMAL" and not a.native and a.rc is None


def test_abi_13_layout():
    """API 13: rc_fixing takes reserved_p's place (nep_bnb_params keeps its size); the call table and the stats grow
    at the end only."""
    import ctypes
    from core.engine import lp as lpmod
    lib = lpmod.load_library()
    assert lib.nep_api_version() == lpmod.API_VERSION == 13
    P = lpmod.BnbParams
    assert P.rc_fixing.offset == P.strong_rel.offset + 4 and P.strong_iters.offset == P.rc_fixing.offset + 4
    assert [n for n, _ in lpmod.BnbEngine._fields_][-1] == "rc_fixings"
    assert [n for n, _ in lpmod.BnbStats._fields_][-4:-2] == ["rc_fixed", "rc_calls"]
    assert ctypes.sizeof(lpmod.BnbStats) % 8 == 0
    for sym in ("nep_lp_get_reduced_costs", "nep_lp_rc_fixings"):
        assert sym in lpmod.EXPORTS and getattr(lib, sym)
    assert math.isfinite(lib.nep_api_version())
