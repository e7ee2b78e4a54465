"""ctypes binding of the MI355X LP engine (`include/neptune_lp.h`, lib/libneptune_lp.so).

This is the product path: there is no CPU fallback.  If the shared library is missing (not built)
or no GPU is visible, every call raises `EngineUnavailable` loudly.
"""
import ctypes
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NEPTUNE_LP_LIB",
                          os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libneptune_lp.so")))

MIN_DELAY, MIN_UTILIZATION, MIN_DELAY_AND_UTILIZATION = 0, 1, 2
STEP1, STEP2_DELETE, STEP2_CREATE = 1, 2, 3
LP_OPTIMAL, LP_ITERATION_LIMIT, LP_INFEASIBLE, LP_CUTOFF, LP_NUMERICAL, LP_BOUND = 0, 1, 2, 3, 4, 5
VARIANTS = {"MinDelay": MIN_DELAY, "MinUtilization": MIN_UTILIZATION,
            "MinDelayAndUtilization": MIN_DELAY_AND_UTILIZATION}
API_VERSION = 13
RELAX_REFERENCE, RELAX_FACILITY = 0, 1
LEAF_EXACT, LEAF_FEASIBLE, LEAF_NO_POINT, LEAF_INFEASIBLE, LEAF_CUTOFF = 0, 1, 2, 3, 4
MOVE_ADD, MOVE_DROP, MOVE_CLOSE = 0, 1, 2
MOVE_SWAP = 3

_dp = ctypes.POINTER(ctypes.c_double)


class EngineUnavailable(RuntimeError):
    pass


class ModelDesc(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_int32), ("n_functions", ctypes.c_int32), ("variant", ctypes.c_int32),
                ("step", ctypes.c_int32), ("alpha", ctypes.c_double), ("soften_step1_sol", ctypes.c_double),
                ("max_score", ctypes.c_double), ("prev_network_delay", ctypes.c_double),
                ("big_m", ctypes.c_double), ("epsilon", ctypes.c_double),
                ("delay", _dp), ("workload", _dp), ("core_per_req", _dp), ("function_memory", _dp),
                ("node_memory", _dp), ("node_cores", _dp), ("node_cost", _dp), ("node_budget", ctypes.c_double),
                ("max_delay", _dp), ("old_allocations", _dp), ("relaxation", ctypes.c_int32),
                ("device_inputs", ctypes.c_int32)]


class LpOpts(ctypes.Structure):
    _fields_ = [("tol", ctypes.c_double), ("cutoff", ctypes.c_double), ("max_iters", ctypes.c_int64),
                ("check_every", ctypes.c_int32), ("warm_start", ctypes.c_int32),
                ("warm_omega_floor", ctypes.c_double), ("gap_tol", ctypes.c_double),
                ("warm_omega_cap", ctypes.c_double),
                ("polish_after", ctypes.c_double), ("bound_res", ctypes.c_double)]


class LeafOpts(ctypes.Structure):
    _fields_ = [("rounds", ctypes.c_int32), ("cutoff", ctypes.c_double), ("tol", ctypes.c_double)]


class LeafHeurOpts(ctypes.Structure):
    """nep_leaf_heur_opts: the evaluator's per-round repair on the device (nep_leaf_eval_ex)"""
    _fields_ = [("repair_every", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class LeafSearchOpts(ctypes.Structure):
    """nep_leaf_search_opts: the native placement search (nep_leaf_search)"""
    _fields_ = [(k, ctypes.c_int32) for k in ("rounds", "repair_every", "width", "swaps", "per_fn", "max_passes",
                                              "warm", "verify")] + [("time_limit", ctypes.c_double)]


class ModelInfo(ctypes.Structure):
    _fields_ = [("n_int", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("n_tiles", ctypes.c_int32),
                ("max_batch", ctypes.c_int32), ("x_entries", ctypes.c_int64), ("bytes_per_iter", ctypes.c_int64),
                ("step_size", ctypes.c_double), ("primal_weight0", ctypes.c_double)]


class Stats(ctypes.Structure):
    _fields_ = [("x_pass_launches", ctypes.c_int64), ("x_pass_ms", ctypes.c_double),
                ("x_pass_sampled", ctypes.c_int64), ("x_pass_lp_iters", ctypes.c_int64),
                ("solve_ms", ctypes.c_double), ("lp_iterations", ctypes.c_int64)]


class BnbParams(ctypes.Structure):
    _fields_ = [("c0", ctypes.c_int32), ("c1", ctypes.c_int32), ("n0", ctypes.c_int32), ("n1", ctypes.c_int32),
                ("n_int", ctypes.c_int32), ("F", ctypes.c_int32), ("N", ctypes.c_int32), ("warm", ctypes.c_int32),
                ("batch", ctypes.c_int32), ("batch_b", ctypes.c_int32),
                ("check_every", ctypes.c_int32), ("root_check_every", ctypes.c_int32),
                ("unit_flow_leaves", ctypes.c_int32), ("objective_integral", ctypes.c_int32),
                ("primal_at_root", ctypes.c_int32), ("tol", ctypes.c_double), ("gap", ctypes.c_double),
                ("bound_gap", ctypes.c_double), ("max_iters", ctypes.c_int64), ("node_max_iters", ctypes.c_int64),
                ("root_max_iters", ctypes.c_int64), ("node_bound_res", ctypes.c_double),
                ("retry_res", ctypes.c_double), ("flow_tol", ctypes.c_double), ("upper_bound", ctypes.c_double),
                ("node_limit", ctypes.c_int64), ("time_limit", ctypes.c_double),
                ("world", ctypes.c_int32), ("rank", ctypes.c_int32), ("branching", ctypes.c_int32),
                ("strong_cands", ctypes.c_int32), ("strong_rel", ctypes.c_int32), ("rc_fixing", ctypes.c_int32),
                ("strong_iters", ctypes.c_int64), ("objective_unit", ctypes.c_double),
                ("leaf_eval", ctypes.c_int32), ("leaf_rounds", ctypes.c_int32)]


class LeafStats(ctypes.Structure):
    """nep_bnb_leaf_stats: the native tree's use of the fixed-placement evaluator"""
    _fields_ = [(k, ctypes.c_int64) for k in ("leaf_eval_calls", "leaf_eval_leaves", "leaf_eval_exact",
                                              "leaf_eval_feasible", "leaf_eval_dropped", "leaf_eval_incumbents")] + \
               [("leaf_eval_seconds", ctypes.c_double)]


class BnbStats(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int64) for k in ("nodes", "leaves", "lps", "certified", "lp_iterations", "unresolved",
                                              "drained")] + \
               [("lp_status", ctypes.c_int64 * 7), ("lp_status_kind", (ctypes.c_int64 * 7) * 4)] + \
               [(k, ctypes.c_int64) for k in ("advance_calls", "inflight_sum", "lp_incumbents", "heuristic_incumbents",
                                              "n_lp_iters")] + \
               [(k, ctypes.c_double) for k in ("advance_seconds", "finish_seconds", "submit_seconds", "drain_seconds",
                                               "root_seconds", "bound", "incumbent")] + \
               [(k, ctypes.c_int32) for k in ("incumbent_source", "incumbent_slot", "limit_hit", "any_unresolved",
                                              "unresolved_below", "stalled")] + \
               [("split_hash", ctypes.c_uint32), ("reserved_", ctypes.c_int32)] + \
               [(k, ctypes.c_int64) for k in ("presplit_nodes", "presplit_lps", "presplit_certified", "rebalanced",
                                              "sync_calls")] + \
               [("agreed_incumbent", ctypes.c_double)] + \
               [(k, ctypes.c_int64) for k in ("strong_nodes", "strong_lps", "strong_iterations", "strong_decided",
                                              "rc_fixed", "rc_calls", "rc_children_pruned", "rc_leaves_dropped")]


# nep_bnb_engine (API 12): the calls the native tree makes on one model
_i32p, _i64p, _dblp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
_fltp = ctypes.POINTER(ctypes.c_float)
BNB_SUBMIT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, _i32p, _dblp, _dblp,
                              ctypes.POINTER(LpOpts), _i32p)
BNB_ADVANCE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, _i32p, _i32p, _dblp, _dblp, _i32p,
                               _i64p)
BNB_ACTIVE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)
BNB_COPY = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32)
BNB_PARAMS = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_double)
BNB_FLOWS = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, _i32p, _fltp)
BNB_SOLS = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, _i32p, _dblp)
BNB_DIAG = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, _dblp)
BNB_COPIES = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, _i32p, _i32p)
BNB_FLOWS_SOLS = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, _i32p, _fltp, _dblp)
BNB_SUBMIT_EX = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, _i32p, _dblp, _dblp,
                                 ctypes.POINTER(LpOpts), _i64p, _dblp, _i32p)
BNB_RC_FIX = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int64, _i64p,
                              _i32p, _dblp)
BNB_LEAF_EVAL = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, _dblp, ctypes.POINTER(LeafOpts), _dblp,
                                 _dblp, _dblp, _i32p, _dblp, _dblp)
BNB_LEAF_ROUTING = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, _i64p, _i32p, _i32p,
                                    _dblp)


class BnbEngine(ctypes.Structure):
    _fields_ = [("ctx", ctypes.c_void_p), ("n_int", ctypes.c_int32), ("max_batch", ctypes.c_int32),
                ("submit", BNB_SUBMIT), ("advance", BNB_ADVANCE), ("active", BNB_ACTIVE), ("copy_state", BNB_COPY),
                ("set_params", BNB_PARAMS), ("get_flows", BNB_FLOWS), ("get_solutions", BNB_SOLS),
                ("get_diag", BNB_DIAG), ("submit_ex", BNB_SUBMIT_EX), ("copy_states", BNB_COPIES),
                ("get_flows_solutions", BNB_FLOWS_SOLS), ("rc_fixings", BNB_RC_FIX)]


class PyBnbEngine:
    """A nep_bnb_engine call table over a Python model with LPModel's streaming interface (submit / advance /
    active / copy_state / set_params / flows / solutions / diag, n_int, max_batch): lets the native tree search
    (csrc/nep_bnb.cpp, nep_bnb_create_engines) drive node LPs that are not the engine's — the CPU suite runs it
    over HiGHS (tests/oracle_lp.py).  A Python exception inside a call ends the search with NEP_ERR_STATE and is
    kept in `error` (BranchAndBound re-raises it).  A model with an rc_fixings(slot, cutoff) -> (idx, val) method
    (LPModel.rc_fixings' contract) gives the tree its optional rc_fixings call, unless rc_fixings=False."""

    def __init__(self, model, F, N, per_lp=True, rc_fixings=True, leaf_eval=True):
        self.model, self.F, self.N = model, int(F), int(N)
        self.n_int, self.max_batch = int(model.n_int), int(model.max_batch)
        self.error = None
        self.ex_calls = 0
        self.copies_calls = 0
        self.flows_sols_calls = 0
        self.rc_calls = 0
        ni, mb = self.n_int, self.max_batch
        A = np.ctypeslib.as_array

        def guard(fn):
            def call(*args):
                try:
                    fn(*args)
                    return 0
                except BaseException as e:      # (never unwind through the C frames)
                    self.error = e
                    return -4
            return call

        def submit(_, n, slots, lb, ub, opts, status):
            o = opts.contents
            st = model.submit(A(slots, (n,)).copy(), A(lb, (n, ni)).copy(), A(ub, (n, ni)).copy(), tol=o.tol,
                              cutoff=o.cutoff, max_iters=int(o.max_iters), check_every=int(o.check_every),
                              warm_start=bool(o.warm_start), bound_res=o.bound_res, gap_tol=o.gap_tol)
            A(status, (n,))[:] = np.asarray(st, np.int32)

        def submit_ex(_, n, slots, lb, ub, opts, mi, br, status):
            # per-LP budgets / bound stops: one model.submit per distinct (budget, bound stop), in first-seen order
            o = opts.contents
            sl, lbs, ubs = A(slots, (n,)).copy(), A(lb, (n, ni)).copy(), A(ub, (n, ni)).copy()
            mis = A(mi, (n,)).copy() if mi else np.full(n, o.max_iters, np.int64)
            brs = A(br, (n,)).copy() if br else np.full(n, o.bound_res)
            keys = list(dict.fromkeys(zip(mis.tolist(), brs.tolist())))
            out = A(status, (n,))
            for k_mi, k_br in keys:
                sel = np.flatnonzero((mis == k_mi) & (brs == k_br))
                st = model.submit(sl[sel], lbs[sel], ubs[sel], tol=o.tol, cutoff=o.cutoff,
                                  max_iters=int(k_mi) if k_mi > 0 else int(o.max_iters),
                                  check_every=int(o.check_every), warm_start=bool(o.warm_start),
                                  bound_res=max(float(k_br), 0.0), gap_tol=o.gap_tol)
                out[sel] = np.asarray(st, np.int32)
            self.ex_calls += 1

        def advance(_, min_done, n_done, slots, obj, pobj, status, iters):
            r = model.advance(int(min_done))
            k = len(r["slots"])
            n_done[0] = k
            if k:
                A(slots, (mb,))[:k] = r["slots"]
                A(obj, (mb,))[:k] = r["obj"]
                A(pobj, (mb,))[:k] = r["primal_obj"]
                A(status, (mb,))[:k] = r["status"]
                A(iters, (mb,))[:k] = r["iters"]

        def copy_state(_, src, dst):
            model.copy_state(int(src), int(dst))

        def copy_states(_, n, src, dst):
            # (the Python model copies pair by pair, in order: the contract of nep_lp_copy_states)
            for a, b in zip(A(src, (n,)).tolist(), A(dst, (n,)).tolist()):
                model.copy_state(int(a), int(b))
            self.copies_calls += 1

        def set_params(_, tol, cutoff):
            model.set_params(tol, cutoff)

        def flows(_, n, slots, out):
            A(out, (n * self.F * self.N,))[:] = np.asarray(model.flows(A(slots, (n,)).copy()), np.float32).ravel()

        def sols(_, n, slots, out):
            A(out, (n * ni,))[:] = np.asarray(model.solutions(A(slots, (n,)).copy()), np.float64).ravel()

        def flows_sols(_, n, slots, fout, zout):
            flows(_, n, slots, fout)
            sols(_, n, slots, zout)
            self.flows_sols_calls += 1

        def diag(_, slot, out):
            d = model.diag(int(slot))
            o = A(out, (16,))
            o[:] = 0.0
            o[3] = float(d.get("pres", 0.0))

        def rc_fix(_, slot, cutoff, capacity, n_fix, idx, val):
            ki, kv = model.rc_fixings(int(slot), float(cutoff))
            k = len(ki)
            n_fix[0] = k
            if k and capacity >= k:
                A(idx, (k,))[:] = np.asarray(ki, np.int32)
                A(val, (k,))[:] = np.asarray(kv, np.float64)
            self.rc_calls += 1

        def active(_):
            try:
                return int(model.active())
            except BaseException as e:
                self.error = e
                return 0

        # the fixed-placement evaluator pair (nep_bnb_set_leaf_engine) of a model with leaf_eval(z, rounds, cutoff) ->
        # dict(lower, upper, status) and leaf_routing(k) -> (row, dst, val) (LPModel's contracts), unless leaf_eval=False
        self.leaf_calls = 0
        self.leaf_pair = None

        def leaf_ev(_, n, z, opts, pin, lower, upper, status, pout, cpu):
            o = opts.contents
            r = model.leaf_eval(A(z, (n, ni)).copy(), rounds=int(o.rounds), cutoff=float(o.cutoff))
            A(lower, (n,))[:] = r["lower"]
            A(upper, (n,))[:] = r["upper"]
            A(status, (n,))[:] = np.asarray(r["status"], np.int32)
            self.leaf_calls += 1

        def leaf_rt(_, k, capacity, n_entries, row, dst, val):
            r, d, v = model.leaf_routing(int(k))
            cnt = len(r)
            n_entries[0] = cnt
            if cnt and capacity >= cnt:
                A(row, (cnt,))[:] = np.asarray(r, np.int32)
                A(dst, (cnt,))[:] = np.asarray(d, np.int32)
                A(val, (cnt,))[:] = np.asarray(v, np.float64)

        if leaf_eval and hasattr(model, "leaf_eval") and hasattr(model, "leaf_routing"):
            self.leaf_pair = (BNB_LEAF_EVAL(guard(leaf_ev)), BNB_LEAF_ROUTING(guard(leaf_rt)))
        self.table = BnbEngine(None, ni, mb, BNB_SUBMIT(guard(submit)), BNB_ADVANCE(guard(advance)),
                               BNB_ACTIVE(active), BNB_COPY(guard(copy_state)), BNB_PARAMS(guard(set_params)),
                               BNB_FLOWS(guard(flows)), BNB_SOLS(guard(sols)), BNB_DIAG(guard(diag)),
                               BNB_SUBMIT_EX(guard(submit_ex)) if per_lp else BNB_SUBMIT_EX(),
                               BNB_COPIES(guard(copy_states)) if per_lp else BNB_COPIES(),
                               BNB_FLOWS_SOLS(guard(flows_sols)) if per_lp else BNB_FLOWS_SOLS(),
                               BNB_RC_FIX(guard(rc_fix)) if rc_fixings and hasattr(model, "rc_fixings")
                               else BNB_RC_FIX())


# every entry point declared in include/neptune_lp.h
EXPORTS = ("nep_model_create", "nep_model_destroy", "nep_model_get_info", "nep_lp_solve_batch",
           "nep_lp_submit", "nep_lp_submit_ex", "nep_lp_advance", "nep_lp_active", "nep_lp_copy_states", "nep_lp_get_flows_solutions",
           "nep_lp_get_solution", "nep_lp_get_rows", "nep_lp_copy_state", "nep_get_stats", "nep_reset_stats",
           "nep_lp_get_flows_split",
           "nep_last_error", "nep_api_version", "nep_lp_get_diag", "nep_debug_build", "nep_debug_state",
           "nep_debug_presolve", "nep_debug_sparse_rows", "nep_lp_set_params", "nep_lp_get_flows", "nep_lp_routing_entries",
           "nep_lp_allocation_entries", "nep_lp_score_check", "nep_round_leaf", "nep_lp_copy_routing",
           "nep_lp_get_solutions", "nep_round_leaves", "nep_lp_set_reference_weight",
           "nep_bnb_create", "nep_bnb_destroy", "nep_bnb_add_leaf", "nep_bnb_set_incumbent", "nep_bnb_event_data",
           "nep_bnb_run", "nep_bnb_get_stats", "nep_bnb_get_lp_iters", "nep_bnb_incumbent", "nep_bnb_set_step2",
           "nep_bnb_incumbent_event", "nep_bnb_debug_ibound", "nep_bnb_create_engines", "nep_bnb_sync_get",
           "nep_bnb_sync_set", "nep_bnb_export_nodes", "nep_bnb_import_nodes", "nep_lp_get_reduced_costs",
           "nep_lp_rc_fixings", "nep_debug_block_split", "nep_leaf_eval", "nep_leaf_routing_entries",
           "nep_debug_leaf_repair", "nep_bnb_set_leaf_engine", "nep_bnb_get_leaf_stats", "nep_bnb_incumbent_routing",
           "nep_leaf_eval_ex", "nep_debug_leaf_repair_from", "nep_leaf_moves", "nep_debug_leaf_move_list",
           "nep_debug_fac_state", "nep_leaf_swaps", "nep_debug_leaf_swap_list", "nep_leaf_search",
           "nep_debug_leaf_apply_move", "nep_debug_leaf_expand")
SCORE_FIELDS = ("network_delay", "nodes_used", "node_cost", "bad_c_x", "bad_memory", "bad_handle", "bad_cpu",
                "bad_n_c", "bad_budget", "handle_maxdev", "cpu_maxexcess")

_lib = None


def _host_inputs():
    return os.environ.get("NEP_HOST_INPUTS", "0") not in ("", "0")


def load_library(path=None):
    """Load (once) and type the shared library.  Raises EngineUnavailable when absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise EngineUnavailable(f"MI355X LP engine not built: {p} missing (run __graft_entry__.build())")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (soname libamdhip64.so.7), loaded
    # by file name.  Loaded first, it satisfies the engine's libamdhip64.so.7 dependency; loaded after the
    # engine's /opt/rocm copy, the process holds two runtimes and the second to initialise sees no device.
    # (NEP_HOST_INPUTS=1: host-array descriptors and no PyTorch, the engine on /opt/rocm's runtime — for A/B)
    if not _host_inputs():
        import torch  # noqa: F401
    lib = ctypes.CDLL(p)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    pi32, pi64 = ctypes.POINTER(i32), ctypes.POINTER(i64)
    lib.nep_model_create.argtypes = [ctypes.POINTER(ModelDesc), i32, vp, ctypes.POINTER(vp)]
    lib.nep_model_destroy.argtypes = [vp]
    lib.nep_model_destroy.restype = None
    lib.nep_model_get_info.argtypes = [vp, ctypes.POINTER(ModelInfo)]
    lib.nep_lp_solve_batch.argtypes = [vp, i32, ctypes.POINTER(i32), _dp, _dp, ctypes.POINTER(LpOpts), _dp, _dp,
                                       ctypes.POINTER(i32), ctypes.POINTER(i64)]
    lib.nep_lp_submit.argtypes = [vp, i32, pi32, _dp, _dp, ctypes.POINTER(LpOpts), pi32]
    lib.nep_lp_submit_ex.argtypes = [vp, i32, pi32, _dp, _dp, ctypes.POINTER(LpOpts), pi64, _dp, pi32]
    lib.nep_lp_advance.argtypes = [vp, i32, pi32, pi32, _dp, _dp, pi32, pi64]
    lib.nep_lp_active.argtypes = [vp]
    lib.nep_lp_get_solution.argtypes = [vp, i32, _dp, ctypes.POINTER(ctypes.c_float)]
    lib.nep_lp_get_rows.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(i32),
                                    ctypes.POINTER(i32)]
    lib.nep_lp_copy_state.argtypes = [vp, i32, i32]
    lib.nep_lp_copy_states.argtypes = [vp, i32, vp, vp]
    lib.nep_lp_get_flows_solutions.argtypes = [vp, i32, vp, vp, vp]
    lib.nep_lp_copy_routing.argtypes = [vp, i32, vp, i32]
    lib.nep_lp_get_solutions.argtypes = [vp, i32, pi32, _dp]
    lib.nep_lp_get_reduced_costs.argtypes = [vp, i32, pi32, _dp, _dp]
    lib.nep_lp_rc_fixings.argtypes = [vp, i32, ctypes.c_double, i64, pi64, pi32, _dp]
    lib.nep_round_leaves.argtypes = [i32, i32, _dp, _dp, ctypes.POINTER(ctypes.c_float), _dp, _dp, _dp, i32, pi32, _dp,
                                     _dp, _dp, pi32]
    lib.nep_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    lib.nep_reset_stats.argtypes = [vp]
    lib.nep_reset_stats.restype = None
    lib.nep_lp_get_diag.argtypes = [vp, i32, _dp]
    lib.nep_debug_sparse_rows.argtypes = [vp, i32, vp, vp]
    lib.nep_debug_fac_state.argtypes = [vp, i32, vp, vp, vp]
    lib.nep_debug_build.argtypes = [ctypes.POINTER(ModelDesc), _dp, _dp, _dp, _dp, ctypes.POINTER(i32)]
    lib.nep_debug_state.argtypes = [vp, i32, _dp, _dp, ctypes.POINTER(ctypes.c_float), _dp, _dp]
    lib.nep_debug_presolve.argtypes = [ctypes.POINTER(ModelDesc), i32, _dp, _dp, pi32, pi32, _dp, _dp]
    lib.nep_lp_set_params.argtypes = [vp, ctypes.c_double, ctypes.c_double]
    lib.nep_lp_set_reference_weight.argtypes = [vp, ctypes.c_double]
    lib.nep_bnb_create.argtypes = [vp, vp, ctypes.POINTER(BnbParams), _dp, _dp]
    lib.nep_bnb_create.restype = vp
    lib.nep_bnb_destroy.argtypes = [vp]
    lib.nep_bnb_destroy.restype = None
    lib.nep_bnb_add_leaf.argtypes = [vp, i32, pi32, _dp, ctypes.c_double, i32]
    lib.nep_bnb_set_incumbent.argtypes = [vp, ctypes.c_double]
    lib.nep_bnb_event_data.argtypes = [vp, _dp, ctypes.POINTER(ctypes.c_float)]
    lib.nep_bnb_run.argtypes = [vp, pi32]
    lib.nep_bnb_get_stats.argtypes = [vp, ctypes.POINTER(BnbStats)]
    lib.nep_bnb_get_lp_iters.argtypes = [vp, pi64]
    lib.nep_bnb_incumbent.argtypes = [vp, _dp, pi32, pi32, _dp]
    lib.nep_bnb_set_step2.argtypes = [vp, i32, ctypes.c_double, _dp, i32]
    lib.nep_bnb_set_leaf_engine.argtypes = [vp, vp, BNB_LEAF_EVAL, BNB_LEAF_ROUTING]
    lib.nep_bnb_get_leaf_stats.argtypes = [vp, ctypes.POINTER(LeafStats)]
    lib.nep_bnb_incumbent_routing.argtypes = [vp, i64, pi64, pi32, pi32, _dp]
    lib.nep_bnb_incumbent_event.argtypes = [vp, pi32, pi32, _dp, _dp]
    lib.nep_bnb_debug_ibound.argtypes = [ctypes.POINTER(BnbParams), i32, ctypes.c_double, _dp, i32, pi32, _dp, _dp]
    lib.nep_bnb_create_engines.argtypes = [ctypes.POINTER(BnbEngine), ctypes.POINTER(BnbEngine),
                                           ctypes.POINTER(BnbParams), _dp, _dp]
    lib.nep_bnb_create_engines.restype = vp
    lib.nep_bnb_sync_get.argtypes = [vp, _dp]
    lib.nep_bnb_sync_set.argtypes = [vp, ctypes.c_double, i32, i64]
    lib.nep_bnb_export_nodes.argtypes = [vp, i32, i32, pi32, _dp, pi32, _dp]
    lib.nep_bnb_import_nodes.argtypes = [vp, i32, pi32, _dp, pi32, _dp]
    lib.nep_lp_get_flows.argtypes = [vp, i32, pi32, ctypes.POINTER(ctypes.c_float)]
    lib.nep_lp_get_flows_split.argtypes = [vp, i32, pi32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    lib.nep_lp_routing_entries.argtypes = [vp, i32, ctypes.c_double, i32, i64, pi64, pi32, pi32, _dp]
    lib.nep_lp_allocation_entries.argtypes = [vp, i32, ctypes.c_double, i64, pi64, pi32, pi32]
    lib.nep_lp_score_check.argtypes = [vp, i32, _dp]
    lib.nep_round_leaf.argtypes = [i32, i32, _dp, _dp, ctypes.POINTER(ctypes.c_float), _dp, _dp, _dp, i32,
                                   ctypes.c_double, _dp, _dp]
    lib.nep_leaf_eval.argtypes = [vp, i32, _dp, ctypes.POINTER(LeafOpts), _dp, _dp, _dp, pi32, _dp, _dp]
    lib.nep_leaf_routing_entries.argtypes = [vp, i32, i64, pi64, pi32, pi32, _dp]
    lib.nep_debug_leaf_repair.argtypes = [ctypes.POINTER(ModelDesc), _dp, pi32, _dp, pi32, i64, pi64, pi32, pi32, _dp,
                                          _dp]
    lib.nep_leaf_eval_ex.argtypes = [vp, i32, _dp, ctypes.POINTER(LeafOpts), ctypes.POINTER(LeafHeurOpts), _dp, _dp,
                                     _dp, pi32, _dp, _dp, pi32, _dp, _dp]
    lib.nep_debug_leaf_repair_from.argtypes = [ctypes.POINTER(ModelDesc), _dp, pi32, _dp, _dp, pi32, i64, pi64, pi32,
                                               pi32, _dp, _dp]
    lib.nep_leaf_moves.argtypes = [vp, i32, _dp, _dp, i32, pi32, pi32, pi32, pi32, _dp, _dp, _dp]
    lib.nep_debug_leaf_move_list.argtypes = [ctypes.POINTER(ModelDesc), _dp, _dp, i32, pi32, pi32, pi32, pi32, _dp]
    lib.nep_leaf_swaps.argtypes = [vp, i32, _dp, _dp, i32, i32, pi32, pi32, pi32, pi32, _dp, _dp, _dp, pi32]
    lib.nep_debug_leaf_swap_list.argtypes = [i32, i32, _dp, pi32, i32, i32, pi32, pi32, pi32, pi32, _dp]
    lib.nep_leaf_search.argtypes = [vp, _dp, ctypes.POINTER(LeafSearchOpts), _dp, _dp, _dp, _dp, _dp, pi32, pi64, pi64,
                                    pi32, pi32, pi32, pi32, pi32, _dp, _dp]
    lib.nep_debug_leaf_apply_move.argtypes = [i32, i32, i32, _dp, i32, i32, i32, i32, _dp]
    lib.nep_debug_leaf_expand.argtypes = [vp, _dp, i32, pi32, pi32, pi32, pi32, vp, _dp]
    lib.nep_last_error.restype = ctypes.c_char_p
    lib.nep_api_version.restype = ctypes.c_int
    # array arguments travel as plain addresses (_ptr: the array's data pointer as an int): ctypes' typed
    # pointer casts cost ~2 us each, ~10 % of the B&B's host time at 64x32 (tools/probes/bnb_profile.py)
    scalar_ptrs = tuple(ctypes.POINTER(t) for t in (ctypes.c_double, ctypes.c_float, ctypes.c_int32, ctypes.c_int64))
    for name in EXPORTS:
        if name == "nep_debug_block_split":    # (typed at its call, debug_block_split)
            continue
        fn = getattr(lib, name)
        if fn.argtypes:
            fn.argtypes = [ctypes.c_void_p if t in scalar_ptrs else t for t in fn.argtypes]
    if lib.nep_api_version() != API_VERSION:
        raise EngineUnavailable(f"{p}: API version {lib.nep_api_version()} != {API_VERSION} (rebuild the engine)")
    if path is None:
        _lib = lib
    return lib


def round_leaf(c_fix, n_fix, flow, zc, fn_mem, node_mem, by_flow, flow_threshold):
    """The B&B rounding heuristic (nep_round_leaf, host code of the engine library): c_fix [F, N] / n_fix [N]
    (None: no n) with -1 free and 0 / 1 fixed, flow [F, N], zc [F, N] (None: 0).  Returns (c [F*N], n [N] or
    None) or None when the node has no leaf."""
    lib = load_library()
    c_fix = np.ascontiguousarray(c_fix, np.float64)
    F, N = c_fix.shape
    nf = None if n_fix is None else np.ascontiguousarray(n_fix, np.float64)
    fl = np.ascontiguousarray(flow, np.float32)
    zcv = None if zc is None else np.ascontiguousarray(zc, np.float64)
    fm = np.ascontiguousarray(fn_mem, np.float64)
    nm = np.ascontiguousarray(node_mem, np.float64)
    c_out = np.zeros(F * N)
    n_out = None if nf is None else np.zeros(N)
    rc = lib.nep_round_leaf(F, N, _ptr(c_fix), _ptr(nf), _ptr(fl, ctypes.c_float), _ptr(zcv), _ptr(fm), _ptr(nm),
                            1 if by_flow else 0, float(flow_threshold), _ptr(c_out), _ptr(n_out))
    if rc < 0:
        raise EngineUnavailable(f"nep_round_leaf failed ({rc})")
    return (c_out, n_out) if rc == 1 else None


def round_leaves(c_fix, n_fix, flow, zc, fn_mem, node_mem, modes):
    """round_leaf for several (by_flow, flow_threshold) modes of one node in one call (nep_round_leaves):
    [(c, n or None) or None per mode]."""
    lib = load_library()
    c_fix = np.ascontiguousarray(c_fix, np.float64)
    F, N = c_fix.shape
    k = len(modes)
    nf = None if n_fix is None else np.ascontiguousarray(n_fix, np.float64)
    fl = np.ascontiguousarray(flow, np.float32)
    zcv = None if zc is None else np.ascontiguousarray(zc, np.float64)
    bf = np.array([1 if m[0] else 0 for m in modes], np.int32)
    th = np.array([float(m[1]) for m in modes], np.float64)
    # (every converted array is bound to a local first: _ptr passes a raw address, which does not keep a
    # temporary copy alive through the call)
    fm = np.ascontiguousarray(fn_mem, np.float64)
    nm = np.ascontiguousarray(node_mem, np.float64)
    c_out = np.zeros((k, F * N))
    n_out = None if nf is None else np.zeros((k, N))
    found = np.zeros(k, np.int32)
    rc = lib.nep_round_leaves(F, N, _ptr(c_fix), _ptr(nf), _ptr(fl), _ptr(zcv), _ptr(fm), _ptr(nm), k, _ptr(bf),
                              _ptr(th), _ptr(c_out), _ptr(n_out), _ptr(found))
    if rc < 0:
        raise EngineUnavailable(f"nep_round_leaves failed ({rc})")
    return [((c_out[q], None if n_out is None else n_out[q]) if found[q] else None) for q in range(k)]


def _ptr(a, ctype=ctypes.c_double):
    """The data address of a C-contiguous numpy array (the library's array arguments are void*), or None.
    (ctype documents the element type the C side reads.)"""
    return None if a is None else a.ctypes.data


def _check(lib, rc, what):
    if rc != 0:
        raise EngineUnavailable(f"{what} failed ({rc}): {lib.nep_last_error().decode()}")


def _arrays(data, N, F):
    f64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return dict(
        delay=f64(data.node_delay_matrix).reshape(N, N),
        workload=f64(data.workload_matrix).reshape(F, N),
        cpr=f64(data.core_per_req_matrix).reshape(F, N),
        fmem=f64(data.function_memory_matrix).reshape(F),
        nmem=f64(data.node_memory_matrix).reshape(N),
        ncores=f64(data.node_cores_matrix).reshape(N),
        ncost=f64(data.node_costs).reshape(N),
        maxd=f64(data.max_delay_matrix).reshape(F),
        old=f64(data.old_allocations_matrix).reshape(F, N),
    )


def _desc(k, N, F, variant, step, alpha, soften, max_score, prev_delay, budget, relaxation=RELAX_REFERENCE):
    """The model descriptor over host numpy arrays, or (API 9, device_inputs = 1) over the device memory of
    PyTorch-ROCm tensors (instance_tensors)."""
    dev = not isinstance(k["delay"], np.ndarray)

    def dp(a):   # (structure fields keep their typed pointers)
        return ctypes.cast(ctypes.c_void_p(a.data_ptr()), _dp) if dev else a.ctypes.data_as(_dp)
    return ModelDesc(N, F, variant, step, float(alpha), float(soften), float(max_score), float(prev_delay), 1e6,
                     1e-6, dp(k["delay"]), dp(k["workload"]), dp(k["cpr"]), dp(k["fmem"]), dp(k["nmem"]),
                     dp(k["ncores"]), dp(k["ncost"]), float(budget), dp(k["maxd"]), dp(k["old"]),
                     int(relaxation), 1 if dev else 0)


def instance_tensors(data, device=None):
    """The instance of a Data (core/utils/data.py; input_to_data.py:88-111) as contiguous float64 PyTorch-ROCm
    tensors on the GPU — the constraint data the engine's models are built from (nep_model_desc.device_inputs):
    D [N, N], W [F, N], core_per_req [F, N], function memory [F], node memory / cores / costs [N], max delay
    [F], old allocations [F, N].  Requires a GPU (the product path has no CPU fallback)."""
    import torch
    if not torch.cuda.is_available():
        raise EngineUnavailable("no GPU visible: the engine's instance tensors live on the device")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    host = _arrays(data, len(data.nodes), len(data.functions))
    out = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in host.items()}
    torch.cuda.synchronize(dev)   # (the library reads them on its own streams)
    return out


def debug_build(data, variant, step=STEP1, alpha=0.5, soften_step1_sol=1.3, max_score=0.0, prev_network_delay=0.0,
                relaxation=RELAX_REFERENCE):
    """Host-only model build (no GPU needed): returns eta, rho, gam, rownorm, dims."""
    lib = load_library()
    N, F = len(data.nodes), len(data.functions)
    v = VARIANTS[variant] if isinstance(variant, str) else int(variant)
    k = _arrays(data, N, F)
    d = _desc(k, N, F, v, int(step), alpha, soften_step1_sol, max_score, prev_network_delay, data.node_budget,
              relaxation)
    dims = np.zeros(4, np.int32)
    eta = np.zeros(1)
    _check(lib, lib.nep_debug_build(ctypes.byref(d), _ptr(eta), None, None, None, _ptr(dims, ctypes.c_int32)),
           "nep_debug_build")
    R, T, n_int, n_dual = dims.tolist()
    rho, gam, rn = np.zeros(n_dual), np.zeros(n_int), np.zeros(n_dual)
    _check(lib, lib.nep_debug_build(ctypes.byref(d), _ptr(eta), _ptr(rho), _ptr(gam), _ptr(rn), None),
           "nep_debug_build")
    return {"eta": float(eta[0]), "rho": rho, "gam": gam, "rownorm": rn, "R": R, "T": T, "n_int": n_int,
            "n_dual": n_dual}


def debug_leaf_repair(data, variant, z, asg, alpha=0.5, load=None):
    """Host-only (no GPU needed): the fixed-placement evaluator's repair (nep_debug_leaf_repair) of the step-1
    placement z [n_int] from the assignment asg [R] (a destination per loaded routing row).  load [N] (None: summed
    from asg in row order): the CPU loads of asg the moves start from (nep_debug_leaf_repair_from), as the evaluator
    repairs a later round from that round's loads.  Returns (found, upper, (row, dst, val), cpu [N])."""
    lib = load_library()
    N, F = len(data.nodes), len(data.functions)
    v = VARIANTS[variant] if isinstance(variant, str) else int(variant)
    k = _arrays(data, N, F)
    d = _desc(k, N, F, v, STEP1, alpha, 1.3, 0.0, 0.0, data.node_budget)
    z = np.ascontiguousarray(z, np.float64)
    asg = np.ascontiguousarray(asg, np.int32)
    upper, found, cnt = np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int64)
    cpu = np.zeros(N)
    if load is None:
        def call(cap, row, dst, val):
            return lib.nep_debug_leaf_repair(ctypes.byref(d), _ptr(z), _ptr(asg, ctypes.c_int32), _ptr(upper),
                                             _ptr(found, ctypes.c_int32), cap, _ptr(cnt, ctypes.c_int64), row, dst,
                                             val, _ptr(cpu))
        name = "nep_debug_leaf_repair"
    else:
        load = np.ascontiguousarray(np.asarray(load, np.float64).reshape(N))

        def call(cap, row, dst, val):
            return lib.nep_debug_leaf_repair_from(ctypes.byref(d), _ptr(z), _ptr(asg, ctypes.c_int32), _ptr(load),
                                                  _ptr(upper), _ptr(found, ctypes.c_int32), cap,
                                                  _ptr(cnt, ctypes.c_int64), row, dst, val, _ptr(cpu))
        name = "nep_debug_leaf_repair_from"
    _check(lib, call(0, None, None, None), name)
    n = int(cnt[0])
    row, dst, val = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
    if n:
        _check(lib, call(n, _ptr(row, ctypes.c_int32), _ptr(dst, ctypes.c_int32), _ptr(val)), name)
    return bool(found[0]), float(upper[0]), (row, dst, val), cpu


def debug_leaf_move_list(data, variant, z, table, max_moves, alpha=0.5, step=STEP1, relaxation=RELAX_REFERENCE,
                         max_score=0.0):
    """Host-only (no GPU needed): the move list (nep_debug_leaf_move_list) of the step-1 placement z [n_int] from its
    priced table [F, N] (nep_leaf_moves' composition, screens and order).  Returns dict(n_moves, kind, fn, node, delta)
    with the arrays cut to n_moves."""
    lib = load_library()
    N, F = len(data.nodes), len(data.functions)
    v = VARIANTS[variant] if isinstance(variant, str) else int(variant)
    k = _arrays(data, N, F)
    d = _desc(k, N, F, v, int(step), alpha, 1.3, max_score, 0.0, data.node_budget, relaxation)
    z = np.ascontiguousarray(z, np.float64)
    table = None if table is None else np.ascontiguousarray(np.asarray(table, np.float64).reshape(F, N))
    mm = int(max_moves)
    cnt = np.zeros(1, np.int32)
    kind, fn, node = (np.zeros(max(mm, 0), np.int32) for _ in range(3))
    delta = np.zeros(max(mm, 0))
    _check(lib, lib.nep_debug_leaf_move_list(ctypes.byref(d), _ptr(z), _ptr(table), mm, _ptr(cnt, ctypes.c_int32),
                                             _ptr(kind, ctypes.c_int32), _ptr(fn, ctypes.c_int32),
                                             _ptr(node, ctypes.c_int32), _ptr(delta)), "nep_debug_leaf_move_list")
    n = int(cnt[0])
    return {"n_moves": n, "kind": kind[:n], "fn": fn[:n], "node": node[:n], "delta": delta[:n]}


def debug_leaf_apply_move(z, F, N, has_n, kind, fn, node, src=None):
    """Host-only (no GPU needed): the native search's move application (nep_debug_leaf_apply_move) on the placement z
    [F N (+ N where has_n)]; core.engine.heuristics.apply_move is its mirror.  Returns z'."""
    lib = load_library()
    z = np.ascontiguousarray(np.asarray(z, np.float64).reshape(-1))
    out = np.zeros_like(z)
    _check(lib, lib.nep_debug_leaf_apply_move(int(F), int(N), 1 if has_n else 0, _ptr(z), int(kind), int(fn), int(node),
                                              -1 if src is None else int(src), _ptr(out)),
           "nep_debug_leaf_apply_move")
    return out


def debug_leaf_swap_list(best, best_from, per_fn, max_moves):
    """Host-only (no GPU needed): the swap list (nep_debug_leaf_swap_list) of one placement from its tables best [F, N]
    and best_from [F, N] (nep_leaf_swaps' selection of the per_fn cheapest per function, and its merge).  Returns
    dict(n_moves, fn, from, to, delta) with the arrays at their full length max_moves (-1 / inf past n_moves)."""
    lib = load_library()
    best = np.ascontiguousarray(np.asarray(best, np.float64))
    F, N = best.shape
    best_from = np.ascontiguousarray(np.asarray(best_from, np.int32).reshape(F, N))
    mm = int(max_moves)
    cnt = np.zeros(1, np.int32)
    fn, src, to = (np.zeros(max(mm, 0), np.int32) for _ in range(3))
    delta = np.zeros(max(mm, 0))
    _check(lib, lib.nep_debug_leaf_swap_list(F, N, _ptr(best), _ptr(best_from, ctypes.c_int32), int(per_fn), mm,
                                             _ptr(cnt, ctypes.c_int32), _ptr(fn, ctypes.c_int32),
                                             _ptr(src, ctypes.c_int32), _ptr(to, ctypes.c_int32), _ptr(delta)),
           "nep_debug_leaf_swap_list")
    return {"n_moves": int(cnt[0]), "fn": fn, "from": src, "to": to, "delta": delta}


def debug_block_split(n_nodes, n_functions, na, relaxation=RELAX_REFERENCE):
    """Host-only: how a block of `na` iterating slots is launched (nep_debug_block_split): (slots of the first slot
    group, 0 = one group; waves per x-pass workgroup over na slots, plain; the same, certificate)."""
    lib = load_library()
    # (typed here: an A/B variant library built from an earlier commit loads without this entry point)
    lib.nep_debug_block_split.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_void_p]
    out = np.zeros(3, np.int32)
    _check(lib, lib.nep_debug_block_split(int(n_nodes), int(n_functions), int(relaxation), int(na),
                                          _ptr(out, ctypes.c_int32)), "nep_debug_block_split")
    return tuple(int(t) for t in out)


def debug_presolve(data, variant, lb, ub, step=STEP1, alpha=0.5, soften_step1_sol=1.3, max_score=0.0,
                   prev_network_delay=0.0):
    """Host-only node presolve of [n, n_int] node bounds, from scratch and as the sparse change of
    the base box nep_lp_submit uses: returns (ok_full, ok_node, box_full, box_node)."""
    lib = load_library()
    N, F = len(data.nodes), len(data.functions)
    v = VARIANTS[variant] if isinstance(variant, str) else int(variant)
    k = _arrays(data, N, F)
    d = _desc(k, N, F, v, int(step), alpha, soften_step1_sol, max_score, prev_network_delay, data.node_budget)
    lb = np.ascontiguousarray(lb, np.float64)
    ub = np.ascontiguousarray(ub, np.float64)
    n, ni = lb.shape
    okf = np.zeros(n, np.int32)
    okn = np.zeros(n, np.int32)
    bf = np.zeros((n, 2, ni))
    bn = np.zeros((n, 2, ni))
    _check(lib, lib.nep_debug_presolve(ctypes.byref(d), n, _ptr(lb), _ptr(ub), _ptr(okf, ctypes.c_int32),
                                       _ptr(okn, ctypes.c_int32), _ptr(bf), _ptr(bn)), "nep_debug_presolve")
    return okf.astype(bool), okn.astype(bool), bf, bn


class LPModel:
    """One structured LP family (a reference step model) with `max_batch` device slots."""

    def __init__(self, data, variant, step=STEP1, alpha=0.5, soften_step1_sol=1.3, max_score=0.0,
                 prev_network_delay=0.0, max_batch=1, relaxation=RELAX_REFERENCE):
        self._lib = load_library()
        self.N = len(data.nodes)
        self.F = len(data.functions)
        self.variant = VARIANTS[variant] if isinstance(variant, str) else int(variant)
        self.step = int(step)
        self._keep = _arrays(data, self.N, self.F)
        # the instance as PyTorch-ROCm tensors: the library builds the model from their device memory
        # (nep_model_desc.device_inputs, API 9)
        self.tensors = None if _host_inputs() else instance_tensors(data)
        self.relaxation = int(relaxation)
        d = _desc(self._keep if self.tensors is None else self.tensors, self.N, self.F, self.variant, self.step, alpha, soften_step1_sol, max_score,
                  prev_network_delay, data.node_budget, self.relaxation)
        h = ctypes.c_void_p()
        _check(self._lib, self._lib.nep_model_create(ctypes.byref(d), int(max_batch), None, ctypes.byref(h)),
               "nep_model_create")
        self._h = h
        info = ModelInfo()
        _check(self._lib, self._lib.nep_model_get_info(self._h, ctypes.byref(info)), "nep_model_get_info")
        self.info = info
        self.n_int = info.n_int
        self.max_batch = info.max_batch

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nep_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _bounds(self, B, lb, ub):
        lbp = None if lb is None else np.ascontiguousarray(np.asarray(lb, np.float64).reshape(B, self.n_int))
        ubp = None if ub is None else np.ascontiguousarray(np.asarray(ub, np.float64).reshape(B, self.n_int))
        return lbp, ubp

    def solve(self, slots, lb=None, ub=None, tol=1e-7, cutoff=math.inf, max_iters=200000, check_every=64,
              warm_start=False, warm_omega_floor=0.0, gap_tol=0.0, warm_omega_cap=0.0, polish_after=0.0,
              bound_res=0.0):
        """Solve len(slots) node LPs.  lb/ub: [B, n_int] bounds on the integer vector (None = root).
        Returns dict of numpy arrays: obj (certified LP value = Lagrangian bound), primal_obj, status, iters."""
        slots = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        B = len(slots)
        lbp, ubp = self._bounds(B, lb, ub)
        obj = np.zeros(B)
        pobj = np.zeros(B)
        status = np.zeros(B, np.int32)
        iters = np.zeros(B, np.int64)
        opts = LpOpts(float(tol), float(cutoff), int(max_iters), int(check_every), 1 if warm_start else 0,
                      float(warm_omega_floor), float(gap_tol), float(warm_omega_cap), float(polish_after),
                      float(bound_res))
        _check(self._lib, self._lib.nep_lp_solve_batch(
            self._h, B, _ptr(slots, ctypes.c_int32), _ptr(lbp), _ptr(ubp), ctypes.byref(opts), _ptr(obj), _ptr(pobj),
            _ptr(status, ctypes.c_int32), _ptr(iters, ctypes.c_int64)), "nep_lp_solve_batch")
        return {"obj": obj, "primal_obj": pobj, "status": status, "iters": iters}

    # streaming form (nep_lp_submit / nep_lp_advance): a B&B keeps every slot busy
    def submit(self, slots, lb=None, ub=None, tol=1e-7, cutoff=math.inf, max_iters=200000, check_every=64,
               warm_start=False, warm_omega_floor=0.0, gap_tol=0.0, warm_omega_cap=0.0, polish_after=0.0,
              bound_res=0.0):
        """Start node LPs in free slots; returns their presolve status (LP_INFEASIBLE: proven
        infeasible, not started; LP_ITERATION_LIMIT: iterating).  max_iters / bound_res may be per-LP
        arrays (length len(slots)): then one nep_lp_submit_ex call (API 12) carries them."""
        slots = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        B = len(slots)
        lbp, ubp = self._bounds(B, lb, ub)
        status = np.zeros(B, np.int32)
        per = np.ndim(max_iters) > 0 or np.ndim(bound_res) > 0
        mi = np.ascontiguousarray(np.broadcast_to(np.asarray(max_iters, np.int64), (B,))) if per else None
        br = np.ascontiguousarray(np.broadcast_to(np.asarray(bound_res, np.float64), (B,))) if per else None
        opts = LpOpts(float(tol), float(cutoff), int(mi.max()) if per and B else int(np.max(max_iters)),
                      int(check_every), 1 if warm_start else 0, float(warm_omega_floor), float(gap_tol),
                      float(warm_omega_cap), float(polish_after), 0.0 if per else float(bound_res))
        if per:
            _check(self._lib, self._lib.nep_lp_submit_ex(self._h, B, _ptr(slots, ctypes.c_int32), _ptr(lbp), _ptr(ubp),
                                                         ctypes.byref(opts), _ptr(mi, ctypes.c_int64), _ptr(br),
                                                         _ptr(status, ctypes.c_int32)), "nep_lp_submit_ex")
            return status
        _check(self._lib, self._lib.nep_lp_submit(self._h, B, _ptr(slots, ctypes.c_int32), _ptr(lbp), _ptr(ubp),
                                                  ctypes.byref(opts), _ptr(status, ctypes.c_int32)),
               "nep_lp_submit")
        return status

    def advance(self, min_done=1):
        """Iterate until at least `min_done` LPs finished (0: one block of check_every iterations).
        Returns the finished slots and their results."""
        mb = self.max_batch
        n = ctypes.c_int32(0)
        slots = np.zeros(mb, np.int32)
        obj = np.zeros(mb)
        pobj = np.zeros(mb)
        status = np.zeros(mb, np.int32)
        iters = np.zeros(mb, np.int64)
        _check(self._lib, self._lib.nep_lp_advance(self._h, int(min_done), ctypes.byref(n),
                                                   _ptr(slots, ctypes.c_int32), _ptr(obj), _ptr(pobj),
                                                   _ptr(status, ctypes.c_int32), _ptr(iters, ctypes.c_int64)),
               "nep_lp_advance")
        k = n.value
        return {"slots": slots[:k], "obj": obj[:k], "primal_obj": pobj[:k], "status": status[:k],
                "iters": iters[:k]}

    def active(self):
        """Number of slots iterating (submitted and not yet finished)."""
        return int(self._lib.nep_lp_active(self._h))

    def solution(self, slot, dense_x=True):
        z = np.zeros(self.n_int)
        x = np.zeros((self.N, self.F, self.N), np.float32) if dense_x else None
        _check(self._lib, self._lib.nep_lp_get_solution(self._h, int(slot), _ptr(z),
                                                        _ptr(x, ctypes.c_float) if dense_x else None),
               "nep_lp_get_solution")
        return z, x

    def solutions(self, slots):
        """z_int of several finished slots, [len(slots), n_int], in one device round trip (nep_lp_get_solutions)."""
        slots = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        out = np.zeros((len(slots), self.n_int))
        _check(self._lib, self._lib.nep_lp_get_solutions(self._h, len(slots), _ptr(slots, ctypes.c_int32), _ptr(out)),
               "nep_lp_get_solutions")
        return out

    def reduced_costs(self, slots):
        """(rc [len(slots), n_int], bound [len(slots)]) of finished slots of a facility-relaxation model
        (nep_lp_get_reduced_costs): the reduced costs of c, then n, each slot's bound was computed with — every point
        of the node's box with z_k = t has LP objective >= bound + rc_k t - min(rc_k lb_k, rc_k ub_k)."""
        slots = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        rc = np.zeros((len(slots), self.n_int))
        bound = np.zeros(len(slots))
        _check(self._lib, self._lib.nep_lp_get_reduced_costs(self._h, len(slots), _ptr(slots, ctypes.c_int32), _ptr(rc),
                                                             _ptr(bound)), "nep_lp_get_reduced_costs")
        return rc, bound

    def rc_fixings(self, slot, cutoff):
        """(idx, val): the variables of a finished slot that its reduced costs close at `cutoff`, ascending, and the
        value each is fixed at (nep_lp_rc_fixings, compacted on the device)."""
        n = ctypes.c_int64(0)
        _check(self._lib, self._lib.nep_lp_rc_fixings(self._h, int(slot), float(cutoff), 0, ctypes.byref(n), None, None),
               "nep_lp_rc_fixings")
        k = n.value
        idx = np.zeros(k, np.int32)
        val = np.zeros(k)
        if k:
            _check(self._lib, self._lib.nep_lp_rc_fixings(self._h, int(slot), float(cutoff), k, ctypes.byref(n),
                                                          _ptr(idx, ctypes.c_int32), _ptr(val)), "nep_lp_rc_fixings")
        return idx, val

    def leaf_eval(self, z, rounds=32, cutoff=math.inf, prices=None, tol=0.0, repair_every=None):
        """The fixed-placement evaluator (nep_leaf_eval) on placements z [n, n_int] (every c and n 0 or 1) of a
        step-1 reference model: dict of lower [n] (Lagrangian bound on the leaf LP, best of rounds 0 .. rounds),
        upper [n] (objective of a repaired feasible routing, inf: none), status [n] (LEAF_*), prices [n, N] (behind
        lower) and cpu [n, N] (loads of the returned routing).  prices [n, N] >= 0: the round-0 prices.
        repair_every = k (nep_leaf_eval_ex; None: nep_leaf_eval): the device also repairs the assignments of rounds
        k, 2k, ... and the last one (0: none, nep_leaf_eval's results) and the cheaper of the best round's and round
        0's host-verified point is returned; the dict then also has upper_round [n] (the round behind upper, -1 none),
        device_upper [n] (the device's best objective, inf: none) and round_upper [n, rounds + 1] (the device's
        objective per round, inf: not repaired or no point)."""
        z = np.ascontiguousarray(np.asarray(z, np.float64).reshape(-1, self.n_int))
        n = len(z)
        pin = None if prices is None else np.ascontiguousarray(np.asarray(prices, np.float64).reshape(n, self.N))
        lower, upper, status = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
        pout, cpu = np.zeros((n, self.N)), np.zeros((n, self.N))
        opts = LeafOpts(int(rounds), float(cutoff), float(tol))
        if repair_every is None:
            _check(self._lib, self._lib.nep_leaf_eval(self._h, n, _ptr(z), ctypes.byref(opts), _ptr(pin), _ptr(lower),
                                                      _ptr(upper), _ptr(status, ctypes.c_int32), _ptr(pout),
                                                      _ptr(cpu)), "nep_leaf_eval")
            return {"lower": lower, "upper": upper, "status": status, "prices": pout, "cpu": cpu}
        heur = LeafHeurOpts(int(repair_every), 0)
        rnd, dev = np.zeros(n, np.int32), np.zeros(n)
        per = np.zeros((n, max(0, int(rounds)) + 1))
        _check(self._lib, self._lib.nep_leaf_eval_ex(self._h, n, _ptr(z), ctypes.byref(opts), ctypes.byref(heur),
                                                     _ptr(pin), _ptr(lower), _ptr(upper),
                                                     _ptr(status, ctypes.c_int32), _ptr(pout), _ptr(cpu),
                                                     _ptr(rnd, ctypes.c_int32), _ptr(dev), _ptr(per)),
               "nep_leaf_eval_ex")
        return {"lower": lower, "upper": upper, "status": status, "prices": pout, "cpu": cpu, "upper_round": rnd,
                "device_upper": dev, "round_upper": per}

    def leaf_moves(self, z, prices=None, max_moves=64, table=False):
        """The priced moves (nep_leaf_moves) of placements z [n, n_int] of a step-1 reference model at prices [n, N]
        >= 0 (None: zeros): dict of n_moves [n], kind / fn / node [n, max_moves] (MOVE_ADD / MOVE_DROP / MOVE_CLOSE;
        the function, -1 for CLOSE; the node; -1 past n_moves), delta [n, max_moves] (the exact change of the
        Lagrangian bound at these prices, ascending; inf past n_moves), lagr [n] (that bound) and, with table=True,
        table [n, F, N] (the routing part of the change per (f, j): <= 0 to open a closed one, >= 0 to close an open
        one, inf for a function's only destination)."""
        z = np.ascontiguousarray(np.asarray(z, np.float64).reshape(-1, self.n_int))
        n, mm = len(z), int(max_moves)
        pin = None if prices is None else np.ascontiguousarray(np.asarray(prices, np.float64).reshape(n, self.N))
        cnt = np.zeros(n, np.int32)
        kind, fn, node = (np.zeros((n, max(mm, 0)), np.int32) for _ in range(3))
        delta, lagr = np.zeros((n, max(mm, 0))), np.zeros(n)
        tab = np.zeros((n, self.F, self.N)) if table else None
        _check(self._lib, self._lib.nep_leaf_moves(self._h, n, _ptr(z), _ptr(pin), mm, _ptr(cnt, ctypes.c_int32),
                                                   _ptr(kind, ctypes.c_int32), _ptr(fn, ctypes.c_int32),
                                                   _ptr(node, ctypes.c_int32), _ptr(delta), _ptr(lagr), _ptr(tab)),
               "nep_leaf_moves")
        out = {"n_moves": cnt, "kind": kind, "fn": fn, "node": node, "delta": delta, "lagr": lagr}
        if table:
            out["table"] = tab
        return out

    def leaf_swaps(self, z, prices=None, per_fn=4, max_moves=64, table=False):
        """The priced swaps (nep_leaf_swaps) of placements z [n, n_int] of a step-1 reference model at prices [n, N]
        >= 0 (None: zeros): function fn leaves its open destination `from` for the closed one `to`, priced jointly.
        The device keeps the per_fn (1 .. 8) cheapest destinations per function; dict of n_moves [n], fn / from / to
        [n, max_moves] (-1 past n_moves), delta [n, max_moves] (the exact change of the Lagrangian bound at these
        prices, ascending; inf past n_moves), lagr [n] (that bound) and, with table=True, best [n, F, N] (the
        cheapest swap of f into j; inf: open for f, or screened) and best_from [n, F, N] (its source node, -1: none).
        Without table no [F, N] array leaves the device."""
        z = np.ascontiguousarray(np.asarray(z, np.float64).reshape(-1, self.n_int))
        n, mm = len(z), int(max_moves)
        pin = None if prices is None else np.ascontiguousarray(np.asarray(prices, np.float64).reshape(n, self.N))
        cnt = np.zeros(n, np.int32)
        fn, src, to = (np.zeros((n, max(mm, 0)), np.int32) for _ in range(3))
        delta, lagr = np.zeros((n, max(mm, 0))), np.zeros(n)
        best = np.zeros((n, self.F, self.N)) if table else None
        bfrom = np.zeros((n, self.F, self.N), np.int32) if table else None
        _check(self._lib, self._lib.nep_leaf_swaps(self._h, n, _ptr(z), _ptr(pin), int(per_fn), mm,
                                                   _ptr(cnt, ctypes.c_int32), _ptr(fn, ctypes.c_int32),
                                                   _ptr(src, ctypes.c_int32), _ptr(to, ctypes.c_int32), _ptr(delta),
                                                   _ptr(lagr), _ptr(best), _ptr(bfrom, ctypes.c_int32)),
               "nep_leaf_swaps")
        out = {"n_moves": cnt, "fn": fn, "from": src, "to": to, "delta": delta, "lagr": lagr}
        if table:
            out["best"], out["best_from"] = best, bfrom
        return out

    def leaf_search(self, z0, rounds=32, repair_every=None, width=16, swaps=0, per_fn=4, max_passes=32, warm=True,
                    verify="all", time_limit=None):
        """The placement search as one native call (nep_leaf_search; DESIGN.md §7 "Native search"): the descent of
        core.engine.heuristics.placement_search from z0 [n_int] with the neighbours built on the device.  verify="all":
        placement_search's results to the bit; "lazy" (needs repair_every >= 1): only the neighbours the device's own
        objective ranks as improving are repaired and verified on the host, cheapest first, and the first that
        verifies is accepted.  Returns placement_search's dict (z, upper, lower, prices, row, dst, val, start_upper,
        passes, evaluated, accepted) and verified (host verifications)."""
        if verify not in ("all", "lazy"):
            raise ValueError(f"verify must be 'all' or 'lazy', not {verify!r}")
        z0 = np.ascontiguousarray(np.asarray(z0, np.float64).reshape(-1))
        if z0.size != self.n_int:
            raise ValueError(f"z0 has {z0.size} entries, the model {self.n_int}")
        mp = int(max_passes)
        opts = LeafSearchOpts(int(rounds), 0 if repair_every is None else int(repair_every), int(width), int(swaps),
                              int(per_fn), mp, 1 if warm else 0, 1 if verify == "lazy" else 0,
                              0.0 if time_limit is None else max(float(time_limit), 1e-300))
        z, prices = np.zeros(self.n_int), np.zeros(self.N)
        sc = np.zeros(3)                       # upper, lower, start_upper
        cnt32, cnt64 = np.zeros(2, np.int32), np.zeros(2, np.int64)   # passes, n_accepted; evaluated, verified
        k = max(mp, 0)
        kind, fn, node, src = (np.zeros(k, np.int32) for _ in range(4))
        delta, acc = np.zeros(k), np.zeros(k)
        _check(self._lib, self._lib.nep_leaf_search(
            self._h, _ptr(z0), ctypes.byref(opts), _ptr(z), sc.ctypes.data, sc.ctypes.data + 8, _ptr(prices),
            sc.ctypes.data + 16, cnt32.ctypes.data, cnt64.ctypes.data, cnt64.ctypes.data + 8, cnt32.ctypes.data + 4,
            _ptr(kind, ctypes.c_int32), _ptr(fn, ctypes.c_int32), _ptr(node, ctypes.c_int32),
            _ptr(src, ctypes.c_int32), _ptr(delta), _ptr(acc)), "nep_leaf_search")
        upper = float(sc[0])
        accepted = []
        for q in range(int(cnt32[1])):
            a = (int(kind[q]), int(fn[q]), int(node[q]), float(delta[q]), float(acc[q]))
            accepted.append(a + (int(src[q]),) if kind[q] == MOVE_SWAP else a)
        row, dst, val = self.leaf_routing(0) if math.isfinite(upper) else (None, None, None)
        return {"start_upper": float(sc[2]), "passes": int(cnt32[0]), "evaluated": int(cnt64[0]),
                "verified": int(cnt64[1]), "accepted": accepted, "z": z, "upper": upper, "lower": float(sc[1]),
                "prices": prices, "row": row, "dst": dst, "val": val}

    def debug_leaf_expand(self, z_base, kind, fn, node, src):
        """The native search's device expansion alone (nep_debug_leaf_expand): the neighbours of z_base [n_int] by the
        moves kind / fn / node / src [n].  Returns (open [n, F, N] uint8, nsum [n])."""
        z = np.ascontiguousarray(np.asarray(z_base, np.float64).reshape(-1))
        kind, fn, node, src = (np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1)) for a in (kind, fn, node, src))
        n = len(kind)
        out, nsum = np.zeros((n, self.F, self.N), np.uint8), np.zeros(n)
        _check(self._lib, self._lib.nep_debug_leaf_expand(self._h, _ptr(z), n, _ptr(kind, ctypes.c_int32),
                                                          _ptr(fn, ctypes.c_int32), _ptr(node, ctypes.c_int32),
                                                          _ptr(src, ctypes.c_int32), out.ctypes.data, _ptr(nsum)),
               "nep_debug_leaf_expand")
        return out, nsum

    def leaf_routing(self, k):
        """(row, dst, val) of the routing behind upper[k] of the last leaf_eval call (nep_leaf_routing_entries;
        routing_from_entries makes a SparseRouting of it)."""
        n = ctypes.c_int64(0)
        _check(self._lib, self._lib.nep_leaf_routing_entries(self._h, int(k), 0, ctypes.byref(n), None, None, None),
               "nep_leaf_routing_entries")
        cnt = n.value
        row, dst, val = np.zeros(cnt, np.int32), np.zeros(cnt, np.int32), np.zeros(cnt)
        if cnt:
            _check(self._lib, self._lib.nep_leaf_routing_entries(self._h, int(k), cnt, ctypes.byref(n),
                                                                 _ptr(row, ctypes.c_int32), _ptr(dst, ctypes.c_int32),
                                                                 _ptr(val)), "nep_leaf_routing_entries")
        return row, dst, val

    def rows(self, slot):
        R = self.info.n_rows
        xb = np.zeros((R, self.N), np.float32)
        rf = np.zeros(R, np.int32)
        rs = np.zeros(R, np.int32)
        _check(self._lib, self._lib.nep_lp_get_rows(self._h, int(slot), _ptr(xb, ctypes.c_float),
                                                    _ptr(rf, ctypes.c_int32), _ptr(rs, ctypes.c_int32)),
               "nep_lp_get_rows")
        return xb, rf, rs

    def row_map(self):
        """(row_f, row_src) of the aggregated routing rows (src = -1: the pooled zero-workload sources)."""
        if getattr(self, "_rowmap", None) is None:
            R = self.info.n_rows
            rf = np.zeros(R, np.int32)
            rs = np.zeros(R, np.int32)
            _check(self._lib, self._lib.nep_lp_get_rows(self._h, 0, None, _ptr(rf, ctypes.c_int32),
                                                        _ptr(rs, ctypes.c_int32)), "nep_lp_get_rows")
            self._rowmap = (rf, rs)
        return self._rowmap

    def routing_from_entries(self, row, dst, val):
        from .routing import SparseRouting
        rf, rs = self.row_map()
        return SparseRouting(self.N, self.F, rf, rs, self._keep["workload"], row, dst, val)

    def routing(self, slot):
        """The slot's routing x[i][f][j] as a SparseRouting: every nonzero of the aggregated rows, compacted
        on the device (nep_lp_routing_entries, threshold 0, unrounded) — the dense N*F*N matrix never
        crosses PCIe."""
        row, dst, val = self.routing_entries(slot, threshold=0.0, round3=False)
        return self.routing_from_entries(row, dst, val)

    def set_params(self, tol=1e-7, cutoff=math.inf):
        """tol / cutoff of every LP in flight (nep_lp_set_params): a B&B lowers the cutoff to each new
        incumbent without resubmitting."""
        _check(self._lib, self._lib.nep_lp_set_params(self._h, float(tol), float(cutoff)), "nep_lp_set_params")

    def flows_solutions(self, slots):
        """(flows(slots), solutions(slots)) in one device round trip (nep_lp_get_flows_solutions)."""
        slots = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        fl = np.zeros((len(slots), self.F, self.N), np.float32)
        z = np.zeros((len(slots), self.n_int))
        _check(self._lib, self._lib.nep_lp_get_flows_solutions(self._h, len(slots), _ptr(slots, ctypes.c_int32),
                                                               _ptr(fl, ctypes.c_float), _ptr(z)),
               "nep_lp_get_flows_solutions")
        return fl, z

    def flows(self, slots, split=False):
        """flow[b, f, j] = sum_i x[i, f, j] of finished slots, reduced on the device (nep_lp_get_flows);
        split=True: (flow, workload-source part of it) (nep_lp_get_flows_split)."""
        slots = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        out = np.zeros((len(slots), self.F, self.N), np.float32)
        if split:
            wout = np.zeros_like(out)
            _check(self._lib, self._lib.nep_lp_get_flows_split(
                self._h, len(slots), _ptr(slots, ctypes.c_int32), _ptr(out, ctypes.c_float),
                _ptr(wout, ctypes.c_float)), "nep_lp_get_flows_split")
            return out, wout
        _check(self._lib, self._lib.nep_lp_get_flows(self._h, len(slots), _ptr(slots, ctypes.c_int32),
                                                     _ptr(out, ctypes.c_float)), "nep_lp_get_flows")
        return out

    def routing_entries(self, slot, threshold=0.001, round3=True):
        """Compacted routing entries of the aggregated rows, x > threshold, on the device
        (nep_lp_routing_entries; neptune/utils/output.py:23-31): (row, dst, value) arrays."""
        n = ctypes.c_int64(0)
        _check(self._lib, self._lib.nep_lp_routing_entries(self._h, int(slot), float(threshold), int(round3), 0,
                                                           ctypes.byref(n), None, None, None), "nep_lp_routing_entries")
        k = n.value
        row = np.zeros(k, np.int32)
        dst = np.zeros(k, np.int32)
        val = np.zeros(k)
        if k:
            _check(self._lib, self._lib.nep_lp_routing_entries(
                self._h, int(slot), float(threshold), int(round3), k, ctypes.byref(n), _ptr(row, ctypes.c_int32),
                _ptr(dst, ctypes.c_int32), _ptr(val)), "nep_lp_routing_entries")
        return row, dst, val

    def allocation_entries(self, slot, threshold=0.001):
        """(f, j) pairs with c[f, j] > threshold, compacted on the device (output.py:33-39)."""
        n = ctypes.c_int64(0)
        _check(self._lib, self._lib.nep_lp_allocation_entries(self._h, int(slot), float(threshold), 0,
                                                              ctypes.byref(n), None, None),
               "nep_lp_allocation_entries")
        k = n.value
        fn = np.zeros(k, np.int32)
        dst = np.zeros(k, np.int32)
        if k:
            _check(self._lib, self._lib.nep_lp_allocation_entries(
                self._h, int(slot), float(threshold), k, ctypes.byref(n), _ptr(fn, ctypes.c_int32),
                _ptr(dst, ctypes.c_int32)), "nep_lp_allocation_entries")
        return fn, dst

    def score_check(self, slot):
        """The reference's scorers and feasibility checkers on a slot's solution, on the device
        (nep_lp_score_check; efttc/utils/objectives.py, efttc/utils/constraints_step1.py)."""
        out = np.zeros(len(SCORE_FIELDS))
        _check(self._lib, self._lib.nep_lp_score_check(self._h, int(slot), _ptr(out)), "nep_lp_score_check")
        return dict(zip(SCORE_FIELDS, out.tolist()))

    DIAG = ("pobj", "lagr", "best_lagr", "pres", "gap", "omega", "tau", "sigma", "eta", "k", "k_since_restart",
            "status", "active", "restart_fpr", "last_fpr", "sigma_max")

    def sparse_rows(self, slot):
        """Per routing row of a slot: the nonzeros its Halpern anchor is held with (kAnchorDense = 17: the row is
        dense) and (facility relaxation) the nonzeros of its x <= c duals."""
        R = self.info.n_rows
        a = np.zeros(R, np.int32)
        lam = np.zeros(R, np.float32) if self.relaxation == RELAX_FACILITY else None
        _check(self._lib, self._lib.nep_debug_sparse_rows(self._h, int(slot), _ptr(a), _ptr(lam)),
               "nep_debug_sparse_rows")
        return a, lam

    def diag(self, slot):
        out = np.zeros(16)
        _check(self._lib, self._lib.nep_lp_get_diag(self._h, int(slot), _ptr(out)), "nep_lp_get_diag")
        return dict(zip(self.DIAG, out.tolist()))

    def debug_state(self, slot, n_dual):
        """Device state of a slot (nep_debug_state): duals y, row activities kz, node bounds lb / ub."""
        y, kz = np.zeros(n_dual), np.zeros(n_dual)
        lb, ub = np.zeros(self.n_int), np.zeros(self.n_int)
        _check(self._lib, self._lib.nep_debug_state(self._h, int(slot), _ptr(y), _ptr(kz), None, _ptr(lb), _ptr(ub)),
               "nep_debug_state")
        return {"y": y, "kz": kz, "lb": lb, "ub": ub}

    def debug_fac_state(self, slot):
        """Facility relaxation, finished slot (nep_debug_fac_state): the x <= c duals lam [R, N], their per-function
        sums lsum [F, N] and the row scale rho_l [F, N] of those rows, float32 as the device holds them."""
        lam = np.zeros((self.info.n_rows, self.N), np.float32)
        lsum, rho_l = np.zeros((self.F, self.N), np.float32), np.zeros((self.F, self.N), np.float32)
        _check(self._lib, self._lib.nep_debug_fac_state(self._h, int(slot), _ptr(lam), _ptr(lsum), _ptr(rho_l)),
               "nep_debug_fac_state")
        return {"lam": lam, "lsum": lsum, "rho_l": rho_l}

    def set_reference_weight(self, omega_ref):
        """Warm starts take their primal weight in [floor, cap] x omega_ref (nep_lp_set_reference_weight, API 10);
        0: relative to the parent's final weight."""
        _check(self._lib, self._lib.nep_lp_set_reference_weight(self._h, float(omega_ref)),
               "nep_lp_set_reference_weight")

    def copy_state(self, src, dst):
        _check(self._lib, self._lib.nep_lp_copy_state(self._h, int(src), int(dst)), "nep_lp_copy_state")

    def copy_states(self, src, dst):
        """copy_state(src[k], dst[k]) for every k, in order, in as few launches as the pairs allow
        (nep_lp_copy_states)."""
        src = np.ascontiguousarray(np.asarray(src, np.int32).reshape(-1))
        dst = np.ascontiguousarray(np.asarray(dst, np.int32).reshape(-1))
        if src.size != dst.size:
            raise ValueError("copy_states: src and dst differ in length")
        _check(self._lib, self._lib.nep_lp_copy_states(self._h, int(src.size), _ptr(src, ctypes.c_int32),
                                                       _ptr(dst, ctypes.c_int32)), "nep_lp_copy_states")

    def copy_routing_from(self, other, src, dst):
        """x and thresholds of slot `src` of model `other` (same instance and rows, e.g. the facility
        relaxation's) into this model's slot `dst` (nep_lp_copy_routing)."""
        _check(self._lib, self._lib.nep_lp_copy_routing(self._h, int(dst), other._h, int(src)), "nep_lp_copy_routing")

    def stats(self):
        s = Stats()
        _check(self._lib, self._lib.nep_get_stats(self._h, ctypes.byref(s)), "nep_get_stats")
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def reset_stats(self):
        self._lib.nep_reset_stats(self._h)

    # integer-vector layout helpers (include/neptune_lp.h)
    def layout(self):
        FN, N = self.F * self.N, self.N
        has_n = self.variant != MIN_DELAY
        if self.step == STEP1:
            return {"c": (0, FN), "n": (FN, FN + N) if has_n else None}
        out = {"c": (0, FN), "moved_from": (FN, 2 * FN), "moved_to": (2 * FN, 3 * FN),
               "allocated": (3 * FN, 3 * FN + 1), "deallocated": (3 * FN + 1, 3 * FN + 2)}
        out["n"] = (3 * FN + 2, 3 * FN + 2 + N) if has_n else None
        return out
