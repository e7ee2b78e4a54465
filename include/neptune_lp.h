/*
 * neptune_lp.h — C ABI of the MI355X (gfx950) batched LP-relaxation engine for NEPTUNE's
 * node x function placement/routing MIP.
 *
 * What this replaces.  The reference hands the whole MIP to OR-Tools/SCIP through pywraplp:
 *   core/solvers/solver.py:7      pywraplp.Solver.CreateSolver('SCIP')        -> nep_model_create
 *   core/solvers/solver.py:15-20  load_data -> init_vars / init_constraints   -> nep_model_desc
 *   core/solvers/solver.py:35-40  init_objective(); Solver.Solve(); status == OPTIMAL
 *                                 (SCIP solves one LP relaxation per B&B node) -> nep_lp_solve_batch
 *                                                                               (nep_lp_submit/advance)
 *   core/solvers/solver.py:45-46  score() = Objective().Value()               -> obj / primal_obj
 *   neptune/utils/output.py:5-21  x[i,f,j].solution_value(), c[f,j], n[j]     -> nep_lp_get_solution
 * The model rows/columns are exactly those of neptune/utils/variables.py, constraints_step1.py,
 * constraints_step2.py and objectives.py (see DESIGN.md §2 for the row-by-row map).
 *
 * Conventions.  Plain pointers and sizes only.  Every call returns NEP_OK (0) on success or a
 * negative NEP_ERR_*; nep_last_error() gives a thread-local message.  Host arrays are read during
 * the call only.  The library owns all device workspaces; one model serves `max_batch` LP slots
 * (B&B nodes) that can be warm-started from each other.  A model's device work runs on its iteration
 * stream (the caller's or its own) and one auxiliary stream of the highest priority (slot reads, warm-start
 * copies, submits), ordered by events: a slot iterates only after its submit's initialisation; the HIP
 * context is created on first use (safe after fork()).
 *
 * Integer-variable vector ("z_int"), in the reference's variable-creation order minus x:
 *   step 1: c[F*N] (f-major), then n[N] (MinUtilization / MinDelayAndUtilization only)
 *   step 2: c[F*N], moved_from[F*N], moved_to[F*N], allocated, deallocated, then n[N] (MU / MDU)
 */
#ifndef NEPTUNE_LP_H
#define NEPTUNE_LP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (the fixed-placement evaluator below adds entry points only: no existing call or layout changes, so the version
 * that callers and the suite pin stays 13) */
#define NEP_API_VERSION 13

/* variants: neptune.py:41-66 (NeptuneMinDelay / MinUtilization / MinDelayAndUtilization) */
enum { NEP_MIN_DELAY = 0, NEP_MIN_UTILIZATION = 1, NEP_MIN_DELAY_AND_UTILIZATION = 2 };
/* steps: neptune_step1.py (step 1), neptune_step2.py mode="delete" / "create" */
enum { NEP_STEP1 = 1, NEP_STEP2_DELETE = 2, NEP_STEP2_CREATE = 3 };
/* API 7, nep_model_desc.relaxation: which LP the model iterates.
 *   NEP_RELAX_REFERENCE  the reference's own LP relaxation (constraints_step1.py / constraints_step2.py rows
 *                        as built, big-M pairs included): the LP SCIP solves at a B&B node
 *   NEP_RELAX_FACILITY   step 1 (MinUtilization / MinDelayAndUtilization) only: a STRENGTHENED relaxation
 *                        for branch-and-bound bounds: x[i,f,j] <= c[f,j] for every routing
 *                        row and c[f,j] <= n[j] (valid for every integral placement: constraints_step1.py:5-15,
 *                        :69-78 with c, n binary) replace the big-M pairs C1/C2 and C6/C7, which they imply
 *                        for integral c, n (C2 and C7, the eps floors, are relaxed); the capacity rows take n on
 *                        their right-hand side, C3 sum_f mem_f c[f,j] <= Mem_j n[j] and C5 CPU_j <= cores_j n[j]
 *                        (constraints_step1.py:18-23, :57-65: a closed node has neither).  Same variables, z_int
 *                        and objective; C4 and C8 kept.  Its bound is valid for the MIP, not equal to the
 *                        reference LP's */
enum { NEP_RELAX_REFERENCE = 0, NEP_RELAX_FACILITY = 1 };

enum { NEP_OK = 0, NEP_ERR_ARG = -1, NEP_ERR_HIP = -2, NEP_ERR_NOMEM = -3, NEP_ERR_STATE = -4 };

/* per-LP status */
enum {
  NEP_LP_OPTIMAL = 0,          /* certified: gap(primal obj, Lagrangian bound) and residuals <= tol */
  NEP_LP_ITERATION_LIMIT = 1,  /* obj still holds a VALID lower bound (Lagrangian) */
  NEP_LP_INFEASIBLE = 2,       /* proven by presolve (empty routing row, crossed bounds, row activity) */
  NEP_LP_CUTOFF = 3,           /* Lagrangian bound exceeded opts.cutoff: node can be pruned */
  NEP_LP_NUMERICAL = 4,
  NEP_LP_BOUND = 5             /* API 6, opts.bound_res > 0 only: the bound has converged (within gap_tol of
                                  the repaired point's objective, whose residual is <= bound_res) but the
                                  point is not certified feasible at tol; obj = the VALID Lagrangian bound.
                                  For B&B nodes that branch on the bound (not incumbents) */
};

typedef struct {
  int32_t n_nodes;             /* N */
  int32_t n_functions;         /* F */
  int32_t variant;             /* NEP_MIN_* */
  int32_t step;                /* NEP_STEP1 / NEP_STEP2_DELETE / NEP_STEP2_CREATE */
  double alpha;                /* neptune_step1.py:68 (default 0.5) */
  double soften_step1_sol;     /* neptune_step2.py:6 (default 1.3) */
  double max_score;            /* step 2: step-1 objective (neptune.py:22) */
  double prev_network_delay;   /* step 2 MinDelay: sum D[i,j] W[f,i] prev_x[i,f,j] (constraints_step2.py:66-68) */
  double big_m;                /* constraints_step1.py:1 (1e6) */
  double epsilon;              /* constraints_step1.py:2 (1e-6) */
  const double *delay;         /* [N*N] node_delay_matrix D[i][j] */
  const double *workload;      /* [F*N] workload_matrix W[f][i] (already * workload_coeff) */
  const double *core_per_req;  /* [F*N] core_per_req_matrix cpr[f][j] */
  const double *function_memory; /* [F] */
  const double *node_memory;   /* [N] */
  const double *node_cores;    /* [N] */
  const double *node_cost;     /* [N] (input_to_data.py:186: 5) */
  double node_budget;          /* (input_to_data.py:187: 300) */
  const double *max_delay;     /* [F] max_delay_matrix (input_to_data.py:136: 1000) */
  const double *old_allocations; /* [F*N] step 2 only (0/1) */
  int32_t relaxation;          /* API 7: NEP_RELAX_REFERENCE (0) or NEP_RELAX_FACILITY */
  int32_t device_inputs;       /* API 9: 1 = every array above is DEVICE memory (e.g. the data_ptr() of contiguous
                                  float64 PyTorch-ROCm tensors on the model's GPU); nep_model_create reads the
                                  O(F N + N^2) instance from there and builds the model (scaling on the host, the
                                  step size on the device).  0 = host arrays (nep_debug_* take host arrays only) */
} nep_model_desc;

typedef struct {
  double tol;                  /* certified relative tolerance (default 1e-7) */
  double cutoff;               /* stop when the Lagrangian bound exceeds this (default +inf) */
  int64_t max_iters;           /* default 200000 */
  int32_t check_every;         /* PDHG iterations between certificate checks (default 64) */
  int32_t warm_start;          /* 1: continue from the slot's current state (after nep_lp_copy_state) */
  double warm_omega_floor;     /* warm starts: the primal weight stays >= this x the parent's
                                  (0: default 2; < 0: no floor) */
  double gap_tol;              /* API 5: certified objective gap (relative, as tol); 0: = tol.  A tighter
                                  gap for an LP whose state warm-starts others (a B&B root) */
  double warm_omega_cap;       /* API 5: warm starts: the primal weight stays <= this x the parent's
                                  (0: default 4; < 0: no cap).  DESIGN.md §4 "Warm starts" */
  double polish_after;         /* API 5: primal feasibility polishing may start after this many
                                  iterations (0: default — 256 for warm starts, never for cold starts;
                                  < 0: never).  DESIGN.md §4 "Polishing" */
  double bound_res;            /* API 6: > 0: an LP whose bound has converged (gap <= gap_tol) while its
                                  repaired point's residual is within bound_res stops with NEP_LP_BOUND
                                  (0: never; a B&B sets it on branching nodes, never on leaves) */
} nep_lp_opts;

typedef struct {
  int32_t n_int;               /* length of z_int */
  int32_t n_rows;              /* R: routing rows after exact zero-workload source aggregation */
  int32_t n_tiles;             /* x-pass workgroups per LP (one per function) */
  int32_t max_batch;
  int64_t x_entries;           /* R*N per LP */
  int64_t bytes_per_iter;      /* algorithmic HBM bytes of one PDHG iteration of one LP */
  double step_size;            /* eta = 0.95 / ||K||_2 (scaled) */
  double primal_weight0;       /* API 10: the cold start's PDHG primal weight omega0 = ||c~|| / ||b~|| (scaled) */
} nep_model_info;

typedef struct {
  int64_t x_pass_launches;     /* launches of the fused routing-row kernel */
  double x_pass_ms;            /* summed HIP-event duration of the sampled x-pass launches */
  int64_t x_pass_sampled;      /* number of sampled launches in x_pass_ms */
  int64_t x_pass_lp_iters;     /* LP-iterations carried by the sampled launches */
  double solve_ms;             /* wall time inside nep_lp_solve_batch / nep_lp_advance (device-synchronised) */
  int64_t lp_iterations;       /* PDHG iterations summed over LPs */
} nep_stats;

int nep_model_create(const nep_model_desc *desc, int32_t max_batch, void *hip_stream, void **out_model);
void nep_model_destroy(void *model);
int nep_model_get_info(void *model, nep_model_info *info);

/* Solve B node LPs in slots[0..B-1] to completion.  lb_int/ub_int: host [B][n_int] bounds on z_int
 * (branching fixings; pass NULL for the root bounds).  Outputs (host, length B): obj = certified LP
 * value (Lagrangian lower bound), primal_obj = objective of the primal iterate, status, iters.
 * Equivalent to nep_lp_submit + nep_lp_advance until no slot iterates. */
int nep_lp_solve_batch(void *model, int32_t B, const int32_t *slots, const double *lb_int, const double *ub_int,
                       const nep_lp_opts *opts, double *obj, double *primal_obj, int32_t *status, int64_t *iters);

/* Streaming form, for a branch-and-bound that keeps every slot busy.
 * nep_lp_submit: start n node LPs in free slots (host presolve, then the slot's initialisation on
 *   the device).  status[b] = NEP_LP_INFEASIBLE when presolve proves node b infeasible (it does not
 *   iterate), NEP_LP_ITERATION_LIMIT when it starts iterating.  max_iters, warm_start and
 *   warm_omega_floor apply to the LPs of this call; tol and cutoff (the last submit's) to every LP
 *   in flight; check_every cannot change while any slot iterates.
 * nep_lp_advance: run blocks of check_every PDHG iterations on every iterating slot until at least
 *   min_done of them finished (min_done <= 0: exactly one block).  The finished slots and their
 *   results go to the first *n_done entries of the outputs (each sized max_batch).
 * nep_lp_active: number of iterating slots. */
int nep_lp_submit(void *model, int32_t n, const int32_t *slots, const double *lb_int, const double *ub_int,
                  const nep_lp_opts *opts, int32_t *status);
/* API 12: nep_lp_submit with a per-LP iteration budget and bound stop (max_iters[b] / bound_res[b] for node
 * b; a NULL array takes the opts' value, an entry <= 0 opts->max_iters / no bound stop), so a
 * branch-and-bound starts its strong-branching probes, children and re-solves in one submit group. */
int nep_lp_submit_ex(void *model, int32_t n, const int32_t *slots, const double *lb_int, const double *ub_int,
                     const nep_lp_opts *opts, const int64_t *max_iters, const double *bound_res, int32_t *status);
int nep_lp_advance(void *model, int32_t min_done, int32_t *n_done, int32_t *done_slots, double *obj,
                   double *primal_obj, int32_t *status, int64_t *iters);
int nep_lp_active(void *model);

/* z_int (host, n_int) and optionally the dense routing x[i][f][j] (host float, N*F*N) of a slot.  For a
 * certified slot (NEP_LP_OPTIMAL) z_int is the certificate's repaired point — the primal solution
 * whose objective primal_obj is and whose rows the certificate checked — else the PDHG iterate. */
int nep_lp_get_solution(void *model, int32_t slot, double *z_int, float *x_dense);
/* API 8: z_int of n finished slots at once (z_out [n][n_int], each as nep_lp_get_solution's): one device
 * round trip for all the branching nodes an advance returned. */
int nep_lp_get_solutions(void *model, int32_t n, const int32_t *slots, double *z_out);
/* API 12: nep_lp_get_flows and nep_lp_get_solutions of the same n slots in one device round trip (one wait) */
int nep_lp_get_flows_solutions(void *model, int32_t n, const int32_t *slots, float *flows, double *z_out);
/* API 13, NEP_RELAX_FACILITY models: the reduced costs of z_int (c, then n) that the slot's bound was computed
 * with, in the objective's units, and that bound: for every k and every t in [lb_k, ub_k], each point of the
 * node's box with z_k = t has LP objective >= bound[b] + rc[b][k] * t - min(rc[b][k] * lb_k, rc[b][k] * ub_k).
 * (The box is the node's as the engine holds it after presolve: nep_debug_state's lb / ub.)  bound[b] is the
 * Lagrangian value those reduced costs priced — the best one among the slot's certificate checks — and never
 * exceeds the obj nep_lp_advance reported for that LP.  NEP_ERR_STATE for an iterating slot and for a slot that
 * has kept none: no certificate check yet, an LP presolve refused, or an LP whose box fixes every variable that
 * carries cost (its value is the fixed point's objective, not a Lagrangian).  NEP_ERR_ARG for a reference-relaxation
 * model (its bound uses repaired big-M prices and, in step 2, the exact disruption block, where a c has a
 * piecewise-linear cost, not a reduced cost), a bad slot, or a NULL output.  nep_lp_copy_state(s) copies them with
 * the rest of a slot's state (the node box is not part of that state: it is the destination's own). */
int nep_lp_get_reduced_costs(void *model, int32_t n, const int32_t *slots, double *rc /* [n][n_int] */,
                             double *bound /* [n] */);
/* the variables that inequality closes at `cutoff`: k with lb_k < ub_k, rc_k != 0 and bound + |rc_k| (ub_k - lb_k) >
 * cutoff (fp64, the product rounded before the sum), in ascending k, with the value to fix z_k at (lb_k if rc_k > 0,
 * else ub_k): for a binary z_k, every point of the box with z_k at its other value costs more than cutoff.  The box
 * is the slot's own (the LP it solved).  Count-only when capacity is too small, as nep_lp_routing_entries.  Compacted
 * on the device: one small read per call. */
int nep_lp_rc_fixings(void *model, int32_t slot, double cutoff, int64_t capacity, int64_t *n_fix,
                      int32_t *idx, double *val);
/* aggregated routing rows (host float, R*N) and the row map (row_f, row_src; src = -1: pooled
 * zero-workload sources of function f, each routed identically). */
int nep_lp_get_rows(void *model, int32_t slot, float *xbar, int32_t *row_f, int32_t *row_src);
/* copy a slot's primal/dual state to another (not iterating) slot: warm start of a child node */
int nep_lp_copy_state(void *model, int32_t src_slot, int32_t dst_slot);
/* API 12: n such copies with the result of n nep_lp_copy_state calls in order, in as few launches as their overlaps
 * allow (a B&B submit's warm-start copies: usually one) */
int nep_lp_copy_states(void *model, int32_t n, const int32_t *src_slots, const int32_t *dst_slots);

/* tol / cutoff of every LP in flight, effective from the next iteration block (a B&B lowers the
 * cutoff to each new incumbent without resubmitting). */
int nep_lp_set_params(void *model, double tol, double cutoff);

/* API 10: the primal-weight band of warm starts.  omega_ref > 0: a warm-started LP takes its weight in
 * [warm_omega_floor, warm_omega_cap] x omega_ref (its parent's weight clamped into that band) instead of
 * relative to its parent's final weight, which ratchets up along a lineage of warm starts (DESIGN.md §4
 * "Warm-start primal weight"); 0 restores the parent-relative band.  Applies to later submits. */
int nep_lp_set_reference_weight(void *model, double omega_ref);

/* flow[b][f][j] = sum_i x[i,f,j] of finished slots (host float, n x F x N), computed on the device:
 * the branch-and-bound's branching / rounding input (replaces copying the R x N routing rows). */
int nep_lp_get_flows(void *model, int32_t n, const int32_t *slots, float *flows);
/* API 6: the same flows and, in wflows, their part carried by workload sources only (W[f,i] > 0: the
 * pooled zero-workload row excluded — its mass is free to go to any open placement); the B&B's
 * rounding opens placements for workload, not for that free mass. */
int nep_lp_get_flows_split(void *model, int32_t n, const int32_t *slots, float *flows, float *wflows);

/* Wire format on the device (neptune/utils/output.py:23-39).  Routing entries of the aggregated rows
 * with x > threshold (0.001), value rounded as np.round(x, 3) when round3; allocation entries c[f,j] >
 * threshold.  Row-major order.  Call with capacity 0 (or too small) to get *n_entries only; the row
 * map of nep_lp_get_rows expands a pooled row (src = -1) to all zero-workload sources of its f. */
int nep_lp_routing_entries(void *model, int32_t slot, double threshold, int32_t round3, int64_t capacity,
                           int64_t *n_entries, int32_t *row, int32_t *dst, double *val);
int nep_lp_allocation_entries(void *model, int32_t slot, double threshold, int64_t capacity, int64_t *n_entries,
                              int32_t *fn, int32_t *dst);

/* The fixed-placement evaluator (csrc/nep_leaf.hip, csrc/nep_leaf_repair.cpp; DESIGN.md §7 "Fixed-placement
 * evaluator"), step-1 reference-relaxation models of every variant.  A leaf fixes every c and n; its LP is then one
 * routing simplex per row (C4) coupled by the N CPU rows (C5) and the column floors (C2) only.  For each of the n
 * placements z_leaf[b] (every c and n 0 or 1):
 *   lower[b]   the best value over rounds 0 .. opts->rounds of the Lagrangian that prices C5 with y >= 0 and drops C2,
 *                L(y) = cost_n sum n + sum_rows min_{j open for f} (obj_r D[src_r, j] + y_j W[f, i] cpr[f, j]) - sum_j y_j cores_j
 *              over the loaded routing rows, in fp64 from the instance's fp64 D / W / cpr and the objective's
 *              coefficients in reference units: a valid lower bound on the leaf LP at every y.  Round 0 uses prices_in
 *              (NULL: zeros); the later rounds take subgradient steps (nep_leaf.h).  Rounds run on the device, on the
 *              model's auxiliary stream, without touching any slot; no float atomics (two calls on the same input
 *              return the same bits).
 *   upper[b]   the objective of a routing that meets every reference step-1 row at the placement (C2 at 1 - epsilon,
 *              the pooled row's mass spent on the loaded flow's deficits; C5 at CPU_j <= cores_j), repaired on the
 *              host from the round-0 assignment; +inf when none was found (chained moves are not tried)
 *   status[b]  NEP_LEAF_INFEASIBLE: a row without x rejects the placement (C3 memory, C6/C7 n against c, C8, a function
 *              with no open destination; lower = upper = +inf); NEP_LEAF_CUTOFF: lower >= opts->cutoff (the placement's
 *              rounds stop early, no routing is sought); NEP_LEAF_EXACT: upper - lower <= tol max(1, |lower|);
 *              NEP_LEAF_FEASIBLE: a routing with a wider bracket; NEP_LEAF_NO_POINT: the bound only
 *   prices_out [n][N] (or NULL) the prices behind lower; cpu [n][N] (or NULL) the CPU loads of the returned routing, or
 *              of the last round's assignment when there is none
 * Any n >= 1 (chunked over a workspace allocated on the first call; a model that never calls the evaluator allocates
 * and launches nothing for it).  That first call allocates and uploads with blocking calls: LPs in flight keep their
 * results but wait for it, so a caller that streams LPs makes its first call before it submits.  NEP_ERR_ARG: a step-2 or facility-relaxation model, an entry that is not 0 or 1, a
 * negative price, a NULL required argument.  opts NULL: 32 rounds, no cutoff, tol 1e-6. */
enum { NEP_LEAF_EXACT = 0, NEP_LEAF_FEASIBLE = 1, NEP_LEAF_NO_POINT = 2, NEP_LEAF_INFEASIBLE = 3, NEP_LEAF_CUTOFF = 4 };
typedef struct {
  int32_t rounds;              /* price rounds after round 0 */
  double cutoff;               /* +inf: none */
  double tol;                  /* NEP_LEAF_EXACT's relative bracket (0: 1e-6) */
} nep_leaf_opts;
int nep_leaf_eval(void *model, int32_t n, const double *z_leaf /* [n][n_int] */, const nep_leaf_opts *opts,
                  const double *prices_in /* [n][N] >= 0, or NULL */, double *lower, double *upper, int32_t *status,
                  double *prices_out /* [n][N] or NULL */, double *cpu /* [n][N] or NULL */);
/* the routing behind upper[k] of the last nep_leaf_eval call, in nep_lp_routing_entries' format and order (rows of
 * nep_lp_get_rows, row-major, ascending destination; a pooled row's value is per source), unrounded; count-only when
 * capacity is too small.  NEP_ERR_STATE for a placement without a routing. */
int nep_leaf_routing_entries(void *model, int32_t k, int64_t capacity, int64_t *n_entries, int32_t *row, int32_t *dst,
                             double *val);
/* host-only (no device work): the evaluator's repair of one placement from an assignment asg [R] (a destination per
 * loaded routing row of the model's row layout, e.g. the nearest open one); *found = 0 / 1, *upper, the entries as
 * nep_leaf_routing_entries returns them (count-only when capacity is too small), cpu [N] (may be NULL).  Lets the CPU
 * test-suite check the repair without a GPU. */
int nep_debug_leaf_repair(const nep_model_desc *desc, const double *z_leaf, const int32_t *asg, double *upper,
                          int32_t *found, int64_t capacity, int64_t *n_entries, int32_t *row, int32_t *dst, double *val,
                          double *cpu);
/* nep_debug_leaf_repair from given CPU loads load [N] of asg (NULL: summed from asg in row order, which is
 * nep_debug_leaf_repair), as nep_leaf_eval_ex repairs the round the device chose from that round's loads. */
int nep_debug_leaf_repair_from(const nep_model_desc *desc, const double *z_leaf, const int32_t *asg, const double *load,
                               double *upper, int32_t *found, int64_t capacity, int64_t *n_entries, int32_t *row,
                               int32_t *dst, double *val, double *cpu);

/* nep_leaf_eval with a repair of later rounds' assignments as well (csrc/nep_leaf_heur.hip).  Every price round ends in
 * an assignment that pushes load off congested nodes; with heur->repair_every = k >= 1 the device repairs the
 * assignments of rounds k, 2k, ... and of the last round by the host repair's rules (one workgroup per placement, at
 * most kLeafDevMoves moves a round, no entries), keeps per placement the cheapest round (the earliest on ties) with its
 * assignment and loads, and the host runs its fp64-verified repair on that round's assignment as well as on round 0's
 * and returns the cheaper point: the device only chooses the round, every returned routing is the host's.
 * heur NULL or repair_every = 0: nep_leaf_eval's results bit for bit (and no further allocation or launch).
 *   upper_round [n]   the round behind upper[b]: 0 the round-0 repair, -1 no point
 *   device_upper [n]  the device's own best objective (+inf: none); a verdict the host does not confirm costs a
 *                     candidate, never correctness
 *   round_upper [n][rounds + 1] (or NULL) the device's objective per round, +inf where the round was not repaired or
 *                     ended without a point (for tests and probes)
 * lower, prices_out and the statuses' meaning are nep_leaf_eval's; status, cpu and nep_leaf_routing_entries follow the
 * returned point.  Placements that are cut off or whose prices became optimal stop their repairs with their rounds. */
typedef struct {
  int32_t repair_every;        /* 0: off */
  int32_t reserved;
} nep_leaf_heur_opts;
int nep_leaf_eval_ex(void *model, int32_t n, const double *z_leaf /* [n][n_int] */, const nep_leaf_opts *opts,
                     const nep_leaf_heur_opts *heur, const double *prices_in, double *lower, double *upper,
                     int32_t *status, double *prices_out, double *cpu, int32_t *upper_round /* [n] or NULL */,
                     double *device_upper /* [n] or NULL */, double *round_upper /* [n][rounds + 1] or NULL */);

/* Priced moves of fixed placements (csrc/nep_leaf_moves.hip, csrc/nep_leaf_moves.cpp; DESIGN.md §7 "Priced moves"): the
 * exact change of the Lagrangian bound L(C, y) of nep_leaf_eval when one closed placement (f, j) opens or an open one
 * closes, for every (f, j) of each placement at once, at given prices y >= 0 (NULL: zeros).  A loaded row r = (f, i)
 * costs rho_r(j) = (kobj w) D[i, j] + w (y_j cpr[f, j]) at j; m1_r / j1_r are its minimum and argmin over the open
 * destinations of f (ties to the lowest j), m2_r the minimum over the others (+inf: none).
 *   table [n][F][N]  (f, j) closed: -sum_r max(0, m1_r - rho_r(j)) <= 0; (f, j) open: sum_{r: j1_r = j} (m2_r - m1_r)
 *                    >= 0, +inf when it is the function's only destination; rows in ascending order (device, fp64)
 *   lagr [n]         L(C, y): nep_leaf_eval's `lower` at rounds = 0 with prices_in = y
 * The moves are composed and screened on the host from the table (a node is open when its column of c has a 1):
 *   NEP_MOVE_ADD    a closed (f, j): delta = table + cost_n where the node opens (variants with n); kept only while the
 *                   node's memory holds f too and an opened node's cost is within the budget (the INFEASIBLE rules)
 *   NEP_MOVE_DROP   an open (f, j) with a finite entry: delta = table - cost_n where it is the node's only placement
 *   NEP_MOVE_CLOSE  a node with at least two placements, all finite: delta = their entries summed in ascending f, minus
 *                   cost_n; fn = -1
 * and returned in ascending (delta, kind, node, fn) order, at most max_moves per placement (n_moves [n] of them; the
 * rest of kind / fn / node is -1, of delta +inf).  Applying a move (ADD sets c and n_j; DROP clears c, and n_j with the
 * column; CLOSE clears the column and n_j) gives a placement C' that passes the INFEASIBLE rules, with
 * L(C', y) = L(C, y) + delta up to fp64 rounding.  A placement the evaluator rejects as INFEASIBLE gets n_moves = 0,
 * lagr = +inf and a table of +inf.  max_moves = 0 (kind .. delta may be NULL) prices only.  Runs on the auxiliary
 * stream in the evaluator's workspace, between evaluator calls; no slot state is read or written.  NEP_ERR_ARG as
 * nep_leaf_eval (step-2 / facility models, an entry not 0 or 1, a negative price, a NULL required pointer), for
 * max_moves < 0, and for a model of more than 1169 nodes: the kernel keeps 56 (N + 1) + 16 bytes of LDS per workgroup
 * and is held to 64 KiB (nep_leaf_eval itself takes every admitted N). */
enum { NEP_MOVE_ADD = 0, NEP_MOVE_DROP = 1, NEP_MOVE_CLOSE = 2 };
int nep_leaf_moves(void *model, int32_t n, const double *z_leaf /* [n][n_int] */,
                   const double *prices /* [n][N] >= 0, or NULL: zeros */, int32_t max_moves,
                   int32_t *n_moves /* [n] */, int32_t *kind, int32_t *fn, int32_t *node, double *delta /* [n][max_moves] */,
                   double *lagr /* [n] or NULL */, double *table /* [n][F][N] or NULL */);
/* host-only: the move list of one placement from a given table (composition, screens, order), so the CPU suite
 * checks it without a GPU, in the manner of nep_debug_leaf_repair */
int nep_debug_leaf_move_list(const nep_model_desc *desc, const double *z_leaf, const double *table /* [F][N] */,
                             int32_t max_moves, int32_t *n_moves, int32_t *kind, int32_t *fn, int32_t *node, double *delta);

/* Priced swaps of fixed placements (csrc/nep_leaf_swaps.hip, csrc/nep_leaf_swaps.cpp; DESIGN.md §7 "Priced swaps"): the
 * exact change of L(C, y) when function f leaves an open destination j for a closed one j', priced jointly — rows of j
 * fall back to the cheaper of their second choice and j' — for every (f, j, j') of each placement at once.  With bucket
 * k the loaded rows of f whose minimum is at the k-th open destination oj[k], in ascending row order:
 *   A_k(j') = sum_{r in bucket k} (min(m1_r, rho_r(j')) - m1_r),  S_k(j') = sum_{r in bucket k} (min(m2_r, rho_r(j')) - m1_r)
 *   delta(f, oj[k] -> j') = (sum_k A_k + ((S_k - A_k) - cost_n [node oj[k] holds only this placement]))
 *                           + cost_n [node j' holds none]                     (the cost_n terms: variants with n)
 * finite even for a function with one destination.  j' must pass NEP_MOVE_ADD's screens (memory, and the budget where
 * the node opens).  Per (f, j') the source is the k of the smallest delta (ties to the lowest k); per function the
 * device keeps the per_fn (1 .. 8) cheapest (delta, j'), so per_fn records per (placement, function) are read back
 * and no [F][N] array crosses to the host unless best / best_from ask for one:
 *   best [n][F][N]       the cheapest swap of f into j' (+inf: j' open for f, or screened)
 *   best_from [n][F][N]  its source node (-1: none)
 * The kept swaps are returned in ascending (delta, fn, to, from) order, at most max_moves per placement (n_moves [n]
 * of them; the rest of fn / from / to is -1, of delta +inf); the move kind of a swap is NEP_MOVE_SWAP.  Applying one
 * (clear c[fn, from], and n of that node with its column; set c[fn, to] and n of that node) gives a placement that
 * passes the INFEASIBLE rules, with L(C', y) = L(C, y) + delta up to fp64 rounding.  lagr, rejected placements
 * (n_moves = 0, lagr = +inf, best +inf, best_from -1), max_moves = 0, the stream and the refusals are nep_leaf_moves';
 * per_fn outside 1 .. 8 is NEP_ERR_ARG too. */
enum { NEP_MOVE_SWAP = 3 };
int nep_leaf_swaps(void *model, int32_t n, const double *z_leaf /* [n][n_int] */,
                   const double *prices /* [n][N] >= 0, or NULL: zeros */, int32_t per_fn /* 1..8 */, int32_t max_moves,
                   int32_t *n_moves /* [n] */, int32_t *fn, int32_t *from, int32_t *to, double *delta /* [n][max_moves] */,
                   double *lagr /* [n] or NULL */, double *best /* [n][F][N] or NULL */,
                   int32_t *best_from /* [n][F][N] or NULL */);
/* host-only: the selection (per_fn cheapest per function) and merge of one placement from given tables, so the CPU
 * suite checks them without a GPU */
int nep_debug_leaf_swap_list(int32_t F, int32_t N, const double *best, const int32_t *best_from, int32_t per_fn,
                             int32_t max_moves, int32_t *n_moves, int32_t *fn, int32_t *from, int32_t *to,
                             double *delta);

/* The placement search as one call (csrc/nep_leaf_search.hip, csrc/nep_leaf_search.cpp; DESIGN.md §7 "Native search"):
 * the descent of core/engine/heuristics.py placement_search over nep_leaf_eval_ex, nep_leaf_moves and nep_leaf_swaps.
 * The current placement stays in one slot of the evaluator's chunk; the neighbours of a pass are written beside it on
 * the device from move records, so after the start no placement crosses to the device as z.
 * verify = 0: placement_search's results to the bit — z0 evaluated cold without a cutoff; per pass the `width` cheapest
 * single moves at the current best prices, then the `swaps` cheapest swaps at the same prices; every neighbour evaluated
 * with cutoff = the current upper (from the current prices when warm, else from zeros) and every one that is not cut
 * off repaired and verified on the host; the lowest-index minimum of the verified uppers accepted when it is below
 * upper - 1e-9 max(1, |upper|); a start without a point takes the first neighbour that has one; stops at the first pass
 * without an acceptance, when no move exists, at max_passes or at time_limit.
 * verify = 1 (lazy; needs repair_every >= 1): after a pass's rounds only each neighbour's bounds, flags and device
 * objective d_q are read (48 bytes).  The candidates — not cut off, d_q finite and, for a finite upper, d_q < upper -
 * 1e-9 max(1, |upper|) — are taken in ascending (d_q, q); for each the host copies that neighbour's round-0 and best
 * round's assignments and loads, repairs both as nep_leaf_eval_ex does and takes the cheaper verified point; the first
 * whose verified upper improves (a start without a point: is finite) is accepted; if none verifies the search ends.
 * Another acceptance rule, not an approximation of soundness: every accepted point is host-verified in fp64.
 * Outputs: z_out, upper, lower and prices_out of the end placement, start_upper, passes, evaluated (neighbours),
 * verified (host verifications; verify = 0: the neighbours not cut off), n_accepted and per accepted move its kind, fn
 * (-1: CLOSE), node, src (a swap's source, else -1), delta and the verified upper.  nep_leaf_routing_entries(model, 0,
 * ...) then returns the end placement's host-verified routing (NEP_ERR_STATE without one).  NEP_ERR_ARG as
 * nep_leaf_swaps and in its order (step-2 / facility models, the options, the 64 KiB LDS bound, an entry of z0 not 0 or
 * 1), and for verify = 1 with repair_every = 0. */
typedef struct {
  int32_t rounds;        /* price rounds per evaluation (<= 0: 32) */
  int32_t repair_every;  /* nep_leaf_heur_opts' (0: no per-round repair) */
  int32_t width;         /* single moves per pass (nep_leaf_moves' max_moves) */
  int32_t swaps;         /* swaps per pass (0: none), per_fn 1..8 as nep_leaf_swaps */
  int32_t per_fn;
  int32_t max_passes;
  int32_t warm;          /* neighbours start from the current placement's best prices */
  int32_t verify;        /* 0: every neighbour that is not cut off is verified on the host; 1: lazy */
  double time_limit;     /* seconds, <= 0: none */
} nep_leaf_search_opts;
int nep_leaf_search(void *model, const double *z0 /* [n_int] */, const nep_leaf_search_opts *opts,
                    double *z_out /* [n_int] */, double *upper, double *lower, double *prices_out /* [N] or NULL */,
                    double *start_upper, int32_t *passes, int64_t *evaluated, int64_t *verified, int32_t *n_accepted,
                    int32_t *kind, int32_t *fn, int32_t *node, int32_t *src, double *delta,
                    double *acc_upper /* each [max_passes] */);
/* host-only: the search's move application (it rebuilds z_out and the verified neighbours' bytes), so the CPU suite
 * checks it against heuristics.apply_move without a GPU; z [F N (+ N where has_n)] */
int nep_debug_leaf_apply_move(int32_t F, int32_t N, int32_t has_n, const double *z_in, int32_t kind, int32_t fn,
                              int32_t node, int32_t src /* a swap's source, else ignored */, double *z_out);
/* the device expansion alone: z_base staged, its n neighbours of the given moves expanded (leaf_search_expand) and read
 * back — open_out [n][F][N] their c, nsum_out [n] the open-node count each record carried */
int nep_debug_leaf_expand(void *model, const double *z_base, int32_t n, const int32_t *kind, const int32_t *fn,
                          const int32_t *node, const int32_t *src, uint8_t *open_out, double *nsum_out);

/* The reference's offline scorers and feasibility checkers on a slot's solution, on the device
 * (efttc/utils/objectives.py:23-98, efttc/utils/constraints_step1.py:5-133; booleans are the
 * reference's truthiness, value != 0).  out[NEP_SC_COUNT]: */
enum {
  NEP_SC_NETWORK_DELAY = 0,   /* score_minimize_network_delay: sum W[f,i] D[i,j] x[i,f,j] */
  NEP_SC_NODES_USED = 1,      /* score_minimize_node_utilization: #{j : n[j] != 0} */
  NEP_SC_NODE_COST = 2,       /* sum n[j] cost[j] (constrain_budget) */
  NEP_SC_BAD_C_X = 3,         /* constrain_c_according_to_x violations (f, j) */
  NEP_SC_BAD_MEMORY = 4,      /* constrain_memory_usage violations (nodes) */
  NEP_SC_BAD_HANDLE = 5,      /* constrain_handle_all_requests: (i, f) with |sum_j x - 1| >= 0.1 */
  NEP_SC_BAD_CPU = 6,         /* constrain_CPU_usage violations (nodes, + 1e-6) */
  NEP_SC_BAD_N_C = 7,         /* constrain_n_according_to_c violations (nodes) */
  NEP_SC_BAD_BUDGET = 8,      /* constrain_budget (0 / 1) */
  NEP_SC_HANDLE_MAXDEV = 9,   /* max |sum_j x - 1| */
  NEP_SC_CPU_MAXEXCESS = 10,  /* max (CPU use - cores, 0) */
  NEP_SC_COUNT = 11
};
int nep_lp_score_check(void *model, int32_t slot, double *out);

int nep_get_stats(void *model, nep_stats *stats);

/* diagnostics: out16 = {primal obj, Lagrangian, best Lagrangian, primal residual, gap, omega, tau,
 * sigma, eta, iterations, iterations since restart, status, active, fpr at restart, last fpr, ||K||} */
int nep_lp_get_diag(void *model, int32_t slot, double *out16);
/* device state of a slot (any pointer may be NULL): duals [n_dual], row activities [n_dual],
 * packed f32 duals of the x pass [F*NP+NP+4], node bounds [n_int] */
int nep_debug_state(void *model, int32_t slot, double *y, double *kz, float *kty, double *lb, double *ub);
/* API 12: per routing row of a slot (length R), the nonzeros its Halpern anchor is held with (17 = dense) and, on a
 * facility-relaxation model, the nonzeros of its x <= c duals (counted on the host) */
int nep_debug_sparse_rows(void *model, int32_t slot, int32_t *anchor_cnt, float *lambda_nnz);
/* facility-relaxation model, finished slot (any pointer may be NULL; padding columns dropped): the duals of the rows
 * x[r, j] - c[f, j] <= 0 as the device holds them, lambda [R][N] — they live outside the dual vector nep_debug_state
 * reads —, their sums over the routing rows of each function as fac_x_pass left them, lsum [F][N], and the row scale
 * of those rows, rho_l [F][N] (f32, the value the kernels multiply with).  NEP_ERR_STATE for an iterating slot,
 * NEP_ERR_ARG for a reference-relaxation model.  Lets the suite compare single iterations with a mirror. */
int nep_debug_fac_state(void *model, int32_t slot, float *lambda, float *lsum, float *rho_l);
/* host-only model build (no device work): step size, scalings, row norms, dims = {R, F, n_int,
 * n_dual}.  Lets the CPU test-suite check the model build without a GPU. */
int nep_debug_build(const nep_model_desc *desc, double *eta, double *rho, double *gam, double *rownorm,
                    int32_t *dims);
/* host-only node presolve of n nodes (lb_int/ub_int as for nep_lp_submit), evaluated twice: from
 * scratch and as the sparse change of the model's base box that nep_lp_submit uses.  ok_* [n]:
 * 1 = feasible; box_* [n][2][n_int] (may be NULL): the resulting node bounds (lb then ub). */
int nep_debug_presolve(const nep_model_desc *desc, int32_t n, const double *lb_int, const double *ub_int,
                       int32_t *ok_full, int32_t *ok_node, double *box_full, double *box_node);
/* host-only: how a block of `na` iterating slots of a model of n_nodes x n_functions (relaxation as in
 * nep_model_desc) is launched.  out3 = {slots of the first slot group when the block runs as two groups
 * (NEP_BLOCK_GROUPS=2), 0 when it runs as one; waves per x-pass workgroup of a launch over na slots, plain
 * variant; the same, certificate variant}.  Lets the CPU test-suite check the split rule without a GPU. */
int nep_debug_block_split(int32_t n_nodes, int32_t n_functions, int32_t relaxation, int32_t na, int32_t *out3);
void nep_reset_stats(void *model);

/* API 8: the routing state (x and its projection thresholds) of a finished slot of ANOTHER model of the same
 * instance and row layout (e.g. a NEP_RELAX_FACILITY branching node) copied into a finished slot of this one —
 * a leaf's warm start from its branching node's routing; the slot's other state (small variables, duals) is
 * left as it is (typically the root's, nep_lp_copy_state); the next submit with warm_start iterates from it.
 * NEP_ERR_ARG when the row layouts differ.  Replaces SCIP's LP warm start across its own node LPs. */
int nep_lp_copy_routing(void *dst_model, int32_t dst_slot, void *src_model, int32_t src_slot);

/* API 8: branch-and-bound rounding heuristic (host only, no model; core/engine/bnb.py): one branching
 * node's LP -> a leaf fixing every c (and n).  c_fix [F*N] / n_fix [N] (n_fix NULL: no n): -1 free, 0 / 1
 * fixed by the node; flow [F*N] the node's flows, zc [F*N] its c (NULL: 0).  Fixed-open c first, then the free
 * c with zc >= 1/2 (largest first), then (by_flow) the free (f, j) with flow > flow_threshold (largest
 * first), each while node j's memory has room (constraints_step1.py:18-23); a function left without a
 * destination gets the one with the largest c, then flow; n = any c; a node fixed open gets its smallest
 * fitting function.  Returns 1 and fills c_out [F*N] (n_out [N]) with the leaf, 0 when the node has none,
 * < 0 on a bad argument.  Replaces the reference's nothing: SCIP's own primal heuristics run inside
 * Solve() (core/solvers/solver.py:37). */
int nep_round_leaf(int32_t F, int32_t N, const double *c_fix, const double *n_fix, const float *flow, const double *zc,
                   const double *fn_mem, const double *node_mem, int32_t by_flow, double flow_threshold, double *c_out,
                   double *n_out);
/* API 8: nep_round_leaf for `modes` (by_flow[k], flow_threshold[k]) pairs of one node in one call: c_out
 * [modes][F*N], n_out [modes][N] (NULL without n), found[k] = 1 / 0 (< 0 returned on a bad argument). */
int nep_round_leaves(int32_t F, int32_t N, const double *c_fix, const double *n_fix, const float *flow, const double *zc,
                     const double *fn_mem, const double *node_mem, int32_t modes, const int32_t *by_flow,
                     const double *flow_threshold, double *c_out, double *n_out, int32_t *found);

/* API 11: the branch-and-bound's tree search, native (csrc/nep_bnb.cpp; core/engine/bnb.py delegates its
 * single-rank step-1 search here, DESIGN.md §7 "Native tree search").  Replaces the host loop of
 * BranchAndBound.solve (core/engine/bnb.py) — the tree SCIP searches inside Solver.Solve()
 * (core/solvers/solver.py:35-40): best-first open nodes, rounding leaves, retries of uncertified leaves,
 * warm starts from the parent's slot or the root's state, one submit / advance stream per model (the leaf
 * model = the reference LP; the optional bound model = the facility relaxation), prune / branch / round per
 * finished LP.  The tree drives the models through this header's nep_lp_* calls only. */
typedef struct {
  int32_t c0, c1, n0, n1, n_int;   /* integer layout: c = z_int[c0:c1] (F x N), n = z_int[n0:n1] (n0 < 0: none) */
  int32_t F, N;
  int32_t warm;                    /* warm starts (reserves the leaf model's last two slots: root / incumbent state) */
  int32_t batch, batch_b;          /* LPs in flight per model (leaf, bound); further free slots keep finished states */
  int32_t check_every, root_check_every;
  int32_t unit_flow_leaves;        /* a third rounding mode: (f, j) carrying a unit of flow */
  int32_t objective_integral;      /* every integral point's objective is integral: prune at incumbent - 1 */
  int32_t primal_at_root;          /* nep_bnb_run returns NEP_BNB_ROOT once the root branching node finished */
  double tol, gap, bound_gap;      /* LP tolerance, relative MIP gap, the bound model's gap_tol */
  int64_t max_iters, node_max_iters, root_max_iters;
  double node_bound_res, retry_res, flow_tol;
  double upper_bound;              /* a-priori cutoff (+inf: none) */
  int64_t node_limit;
  double time_limit;               /* seconds (<= 0: none) */
  int32_t world, rank;             /* API 12: the sharded search (world > 1: NEP_BNB_SYNC once per loop) */
  int32_t branching;               /* API 12: 0 n by inflow, then c by flow; 1 pseudo-cost (product score);
                                      2 reliability branching: pseudo-costs, strong-branching probes while unreliable */
  int32_t strong_cands, strong_rel;  /* branching 2: candidates scored, observations per direction to be reliable */
  int32_t rc_fixing;               /* API 13: 1 = reduced-cost fixing at the bound model's branching nodes (needs the
                                      engine's rc_fixings call and an incumbent); 0 (default): off */
  int64_t strong_iters;            /* branching 2: iteration budget of a probe LP */
  double objective_unit;           /* with objective_integral: the objective's integral unit (<= 0: 1) — e.g. alpha / N
                                      for MinDelayAndUtilization without workload, whose objective is alpha / N sum n */
  int32_t leaf_eval;               /* 1 = queued leaves and retries go through the fixed-placement evaluator in one call
                                      before their LPs are submitted (needs the leaf engine's evaluator pair, see
                                      nep_bnb_set_leaf_engine; single rank only); 2 = the same, and nep_bnb_create installs
                                      the evaluator with every round's assignment repaired on the device
                                      (nep_leaf_eval_ex, repair_every = 1); 0 (default): off */
  int32_t leaf_rounds;             /* the evaluator's price rounds per call (<= 0: 32) */
} nep_bnb_params;

typedef struct {
  int64_t nodes, leaves, lps, certified, lp_iterations, unresolved, drained;
  int64_t lp_status[7];            /* certified, bound, limit, infeasible, cutoff, numerical, presolve-infeasible */
  int64_t lp_status_kind[4][7];    /* per node kind: node, leaf, retry, refroot */
  int64_t advance_calls, inflight_sum, lp_incumbents, heuristic_incumbents, n_lp_iters;
  double advance_seconds, finish_seconds, submit_seconds, drain_seconds, root_seconds;
  double bound, incumbent;         /* at the end: best proven bound, incumbent value (+inf: none) */
  int32_t incumbent_source;        /* 0 none, 1 a certified leaf LP, 2 nep_bnb_set_incumbent, 3 a routing of the
                                      fixed-placement evaluator (nep_bnb_incumbent_routing) */
  int32_t incumbent_slot;          /* leaf-model slot holding the incumbent LP's state (source 1) */
  int32_t limit_hit, any_unresolved, unresolved_below;
  int32_t stalled;                 /* API 12: ended because open nodes could never get a slot (reported as a limit) */
  uint32_t split_hash;             /* sharded: crc32 of the frontier every rank dealt (bnb.py _frontier_hash) */
  int32_t reserved_;
  int64_t presplit_nodes, presplit_lps, presplit_certified;   /* sharded: counts when the frontier was dealt */
  int64_t rebalanced, sync_calls;  /* sharded: open nodes imported from other ranks; collectives answered */
  double agreed_incumbent;         /* min(this rank's incumbent, the ranks' agreed one) */
  int64_t strong_nodes, strong_lps, strong_iterations, strong_decided;   /* branching 2: nodes that probed, probes */
  int64_t rc_fixed, rc_calls;      /* API 13, rc_fixing: variables fixed by reduced cost, rc_fixings calls made */
  int64_t rc_children_pruned, rc_leaves_dropped;   /* children whose branching value / rounding leaves whose
                                                      placement a fixing contradicts (no LP) */
} nep_bnb_stats;

#define NEP_BNB_DONE 0   /* the search ended (no open node, or a stop): stats / incumbent are final */
#define NEP_BNB_ROOT 1   /* the root branching node finished: nep_bnb_event_data, then nep_bnb_add_leaf(where = 1) /
                            nep_bnb_set_incumbent for the caller's primal heuristic, then nep_bnb_run again */
#define NEP_BNB_INCUMBENT 2   /* (nep_bnb_set_step2 with incumbent_events) a new LP incumbent: nep_bnb_incumbent_event,
                                 then nep_bnb_add_leaf(where = 2) for each neighbour leaf, then nep_bnb_run again */
#define NEP_BNB_SYNC 3   /* (world > 1) the loop's collective is due: nep_bnb_sync_get, the caller's all-reduce over the
                            ranks (incumbent MIN, stop OR, open SUM; core/engine/comm.py agree), nep_bnb_sync_set,
                            optionally a rebalance (nep_bnb_export_nodes / nep_bnb_import_nodes), then nep_bnb_run */

/* API 12: the calls the tree makes on one model, with the model's integer vector length and slot count.
 * nep_bnb_create fills one from an engine handle (the nep_lp_* functions, ctx = the handle); a caller may pass its
 * own (the CPU suite: HiGHS node LPs behind ctypes callbacks).  Same contracts as the nep_lp_* functions. */
typedef struct {
  void *ctx;
  int32_t n_int, max_batch;
  int (*submit)(void *ctx, int32_t n, const int32_t *slots, const double *lb_int, const double *ub_int,
                const nep_lp_opts *opts, int32_t *status);
  int (*advance)(void *ctx, int32_t min_done, int32_t *n_done, int32_t *done_slots, double *obj, double *primal_obj,
                 int32_t *status, int64_t *iters);
  int (*active)(void *ctx);
  int (*copy_state)(void *ctx, int32_t src_slot, int32_t dst_slot);
  int (*set_params)(void *ctx, double tol, double cutoff);
  int (*get_flows)(void *ctx, int32_t n, const int32_t *slots, float *flows);
  int (*get_solutions)(void *ctx, int32_t n, const int32_t *slots, double *z_out);
  int (*get_diag)(void *ctx, int32_t slot, double *out16);
  /* optional (NULL: one submit per budget / bound-stop group): nep_lp_submit_ex's contract */
  int (*submit_ex)(void *ctx, int32_t n, const int32_t *slots, const double *lb_int, const double *ub_int,
                   const nep_lp_opts *opts, const int64_t *max_iters, const double *bound_res, int32_t *status);
  /* optional (NULL: copy_state per pair): nep_lp_copy_states' contract */
  int (*copy_states)(void *ctx, int32_t n, const int32_t *src_slots, const int32_t *dst_slots);
  /* optional (NULL: get_flows, then get_solutions): nep_lp_get_flows_solutions' contract */
  int (*get_flows_solutions)(void *ctx, int32_t n, const int32_t *slots, float *flows, double *z_out);
  /* API 13, optional (NULL: the tree never fixes by reduced cost): nep_lp_rc_fixings' contract */
  int (*rc_fixings)(void *ctx, int32_t slot, double cutoff, int64_t capacity, int64_t *n_fix, int32_t *idx,
                    double *val);
} nep_bnb_engine;

/* NULL on a bad argument (nep_last_error says which): batch < 1, a layout outside n_int, no working slot left
 * after the reserved ones, world / rank out of range. */
void *nep_bnb_create(void *leaf_model, void *bound_model, const nep_bnb_params *params, const double *fn_mem,
                     const double *node_mem);
void *nep_bnb_create_engines(const nep_bnb_engine *leaf, const nep_bnb_engine *bound, const nep_bnb_params *params,
                             const double *fn_mem, const double *node_mem);
void nep_bnb_destroy(void *tree);
/* a leaf (a full c / n assignment, or any box): where = 0 a seed leaf queued when the root LP finishes;
 * where = 1 a leaf of the NEP_BNB_ROOT event's node, where = 2 a neighbour of the NEP_BNB_INCUMBENT event's
 * leaf, both at the front of the leaf queue */
int nep_bnb_add_leaf(void *tree, int32_t n, const int32_t *idx, const double *val, double bound, int32_t where);
/* step 2 (before the first nep_bnb_run): the closed-form integer bound of NeptuneStep2Base.integer_bound
 * (core/solvers/neptune/neptune_step.py; create != 0: create mode, node_cap: the most nodes an integral placement
 * opens, +inf: none; old_alloc [F*N]) on every node / leaf, and (incumbent_events) NEP_BNB_INCUMBENT events */
int nep_bnb_set_step2(void *tree, int32_t create, double node_cap, const double *old_alloc, int32_t incumbent_events);
int nep_bnb_incumbent_event(void *tree, int32_t *n_fix, int32_t *idx, double *val, double *value);
/* host only: that integer bound of one box (params: the layout fields), for the CPU suite */
int nep_bnb_debug_ibound(const nep_bnb_params *params, int32_t create, double node_cap, const double *old_alloc,
                         int32_t n, const int32_t *idx, const double *val, double *out);
/* an incumbent found outside the tree (a checked heuristic point): its value becomes the cutoff */
int nep_bnb_set_incumbent(void *tree, double value);
int nep_bnb_event_data(void *tree, double *z_int, float *flow);
int nep_bnb_run(void *tree, int32_t *event);
/* NEP_BNB_SYNC: out6 = {incumbent, stop, open + in-flight nodes, heap size, frontier dealt, collectives so far};
 * the caller answers with the agreed values (a lower incumbent becomes every model's cutoff at once) */
int nep_bnb_sync_get(void *tree, double *out6);
int nep_bnb_sync_set(void *tree, double incumbent, int32_t stop, int64_t open_total);
/* rebalance (bnb.py _rebalance): the k best-bound open nodes leave this rank's heap (lens[k]; meta[k][3] = bound,
 * depth, kind; idx / val concatenated, at most cap entries) / enter it (pruned against the incumbent; they start
 * from the model's root state) */
int nep_bnb_export_nodes(void *tree, int32_t k, int32_t cap, int32_t *lens, double *meta, int32_t *idx, double *val);
int nep_bnb_import_nodes(void *tree, int32_t k, const int32_t *lens, const double *meta, const int32_t *idx,
                         const double *val);
int nep_bnb_get_stats(void *tree, nep_bnb_stats *out);
int nep_bnb_get_lp_iters(void *tree, int64_t *out);
/* the LP incumbent's (source 1) or the evaluator incumbent's (source 3) integer vector (n_int) and its leaf box (at most
 * c1 - c0 + n1 - n0 entries: a leaf fixes every c and n; *n_fix = -1: neither) */
int nep_bnb_incumbent(void *tree, double *z_int, int32_t *n_fix, int32_t *idx, double *val);

/* The tree's use of the fixed-placement evaluator (params.leaf_eval = 1).  Before leaves or retries are
 * submitted, the queued ones that fix every c and n are evaluated in one call at the current cutoff: INFEASIBLE or CUTOFF
 * drops the leaf with no LP; a finite `upper` below the incumbent (beyond the gap) becomes the incumbent (source 3: the
 * tree keeps z and the entries, the new cutoff goes to every model); EXACT resolves the leaf; FEASIBLE or NO_POINT
 * raises the leaf's bound to max(own, lower) and its LP is submitted as before if that is still below the cutoff.
 * The evaluator pair is the leaf engine's: nep_bnb_create sets nep_leaf_eval / nep_leaf_routing_entries of a step-1
 * reference model; a caller with its own engines sets its pair here (before the first nep_bnb_run).  A NULL pair, or
 * leaf_eval = 0, gives the search without the evaluator.  (The pair and the counters live beside nep_bnb_engine and
 * nep_bnb_stats, whose layouts stay as they are.) */
typedef int (*nep_bnb_leaf_eval_fn)(void *ctx, int32_t n, const double *z_leaf, const nep_leaf_opts *opts,
                                    const double *prices_in, double *lower, double *upper, int32_t *status,
                                    double *prices_out, double *cpu);
typedef int (*nep_bnb_leaf_routing_fn)(void *ctx, int32_t k, int64_t capacity, int64_t *n_entries, int32_t *row,
                                       int32_t *dst, double *val);
int nep_bnb_set_leaf_engine(void *tree, void *ctx, nep_bnb_leaf_eval_fn leaf_eval,
                            nep_bnb_leaf_routing_fn leaf_routing_entries);
typedef struct {
  int64_t leaf_eval_calls, leaf_eval_leaves;   /* evaluator calls, leaves evaluated */
  int64_t leaf_eval_exact, leaf_eval_feasible; /* leaves resolved EXACT; FEASIBLE (their LP still runs) */
  int64_t leaf_eval_dropped;                   /* leaves dropped with no LP (INFEASIBLE, CUTOFF, bound at the cutoff) */
  int64_t leaf_eval_incumbents;
  double leaf_eval_seconds;
} nep_bnb_leaf_stats;
int nep_bnb_get_leaf_stats(void *tree, nep_bnb_leaf_stats *out);
/* the entries of the evaluator incumbent (source 3), as nep_leaf_routing_entries returns them; count-only when capacity
 * is too small; *n_entries = -1 when the incumbent has another source */
int nep_bnb_incumbent_routing(void *tree, int64_t capacity, int64_t *n_entries, int32_t *row, int32_t *dst, double *val);

const char *nep_last_error(void);
int nep_api_version(void);

#ifdef __cplusplus
}
#endif
#endif
