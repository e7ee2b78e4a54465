#!/usr/bin/env python3
"""Dev probe (GPU box): the product's step-1 search with the fixed-placement evaluator off and on (DESIGN.md §7
"Fixed-placement evaluator") — incumbent, bound, gap, certified leaves and the leaf_eval_* counters per run; and the
evaluator alone on capacity-greedy leaves, by batch size and rounds.

  python3 tools/probe.py leaf_eval_probe 512x256:60 256x128:20      the searches (default): leaf_eval 0, 1, 2 per size
  python3 tools/probe.py leaf_eval_probe --alone 256x128 512x256    the evaluator alone
  python3 tools/probe.py leaf_eval_probe --alone 256x128 --repair-every 0,4,1
                                the evaluator alone at 32 rounds with the per-round repair on the device
                                (nep_leaf_eval_ex): wall time, what the repair adds, brackets, NO_POINT, chosen rounds

Every run (one search, or one size of the evaluator alone) is a child process under its own time limit; the first
one that does not end well (a time limit, a non-zero exit status) ends the probe: nothing more is started.
"""
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, "neptune-mip_amd"), REPO]

import numpy as np  # noqa: E402

ALONE_LIMIT_S = 240
SEARCH_SLACK_S = 150      # model builds, the root LP and the end of the search on top of its own time limit


def search(size, secs, leaf_eval):
    from core.engine.lp import LPModel
    from core.solvers.neptune.neptune_step import NeptuneStep1CPUMinDelayAndUtilization
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    N, F = (int(t) for t in size.split("x"))
    d = data_to_solver_input(synthetic_payload(N, F, seed=0), with_db=False)
    batch = 32
    st1 = NeptuneStep1CPUMinDelayAndUtilization(alpha=0.5, verbose=False, batch=batch, lp_tol=1e-6)
    st1.leaf_eval = int(leaf_eval)
    st1.load_data(d)
    m = LPModel(d, "MinDelayAndUtilization", step=1, alpha=0.5, max_batch=batch + 2)
    bm = st1.bound_model(d, batch + 1)
    try:
        if leaf_eval:
            m.leaf_eval(np.zeros((1, m.n_int)), rounds=0)      # (the workspace, before LPs stream)
        res = st1.branch_and_bound(m, bm, time_limit=float(secs), root_max_iters=400000).solve()
    finally:
        m.close()
        bm.close()
    gap = None if res.objective is None else (res.objective - res.bound) / max(1.0, abs(res.objective))
    print(f"{size} {secs:g} s leaf_eval {int(leaf_eval)}: {res.status} incumbent {res.objective} (source "
          f"{res.incumbent_source}) bound {res.bound} gap {gap} nodes {res.nodes} leaves {res.leaves} lps {res.lps} "
          f"certified leaves {res.lp_status_kind['leaf']['certified'] + res.lp_status_kind['retry']['certified']} "
          f"{res.seconds:.1f}s", flush=True)
    print(f"   leaf_eval stats {res.leaf_stats}", flush=True)


def alone(size, every=None):
    from core.engine.heuristics import capacity_greedy
    from core.engine.lp import LPModel
    from core.solvers.neptune.neptune_step import NeptuneStep1CPUMinDelayAndUtilization
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    N, F = (int(t) for t in size.split("x"))
    d = data_to_solver_input(synthetic_payload(N, F, seed=0), with_db=False)
    st1 = NeptuneStep1CPUMinDelayAndUtilization(alpha=0.5, verbose=False)
    st1.load_data(d)
    wts = st1.objective_weights()
    t0 = time.time()
    leaves = capacity_greedy(d.workload_matrix, d.node_delay_matrix, d.core_per_req_matrix, d.node_cores_matrix,
                             d.function_memory_matrix, d.node_memory_matrix, np.asarray(d.node_cores_matrix, float),
                             tries=4, node_cost=wts[0], delay_coef=wts[1], new_pen=1.0)
    print(f"{size}: {len(leaves)} greedy leaves in {time.time() - t0:.2f}s, estimates "
          f"{[round(float(e), 5) for _, _, e, _ in leaves]}", flush=True)
    Z = []
    for C, n, _, _ in leaves:
        Z.append(np.concatenate([C.ravel(), n]))
        for j in np.flatnonzero(n > 0.5)[-7:]:      # the same leaf with one open node closed
            C2, n2 = C.copy(), n.copy()
            C2[:, j] = 0.0
            n2[j] = 0.0
            Z.append(np.concatenate([C2.ravel(), n2]))
    Z = np.asarray(Z)
    m = LPModel(d, "MinDelayAndUtilization", step=1, alpha=0.5, max_batch=1)
    print(f"   {len(Z)} placements, R = {m.info.n_rows}", flush=True)
    try:
        m.leaf_eval(Z, rounds=0)                    # (the workspace and the host's point storage: first call)
        if every is not None:
            return alone_repair(m, Z, every)
        for n_pl in (1, 8, len(Z)):
            for rounds in (0, 32, 128):
                t1 = time.time()
                r = m.leaf_eval(Z[:n_pl], rounds=rounds)
                dt = time.time() - t1
                fin = np.isfinite(r["upper"])
                gap = (r["upper"][fin] - r["lower"][fin]) / np.maximum(1.0, np.abs(r["lower"][fin]))
                print(f"   n {n_pl:3d} rounds {rounds:3d}: {1e3 * dt:8.2f} ms  status counts "
                      f"{np.bincount(r['status'], minlength=5).tolist()} (exact, feasible, no point, infeasible, cutoff)"
                      f"  bracket median {np.median(gap) if gap.size else float('nan'):.2e} max "
                      f"{gap.max() if gap.size else float('nan'):.2e}", flush=True)
    finally:
        m.close()


def alone_repair(m, Z, every):
    """32 rounds, 1 and all placements, per repair_every: the best of 5 wall times, what the repair adds to the call
    without it (the repair kernels are serial in the rounds' stream, so the difference is their time), the brackets"""
    rounds = 32
    m.leaf_eval(Z, rounds=1, repair_every=1)        # (the repair's workspace: first call)
    for n_pl in (1, len(Z)):
        base = None
        for k in every:
            best, r = float("inf"), None
            for _ in range(5):
                t1 = time.time()
                r = m.leaf_eval(Z[:n_pl], rounds=rounds, repair_every=k)
                best = min(best, time.time() - t1)
            if k == 0:
                base = best
            fin = np.isfinite(r["upper"])
            gap = (r["upper"][fin] - r["lower"][fin]) / np.maximum(1.0, np.abs(r["lower"][fin]))
            rep = np.isfinite(r["round_upper"]).sum(axis=1)
            conf = int(((r["upper_round"] > 0) | ((r["upper_round"] == 0) & (r["upper"] <= r["device_upper"]))).sum())
            added = "" if base is None or k == 0 else f" repair adds {1e3 * (best - base):.2f} ms " \
                                                      f"({100 * (best - base) / best:.0f} % of the call)"
            print(f"   n {n_pl:3d} rounds {rounds} repair_every {k}: {1e3 * best:8.2f} ms{added}  status counts "
                  f"{np.bincount(r['status'], minlength=5).tolist()}  bracket median "
                  f"{np.median(gap) if gap.size else float('nan'):.2e} max {gap.max() if gap.size else float('nan'):.2e}"
                  f"  chosen rounds {r['upper_round'].tolist()}  rounds with a device point (min/median/max) "
                  f"{int(rep.min())}/{int(np.median(rep))}/{int(rep.max())}  device picks the host kept or beat {conf}",
                  flush=True)


def child(args, limit):
    """one run in a fresh process under its own time limit: True when it ended well"""
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, check=False, timeout=limit).returncode
    except subprocess.TimeoutExpired:
        print(f"{' '.join(args)}: no result within {limit:g} s — the probe ends here", flush=True)
        return False
    if rc != 0:
        print(f"{' '.join(args)}: exit status {rc} — the probe ends here", flush=True)
        return False
    return True


def main():
    a = sys.argv[1:]
    every = None
    if "--repair-every" in a:
        q = a.index("--repair-every")
        every = a[q + 1]
        a = a[:q] + a[q + 2:]
    if a[:1] == ["--search"]:
        return search(a[1], float(a[2]), int(a[3]))
    if a[:1] == ["--alone-one"]:
        return alone(a[1], None if every is None else [int(t) for t in every.split(",")])
    if a[:1] == ["--alone"]:
        for size in a[1:] or ["256x128", "512x256"]:
            if not child(["--alone-one", size] + ([] if every is None else ["--repair-every", every]), ALONE_LIMIT_S):
                raise SystemExit(1)
        return
    for arg in a or ["512x256:60", "256x128:20"]:
        size, secs = arg.split(":")
        for on in ("0", "1", "2"):
            if not child(["--search", size, secs, on], float(secs) + SEARCH_SLACK_S):
                raise SystemExit(1)


if __name__ == "__main__":
    main()
