#!/usr/bin/env python3
"""Dev probe (GPU box): the priced moves of a fixed placement and the placement search (DESIGN.md §7 "Priced moves") —
the pricing call's time beside the evaluator's per-round time, placement_search from the cheapest capacity-greedy leaf,
and the product's step-1 search with NeptuneStepBase.placement_search off and on.

  python3 tools/probe.py leaf_moves_probe --price 256x128 512x256      nep_leaf_moves for 1 and 32 placements
  python3 tools/probe.py leaf_moves_probe --descend 256x128 512x256 1024x512
                                placement_search: repair_every None / 4 x width 16 / 64; start and end upper,
                                passes, seconds
  python3 tools/probe.py leaf_moves_probe --swaps 256x128 512x256      nep_leaf_swaps beside nep_leaf_moves for 1 and 32
                                placements, then the --descend table with swaps 0 and 16 (DESIGN.md §7 "Priced swaps")
  python3 tools/probe.py leaf_moves_probe --native 256x128 512x256     the --descend rows of width 16 three ways: the
                                Python search, nep_leaf_search verify 0 and verify 1 (DESIGN.md §7 "Native search")
  python3 tools/probe.py leaf_moves_probe 256x128:20 512x256:60        the searches (default): width 0 and 16

Every run is a child process under its own time limit; the first one that does not end well (a time limit, a non-zero
exit status) ends the probe: nothing more is started.
"""
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, "neptune-mip_amd"), REPO]

import numpy as np  # noqa: E402

ALONE_LIMIT_S = 420
DESCEND_LIMIT_S = 20.0    # per placement_search of --descend
SEARCH_SLACK_S = 150      # model builds, the root LP and the end of the search on top of its own time limit


def _instance(size):
    from core.utils import data_to_solver_input
    from core.utils.synthetic import synthetic_payload
    N, F = (int(t) for t in size.split("x"))
    return data_to_solver_input(synthetic_payload(N, F, seed=0), with_db=False)


def _greedy(d, size):
    """the capacity-greedy leaves of the instance, the nodes ranked by their cores (no LP), cheapest first"""
    from core.engine.heuristics import capacity_greedy
    from core.solvers.neptune.neptune_step import NeptuneStep1CPUMinDelayAndUtilization
    st1 = NeptuneStep1CPUMinDelayAndUtilization(alpha=0.5, verbose=False)
    st1.load_data(d)
    wts = st1.objective_weights()
    t0 = time.time()
    leaves = capacity_greedy(d.workload_matrix, d.node_delay_matrix, d.core_per_req_matrix, d.node_cores_matrix,
                             d.function_memory_matrix, d.node_memory_matrix, np.asarray(d.node_cores_matrix, float),
                             tries=4, node_cost=wts[0], delay_coef=wts[1], new_pen=1.0)
    print(f"{size}: {len(leaves)} greedy leaves in {time.time() - t0:.2f}s, estimates "
          f"{[round(float(e), 5) for _, _, e, _ in leaves]}", flush=True)
    return [np.concatenate([np.asarray(C, np.float64).ravel(), np.asarray(n, np.float64)]) for C, n, _, _ in leaves]


def _spread(d):
    """a start where the capacity greedy has no leaf: every function on the node with the most memory left (ties to
    the most cores) — it passes the evaluator's INFEASIBLE rules, its CPU rows need not hold"""
    N, F = len(d.nodes), len(d.functions)
    fmem = np.asarray(d.function_memory_matrix, np.float64).reshape(F)
    left = np.asarray(d.node_memory_matrix, np.float64).reshape(N).copy()
    cores = np.asarray(d.node_cores_matrix, np.float64).reshape(N)
    C, n = np.zeros((F, N)), np.zeros(N)
    for f in np.argsort(-fmem, kind="stable"):
        j = int(np.lexsort((-cores, -left))[0])
        if fmem[f] > left[j]:
            return None
        C[f, j], n[j] = 1.0, 1.0
        left[j] -= fmem[f]
    return np.concatenate([C.ravel(), n])


def _best(fn, reps=5):
    best, out = float("inf"), None
    for _ in range(reps):
        t = time.time()
        out = fn()
        best = min(best, time.time() - t)
    return best, out


def price(size):
    from core.engine.heuristics import apply_move
    from core.engine.lp import LPModel
    d = _instance(size)
    N, F = len(d.nodes), len(d.functions)
    z0 = _greedy(d, size)[0]
    m = LPModel(d, "MinDelayAndUtilization", step=1, alpha=0.5, max_batch=1)
    try:
        r = m.leaf_eval(z0[None, :], rounds=16)
        y = r["prices"][0]
        mv = m.leaf_moves(z0[None, :], prices=y[None, :], max_moves=31)     # (first call: the staging)
        Z = np.stack([z0] + [apply_move(z0, F, N, True, mv["kind"][0, q], mv["fn"][0, q], mv["node"][0, q])
                             for q in range(int(mv["n_moves"][0]))])
        print(f"   R = {m.info.n_rows}, open placements {int(z0[:F * N].sum())}, open nodes {int(z0[F * N:].sum())}, "
              f"moves of the start {int(m.leaf_moves(z0[None, :], prices=y[None, :], max_moves=2 * F * N + N)['n_moves'][0])}",
              flush=True)
        for n_pl in (1, len(Z)):
            P = np.tile(y, (n_pl, 1))
            t0r, _ = _best(lambda: m.leaf_eval(Z[:n_pl], rounds=0, prices=P))
            t32, _ = _best(lambda: m.leaf_eval(Z[:n_pl], rounds=32, prices=P))
            tp, _ = _best(lambda: m.leaf_moves(Z[:n_pl], prices=P, max_moves=0))
            tm, _ = _best(lambda: m.leaf_moves(Z[:n_pl], prices=P, max_moves=64))
            tt, _ = _best(lambda: m.leaf_moves(Z[:n_pl], prices=P, max_moves=64, table=True))
            per = (t32 - t0r) / 32
            print(f"   n {n_pl:3d}: leaf_moves prices only {1e3 * tp:8.2f} ms, 64 moves {1e3 * tm:8.2f} ms, with the "
                  f"table {1e3 * tt:8.2f} ms | leaf_eval rounds 0 {1e3 * t0r:8.2f} ms, 32 {1e3 * t32:8.2f} ms: "
                  f"{1e3 * per:.3f} ms a round -> pricing = {tp / per if per > 0 else float('nan'):.1f} rounds",
                  flush=True)
    finally:
        m.close()


def swaps_price(size):
    """nep_leaf_swaps beside nep_leaf_moves on price()'s placements"""
    from core.engine.heuristics import apply_move
    from core.engine.lp import LPModel
    d = _instance(size)
    N, F = len(d.nodes), len(d.functions)
    z0 = _greedy(d, size)[0]
    m = LPModel(d, "MinDelayAndUtilization", step=1, alpha=0.5, max_batch=1)
    try:
        y = m.leaf_eval(z0[None, :], rounds=16)["prices"][0]
        mv = m.leaf_moves(z0[None, :], prices=y[None, :], max_moves=31)     # (first calls: the stagings)
        sw = m.leaf_swaps(z0[None, :], prices=y[None, :], per_fn=8, max_moves=8 * F, table=True)
        Z = np.stack([z0] + [apply_move(z0, F, N, True, mv["kind"][0, q], mv["fn"][0, q], mv["node"][0, q])
                             for q in range(int(mv["n_moves"][0]))])
        print(f"   R = {m.info.n_rows}, open placements {int(z0[:F * N].sum())}, swaps of the start "
              f"{int(np.isfinite(sw['best'][0]).sum())} (f, to), cheapest {sw['delta'][0, :4].tolist()}", flush=True)
        for n_pl in (1, len(Z)):
            P = np.tile(y, (n_pl, 1))
            tm, _ = _best(lambda: m.leaf_moves(Z[:n_pl], prices=P, max_moves=64))
            tp, _ = _best(lambda: m.leaf_moves(Z[:n_pl], prices=P, max_moves=0))
            ts, _ = _best(lambda: m.leaf_swaps(Z[:n_pl], prices=P, per_fn=4, max_moves=64))
            t8, _ = _best(lambda: m.leaf_swaps(Z[:n_pl], prices=P, per_fn=8, max_moves=64))
            tt, _ = _best(lambda: m.leaf_swaps(Z[:n_pl], prices=P, per_fn=4, max_moves=64, table=True))
            print(f"   n {n_pl:3d}: leaf_moves 64 moves {1e3 * tm:8.2f} ms (prices only {1e3 * tp:8.2f} ms) | leaf_swaps "
                  f"64 swaps per_fn 4 {1e3 * ts:8.2f} ms, per_fn 8 {1e3 * t8:8.2f} ms, with the tables "
                  f"{1e3 * tt:8.2f} ms", flush=True)
    finally:
        m.close()


def swaps(size):
    """the swaps' pricing times, then descend() without and with swaps"""
    swaps_price(size)
    descend(size, (0, 16))


def descend(size, swaps_each=(0,)):
    from core.engine.heuristics import placement_search
    from core.engine.lp import LPModel
    d = _instance(size)
    zs = _greedy(d, size)
    if not zs:
        zs = [_spread(d)]
        print("   no capacity-greedy leaf: the start is every function on the node with the most memory left"
              if zs[0] is not None else "   no capacity-greedy leaf and no spread start: nothing to search from",
              flush=True)
        if zs[0] is None:
            return
    m = LPModel(d, "MinDelayAndUtilization", step=1, alpha=0.5, max_batch=1)
    try:
        r = m.leaf_eval(np.asarray(zs), rounds=32, repair_every=4)
        print(f"   starts: upper {r['upper'].tolist()} lower {r['lower'].tolist()} status {r['status'].tolist()}",
              flush=True)
        m.leaf_moves(zs[0][None, :], max_moves=1)
        for every in (None, 4):
            for width, nsw in ((w, s) for w in (16, 64) for s in swaps_each):
                t0 = time.time()
                res = placement_search(m, zs[0], rounds=32, repair_every=every, width=width, max_passes=1000,
                                       time_limit=DESCEND_LIMIT_S, swaps=nsw)
                kinds = np.bincount(np.asarray([a[0] for a in res["accepted"]], np.int64), minlength=4).tolist()
                print(f"   repair_every {every} width {width:2d} swaps {nsw:2d}: upper {res['start_upper']:.6f} -> "
                      f"{res['upper']:.6f} (lower {res['lower']:.6f}) passes {res['passes']} evaluated "
                      f"{res['evaluated']} accepted {len(res['accepted'])} (add, drop, close, swap) {kinds} "
                      f"{time.time() - t0:.2f}s", flush=True)
    finally:
        m.close()


def native(size):
    """the --descend table's width-16 rows three ways in one process: the Python search, nep_leaf_search verify 0 and
    verify 1 (lazy; the rows with a per-round repair only) — DESIGN.md §7 "Native search" """
    from core.engine.heuristics import placement_search
    from core.engine.lp import LPModel
    d = _instance(size)
    zs = _greedy(d, size)
    if not zs:
        zs = [_spread(d)]
        if zs[0] is None:
            print("   no capacity-greedy leaf and no spread start: nothing to search from", flush=True)
            return
    m = LPModel(d, "MinDelayAndUtilization", step=1, alpha=0.5, max_batch=1)
    try:
        # (first calls: every staging the three ways use)
        m.leaf_search(zs[0], rounds=32, repair_every=4, width=16, swaps=16, max_passes=1, verify="lazy")
        placement_search(m, zs[0], rounds=32, repair_every=4, width=16, swaps=16, max_passes=1)
        for every in (None, 4):
            for nsw in (0, 16):
                kw = dict(rounds=32, repair_every=every, width=16, max_passes=1000, time_limit=DESCEND_LIMIT_S,
                          swaps=nsw)
                ways = [("python", dict(kw)), ("native verify 0", dict(kw, native=True))]
                if every:
                    ways.append(("native verify 1", dict(kw, native=True, verify="lazy")))
                for way, k in ways:
                    t0 = time.time()
                    res = placement_search(m, zs[0], **k)
                    secs = time.time() - t0
                    per = 1e3 * secs / max(1, res["passes"])
                    print(f"   repair_every {every} width 16 swaps {nsw:2d} {way:16s}: {secs:6.2f}s passes "
                          f"{res['passes']:4d} {per:7.2f} ms/pass evaluated {res['evaluated']:6d} verified "
                          f"{res['verified']:6d} upper {res['start_upper']:.6f} -> {res['upper']:.6f}", flush=True)
    finally:
        m.close()


def search(size, secs, width):
    from core.engine.lp import LPModel
    from core.solvers.neptune.neptune_step import NeptuneStep1CPUMinDelayAndUtilization
    d = _instance(size)
    batch = 32
    st1 = NeptuneStep1CPUMinDelayAndUtilization(alpha=0.5, verbose=False, batch=batch, lp_tol=1e-6)
    st1.placement_search = int(width)
    st1.load_data(d)
    m = LPModel(d, "MinDelayAndUtilization", step=1, alpha=0.5, max_batch=batch + 2)
    bm = st1.bound_model(d, batch + 1)
    try:
        res = st1.branch_and_bound(m, bm, time_limit=float(secs), root_max_iters=400000).solve()
    finally:
        m.close()
        bm.close()
    gap = None if res.objective is None else (res.objective - res.bound) / max(1.0, abs(res.objective))
    print(f"{size} {secs:g} s placement_search {int(width)}: {res.status} incumbent {res.objective} (source "
          f"{res.incumbent_source}) bound {res.bound} gap {gap} nodes {res.nodes} leaves {res.leaves} lps {res.lps} "
          f"certified leaves {res.lp_status_kind['leaf']['certified'] + res.lp_status_kind['retry']['certified']} "
          f"primal {res.timing['primal']:.1f}s {res.seconds:.1f}s", flush=True)


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
    if a[:1] == ["--search"]:
        return search(a[1], float(a[2]), int(a[3]))
    if a[:1] == ["--price-one"]:
        return price(a[1])
    if a[:1] == ["--descend-one"]:
        return descend(a[1])
    if a[:1] == ["--swaps-one"]:
        return swaps(a[1])
    if a[:1] == ["--native-one"]:
        return native(a[1])
    if a[:1] in (["--price"], ["--descend"], ["--swaps"], ["--native"]):
        for size in a[1:] or ["256x128", "512x256"]:
            if not child([a[0] + "-one", size], ALONE_LIMIT_S):
                raise SystemExit(1)
        return
    for arg in a or ["256x128:20", "512x256:60"]:
        size, secs = arg.split(":")
        for width in ("0", "16"):
            if not child(["--search", size, secs, width], float(secs) + SEARCH_SLACK_S):
                raise SystemExit(1)


if __name__ == "__main__":
    main()
