"""Primal heuristics of the branch-and-bound (core/engine/bnb.py) that need the instance's data.

`capacity_greedy` — a leaf (every c and n fixed) that is feasible by construction for the reference's rows:
open nodes in the order an LP ranks them (the node values n of the facility relaxation), then
route every loaded source of every function, heaviest first, to the open node of least delay that still has
CPU room for it (constraints_step1.py:57-65) and memory for the function (:18-23), opening that placement;
a function without loaded sources gets the open node with memory room the LP prefers.  Every open
placement then carries >= 1 unit of flow (C2, :5-15) and every source is routed (C4, :27-34), so the leaf LP
has a feasible point — the greedy routing itself; more nodes are opened until the routing succeeds.  The
node box's fixings are kept (closed nodes / placements excluded, fixed-open ones opened first).

`placement_search` — local search over placements with the fixed-placement evaluator and its priced add / drop /
close moves (nep_leaf_eval, nep_leaf_moves; DESIGN.md §7 "Priced moves"); `apply_move` applies one move.
"""
import numpy as np


def capacity_greedy(W, D, cpr, cores, fmem, nmem, n_rank, flow=None, start=None, step=None, tries=4,
                    node_cost=0.0, delay_coef=0.0, c_fix=None, n_fix=None, new_pen=0.5):
    """Leaves [(c [F, N] 0/1, n [N] 0/1, estimate, route)], best estimate first (at most `tries`, one per node
    count); route = (f, i, j) arrays: the loaded source i of f sends all of its workload to j.

    W [F, N] workload, D [N, N] delay, cpr [F, N], cores [N], fmem [F], nmem [N]; n_rank [N]: the order in
    which nodes are opened (descending); flow [F, N] (optional): the LP's flows, tie-break among equal delays.
    start: nodes opened first (default: enough cores for the total CPU demand at each function's cheapest
    cpr); step: nodes added per retry.  estimate = node_cost * open nodes + delay_coef * sum W D of the greedy
    routing (the objective of a feasible point of the leaf, so an upper bound on its LP value).
    c_fix [F, N] / n_fix [N]: -1 free, 0 / 1 fixed (the node's box).  new_pen: a new placement is charged
    new_pen x the median delay between open nodes in the routing choice."""
    W = np.asarray(W, np.float64)
    F, N = W.shape
    D = np.asarray(D, np.float64)
    cpr = np.asarray(cpr, np.float64)
    cores = np.asarray(cores, np.float64)
    fmem = np.asarray(fmem, np.float64)
    nmem = np.asarray(nmem, np.float64)
    rank = np.asarray(n_rank, np.float64).copy()
    cfx = np.full((F, N), -1.0) if c_fix is None else np.asarray(c_fix, np.float64).reshape(F, N)
    nfx = np.full(N, -1.0) if n_fix is None else np.asarray(n_fix, np.float64).reshape(N)
    forced = (nfx == 1.0) | (cfx == 1.0).any(axis=0)
    rank[forced] = np.inf
    allowed_j = nfx != 0.0
    order = [j for j in np.lexsort((-cores, -rank)) if allowed_j[j]]
    nf = int(forced.sum())
    fs, src = np.nonzero(W > 0)
    load = W[fs, src]
    rows = np.argsort(-load, kind="stable")
    demand = float((W * np.where(cfx == 0.0, np.inf, cpr).min(axis=1, keepdims=True)).sum())
    if start is None:
        cum = np.cumsum(cores[order])
        start = int(np.searchsorted(cum, demand)) + 1
    step = step or max(1, N // 32)
    k = max(1, nf, min(start, len(order)))
    fl = None if flow is None else np.asarray(flow, np.float64).reshape(F, N)
    out = []
    while k <= len(order) and len(out) < tries:
        openj = np.asarray(order[:k])
        is_open = np.zeros(N, bool)
        is_open[openj] = True
        cap = cores.copy()
        mem = nmem.copy()
        C = np.zeros((F, N))
        ok = True
        for f, j in zip(*np.nonzero(cfx == 1.0)):                  # fixed-open placements first
            if not is_open[j] or fmem[f] > mem[j] + 1e-12:
                ok = False
                break
            C[f, j] = 1.0
            mem[j] -= fmem[f]
        delay = 0.0
        rf, ri, rj = [], [], []
        pen = new_pen * float(np.median(D[np.ix_(openj, openj)])) if k > 1 else 0.0
        for r in rows if ok else ():
            f, i = int(fs[r]), int(src[r])
            need = load[r] * cpr[f]                               # CPU at each destination
            fit = is_open & (cfx[f] != 0.0) & (need <= cap + 1e-12) & ((C[f] > 0) | (fmem[f] <= mem + 1e-12))
            if not fit.any():
                ok = False
                break
            # least delay, a new placement charged `pen` (memory is the scarce resource: a function spread over
            # every open node crowds the others out)
            key = np.where(fit, D[i] + pen * (C[f] == 0), np.inf)
            best = np.flatnonzero(key == key.min())
            j = int(best[np.argmax(fl[f, best])] if fl is not None and len(best) > 1 else best[0])
            cap[j] -= need[j]
            delay += load[r] * D[i, j]
            rf.append(f)
            ri.append(i)
            rj.append(j)
            if C[f, j] == 0:
                C[f, j] = 1.0
                mem[j] -= fmem[f]
        if ok:
            for f in np.flatnonzero(C.sum(axis=1) < 1):             # functions with no loaded source
                cand = np.flatnonzero(is_open & (cfx[f] != 0.0) & (fmem[f] <= mem + 1e-12))
                if cand.size == 0:
                    ok = False
                    break
                j = int(cand[np.argmax(rank[cand] if fl is None else fl[f, cand])])
                C[f, j] = 1.0
                mem[j] -= fmem[f]
        if ok:
            n = (C.sum(axis=0) > 0).astype(np.float64)
            n[nfx == 1.0] = 1.0
            out.append((C, n, node_cost * float(n.sum()) + delay_coef * delay,
                        (np.asarray(rf, np.int64), np.asarray(ri, np.int64), np.asarray(rj, np.int64))))
        k += step
    out.sort(key=lambda t: t[2])
    return out


def apply_move(z, F, N, has_n, kind, fn, node, src=None):
    """z' = the placement z (c f-major [F N], then n [N] where the variant has n) after one priced move (nep_leaf_moves,
    nep_leaf_swaps): ADD (0) opens (fn, node) and the node; DROP (1) closes (fn, node), and the node with its last
    placement; CLOSE (2) closes the node and every placement on it; SWAP (3) moves fn from the node `src` to `node`:
    closes (fn, src), and that node with its last placement, and opens (fn, node) and the node."""
    z = np.array(z, np.float64, copy=True)
    C = z[:F * N].reshape(F, N)
    kind, fn, node = int(kind), int(fn), int(node)
    if kind == 0:
        C[fn, node] = 1.0
        opened = 1.0
    elif kind == 1:
        C[fn, node] = 0.0
        opened = 1.0 if C[:, node].any() else 0.0
    elif kind == 2:
        C[:, node] = 0.0
        opened = 0.0
    elif kind == 3:
        if src is None:
            raise ValueError("a swap needs its source node")
        C[fn, int(src)] = 0.0
        C[fn, node] = 1.0
        opened = 1.0
        if has_n:
            z[F * N + int(src)] = 1.0 if C[:, int(src)].any() else 0.0
    else:
        raise ValueError(f"unknown move kind {kind}")
    if has_n:
        z[F * N + node] = opened
    return z


def placement_search(model, z0, rounds=32, repair_every=None, width=16, max_passes=32, time_limit=None, warm=True,
                     log=None, swaps=0, per_fn=4, native=False, verify="all"):
    """Local search over placements from z0 [n_int] with the fixed-placement evaluator and its priced moves (DESIGN.md
    §7 "Priced moves").  model: anything with F, N, n_int and leaf_eval / leaf_moves / leaf_routing (LPModel's
    contracts).  Per pass: the moves of the current placement at its evaluated prices, the first `width` applied, the
    neighbours evaluated in one leaf_eval call cut off at the incumbent's upper (from the current prices when `warm`),
    the best accepted when it improves upper by more than 1e-9 max(1, |upper|) (ties: the earlier move); a start
    without a point takes the first neighbour that has one.  Stops at the first pass without an acceptance, at
    max_passes or at time_limit seconds.  swaps > 0 (the model then has leaf_swaps too): each pass also asks for that
    many priced swaps (nep_leaf_swaps, the per_fn cheapest destinations per function) at the same prices; their
    neighbours follow the single moves' in the same leaf_eval call.  Deterministic.  Returns dict(z, upper, lower, row,
    dst, val (the routing of z, None without a point), start_upper, passes, evaluated, verified, accepted [(kind, fn,
    node, delta, upper), and for a swap (3, fn, to, delta, upper, from)]); verified counts the neighbours whose
    host-verified upper the search used (verify="all": those that reached the device and were not cut off).
    verify="lazy" (needs repair_every >= 1) is nep_leaf_search's lazy rule on leaf_eval's device_upper d_q: the
    candidates are the neighbours that are not cut off with a finite d_q (below upper - 1e-9 max(1, |upper|) when upper
    is finite), taken in ascending (d_q, q); the first whose host-verified upper improves (a start without a point: is
    finite) is accepted, and the search ends when none does.  native=True: model.leaf_search(...) with the same
    arguments (the descent as one native call; `log` is not called)."""
    import time
    if verify not in ("all", "lazy"):
        raise ValueError(f"verify must be 'all' or 'lazy', not {verify!r}")
    if verify == "lazy" and not repair_every:
        raise ValueError("verify='lazy' needs the device objectives of repair_every >= 1")
    if native:
        return model.leaf_search(z0, rounds=rounds, repair_every=repair_every, width=width, swaps=swaps, per_fn=per_fn,
                                 max_passes=max_passes, warm=warm, verify=verify, time_limit=time_limit)
    F, N = int(model.F), int(model.N)
    has_n = int(model.n_int) == F * N + N
    t0 = time.monotonic() if time_limit is not None else 0.0
    z = np.array(np.asarray(z0, np.float64).reshape(-1), copy=True)
    r = model.leaf_eval(z[None, :], rounds=rounds, repair_every=repair_every)
    upper, lower = float(r["upper"][0]), float(r["lower"][0])
    prices = np.array(r["prices"][0], np.float64, copy=True)
    entries = model.leaf_routing(0) if np.isfinite(upper) else (None, None, None)
    out = {"start_upper": upper, "passes": 0, "evaluated": 0, "verified": 0, "accepted": []}
    while out["passes"] < max_passes and np.isfinite(lower):
        if time_limit is not None and time.monotonic() - t0 >= time_limit:
            break
        mv = model.leaf_moves(z[None, :], prices=prices[None, :], max_moves=int(width))
        k = int(mv["n_moves"][0])
        cand = [(int(mv["kind"][0, q]), int(mv["fn"][0, q]), int(mv["node"][0, q]), float(mv["delta"][0, q]))
                for q in range(k)]
        if swaps > 0:
            sw = model.leaf_swaps(z[None, :], prices=prices[None, :], per_fn=int(per_fn), max_moves=int(swaps))
            cand += [(3, int(sw["fn"][0, q]), int(sw["to"][0, q]), float(sw["delta"][0, q]), int(sw["from"][0, q]))
                     for q in range(int(sw["n_moves"][0]))]
            k = len(cand)
        if k == 0:
            break
        out["passes"] += 1
        Z = np.stack([apply_move(z, F, N, has_n, c[0], c[1], c[2], *c[4:]) for c in cand])
        r = model.leaf_eval(Z, rounds=rounds, cutoff=upper, prices=np.tile(prices, (k, 1)) if warm else None,
                            repair_every=repair_every)
        out["evaluated"] += k
        ups = np.asarray(r["upper"], np.float64)
        live = (np.asarray(r["status"]) != 3) & (np.asarray(r["status"]) != 4)   # not INFEASIBLE, not CUTOFF
        if verify == "all":
            out["verified"] += int(live.sum())
        if verify == "lazy":
            dq = np.asarray(r["device_upper"], np.float64)
            ok = live & np.isfinite(dq)
            if np.isfinite(upper):
                ok &= dq < upper - 1e-9 * max(1.0, abs(upper))
            q = -1
            for t in sorted(np.flatnonzero(ok).tolist(), key=lambda t: (dq[t], t)):
                out["verified"] += 1
                better = ups[t] < upper - 1e-9 * max(1.0, abs(upper)) if np.isfinite(upper) else np.isfinite(ups[t])
                if better:
                    q = t
                    break
            if q < 0:
                break
        elif np.isfinite(upper):
            q = int(np.argmin(ups))
            if not ups[q] < upper - 1e-9 * max(1.0, abs(upper)):
                break
        else:
            has = np.flatnonzero(np.isfinite(ups))
            if has.size == 0:
                break
            q = int(has[0])
        entries = model.leaf_routing(q)
        z, upper, lower = Z[q], float(ups[q]), float(r["lower"][q])
        prices = np.array(r["prices"][q], np.float64, copy=True)
        out["accepted"].append(cand[q][:4] + (upper,) + cand[q][4:])
        if log is not None:
            log(f"placement search: pass {out['passes']} move {out['accepted'][-1][:3]} upper {upper:.10g}")
    out.update(z=z, upper=upper, lower=lower, row=entries[0], dst=entries[1], val=entries[2])
    return out
